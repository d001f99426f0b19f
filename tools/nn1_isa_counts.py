#!/usr/bin/env python3
"""Static instruction counts of one instantiation of a kernel of flux3d.jl_amd/csrc/chamfer.hip, from gfx950 assembly.

Cross-compiles the unit to assembly with the Makefile's flags (no GPU needed), then prints for the named instantiation the
register and spill counts of its metadata and, per basic block, the instructions by class.  Classes go by mnemonic prefix only:

  VALU   v_*  other than the next three            MFMA   v_mfma*
  lrd    v_readlane*  (spill reloads, shuffles)    lwr    v_writelane*  (spills)
  LDS    ds_*                                      mem    global_* / buffer_* / flat_* / scratch_*
  SALU   s_*  other than s_nop                     nop    cycles of s_nop (operand + 1)

A block that branches back to its own label is marked `loop`; `->` lists the labels a block branches to, so that regions
(the staging loop, a pass's setup up to its first MFMA, the filter loop's six-block body) can be read off in order.

  python tools/nn1_isa_counts.py                        # nn1_f16_kernel<false, false, true>, the instantiation bench.py times
  python tools/nn1_isa_counts.py --kernel ILb1ELb0ELb1E  # any substring of the mangled name
  python tools/nn1_isa_counts.py --asm file.s            # count an assembly file instead of compiling
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flux3d.jl_amd", "csrc")
CLASSES = ("VALU", "MFMA", "lrd", "lwr", "LDS", "mem", "SALU", "nop")


def makefile_flags():
    """CXXFLAGS of csrc/Makefile with $(EXTRA) dropped and the continuation joined."""
    txt = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    line = next(ln for ln in txt.splitlines() if ln.startswith("CXXFLAGS"))
    return [f for f in line.split("=", 1)[1].split() if f != "$(EXTRA)"]


def compile_asm(unit, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(tempfile.mkdtemp(prefix="nn1_isa_"), unit + ".s")
    cmd = [hipcc, "--offload-arch=gfx950", *makefile_flags(), *extra, "--cuda-device-only", "-S", unit + ".hip", "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    return out


def classify(mn, ops):
    if mn.startswith("v_mfma"):
        return "MFMA", 1
    if mn.startswith("v_readlane"):
        return "lrd", 1
    if mn.startswith("v_writelane"):
        return "lwr", 1
    if mn.startswith("v_"):
        return "VALU", 1
    if mn.startswith("ds_"):
        return "LDS", 1
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "mem", 1
    if mn == "s_nop":
        return "nop", int(ops.split()[0], 0) + 1
    if mn.startswith("s_"):
        return "SALU", 1
    return None, 0


def function_body(lines, pat):
    """(mangled name, [(line number, text)]) of the first function whose label contains `pat`."""
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and pat in m.group(1):
            body = []
            for j in range(i + 1, len(lines)):
                if lines[j].startswith(".Lfunc_end"):
                    return m.group(1), body
                body.append((j + 1, lines[j]))
    sys.exit(f"no function matching {pat!r}")


def metadata(lines, name):
    keys = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "agpr_count", "private_segment_fixed_size",
            "group_segment_fixed_size")
    at = next(i for i, ln in enumerate(lines) if ln.strip() == f".name:           {name}" or ln.strip().split() == [".name:", name])
    found = {}
    for ln in lines[max(0, at - 12):at + 16]:  # one kernel's metadata entry: a few keys either side of its .name
        m = re.match(r"^\s+\.(\w+):\s+(\S+)", ln)
        if m and m.group(1) in keys:
            found[m.group(1)] = m.group(2)
    return found


def blocks_of(body):
    blocks = [{"label": "entry", "line": body[0][0] if body else 0, "n": dict.fromkeys(CLASSES, 0), "to": []}]
    for no, ln in body:
        s = ln.split(";")[0].rstrip()
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            blocks.append({"label": m.group(1), "line": no, "n": dict.fromkeys(CLASSES, 0), "to": []})
            continue
        s = s.strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        parts = s.split(None, 1)
        mn, ops = parts[0], parts[1] if len(parts) > 1 else ""
        cls, n = classify(mn, ops)
        if cls:
            blocks[-1]["n"][cls] += n
        if mn.startswith(("s_cbranch", "s_branch")):
            blocks[-1]["to"].append(ops.strip())
    return blocks


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--unit", default="chamfer")
    ap.add_argument("--kernel", default="nn1_f16_kernelILb0ELb0ELb1E", help="substring of the mangled name")
    ap.add_argument("--asm", help="an assembly file to count instead of compiling the unit")
    ap.add_argument("--extra", default="", help="extra compiler flags, e.g. '-DFX3D_HFIFO=4'")
    a = ap.parse_args()
    path = a.asm or compile_asm(a.unit, a.extra.split())
    lines = open(path).read().splitlines()
    name, body = function_body(lines, a.kernel)
    print(f"# {name}")
    print("# " + "  ".join(f"{k}={v}" for k, v in metadata(lines, name).items()))
    blocks = blocks_of(body)
    hdr = f"{'block':<12}{'line':>7} " + "".join(f"{c:>6}" for c in CLASSES) + "  notes"
    print(hdr)
    tot = dict.fromkeys(CLASSES, 0)
    base = blocks[0]["line"]
    for b in blocks:
        for c in CLASSES:
            tot[c] += b["n"][c]
        notes = ("loop " if b["label"] in b["to"] else "") + ("-> " + " ".join(b["to"]) if b["to"] else "")
        print(f"{b['label']:<12}{b['line'] - base:>7} " + "".join(f"{b['n'][c]:>6}" for c in CLASSES) + "  " + notes)
    print(f"{'total':<12}{'':>7} " + "".join(f"{tot[c]:>6}" for c in CLASSES))


if __name__ == "__main__":
    main()
