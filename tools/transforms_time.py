#!/usr/bin/env python3
"""PointCloud / TriMesh transforms on the device, per call and per kernel, beside the numpy restatement (tests/transforms_ref.py)
and a plain torch-on-device expression for context -- at B = 32 x 1024 clouds (a ModelNet batch, the fused plan), B = 8 teapots,
and the jittered 1400 x 1400-cell sheet (1.96 M vertices in one mesh, the two-launch plan).

Per op: the host-clock time of one call ended by a device synchronisation (median of --reps), the kernel time from the
library's own HIP events around the op's launches (fx3d_profile_enable), the algorithmic bytes over that time (normalize:
two reads and one write on the two-launch plan, one read and one write on the fused plan; realign and segment_minmax likewise;
every other map one read and one write), the restatement's host time, and a torch expression of the same math on the device.
Every device map is checked bit for bit against the restatement.  One JSON line per (shape, op).

  python tools/transforms_time.py [--reps 20] [--only clouds|teapot8|sheet]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flux3d_jl_amd as fx  # noqa: E402
from flux3d_jl_amd import _lib  # noqa: E402
import normals_ref  # noqa: E402
import transforms_ref as ref  # noqa: E402


def kernel_ms(name, fn, reps):
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(reps):
        fn()
    fx.synchronize()
    avg, mn, mx, cnt = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), C.byref(mn), C.byref(mx), C.byref(cnt))
    _lib.call("fx3d_profile_enable", 0)
    return avg.value, mn.value


def call_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def host_ms(fn, reps):
    ts, r = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), r


def torch_ms(x_np, op, reps):
    """The same math as a torch expression on the device (context only: a different summation order for the statistics)."""
    try:
        import torch
    except ImportError:
        return None
    if not torch.cuda.is_available():
        return None
    t = torch.from_numpy(np.ascontiguousarray(x_np.reshape(x_np.shape[0], -1, order="F").T.copy())).cuda()  # (cols, D)
    R = torch.randn(3, 3, device="cuda")
    f = {"normalize": lambda: (t - t.mean(0)) / (t.std(0) + 1e-6),
         "scale": lambda: 2.0 * t,
         "rotate": (lambda: t @ R) if t.shape[1] == 3 else None,
         "realign": lambda: (t - t.amin(0)) / ((t.amax(0) - t.amin(0)) + 1e-6) * 2.0 - 1.0}.get(op)
    if f is None:
        return None
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    return call_ms(f, reps, torch.cuda.synchronize)


def report(shape, op, plan, nbytes, k, got, want, t_call, t_host, t_torch):
    print(json.dumps({"shape": shape, "op": op, "plan": plan, "bit_identical": ref.same_bits(got, want),
                      "call_ms": round(t_call, 4), "kernel_ms": round(k[0], 4), "kernel_min_ms": round(k[1], 4),
                      "algorithmic_MB": round(nbytes / 1e6, 3), "GBps": round(nbytes / (k[0] * 1e-3) / 1e9, 1),
                      "host_restatement_ms": round(t_host, 2), "torch_call_ms": None if t_torch is None else round(t_torch, 4)}),
          flush=True)


def measure(shape, obj, reps, host_reps):
    is_mesh = isinstance(obj, fx.TriMesh)
    if is_mesh:
        x = obj.get_verts_packed().to_host()
        lens = obj._verts_len
        D, n_max, B = 3, obj.V, obj.N
    else:
        x = obj.points.to_host()
        D, n_max, B = x.shape
    plan = fx.transform_plan(D, n_max, B).split()[0].split("=")[1]
    nb = x.nbytes
    rng = np.random.default_rng(2)
    R = np.asfortranarray(rng.standard_normal((3, 3)).astype(np.float32))
    tmin, tmax = np.full((D, 1), -1.0, np.float32), np.ones((D, 1), np.float32)
    pts = (lambda r: r.get_verts_packed()) if is_mesh else (lambda r: r.points)
    stats_reads = 2 if plan == "two_launch" else 1
    _, c, s = fx.normalize(obj, return_stats=True)
    c, s = c.to_host(), s.to_host()
    ops = {
        "normalize": ((stats_reads + 1) * nb, lambda: fx.normalize(obj),
                      (lambda: ref.mesh_normalize(x, lens, c, s)) if is_mesh else (lambda: ref.pcloud_normalize(x, c, s))),
        "scale": (2 * nb, lambda: fx.scale(obj, 2.0), lambda: (ref.mesh_scale if is_mesh else ref.pcloud_scale)(x, 2.0)),
        "realign": ((stats_reads + 1) * nb + nb, lambda: fx.realign(obj, tmin, tmax),
                    (lambda: ref.mesh_realign(x, lens, tmin, tmax)) if is_mesh else (lambda: ref.pcloud_realign(x, tmin, tmax))),
    }
    if D == 3:
        ops["rotate"] = (2 * nb, lambda: fx.rotate(obj, R),
                         (lambda: ref.mesh_rotate(x, lens, R)) if is_mesh else (lambda: ref.pcloud_rotate(x, R)))
    if is_mesh:
        ops["translate"] = (2 * nb, lambda: fx.translate(obj, [1.0, 2.0, 3.0]), lambda: ref.mesh_translate(x, [1.0, 2.0, 3.0]))
    kernels = {"normalize": ["normalize"], "scale": ["scale"], "translate": ["translate"], "rotate": ["rotate"],
               "realign": ["segment_minmax", "realign"]}
    for op, (nbytes, dev, host) in ops.items():
        for _ in range(3):
            r = dev()
        fx.synchronize()
        got = pts(r)
        got = got.to_host() if hasattr(got, "to_host") else got
        t_host, want = host_ms(host, host_reps)
        ks = [kernel_ms(k, dev, reps) for k in kernels[op]]
        k = (sum(a for a, _ in ks), sum(b for _, b in ks))
        report(shape, op, plan, nbytes, k, got, want, call_ms(dev, reps, fx.synchronize), t_host, torch_ms(x, op, reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["clouds", "teapot8", "sheet"])
    a = ap.parse_args()
    assert fx.functional(), "transforms_time.py needs a GPU"
    if a.only in (None, "clouds"):
        x = np.asfortranarray(np.random.default_rng(0).standard_normal((3, 1024, 32)).astype(np.float32))
        measure("clouds 32 x 1024", fx.PointCloud(fx.gpu(x)), a.reps, 5)
    if a.only in (None, "teapot8"):
        t = os.path.join(ROOT, "tests", "golden", "teapot.obj")
        measure("teapot x 8", fx.gpu(fx.load_trimesh(*([t] * 8))), a.reps, 5)
    if a.only in (None, "sheet"):
        v, f = normals_ref.sheet(1400, 1400)
        measure("sheet 1400^2", fx.gpu(fx.TriMesh([v], [f], index_base=0)), a.reps, 1)


if __name__ == "__main__":
    main()
