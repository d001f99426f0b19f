"""tests/dirty_ws.py against a stand-in allocator over host memory -- the fills, the exact size, the guard pads, the order of the
patterns -- and the case table of tests/test_gpu_workspace.py against ``_lib.SIGNATURES`` and the header.  No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import dirty_ws as dirty
from conftest import ROOT
from test_misaligned_host import _FakeFx


def _poke(ws, rel, value=0):
    ctypes.c_uint8.from_address(ws.ptr + rel).value = value


def test_pattern_words_are_as_documented():
    z, i, o = (dirty.fill_bytes(64, p) for p in ("ZERO", "INF", "ONES"))
    assert not z.any()
    assert np.all(i.view(np.uint32) == 0x7F800000) and np.all(np.isposinf(i.view(np.float32)))
    assert np.all(i.view(np.int32) == 2139095040) and i.view(np.int32)[0] > 2.1e9
    d = i.view(np.float64)
    assert np.all(np.isfinite(d)) and np.all(d > 1e306) and np.all(d < 1e307)
    assert np.all(o == 0xFF) and np.all(np.isnan(o.view(np.float32))) and np.all(np.isnan(o.view(np.float64)))
    assert np.all(o.view(np.int32) == -1) and np.all(o.view(np.uint16) == 65535)
    assert dirty.fill_bytes(7, "INF").size == 7 and dirty.fill_bytes(0, "ONES").size == 0
    assert dirty.PATTERNS == ("ZERO", "STALE", "INF", "ONES")   # benign before adversarial
    with pytest.raises(AssertionError):
        dirty.fill_bytes(8, "STALE")


@pytest.mark.parametrize("nbytes", [1, 8, 255, 256, 1000, 4097])
def test_address_is_256_aligned_and_the_size_exact(nbytes):
    ws = dirty.Workspace(_FakeFx, nbytes)
    assert ws.ptr % 256 == 0 and ws.nbytes == nbytes and ws.placed.arr.nbytes == nbytes and ws.image().size == nbytes
    assert ws.placed.lo >= dirty.GUARD and ws.placed.buf.nbytes - ws.placed.hi >= dirty.GUARD   # a row, not a word
    img = ws.placed.buf.to_host()
    assert np.all(img[:ws.placed.lo] == 0xA5) and np.all(img[ws.placed.hi:] == 0xA5)
    for pattern in ("ZERO", "INF", "ONES"):
        ws.fill(pattern)
        assert np.array_equal(ws.image(), dirty.fill_bytes(nbytes, pattern))
        ws.check(pattern)


def test_a_zero_byte_query_is_a_null_workspace():
    ws = dirty.Workspace(_FakeFx, 0)
    assert ws.ptr is None and ws.nbytes == 0 and ws.image().size == 0
    ws.fill("ONES")
    ws.check()
    assert list(dirty.patterns(ws, prime=lambda: None)) == list(dirty.PATTERNS)


@pytest.mark.parametrize("nbytes", [1, 260, 4096])
def test_pokes_at_the_edges(nbytes):
    for rel, seen in ((-1, True), (nbytes, True), (nbytes - 1, False), (0, False), (-dirty.GUARD, True), (nbytes + dirty.GUARD - 1, True)):
        ws = dirty.Workspace(_FakeFx, nbytes)
        ws.fill("ONES")
        _poke(ws, rel, 0x00)
        if seen:
            assert list(ws.placed.touched()) == [rel]
            with pytest.raises(AssertionError, match="pad bytes written"):
                ws.check("probe")
        else:
            ws.check("probe")


def test_stale_primes_and_does_not_refill():
    ws = dirty.Workspace(_FakeFx, 64)
    log = []

    def prime():
        log.append(("prime", ws.image().copy()))
        ctypes.memset(ws.ptr, 0x3C, 64)            # what the priming run leaves
    for pattern in dirty.patterns(ws, prime):
        log.append((pattern, ws.image().copy()))
        ctypes.memset(ws.ptr, 0x11, 64)            # what the run under test leaves
    names = [n for n, _ in log]
    assert names == ["ZERO", "prime", "STALE", "INF", "ONES"]
    img = dict(log)
    assert not img["ZERO"].any()
    assert np.all(img["prime"] == 0x11)            # primed in this very buffer, on what the ZERO run left
    assert np.all(img["STALE"] == 0x3C)            # ... and nothing written between the priming run and the STALE run
    assert np.array_equal(img["INF"], dirty.fill_bytes(64, "INF")) and np.all(img["ONES"] == 0xFF)


def test_other_inputs_keep_shape_values_and_indices():
    x = np.asfortranarray(np.arange(24, dtype=np.float32).reshape(3, 4, 2, order="F"))
    y = dirty.other_inputs(x)
    assert y.shape == x.shape and y.dtype == x.dtype and y.flags.f_contiguous and not np.array_equal(x, y)
    assert np.array_equal(np.sort(y.ravel()), np.sort(x.ravel())) and np.array_equal(y[:, :, 0], x[::-1, ::-1, 1])
    idx = np.arange(6, dtype=np.int32)
    assert dirty.other_inputs(idx) is not None and np.array_equal(dirty.other_inputs(idx), idx)
    assert np.array_equal(dirty.other_inputs(np.ones(3, np.uint8)), np.ones(3, np.uint8))


# --------------------------------------------------------------------------------------------------------------- completeness
def _header_workspace_entries():
    with open(os.path.join(ROOT, "include", "flux3d_hip.h")) as fh:
        decl = re.findall(r"FX3D_API fx3d_status (fx3d_\w+)\(([^;]*?)\);", fh.read(), re.S)
    return {name for name, params in decl if re.search(r"void \*\w*ws\w*,\s*size_t", params)}


def _signature_module():
    """flux3d.jl_amd/_lib.py as a module of its own: SIGNATURES is plain data, it needs neither the package nor the built library."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_fx3d_signatures", os.path.join(ROOT, "flux3d.jl_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _signature_workspace_entries():
    _lib = _signature_module()
    out = set()
    for name, args in _lib.SIGNATURES.items():
        pairs = [i for i in range(len(args) - 1) if args[i] is _lib.vp and args[i + 1] is _lib.sz]
        # (void *, size_t) in a row is a workspace, but for the copies (bytes) and the two (pointer, uint64 increment) entries
        if pairs and not name.startswith("fx3d_memcpy") and name not in ("fx3d_counter_add", "fx3d_momentum_step_offset"):
            out.add(name)
    return out


def test_every_workspace_entry_point_and_every_query_has_a_case():
    _lib = _signature_module()
    import test_gpu_workspace as tw
    entries = _signature_workspace_entries()
    assert entries == _header_workspace_entries()      # the two ways of finding them agree: neither rule has gone stale
    queries = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    assert len(queries) >= 31 and len(entries) >= 47
    cased = {e for c in tw.CASES for e in c.entries}
    asked = {q for c in tw.CASES for q in c.queries}
    assert entries <= cased, sorted(entries - cased)
    assert queries <= asked, sorted(queries - asked)
    assert cased <= set(_lib.SIGNATURES) and asked <= queries
    # every entry point that refuses a workspace has its refusal case; fx3d_knn_ws alone falls back instead (test_fall_backs_...)
    refused = {e for c in tw.CASES for e in c.refuse}
    assert entries - {"fx3d_knn_ws"} <= refused, sorted(entries - refused)
    assert all(s in (tw.INVALID, tw.WORKSPACE) for c in tw.CASES for s in c.refuse.values())
    # two shapes per entry point
    for e in entries:
        assert sum(e in c.entries for c in tw.CASES) >= 2, e
    assert len({c.name for c in tw.CASES}) == len(tw.CASES)
    for cited in tw.CITED.values():
        path, name = cited.split("::")
        with open(os.path.join(ROOT, path)) as fh:
            assert f"def {name}(" in fh.read(), cited


def test_no_case_is_skipped_or_expected_to_fail():
    import abi_families
    import test_gpu_workspace as tw
    for mod in (tw, abi_families):
        with open(mod.__file__) as fh:
            text = fh.read()
        for word in ("pytest.skip", "mark.skip", "xfail", "importorskip"):
            assert word not in text, (mod.__name__, word)
        for obj in vars(mod).values():
            marks = getattr(obj, "pytestmark", [])
            assert all(m.name in ("gpu", "parametrize") for m in marks), obj
    for case in tw.CASES + tw.REFUSAL_ONLY:
        assert isinstance(case, tw.Case) and not hasattr(case, "marks")
