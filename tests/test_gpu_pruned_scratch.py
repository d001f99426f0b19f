"""GPU parity of the pruned nearest-neighbour launch's scratch (nn1_f16_kernel<.., PRUNE = true>, csrc/chamfer.hip): a block keeps
its candidate cloud's image order and its window of the query cloud as 16-bit ORIGINAL INDICES in the workspace, and every reader
fetches the point from the input cloud by that index.  What can go wrong with that: a slot the launch did not write becomes an
address (stale workspace contents, the slots between a cloud's size and its padded size), a gathered point that is not the
row the image held (ties, duplicates), the identity order of clouds that are not sorted, the far candidates' side list.

Shapes: the smallest pruned ones, (1087, 1025, 128) and its transpose -- point counts that are no multiple of 4, 32 or 64, N != M,
one direction with a folded remainder --, and one 4096-point pair where the case is about reusing a workspace.  Each case checks
that its shape takes the pruned launch; indices are the oracle's brute force bit for bit, loss bits those of nn1_prune = 0
(_check_pruned of tests/test_gpu_pruned.py)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_pruned import _assert_pruned, _bits, _check_pruned, _data, _f, _lib, _oracle_nn, _ws_bytes

pytestmark = pytest.mark.gpu

SMALL = [(1087, 1025, 128), (1025, 1087, 128)]


def _behind(fx, host):
    """The cloud batch at the front of a larger allocation (>= 1 MiB of zeros behind it): an index past the cloud reads a wrong
    point -- wrong bits -- instead of unmapped memory."""
    D, n, B = host.shape
    extra = (1 << 20) // (4 * D * n) + 1
    big = fx.DeviceArray.zeros((D, n, B + extra), np.float32)
    view = big.slab(0, B)
    view.copy_(host)
    return view


def _scratch_range(N, M, B):
    full, part = _assert_pruned(N, M, B)
    poff = (part + 255) & ~255
    return full, poff, full - poff


def _fill(fx, ws, poff, nscr, pattern):
    st = fx.current_stream().handle
    if isinstance(pattern, int):
        _lib().call("fx3d_memset", ws.ptr + poff, pattern, nscr, st)
    else:
        _lib().call("fx3d_memcpy_h2d", ws.ptr + poff, pattern.ctypes.data, nscr, st)


def _entries(fx, dx, dy, ws, nbytes):
    """The four entry points that prune, on the caller's workspace: loss bits, indices, gradients, sums."""
    lib = _lib().load()
    D, N, B = dx.shape
    M = dy.shape[1]
    st = fx.current_stream().handle
    out = {}
    for want_idx in (True, False):
        ix, iy = fx.DeviceArray.zeros((N, B), np.int32), fx.DeviceArray.zeros((M, B), np.int32)
        loss_dev, host = fx.DeviceArray.empty((1,), np.float32), C.c_float(0)
        rc = lib.fx3d_chamfer_fwd(dx.ptr, N, dy.ptr, M, B, D, 0.7, 1.3, loss_dev.ptr, C.byref(host), ix.ptr if want_idx else None,
                                  iy.ptr if want_idx else None, ws.ptr, nbytes, st)
        assert rc == 0, _lib().last_error()
        out["fwd_idx" if want_idx else "fwd"] = _bits(host.value)
        if want_idx:
            out["ix"], out["iy"] = ix.to_host(), iy.to_host()
    gx, gy = fx.DeviceArray.empty((D, N, B), np.float32), fx.DeviceArray.empty((D, M, B), np.float32)
    ix, iy = fx.DeviceArray.zeros((N, B), np.int32), fx.DeviceArray.zeros((M, B), np.int32)
    loss_dev, host = fx.DeviceArray.empty((1,), np.float32), C.c_float(0)
    rc = lib.fx3d_chamfer_fwd_bwd(dx.ptr, N, dy.ptr, M, B, D, 0.7, 1.3, 2.0, B, loss_dev.ptr, C.byref(host), gx.ptr, gy.ptr, ix.ptr, iy.ptr,
                                  ws.ptr, nbytes, st)
    assert rc == 0, _lib().last_error()
    out["fwd_bwd"] = _bits(host.value)
    out["bx"], out["by"], out["gx"], out["gy"] = ix.to_host(), iy.to_host(), gx.to_host(), gy.to_host()
    sums = fx.DeviceArray.zeros((2,), np.float64)
    rc = lib.fx3d_chamfer_sums(dx.ptr, N, dy.ptr, M, B, D, sums.ptr, None, None, ws.ptr, nbytes, st)
    assert rc == 0, _lib().last_error()
    out["sums"] = sums.to_host().view(np.uint64).tolist()
    return out


def _same(a, b, what):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _fwd_bwd_bytes(N, M, B):
    n = _ws_bytes(N, M, B, 1, "fx3d_chamfer_fwd_bwd_workspace_bytes")
    assert n > _ws_bytes(N, M, B, 0, "fx3d_chamfer_fwd_bwd_workspace_bytes")
    return n


@pytest.mark.parametrize("N,M,B", SMALL)
def test_scratch_ragged_everything_and_stale_contents(gpu_fx, oracle, N, M, B):
    """Ragged point counts, N != M; the scratch pre-filled with 0x00, 0xFF (index 65535: 770 KB past a 1025-point cloud) and random
    VALID indices (a zero-distance match of a real point if a masked slot were used); every entry point gives the clean run's bits."""
    fx = gpu_fx
    full, poff, nscr = _scratch_range(N, M, B)
    nb = _fwd_bwd_bytes(N, M, B)
    rng = np.random.default_rng(N * 3 + M)
    x, y = _f(rng.random((3, N, B))), _f(rng.random((3, M, B)))
    loss, ox, oy = _check_pruned(fx, oracle, x, y)
    dx, dy = _behind(fx, x), _behind(fx, y)
    clean = _entries(fx, dx, dy, fx.DeviceArray.zeros((nb,), np.uint8), nb)
    assert clean["fwd_idx"] == clean["fwd"] == _bits(loss)
    assert np.array_equal(clean["ix"], ox) and np.array_equal(clean["iy"], oy)
    assert np.array_equal(clean["bx"], ox) and np.array_equal(clean["by"], oy)
    ogx, ogy = oracle.chamfer_bwd(x, y, ox, oy, 0.7, 1.3, 2.0)
    assert np.array_equal(clean["gx"], ogx) and np.array_equal(clean["gy"], ogy)
    ws = fx.DeviceArray.empty((nb,), np.uint8)
    valid = rng.integers(0, min(N, M), nscr // 2 + 1).astype(np.uint16)
    for pattern in (0x00, 0xFF, valid):
        for entry_pass in range(2):   # (the second pass runs on what the first left behind)
            if entry_pass == 0:
                _fill(fx, ws, poff, nscr, pattern)
            _same(clean, _entries(fx, dx, dy, ws, nb), pattern if isinstance(pattern, int) else "valid indices")


def test_scratch_workspace_reuse_large_then_small(gpu_fx, oracle):
    """A 4096-point pair, then a 1087 / 1025-point pair in the same workspace -- the large pair's indices, all above the small
    clouds' sizes, lie in the small launch's masked slots --, then the large pair again: each as with a fresh workspace."""
    fx = gpu_fx
    big, small = (4096, 4096, 17), SMALL[0]
    nb = max(_fwd_bwd_bytes(*big), _fwd_bwd_bytes(*small))
    _assert_pruned(*big), _assert_pruned(*small)
    rng = np.random.default_rng(17)
    pairs, fresh = [], []
    for N, M, B in (big, small):
        x, y = _f(rng.random((3, N, B))), _f(rng.random((3, M, B)))
        ox, oy = _oracle_nn(oracle, x, y)
        dx, dy = _behind(fx, x), _behind(fx, y)
        pairs.append((dx, dy))
        ref = _entries(fx, dx, dy, fx.DeviceArray.zeros((nb,), np.uint8), nb)
        assert np.array_equal(ref["ix"], ox) and np.array_equal(ref["iy"], oy)
        with _lib().option("nn1_prune", 0):
            assert _bits(fx.chamfer_distance(dx, dy, w1=0.7, w2=1.3)) == ref["fwd"]
        fresh.append(ref)
    ws = fx.DeviceArray.zeros((nb,), np.uint8)
    for k in (0, 1, 0, 1):
        _same(fresh[k], _entries(fx, *pairs[k], ws, nb), ("reuse", k))


@pytest.mark.parametrize("N,M,B", SMALL)
@pytest.mark.parametrize("layout", ["consecutive", "scattered"])
def test_scratch_tie_break_through_the_gather(gpu_fx, oracle, layout, N, M, B):
    """Every point four times, as consecutive copies or scattered over the cloud: the image order separates the copies' positions
    from their original indices, and the lowest ORIGINAL index must win every tie (queries = candidates included)."""
    rng = np.random.default_rng(M + len(layout))

    def four(n):
        h = rng.random((3, (n + 3) // 4, B))
        c = np.repeat(h, 4, axis=1) if layout == "consecutive" else np.concatenate([h] * 4, 1)[:, rng.permutation(4 * h.shape[1]), :]
        return _f(c[:, :n, :])
    x, y = four(N), four(M)
    _check_pruned(gpu_fx, oracle, x, y)
    if N > M:
        _check_pruned(gpu_fx, oracle, y, y)


@pytest.mark.parametrize("N,M,B", SMALL)
def test_scratch_identity_order(gpu_fx, oracle, N, M, B):
    """One non-finite point per cloud: neither is `sane`, nothing is sorted, the slots hold the identity."""
    rng = np.random.default_rng(N)
    x, y = rng.random((3, N, B)), rng.random((3, M, B))
    x[1, N - 1, :] = np.nan
    y[0, M // 2, :] = np.inf
    with np.errstate(all="ignore"):
        _check_pruned(gpu_fx, oracle, _f(x), _f(y))


@pytest.mark.parametrize("N,M,B", SMALL)
@pytest.mark.parametrize("kind", ["far_candidates", "far_queries", "extent_3e4_off"])
def test_scratch_outliers(gpu_fx, oracle, kind, N, M, B):
    """Far candidates (the side list reads its points through the slots), far queries and clouds of very different extent (a scale
    per query): the inputs of tests/test_gpu_pruned.py's kinds at the ragged shapes."""
    x, y = _data(kind, N, M, B, N + len(kind))
    _check_pruned(gpu_fx, oracle, x, y)
