"""GPU parity of the pruned nearest-neighbour block's one-wave stretches (nn1_f16_kernel<.., PRUNE = true>, csrc/chamfer.hip): the
query cloud's key box, reduced by sixteen waves over their 64-query rows; the queries' grid frame, computed from it once per block
by three waves (a dimension each) and handed to all through LDS; the one-wave scans along the Hilbert curve.  (The cases were
written for four steps of which the frame is the one kept -- DESIGN.md 3.1, "One-wave stretches"; the box cases are aimed at a
split of the first wave's four rows among other waves, the scan cases at a scan on the DPP path: they hold any such change
to the same slots.)

A wrong key box or frame still gives the right neighbours -- it only reorders the block's window of the query cloud -- so beside
_check_pruned of tests/test_gpu_pruned.py (indices the oracle's brute force, loss bits those of nn1_prune = 0, both stable from
call to call and over a second workspace) the cases read the window's slots back from the workspace (the 16-bit original indices
behind a block's kHScrCand candidate slots) and hold them to a numpy restatement of the queries' order: the cell along
hilbert_cells() of tools/nn1_prune_model.py, then the index.  Coordinates are multiples of 1/64 and every frame spans a power of
two, so each frame expression is exact in Float32 and the restatement needs no fused multiply-add; the restatement itself is
checked against curve_order() of the model on the CPU.

The slots are compared wherever the CANDIDATE cloud of a direction is a plain box-filling one (its grid frame is its bounding
box: no far outliers, no robust range); the aimed clouds are the queries of direction x -> y.

Shapes: the smallest pruned ones, (1087, 1025, 128) and its transpose (waves 5 .. 15 hold no query, the ragged last wave 63 rows or
one row), and (1024, 513, 128): no pruned shape has a query cloud of at most 256 points -- a block needs two passes of 512 queries
in both directions, test_smallest_pruned_query_cloud -- and 513 is the smallest that prunes (waves 3 .. 15 hold nothing, wave 2 one
query).  One batch element per variant of a case (b mod the number of variants): a case is one call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_pruned import _assert_pruned, _check_pruned, _f, _lib

sys.path.insert(0, os.path.join(ROOT, "tools"))
from nn1_prune_model import curve_order, hilbert_cells  # noqa: E402

gpu = pytest.mark.gpu

K_SCR_CAND = 4096 + 64   # kHScrCand of csrc/nn1_common.h: candidate slots in front of a block's window
SHAPES = [(1087, 1025, 128), (1025, 1087, 128), (1024, 513, 128)]
F32 = np.float32


# ------------------------------------------------------------------------------ the queries' order, restated
def _query_order(q, c):
    """Order of the queries q (n, 3) of a block whose candidates c (m, 3) fill their bounding box (grid frame = box): chamfer.hip's
    frame expressions in Float32 -- every one exact on the dyadic inputs of this file, which is asserted --, the cell along the
    curve, then the index."""
    q, c = np.asarray(q, F32), np.asarray(c, F32)
    cfl, cfh = c.min(0), c.max(0)
    ext = F32(np.max(cfh - cfl))
    with np.errstate(all="ignore"):
        ql, qh = np.fmin.reduce(q, 0), np.fmax.reduce(q, 0)     # (the key box: NaNs are not in this file's slot cases)
        grow = np.where(qh - ql > F32(4) * ext, F32(0.25) * ext, ext).astype(F32)
        lo, hi = np.fmax(ql, cfl - grow), np.fmin(qh, cfh + grow)
        ok = (hi > lo) & (hi - lo < np.inf)
        qinv = np.where(ok, F32(8) / np.where(ok, hi - lo, F32(1)), F32(0)).astype(F32)
        qoff = np.where(qinv != 0, -lo * qinv, F32(0)).astype(F32)
        t64 = q.astype(np.float64) * qinv.astype(np.float64) + qoff.astype(np.float64)
    t = t64.astype(F32)
    assert np.array_equal(t.astype(np.float64), t64), "the frame is not exact in Float32: not a case for this restatement"
    assert np.array_equal((F32(8) / np.where(ok, hi - lo, F32(1))).astype(np.float64), 8.0 / np.where(ok, hi - lo, 1).astype(np.float64))
    u = np.clip(t, 0, 7).astype(np.int64)
    cell = u[:, 0] | (u[:, 1] << 3) | (u[:, 2] << 6)
    pos = np.empty(512, np.int64)
    pos[hilbert_cells()] = np.arange(512)
    return np.argsort(pos[cell], kind="stable")


def _dyadic(rng, n, lo, hi):
    """n points on the 1/64 grid in the box [lo, hi] (per dimension), its corners lo and hi among them at random indices."""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (3,)), np.broadcast_to(np.asarray(hi, np.float64), (3,))
    p = np.stack([rng.integers(int(lo[d] * 64), int(hi[d] * 64) + 1, n) / 64.0 for d in range(3)], 1)
    i, j = rng.choice(n, 2, replace=False)
    p[i], p[j] = lo, hi
    return p


def test_restatement_against_the_model():
    """Queries inside the candidates' grown frame are ordered in their own box: curve_order() of tools/nn1_prune_model.py."""
    rng = np.random.default_rng(1)
    c = _dyadic(rng, 1025, 0.0, 8.0)
    for lo, hi in ((0.0, 8.0), (2.0, 6.0), (-4.0, 4.0), ((8.0, 0.0, -8.0), (16.0, 4.0, 8.0))):
        q = _dyadic(rng, 1087, lo, hi)
        assert np.array_equal(_query_order(q, c), curve_order(q))
    one = np.tile(np.array([[3.0, 1.0, 2.0]]), (600, 1))         # no extent: one cell, index order
    assert np.array_equal(_query_order(one, c), np.arange(600))


def test_smallest_pruned_query_cloud(fx):
    """No query cloud of 512 points or fewer takes the pruned launch (so none of at most 256 does); 513 is the smallest."""
    n = C.c_size_t(0)

    def pruned(N, M, B):
        sizes = []
        for prune in (1, 0):
            with _lib().option("nn1_prune", prune):
                _lib().call("fx3d_chamfer_workspace_bytes", N, M, B, 3, C.byref(n))
            sizes.append(n.value)
        return sizes[0] > sizes[1]
    for big in (1024, 2048, 4096):
        for B in (128, 512):
            assert not any(pruned(big, m, B) for m in (64, 128, 255, 256, 257, 400, 511, 512))
    assert pruned(1024, 513, 128)


# ------------------------------------------------------------------------------ the window's slots, read back
def _plan(N, M, B):
    buf = C.create_string_buffer(512)
    _lib().call("fx3d_nn1_plan_describe", N, M, B, 3, buf, 512)
    return {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (f.split("=") for f in buf.value.decode().split())}


def _windows(fx, dx, dy, loss_bits):
    """One more call on a workspace of this test's: {(direction, cloud): the cloud's window slots, tile after tile}."""
    from test_gpu_pruned import _bits, _fwd
    D, N, B = dx.shape
    M = dy.shape[1]
    full, part = _assert_pruned(N, M, B)
    poff = (part + 255) & ~255
    pl = _plan(N, M, B)
    assert pl["nsplit"] == 1 and 2 * B >= 8 and 2 * B % 8 == 0
    stride = (full - poff) // 2 // pl["grid"]
    assert stride * pl["grid"] * 2 == full - poff and stride > K_SCR_CAND
    ws = fx.DeviceArray.zeros((full,), np.uint8)
    rc, loss, _, _ = _fwd(fx, dx, dy, ws, full)
    assert rc == 0 and _bits(loss) == loss_bits
    scr = ws.to_host()[poff:].view(np.uint16).reshape(pl["grid"], stride)
    per_cloud = max(pl["tiles_x"], pl["tiles_y"])
    out = {}
    for L in range(pl["grid"]):
        slot = L >> 3
        c, tile = (slot // per_cloud) * 8 + (L & 7), slot % per_cloud
        if c >= 2 * B:
            continue
        d, b = (1, c - B) if c >= B else (0, c)
        nq, tiles, tpb = (M, pl["tiles_y"], pl["tpb_y"]) if d else (N, pl["tiles_x"], pl["tpb"])
        if tile >= tiles:
            continue
        q0 = tile * tpb * 512
        q1 = nq if tile == tiles - 1 or q0 + tpb * 512 > nq else q0 + tpb * 512
        out.setdefault((d, b), []).append((q0, scr[L, K_SCR_CAND:K_SCR_CAND + q1 - q0].astype(np.int64)))
    return {k: np.concatenate([w for _, w in sorted(v, key=lambda t: t[0])]) for k, v in out.items()}


def _run(fx, oracle, name, x, y, slots_x=True, slots_y=False, identity_x=False):
    """_check_pruned, then the slots: direction x -> y (queries x) and / or y -> x against the restatement, or the identity."""
    from test_gpu_pruned import _bits
    x, y = _f(x), _f(y)
    with np.errstate(all="ignore"):
        loss, _, _ = _check_pruned(fx, oracle, x, y)
    print(f"LOSSBITS {name} {x.shape[1]}x{y.shape[1]}x{x.shape[2]} {_bits(loss)}")
    if not (slots_x or slots_y or identity_x):
        return
    win = _windows(fx, fx.gpu(x), fx.gpu(y), _bits(loss))
    B = x.shape[2]
    for b in range(B):
        qx, qy = x[:, :, b].T, y[:, :, b].T
        if identity_x:
            assert np.array_equal(win[(0, b)], np.arange(qx.shape[0])), (name, b)
        if slots_x:
            ref = _query_order(qx, qy)
            assert np.array_equal(win[(0, b)], ref), (name, "x -> y", b, np.argwhere(win[(0, b)] != ref)[:4].ravel())
        if slots_y:
            ref = _query_order(qy, qx)
            assert np.array_equal(win[(1, b)], ref), (name, "y -> x", b, np.argwhere(win[(1, b)] != ref)[:4].ravel())


def _batch(N, M, B, make):
    """(3, N, B), (3, M, B) from make(b) -> (x (N, 3), y (M, 3))."""
    xs, ys = zip(*(make(b) for b in range(B)))
    return np.stack(xs, 2).transpose(1, 0, 2), np.stack(ys, 2).transpose(1, 0, 2)


# ------------------------------------------------------------------------------ the key box: the first wave's rows
CORNER_ROWS = [(0, 64), (64, 128), (128, 192), (192, 256), (255, 256), (256, 257)]


def _corner_cloud(rng, n, v):
    """Box [0, 8]^3 whose bounds lie only in the index range CORNER_ROWS[v]: a 64-query row holds both corners beside a bulk in
    [1, 7]^3; a single index holds (0, 0, 8) -- the low bound of x and y, the high one of z -- and the bulk, in [4, 8] x [4, 8] x [0, 4]
    with its own corner (8, 8, 0) far behind, supplies the opposite bounds."""
    r0, r1 = CORNER_ROWS[v]
    if r1 - r0 > 1:
        p = np.stack([rng.integers(64, 7 * 64 + 1, n) / 64.0 for _ in range(3)], 1)
        i, j = r0 + rng.choice(r1 - r0, 2, replace=False)
        p[i], p[j] = 0.0, 8.0
        return p
    p = np.stack([4.0 + rng.integers(1, 256, n) / 64.0, 4.0 + rng.integers(1, 256, n) / 64.0, rng.integers(1, 256, n) / 64.0], 1)
    p[r0] = [0.0, 0.0, 8.0]
    p[n - 1 - rng.integers(0, 200)] = [8.0, 8.0, 0.0]
    return p


@gpu
@pytest.mark.parametrize("N,M,B", SHAPES)
def test_box_corners_in_one_row_of_the_first_wave(gpu_fx, oracle, N, M, B):
    """Both clouds, by batch element: the bounds of the box only in queries 0 .. 63, 64 .. 127, 128 .. 191, 192 .. 255 -- one 64-query row
    of the first wave each --, then only in query 255 (the first wave's last) and only in 256 (the second wave's first).  A row dropped from the box leaves
    the bulk's box as the frame: other cells, other slots.  (Waves past the cloud's end hold no query; the ragged last wave 63 rows or one.)"""
    def make(b):
        rng = np.random.default_rng(1000 * N + b)
        return _corner_cloud(rng, N, b % len(CORNER_ROWS)), _corner_cloud(rng, M, (b // len(CORNER_ROWS)) % len(CORNER_ROWS))
    x, y = _batch(N, M, B, make)
    _run(gpu_fx, oracle, "corner_rows", x, y, slots_x=True, slots_y=True)


# ------------------------------------------------------------------------------ the frame: both branches of `grow`, queries outside
@gpu
@pytest.mark.parametrize("N,M,B", SHAPES)
def test_frame_grow_branches_and_queries_outside(gpu_fx, oracle, N, M, B):
    """Candidates fill [0, 8] x [0, 4] x [0, 8] (largest extent 8).  Queries, by batch element: (0) all outside the candidates' box,
    in [8, 16] x [4, 8] x [-8, 0]; (1) x in [8, 16] outside and unclipped, y in [-32, 32] -- more than four times the extent:
    grown by a quarter, frame [-2, 6] --, z in [0, 16] clipped at the full growth to [0, 16]; (2) a box inside the candidates'."""
    boxes = [((8.0, 4.0, -8.0), (16.0, 8.0, 0.0)), ((8.0, -32.0, 0.0), (16.0, 32.0, 16.0)), ((2.0, 1.0, 2.0), (6.0, 3.0, 6.0))]

    def make(b):
        rng = np.random.default_rng(2000 * N + b)
        lo, hi = boxes[b % 3]
        return _dyadic(rng, N, lo, hi), _dyadic(rng, M, (0.0, 0.0, 0.0), (8.0, 4.0, 8.0))
    x, y = _batch(N, M, B, make)
    _run(gpu_fx, oracle, "grow", x, y, slots_x=True)


# ------------------------------------------------------------------------------ the scans along the curve
@gpu
@pytest.mark.parametrize("N,M,B", SHAPES)
@pytest.mark.parametrize("kind", ["one_cell", "every_cell", "last_cell"])
def test_curve_scan_carries(gpu_fx, oracle, kind, N, M, B):
    """one_cell: every query one point and every candidate another -- each scan's total sits in one lane; every_cell: point i in the
    cell at curve position i mod 512 -- every lane carries into the next; last_cell: all but the box's far corner in the curve's
    LAST cell (7, 0, 0) -- the total crosses every row of the wave.  The aimed cloud is x; in one_cell y as well (parity: a one-point
    candidate cloud has no extent, its queries' frame is their own box)."""
    cells = hilbert_cells()

    def aimed(rng, n, b):
        if kind == "one_cell":
            return np.tile(np.array([[3.0 + (b % 4), 1.5, 2.25]]), (n, 1))
        if kind == "every_cell":
            t = cells[(np.arange(n) + b) % 512]
            g = np.stack([t & 7, (t >> 3) & 7, t >> 6], 1).astype(np.float64)
            p = g + rng.integers(1, 64, (n, 3)) / 64.0
            p[(37 + b) % n], p[(300 + b) % n] = 0.0, 8.0
            return p
        p = np.stack([7.0 + rng.integers(1, 64, n) / 64.0, rng.integers(0, 64, n) / 64.0, rng.integers(0, 64, n) / 64.0], 1)
        p[(b * 7) % n] = [0.0, 8.0, 8.0]                       # the box's other bounds: cell (0, 7, 7)
        p[(b * 7 + 1) % n] = [8.0, 0.0, 0.0]
        return p

    def make(b):
        rng = np.random.default_rng(3000 * N + b)
        if kind == "one_cell":
            return aimed(rng, N, b), np.tile(np.array([[2.0, 6.5 - (b % 3), 4.0]]), (M, 1))
        return aimed(rng, N, b), _dyadic(rng, M, 0.0, 8.0)
    x, y = _batch(N, M, B, make)
    _run(gpu_fx, oracle, kind, x, y, slots_x=True, slots_y=kind == "one_cell")


# ------------------------------------------------------------------------------ parity only: non-finite queries; no sort
@gpu
@pytest.mark.parametrize("N,M,B", SHAPES)
def test_nonfinite_among_the_first_waves_queries(gpu_fx, oracle, N, M, B):
    """A NaN, a +Inf or a -Inf coordinate among queries 0 .. 255 of x (the first wave's rows), the candidates finite: the keys enter the box
    as before.  Parity only."""
    rng = np.random.default_rng(N + 7)
    x, y = rng.integers(0, 513, (3, N, B)) / 64.0, rng.integers(0, 513, (3, M, B)) / 64.0
    for b in range(B):
        x[b % 3, (b * 5) % 256, b] = (np.nan, np.inf, -np.inf)[(b // 3) % 3]
    _run(gpu_fx, oracle, "nonfinite_queries", x, y, slots_x=False)


@gpu
@pytest.mark.parametrize("N,M,B", SHAPES)
def test_unsorted_pair_reads_no_frame(gpu_fx, oracle, N, M, B):
    """A non-finite CANDIDATE (in y): direction x -> y is not sorted -- no frame is computed, stored or read, the window is the
    identity --, direction y -> x sorts its queries y with the non-finite one among them."""
    rng = np.random.default_rng(N + 11)
    x, y = rng.integers(0, 513, (3, N, B)) / 64.0, rng.integers(0, 513, (3, M, B)) / 64.0
    for b in range(B):
        y[b % 3, (b * 11) % M, b] = (np.inf, np.nan, -np.inf)[(b // 3) % 3]
    _run(gpu_fx, oracle, "unsorted", x, y, slots_x=False, identity_x=True)
