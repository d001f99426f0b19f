"""GPU parity of the pruned nearest-neighbour block's entry (nn1_f16_kernel<.., PRUNE = true>, csrc/chamfer.hip): everything in
front of a block's first MFMA -- the cloud pass and its statistics, the query cloud's key box, the candidates' rows on their way
from the cloud pass to the sort's placement (or, for a cloud that is not sorted, to the staging), the window's slots -- and the box
of a wave's 32 queries, which the wave reduces itself at the top of its pass from the queries it has just loaded.  The cases were
written with the five steps of profiles/nn1_entry_ab.txt; the box in the wave is the one that is kept, the others' cases stay as
guards of the paths they aim at.

A wrong box can only cost time, so what is checked is what such steps could break: rows that reach the image from the wrong place,
a window slot read from where nothing wrote it, a box that drops a tile it needed.  Shapes: the smallest pruned ones,
(1087, 1025, 128) and its transpose -- one block per cloud and direction, windows of 1087 and 1025 queries (no multiple of 32, a
folded remainder of 63 and of one query), 1025 candidates leave most threads without a row in the second sweep -- and one
eight-pass shape on the other side of the window's switch.  Every case checks that its shape still prunes; indices are the oracle's
brute force bit for bit, loss bits those of nn1_prune = 0, both identical over two calls and a second workspace (_check_pruned of
tests/test_gpu_pruned.py)."""
import numpy as np
import pytest

from test_gpu_pruned import _assert_pruned, _bits, _check_pruned, _data, _f, _fwd, _lib, _oracle_nn

pytestmark = pytest.mark.gpu

SMALL = [(1087, 1025, 128), (1025, 1087, 128)]
EIGHT_PASSES = (4096, 1024, 128)


def _fill(fx, ws, poff, nscr, pattern):
    st = fx.current_stream().handle
    if isinstance(pattern, int):
        _lib().call("fx3d_memset", ws.ptr + poff, pattern, nscr, st)
    else:
        _lib().call("fx3d_memcpy_h2d", ws.ptr + poff, pattern.ctypes.data, nscr, st)


def _last_wave_rows(n):
    """Rows of a cloud's last, ragged 256-point share (the sort's wave w holds rows 256 w .. 256 w + 255)."""
    return np.arange(256 * ((n - 1) // 256), n)


# ------------------------------------------------------------------------------ rows in registers
@pytest.mark.parametrize("N,M,B", SMALL)
def test_entry_rows_sorted_and_unsorted_blocks_in_one_launch(gpu_fx, oracle, N, M, B):
    """One NaN candidate in a third of the clouds, one +-Inf candidate in another third: those blocks are not sorted and stage
    the rows where the cloud pass parked them, the others stage what the sort placed."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(N + 11)
    x, y = rng.random((3, N, B)), rng.random((3, M, B))
    for b in range(B):
        if b % 3 == 0:
            y[b % 3, rng.integers(M), b] = np.nan
        elif b % 3 == 1:
            y[rng.integers(3), rng.integers(M), b] = np.inf if b % 2 else -np.inf
    with np.errstate(all="ignore"):
        _check_pruned(gpu_fx, oracle, _f(x), _f(y))


@pytest.mark.parametrize("N,M,B", SMALL)
def test_entry_rows_robust_range_reads_parked_rows(gpu_fx, oracle, N, M, B):
    """One candidate 1e5 extents away per cloud: the robust range runs on parked rows, the point goes to the far list, the bulk
    is sorted."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(M + 12)
    x, y = rng.random((3, N, B)), rng.random((3, M, B))
    for b in range(B):
        y[:, rng.integers(M), b] = 1e5 * (1.0 + rng.random(3))
        if b % 2:
            x[:, rng.integers(N), b] = -1e5 * (1.0 + rng.random(3))
    _check_pruned(gpu_fx, oracle, _f(x), _f(y))


# ------------------------------------------------------------------------------ the query cloud's key box
def _extremes_at(rng, n, B, rows):
    """A bulk in [0.25, 0.75]^3 whose extreme coordinates 0 and 1 lie only in `rows` (one row holds a corner of the box)."""
    p = 0.25 + 0.5 * rng.random((3, n, B))
    corners = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    for k, r in enumerate(rows[:8]):
        p[:, r, :] = corners[k % 4][:, None]
    return p


@pytest.mark.parametrize("where", ["first_wave", "last_ragged_wave"])
@pytest.mark.parametrize("N,M,B", SMALL)
def test_entry_key_box_extremes_in_one_wave(gpu_fx, oracle, where, N, M, B):
    """The query cloud's box rests on rows of the first wave alone (which takes its box behind its cross-wave reduction) or of the last,
    ragged wave alone (1087: 63 rows; 1025: one row, a corner of the box)."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(N + len(where))
    rows = (lambda n: rng.permutation(256)) if where == "first_wave" else (lambda n: _last_wave_rows(n)[::-1])
    _check_pruned(gpu_fx, oracle, _f(_extremes_at(rng, N, B, rows(N))), _f(_extremes_at(rng, M, B, rows(M))))


@pytest.mark.parametrize("N,M,B", SMALL)
def test_entry_key_box_queries_outside_the_candidates(gpu_fx, oracle, N, M, B):
    """Disjoint clouds: every query lies outside the candidates' box, in both directions."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(N + 14)
    x, y = rng.random((3, N, B)), rng.random((3, M, B)) + np.array([3.0, -2.0, 1.5])[:, None, None]
    _check_pruned(gpu_fx, oracle, _f(x), _f(y))


# ------------------------------------------------------------------------------ the boxes of 32 queries
@pytest.mark.parametrize("N,M,B", SMALL)
def test_entry_group_box_nonfinite_queries(gpu_fx, oracle, N, M, B):
    """A NaN or an Inf query in the middle of a group, or as the window's LAST query -- the one the lanes past the window repeat:
    row N - 1 in the last cell of the curve (x at the top of the box, y and z at its bottom; a NaN coordinate sorts as the bottom).
    Their wave keeps every tile.  The clouds with such a point are not sorted as candidates: their windows are in index order."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(M + 15)
    x, y = rng.random((3, N, B)), rng.random((3, M, B))
    for b in range(B):
        if b % 4 == 0:
            x[rng.integers(3), N // 2 + 7, b] = np.nan
        elif b % 4 == 1:
            x[rng.integers(3), N // 3, b] = np.inf if b % 8 == 1 else -np.inf
        elif b % 4 == 2:
            x[:, N - 1, b] = (1.0, np.nan, 0.0)
        else:
            x[:, N - 1, b] = (np.inf, 0.0, 0.0)
    with np.errstate(all="ignore"):
        _check_pruned(gpu_fx, oracle, _f(x), _f(y))


@pytest.mark.parametrize("N,M,B", SMALL)
def test_entry_group_box_duplicated_queries(gpu_fx, oracle, N, M, B):
    """Every query four times, scattered over the cloud: groups of one point's copies have boxes without extent."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(N + 16)
    h = rng.random((3, (N + 3) // 4, B))
    x = np.concatenate([h] * 4, 1)[:, rng.permutation(4 * h.shape[1])[:N], :]
    _check_pruned(gpu_fx, oracle, _f(x), _f(rng.random((3, M, B))))


# ------------------------------------------------------------------------------ the window's slots
@pytest.mark.parametrize("N,M,B", [SMALL[0], EIGHT_PASSES])
def test_entry_window_slots_either_side_of_the_switch(gpu_fx, oracle, N, M, B):
    """A window of two passes + a remainder, and windows of eight passes."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(N + M + 17)
    _check_pruned(gpu_fx, oracle, _f(rng.standard_normal((3, N, B))), _f(rng.standard_normal((3, M, B))))


@pytest.mark.parametrize("N,M,B", SMALL)
def test_entry_window_slots_poisoned_workspace(gpu_fx, oracle, N, M, B):
    """The workspace's scratch -- the window's slots with it -- holds 0xFF bytes or indices of real points before the call."""
    fx = gpu_fx
    full, part = _assert_pruned(N, M, B)
    poff = (part + 255) & ~255
    rng = np.random.default_rng(N + 18)
    x, y = _f(rng.random((3, N, B))), _f(rng.random((3, M, B)))
    loss, ox, oy = _check_pruned(fx, oracle, x, y)
    dx, dy = fx.gpu(x), fx.gpu(y)
    ws = fx.DeviceArray.empty((full,), np.uint8)
    valid = rng.integers(0, min(N, M), (full - poff) // 2 + 1).astype(np.uint16)
    for pattern in (0xFF, valid):
        for _ in range(2):
            _fill(fx, ws, poff, full - poff, pattern)
            rc, loss2, ix2, iy2 = _fwd(fx, dx, dy, ws, full)
            assert rc == 0 and _bits(loss2) == _bits(loss)
            assert np.array_equal(ix2, ox) and np.array_equal(iy2, oy)


# ------------------------------------------------------------------------------ keys and floats
@pytest.mark.parametrize("N,M,B", SMALL)
def test_entry_signed_zeros_on_tile_boundaries(gpu_fx, oracle, N, M, B):
    """Coordinates of both signs on a lattice through the origin, zeros of either sign among them: a tile's box may end on +-0."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(N + 19)

    def cloud(n):
        p = rng.integers(-4, 5, (3, n, B)) * 0.25 + (rng.random((3, n, B)) < 0.3) * rng.standard_normal((3, n, B)) * 1e-3
        p[(p == 0.0) & (rng.random(p.shape) < 0.5)] = -0.0
        return p
    _check_pruned(gpu_fx, oracle, _f(cloud(N)), _f(cloud(M)))


@pytest.mark.parametrize("extent", [1e-20, 1e15])
@pytest.mark.parametrize("N,M,B", SMALL)
def test_entry_scale_gates_next_to_the_statistics(gpu_fx, oracle, extent, N, M, B):
    """Clouds of extent 1e-20 (no scale: every candidate is compared exactly) and 1e+15 (just inside the `sane` range)."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(N + 20)
    x, y = (rng.random((3, N, B)) - 0.5) * extent, (rng.random((3, M, B)) - 0.5) * extent
    _check_pruned(gpu_fx, oracle, _f(x), _f(y))
