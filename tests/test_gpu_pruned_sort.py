"""GPU parity of the pruned launch's SORT (nn1_f16_kernel<.., PRUNE = true>, csrc/chamfer.hip): the query cloud's key box, taken
between the cloud pass's two barriers from the rows requested at the kernel's entry; the 8 x 8 x 8 cells of both clouds; the
crowded-cell test, made once per thread and cloud for its four points; and the far query's own scale behind a wave-uniform branch
in the pass set-up.

Each case is tests/test_gpu_pruned.py's check: indices bit for bit against the oracle, the loss bit-identical from call to call,
with a second workspace and under nn1_prune = 0 -- with either cloud as the queries (the check runs both directions of a pair;
_both_ways also swaps the pair, which swaps the blocks the directions run in).  Shapes are the smallest that take the pruned launch
(the check asserts it): B = 17 at N = M = 4096, B = 25 / 28 where N != M.  The pairs of a batch are independent clouds, so one
call carries several variants of a case in different batch elements."""
import numpy as np
import pytest

from test_gpu_pruned import _assert_pruned, _check_pruned, _f

pytestmark = pytest.mark.gpu

N = M = 4096
B = 17


def _both_ways(fx, oracle, x, y):
    with np.errstate(all="ignore"):
        _check_pruned(fx, oracle, x, y)
        _check_pruned(fx, oracle, y, x)


def _uniform(seed, n=N, m=M, b=B):
    rng = np.random.default_rng(seed)
    return rng, rng.random((3, n, b)), rng.random((3, m, b))


# ------------------------------------------------------------------------------ the query cloud's key box, taken early
@pytest.mark.parametrize("NQ,B2", [(4095, 25), (4033, 25), (3841, 28)])
def test_box_ragged_query_cloud(gpu_fx, oracle, NQ, B2):
    """A query cloud that ends inside the entry loads of its last wave: the rows past it are loaded (clamped) and must not enter the
    box.  The cloud's last point sits alone far outside the others in every pair, so the clamped rows repeat the box's corner."""
    _assert_pruned(NQ, 4096, B2)
    rng, x, y = _uniform(NQ, NQ, 4096, B2)
    x[:, NQ - 1, :] = np.array([1.5, -0.5, 2.0])[:, None]
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


def test_box_nonfinite_and_huge_queries(gpu_fx, oracle):
    """One NaN, one +Inf and one 1e30 coordinate among the queries, each in a pair of its own and all three in a fourth: the NaN's key
    lies beyond the infinities' and enters the box as before (the frame drops a NaN bound, and is one cell where it is not finite)."""
    _assert_pruned(N, M, B)
    rng, x, y = _uniform(21)
    x, y = _f(x), _f(y)
    x[1, 700, 3] = np.nan
    x[0, 5, 5] = np.inf
    x[2, 2000, 7] = 1.0e30
    x[1, 4095, 9], x[0, 64, 9], x[2, 1023, 9] = np.nan, np.inf, 1.0e30
    x[0, 300, 11] = -np.inf
    _both_ways(gpu_fx, oracle, x, y)


def test_box_query_cloud_is_one_repeated_point(gpu_fx, oracle):
    """A cloud that is one point, 4096 times (no extent: one cell; every lane of every counting instruction in it), inside the other
    cloud's box, on its border and outside it."""
    _assert_pruned(N, M, B)
    rng, x, y = _uniform(22)
    for b in range(B):
        x[:, :, b] = np.array([[0.25, 0.5, 0.75], [0.0, 1.0, 0.5], [3.0, -2.0, 0.5]][b % 3])[:, None]
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


def test_box_query_cloud_wider_than_four_candidate_extents(gpu_fx, oracle):
    """Query clouds 3.9, 4.1, 10 and 100 times the candidates' extent about the same centre, in one dimension or in all: beyond four
    times the frame grows by a quarter of the candidates' extent only."""
    _assert_pruned(N, M, B)
    rng, x, y = _uniform(23)
    for b in range(B):
        r = (3.9, 4.1, 10.0, 100.0)[b % 4]
        if b % 8 < 4:
            x[:, :, b] = (x[:, :, b] - 0.5) * r + 0.5
        else:
            x[b % 3, :, b] = (x[b % 3, :, b] - 0.5) * r + 0.5
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


# ------------------------------------------------------------------------------ cells
def test_cells_lattice_of_the_box(gpu_fx, oracle):
    """Both clouds on the lattice k / 8 of their box, k = 0 ... 8 (the unit box, and a box of another origin and a power-of-two size):
    the fma lands exactly on the integers, and 8 clamps to 7."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(31)
    x = rng.integers(0, 9, (3, N, B)) / 8.0
    y = rng.integers(0, 9, (3, M, B)) / 8.0
    for c in (x, y):                      # (the box's corners are in every cloud)
        c[:, 0, :], c[:, 1, :] = 0.0, 1.0
    y[:, :, 1::2] = y[:, :, 1::2] * 4.0 - 2.0
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


def test_cells_negative_zero_coordinates(gpu_fx, oracle):
    """Clouds in [-1, 1] with a third of the coordinates exactly -0.0 and a tenth +0.0; in every other pair -0.0 is the box's upper
    corner."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(32)
    x, y = _f(rng.random((3, N, B)) * 2.0 - 1.0), _f(rng.random((3, M, B)) * 2.0 - 1.0)
    for c in (x, y):
        c[:, :, 1::2] = -np.abs(c[:, :, 1::2])
        u = rng.random(c.shape)
        c[u < 1.0 / 3.0] = -0.0
        c[u > 0.9] = 0.0
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    _both_ways(gpu_fx, oracle, x, y)


def test_cells_queries_outside_the_candidates_frame(gpu_fx, oracle):
    """Query clouds wholly outside the candidates' frame, beyond its grown copy (no frame of their own is left: one cell), and with
    one query inside it (the frame ends at the grown copy's border: all the others clamp into one corner cell)."""
    _assert_pruned(N, M, B)
    rng, x, y = _uniform(33)
    for b in range(B):
        sign = np.array([1.0, -1.0 if b & 1 else 1.0, -1.0 if b & 2 else 1.0])
        x[:, :, b] = 0.5 + sign[:, None] * (x[:, :, b] + 4.5)
        if b % 3 == 0:
            x[:, 77, b] = 0.5
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


# ------------------------------------------------------------------------------ the crowded-cell test, once for four points
def test_crowded_tight_cluster_beside_far_outliers(gpu_fx, oracle):
    """A tight cluster beside 40 far outliers, in either cloud and in both."""
    _assert_pruned(N, M, B)
    rng, x, y = _uniform(41)
    for b in range(B):
        for c, on in ((x, b % 3 != 1), (y, b % 3 != 0)):
            if on:
                c[:, :, b] = 0.3 + rng.standard_normal((3, c.shape[1])) * 1e-4
                c[:, rng.choice(c.shape[1], 40, replace=False), b] = rng.standard_normal((3, 40)) * 1e3
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


def test_crowded_runs_of_equal_points_in_a_uniform_cloud(gpu_fx, oracle):
    """Runs of exactly 3, 4, 7 and 8 equal points at consecutive indices inside uniform clouds (a pair has one length), aligned to the
    64-point sweeps and their 16-lane rows or straddling them, in sweeps of one thread's four points and of others: the joint test
    fires for some waves and not for others, and a wave where it fires takes crowded and plain instructions side by side."""
    _assert_pruned(N, M, B)
    rng, x, y = _uniform(42)
    for b in range(B):
        run = (3, 4, 7, 8)[b % 4]
        starts = (0, 16, 32) if (b // 4) % 2 == 0 else (13, 29, 61)
        for c in (x, y):
            for sweep in (2, 3, 20, 33, 40 + b):      # (candidates: thread t has the points t + 1024 e; queries: 256 wave + 64 e + lane)
                for s in starts:
                    p = 64 * sweep + s
                    c[:, p:p + run, b] = c[:, p:p + 1, b]
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


# ------------------------------------------------------------------------------ the far query's own scale, behind a branch
def _far(rng, n, radius):
    d = rng.standard_normal((3, n))
    return 0.5 + d / np.abs(d).sum(axis=0, keepdims=True) * radius


def test_scale_exactly_one_far_query(gpu_fx, oracle):
    """Exactly one query with a scale of its own in the cloud (|q - mu|_1 = 300 ... 3e4; the switch lies at 117 or 234): one lane of one
    wave-pass takes the branch."""
    _assert_pruned(N, M, B)
    rng, x, y = _uniform(51)
    for b in range(B):
        x[:, (97 * b + 5) % N, b] = _far(rng, 1, 300.0 * 10.0 ** (b % 3))[:, 0]
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


def test_scale_waves_of_far_queries(gpu_fx, oracle):
    """A clump of 64 far queries (consecutive in the sorted order: a wave whose 32 queries are all far, in one pass of a block and
    none in its other), and one of 600 (more than a pass of 512) -- in other pairs spread over all directions instead."""
    _assert_pruned(N, M, B)
    rng, x, y = _uniform(52)
    for b in range(B):
        n = 64 if b % 2 == 0 else 600
        at = rng.choice(N, n, replace=False)
        if b % 4 < 2:
            x[:, at, b] = np.array([300.0, 310.0, -290.0])[:, None] + rng.random((3, n))
        else:
            x[:, at, b] = _far(rng, n, 1000.0)
    _both_ways(gpu_fx, oracle, _f(x), _f(y))
