"""GPU parity of the pruned launch's PASS SET-UP (nn1_f16_kernel<.., PRUNE = true>, csrc/chamfer.hip): the per-query constants a
wave computes at the top of a pass -- the power-of-two scale sq of a query far outside the candidate cloud and its exact
reciprocal, the far-query band da_far with its hardware square root, the wave's cut-off radius taken as a maximum on integer
keys -- and the query cloud requested at the kernel's entry instead of behind the cloud pass.

Each case is tests/test_gpu_pruned.py's check: indices bit for bit against the oracle, the loss bit-identical from call to call,
with a second workspace and under nn1_prune = 0.  Shapes are the smallest that take the pruned launch (the check asserts it):
B = 17 at N = M = 4096, B = 25 where N != M.

No pruned shape has a query cloud of more than 4096 = 4 x 1024 points (a pruned launch holds either cloud in one chunk of at
most 4096 candidates, and each cloud is the other direction's candidates), so the entry loads are never issued and left unused
for lack of room in the sort: test_no_pruned_shape_has_a_cloud_above_4096_points pins that."""
import numpy as np
import pytest

from test_gpu_pruned import _assert_pruned, _check_pruned, _f, _ws_bytes

pytestmark = pytest.mark.gpu

N = M = 4096
B = 17


def _both_ways(fx, oracle, x, y):
    _check_pruned(fx, oracle, x, y)
    _check_pruned(fx, oracle, y, x)


def _unit_directions(rng, n):
    d = rng.standard_normal((3, n))
    return d / np.abs(d).sum(axis=0, keepdims=True)     # |d|_1 = 1


# ------------------------------------------------------------------------------ the far-query scale and its reciprocal, da_far
@pytest.mark.parametrize("factor", [300.0, 3.0e4])
def test_setup_scaled_copy_of_the_cloud(gpu_fx, oracle, factor):
    """One cloud in the unit cube, the other the same cloud times 300 (every query of the big cloud gets a scale of its own) and
    times 3e4 (... and the small cloud sinks below the big one's resolution), either as the queries."""
    _assert_pruned(N, M, B)
    x = np.random.default_rng(int(factor)).random((3, N, B))
    _both_ways(gpu_fx, oracle, _f(x), _f(x * factor))


def test_setup_queries_on_a_ray_through_many_binades(gpu_fx, oracle):
    """64 queries on a ray from the cloud's centre at radii 300 x 2^j, j = 0 ... 10: sq runs through eleven powers of two."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(11)
    x, y = rng.random((3, N, B)), rng.random((3, M, B))
    d = _unit_directions(rng, B)                                      # one ray per pair
    r = 300.0 * 2.0 ** (np.arange(64) % 11)
    x[:, 7:7 + 64, :] = 0.5 + d[:, None, :] * r[None, :, None]
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


def test_setup_queries_on_both_sides_of_the_scale_switch(gpu_fx, oracle):
    """S = 2 sc |q - mu|_1 >= 3e4 switches the query's own scale on.  A unit cube's image scale sc is 128 (or 64, by the binade of its
    largest deviation from the mean): the switch lies at |q - mu|_1 = 117 (234).  512 queries step through 100 ... 260."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(12)
    x, y = rng.random((3, N, B)), rng.random((3, M, B))
    l1 = np.linspace(100.0, 260.0, 512)
    for b in range(B):
        x[:, 1000:1512, b] = 0.5 + _unit_directions(rng, 512) * l1[None, :]
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


# ------------------------------------------------------------------------------ degenerate roots
def test_setup_queries_at_the_candidates_mean(gpu_fx, oracle):
    """Candidates h and -h on a 2^-10 lattice: every partial sum is exact, the mean is exactly 0.  64 queries sit on it (qn = 0: the
    root of zero) and on one another."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(13)
    h = rng.integers(-1024, 1025, (3, M // 2, B)) / 1024.0
    y = np.concatenate([h, -h], 1)[:, rng.permutation(M), :]
    x = rng.random((3, N, B)) * 2.0 - 1.0
    x[:, 100:164, :] = 0.0
    _both_ways(gpu_fx, oracle, _f(x), _f(y))


@pytest.mark.parametrize("scale", [1.0e-30, 1.0e-20])
def test_setup_tiny_coordinates(gpu_fx, oracle, scale):
    """Coordinates of order 1e-30 (the `rng > 1e-30f` gate leaves the image unscaled: every product underflows) and 1e-20 (the
    scale is live, the products and the root's argument are tiny)."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(14)
    x, y = _f(rng.random((3, N, B)) * scale), _f(rng.random((3, M, B)) * scale)
    _both_ways(gpu_fx, oracle, x, y)


# ------------------------------------------------------------------------------ non-finite and huge queries
def test_setup_nonfinite_and_huge_queries(gpu_fx, oracle):
    """One +Inf, one NaN and one 1e30 coordinate in the query cloud of one pair: their waves' cut-off is NaN or +Inf and keeps every
    lane tile."""
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(15)
    x, y = _f(rng.random((3, N, B))), _f(rng.random((3, M, B)))
    x[0, 5, 3] = np.inf
    x[1, 700, 3] = np.nan
    x[2, 2000, 3] = 1.0e30
    with np.errstate(all="ignore"):
        _check_pruned(gpu_fx, oracle, x, y)


# ------------------------------------------------------------------------------ the query cloud requested at entry
@pytest.mark.parametrize("NQ,B2", [(4095, 25), (4033, 25), (3841, 28)])
def test_setup_entry_loads_ragged_query_cloud(gpu_fx, oracle, NQ, B2):
    """A query cloud that ends inside the entry loads of its last wave (one row short; one row into the wave's last sweep of 64; one
    row into its first, three sweeps wholly past the end): the clamped rows are loaded and not counted.  B is the smallest batch at
    which the shape takes the pruned launch: 25 down to 3969 x 4096, 28 at 3841 x 4096 (B = 25 ... 27 give the short cloud one pass)."""
    _assert_pruned(NQ, 4096, B2)
    rng = np.random.default_rng(NQ)
    _check_pruned(gpu_fx, oracle, _f(rng.random((3, NQ, B2))), _f(rng.random((3, 4096, B2))))


def test_no_pruned_shape_has_a_cloud_above_4096_points(fx):
    assert not any(_ws_bytes(n, m, 32, 1) > _ws_bytes(n, m, 32, 0) for n, m in ((4097, 4096), (4096, 4097), (5000, 4096), (8192, 8192)))
