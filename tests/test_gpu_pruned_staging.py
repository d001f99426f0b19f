"""GPU parity of the pruned launch's image STAGING (nn1_f16_kernel<.., PRUNE = true>, csrc/chamfer.hip "stage the fp16 split
image"): a wave converts four lane tiles per step and takes one of three paths -- all four tiles full (no per-row test), all
four behind the cloud (constant padding pieces), or the tested body for a ragged last tile.  The cases put the end of the
candidate cloud on every side of those switches, and drive the other forms of the pieces (signed zeros, far candidates, the
unsorted image).

Each case is tests/test_gpu_pruned.py's check: indices bit for bit against the oracle, the loss bit-identical from call to call,
with a second workspace and under nn1_prune = 0.  Shapes are the smallest that still take the pruned launch (the check asserts
it): B = 17 for clouds of equal size, B = 25 where N != M (at B = 17 .. 24 the plan gives one direction a single pass per block
and does not prune)."""
import numpy as np
import pytest

from test_gpu_pruned import _assert_pruned, _check_pruned, _f

pytestmark = pytest.mark.gpu

NQ = 4096
# candidate counts: a full last tile; one row short; 63 tiles + 1 row; + one DPP row of 16; + 17 (a row and one more)
COUNTS = [4096, 4095, 4033, 4048, 4049]


def _B(N, M):
    return 17 if N == M else 25


@pytest.mark.parametrize("N,M", [(NQ, NQ)] + [s for c in COUNTS[1:] for s in ((NQ, c), (c, NQ))])
def test_staging_full_and_ragged_last_tiles(gpu_fx, oracle, N, M):
    """4096, 4095, 4033, 4048 and 4049 candidates against 4096 queries, both ways round (either cloud of the pair is the short one)."""
    B = _B(N, M)
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(N * 3 + M)
    _check_pruned(gpu_fx, oracle, _f(rng.random((3, N, B))), _f(rng.random((3, M, B))))


@pytest.mark.parametrize("cnt", [4095, 4033, 4048, 4049])
def test_staging_ragged_last_tile_equal_clouds(gpu_fx, oracle, cnt):
    """Both directions ragged at once (B = 17: the smallest pruned batch)."""
    _assert_pruned(cnt, cnt, 17)
    rng = np.random.default_rng(cnt)
    _check_pruned(gpu_fx, oracle, _f(rng.random((3, cnt, 17))), _f(rng.random((3, cnt, 17))))


def test_staging_signed_zeros_and_mixed_signs(gpu_fx, oracle):
    """Clouds centred on the origin, a quarter of the coordinates exactly +0.0 or -0.0, one axis constant: the tile boxes' corners
    take both zeros and both signs through the plain minimum / maximum, the pieces' split halves both signs."""
    N = M = 4096
    B = 17
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(5)
    x, y = rng.random((3, N, B)) - 0.5, rng.random((3, M, B)) - 0.5
    for a, s in ((x, 1), (y, 2)):
        z = rng.random(a.shape)
        a[z < 0.125] = 0.0
        a[(z >= 0.125) & (z < 0.25)] = -0.0
        a[s] = -0.0 if s == 1 else 0.25      # a constant axis: -0.0 everywhere in x, 0.25 in y
    x, y = _f(x), _f(y)
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    _check_pruned(gpu_fx, oracle, x, y)


def test_staging_far_candidates(gpu_fx, oracle):
    """Five candidates 1e4 ... 1e7 out in each cloud: the robust range leaves them out of the filter (`has_far`: the pieces' other
    form, padded rows on the exact side list)."""
    N = M = 4096
    B = 17
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(6)
    x, y = rng.random((3, N, B)), rng.random((3, M, B))
    for a in (x, y):
        for k, r in enumerate((1e4, 1e5, 1e6, 1e7, -3e6)):
            a[k % 3, rng.integers(0, a.shape[1]), :] = r
    _check_pruned(gpu_fx, oracle, _f(x), _f(y))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_staging_unsorted_form(gpu_fx, oracle, bad):
    """One non-finite coordinate in one cloud of the batch: that cloud is not `sane`, its blocks stage the image where the cloud
    pass parked it (no sort, original indices from the row numbers)."""
    N = M = 4096
    B = 17
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(7)
    x, y = _f(rng.random((3, N, B))), _f(rng.random((3, M, B)))
    y[1, 1234, 3] = bad
    with np.errstate(all="ignore"):
        _check_pruned(gpu_fx, oracle, x, y)
