"""GPU parity of the two exact nearest-neighbour kernels that are not the default D = 3 path (csrc/nn1_exact.hip):

  * nn1_small_d_kernel<DIM, R, WANT_IDX>: every D = 2 cloud, and D = 3 under option nn1_variant = 0.  Candidates are staged
    through LDS in chunks of at most kChunkMax = 4096 (the last one padded with +Inf to a multiple of 32), tiles of 32 are
    folded by min3, the strict `<` between tiles keeps the first tile holding the minimum, the winning tile is re-scanned while
    its chunk is in LDS, R = 1, 2 or 4 queries per thread by the problem's total query count, a 1-D grid in slots of eight
    clouds (2B % 8 != 0 leaves empty slots), the non-fused chamfer_finalize_partials_kernel.
  * nn1_generic_kernel: D = 1 and D >= 4, one query per thread, 256-query tiles.

Every shape first checks, through fx3d_nn1_plan_describe, that it takes the plan it claims (kernel, R, tile counts, chunks per
direction), so that a planner change fails here instead of quietly testing another instantiation.

Each case: indices (in range) and distances bit for bit against the oracle's brute force, through fx3d_nn1 and through the
chamfer forward; the loss against the oracle; the loss-only instantiation and a second call give the same loss bits;
fx3d_chamfer_sums against the oracle's sums; fx3d_chamfer_fwd_bwd's gradients bit for bit against the oracle's adjoint at the
oracle's indices.  For D = 3 under nn1_variant = 0 the indices also equal those of the default path."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_hardening import LOSS_RTOL, _nonfinite_case
from test_gpu_pruned import _bits, _loss_close

pytestmark = pytest.mark.gpu

W1, W2, GOUT = 0.7, 1.3, 1.5

# (N, M, B) -> the exact loop's plan: R, LDS chunk, query tiles per direction, candidate chunks x -> y (M) and y -> x (N)
EXACT_SHAPES = {
    (1100, 40, 461): dict(R=4, chunk=1120, tiles_x=2, tiles_y=1, chunks=(1, 1)),     # 2B % 8 = 2; 40 candidates pad to 64
    (1100, 40, 240): dict(R=2, chunk=1120, tiles_x=3, tiles_y=1, chunks=(1, 1)),
    (32, 4097, 128): dict(R=4, chunk=4096, tiles_x=1, tiles_y=5, chunks=(2, 1)),     # a last chunk of one candidate
    (600, 9000, 56): dict(R=4, chunk=4096, tiles_x=1, tiles_y=9, chunks=(3, 1)),     # three chunks, rows r = 0 .. 2 in use
    (200, 8193, 61): dict(R=2, chunk=4096, tiles_x=1, tiles_y=17, chunks=(3, 1)),    # 2B % 8 = 2
    (300, 800, 257): dict(R=2, chunk=800, tiles_x=1, tiles_y=2, chunks=(1, 1)),      # 2B % 8 = 2
    (700, 1300, 3): dict(R=1, chunk=1312, tiles_x=3, tiles_y=6, chunks=(1, 1)),      # 2B < 8
    (4097, 300, 3): dict(R=1, chunk=4096, tiles_x=17, tiles_y=2, chunks=(1, 2)),
    (9000, 1000, 1): dict(R=1, chunk=4096, tiles_x=36, tiles_y=4, chunks=(1, 3)),    # B = 1; a last chunk of 808
    (1, 9000, 5): dict(R=1, chunk=4096, tiles_x=1, tiles_y=36, chunks=(3, 1)),       # one query x -> y, one candidate y -> x
}
# (N, M, B) -> 256-query tiles per direction
GENERIC_SHAPES = {
    (1, 257, 3): dict(tiles_x=1, tiles_y=2),
    (255, 256, 5): dict(tiles_x=1, tiles_y=1),
    (257, 3000, 2): dict(tiles_x=2, tiles_y=12),
    (3000, 255, 2): dict(tiles_x=12, tiles_y=1),
    (600, 257, 80): dict(tiles_x=3, tiles_y=2),     # 400 partials: the finalize kernel's strided loop, directions unequal
}
GENERIC_DIMS = [1, 4, 5, 8, 16, 64, 128]
HEAVY = {(600, 9000, 56), (200, 8193, 61)}          # > 100 M pair evaluations: a subset of the data

KINDS = ["uniform", "lattice", "planted", "pad_only", "identical", "offset", "outlier", "subnormal", "huge",
         "nan_candidate", "inf_same_coordinate", "all_nan_cloud", "overflowing_distances", "mixed_everything"]
HEAVY_KINDS = ["uniform", "lattice", "planted", "pad_only", "huge"]
LARGE_D_KINDS = ["uniform", "lattice", "planted", "identical", "offset", "huge", "nan_candidate", "mixed_everything"]
_NONFINITE = {"nan_candidate", "inf_same_coordinate", "all_nan_cloud", "overflowing_distances", "mixed_everything"}


def _lib():
    from flux3d_jl_amd import _lib
    return _lib


def plan_of(N, M, B, D):
    buf = C.create_string_buffer(256)
    _lib().call("fx3d_nn1_plan_describe", N, M, B, D, buf, 256)
    return dict(kv.split("=") for kv in buf.value.decode().split())


def assert_exact_plan(N, M, B, D):
    """The exact loop's plan for (N, M, B) at D = 2, or at D = 3 under nn1_variant = 0 (the caller sets the option)."""
    e = EXACT_SHAPES[(N, M, B)]
    p = plan_of(N, M, B, D)
    got = dict(kernel=p["kernel"], R=int(p["R"]), chunk=int(p["chunk"]), tiles_x=int(p["tiles_x"]), tiles_y=int(p["tiles_y"]))
    assert got == dict(kernel="small_d", **{k: v for k, v in e.items() if k != "chunks"}), (N, M, B, D, p)
    ch = int(p["chunk"])
    assert ((M + ch - 1) // ch, (N + ch - 1) // ch) == e["chunks"], (N, M, B, D, p)
    assert int(p["grid"]) == (2 * B + 7) // 8 * 8 * max(e["tiles_x"], e["tiles_y"]), p


def assert_generic_plan(N, M, B, D):
    e = GENERIC_SHAPES.get((N, M, B), dict(tiles_x=(N + 255) // 256, tiles_y=(M + 255) // 256))
    p = plan_of(N, M, B, D)
    assert p["kernel"] == "generic" and int(p["R"]) == 1, p
    assert (int(p["tiles_x"]), int(p["tiles_y"])) == (e["tiles_x"], e["tiles_y"]), (N, M, B, D, p)
    assert int(p["grid"]) == 2 * B * max(e["tiles_x"], e["tiles_y"]), p


# ------------------------------------------------------------------------------ data
def _f(a):
    return np.asfortranarray(np.asarray(a).astype(np.float32))


def _data(kind, D, N, M, B, seed):
    rng = np.random.default_rng(seed)
    x, y = rng.random((D, N, B)), rng.random((D, M, B))
    if kind == "lattice":                       # values k / 4: exact ties across lanes, tiles and chunks
        x, y = rng.integers(0, 4, (D, N, B)) * 0.25, rng.integers(0, 4, (D, M, B)) * 0.25
    elif kind == "planted":                     # copies of early points later on (the next chunk, or the cloud's end)
        for c, n in ((y, M), (x, N)):
            k = min(n // 2, 96)
            if k:
                c[:, n - k:, :] = c[:, :k, :]
            if n >= 4096 + 71:
                c[:, 4096 + 7:4096 + 71, :] = c[:, 100:164, :]
    elif kind == "pad_only":                    # the nearest candidate only among the last three (the padded last chunk)
        y += 50.0
        y[:, M - 3:, :] = rng.random((D, min(3, M), B))
        x[:, N - 2:, :] = 50.0 + rng.random((D, min(2, N), B))
    elif kind == "identical":                   # every candidate the same point: every index 0
        x[:] = 0.375
        y[:] = 0.625
    elif kind == "offset":                      # cancellation in q - c
        x, y = 1e4 + 1e-2 * x, 1e4 + 1e-2 * y
    elif kind == "outlier":
        x[:, N // 2, :] = 1e6
        y[:, M - 1, :] = -3e5
    elif kind == "subnormal":
        x, y = x * 1e-40, y * 1e-40
        y[:, ::7, :] = 0.0
    elif kind == "huge":                        # every distance overflows to +Inf: the isless scan of the whole cloud
        x, y = 2e38 + 1e38 * x, -(2e38 + 1e38 * y)
        y[0, min(3, M - 1), :] = np.nan
    elif kind in _NONFINITE:
        return _nonfinite_case(kind, N, M, B, seed, D=D)
    else:
        assert kind == "uniform", kind
    return _f(x), _f(y)


def _kinds(N, M, D=2):
    if (N, M) in {(s[0], s[1]) for s in HEAVY}:
        return HEAVY_KINDS
    if D >= 64 and max(N, M) >= 3000:
        return LARGE_D_KINDS
    # (_nonfinite_case writes at fixed indices up to 11)
    return [k for k in KINDS if k not in _NONFINITE or min(N, M) >= 12]


# ------------------------------------------------------------------------------ the oracle, batch slices on the host's cores
def _oracle(oracle, x, y, w1=W1, w2=W2):
    """(ix, iy, dx, dy, sums, loss): oracle.nn1's brute force with distances, run on contiguous batch slices in parallel; the
    sums [sum_i ||x_i - y_ix||^2, sum_j ||y_j - x_iy||^2] of Float32 squares in Float64 at those indices, as
    fx3d_oracle_chamfer_fwd forms them; the loss in the reference's own arithmetic (oracle.chamfer_loss_pairwise)."""
    D, N, B = x.shape
    nt = max(1, min(16, oracle.usable_cores(), B))
    cut = np.linspace(0, B, nt + 1).astype(int)
    with ThreadPoolExecutor(nt) as ex:
        parts = list(ex.map(lambda k: oracle.nn1(x[:, :, cut[k]:cut[k + 1]], y[:, :, cut[k]:cut[k + 1]], want_dist=True), range(nt)))
    ix, iy, dx, dy = (np.asfortranarray(np.concatenate([p[i] for p in parts], axis=1)) for i in range(4))
    b = np.arange(B)[None, :]
    with np.errstate(all="ignore"):
        sums = np.array([np.sum(((x - y[:, ix, b]) ** 2).astype(np.float64)), np.sum(((y - x[:, iy, b]) ** 2).astype(np.float64))])
        loss = oracle.chamfer_loss_pairwise(x, y, ix, iy, w1, w2)
    return ix, iy, dx, dy, sums, loss


def _same_bits(a, b):
    return _bits(a) == _bits(b) or (np.isnan(a) and np.isnan(b))


def _first_diff(a, b):
    return np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a != b))[:5]


def _check(fx, oracle, x, y):
    """Every assertion of the module on one (x, y); returns the nearest-neighbour indices."""
    from flux3d_jl_amd.distributed import chamfer_sums
    D, N, B = x.shape
    M = y.shape[1]
    ox, oy, odx, ody, osums, oloss = _oracle(oracle, x, y)
    dx, dy = fx.gpu(x), fx.gpu(y)

    ix, iy, ddx, ddy = fx.nearest_neighbors(dx, dy, return_dist=True)
    ix, iy = ix.to_host(), iy.to_host()
    assert ix.min() >= 0 and ix.max() < M and iy.min() >= 0 and iy.max() < N
    assert np.array_equal(ix, ox), _first_diff(ix, ox)
    assert np.array_equal(iy, oy), _first_diff(iy, oy)
    hdx, hdy = ddx.to_host(), ddy.to_host()
    assert np.array_equal(hdx, odx, equal_nan=True), _first_diff(hdx, odx)
    assert np.array_equal(hdy, ody, equal_nan=True), _first_diff(hdy, ody)

    loss, jx, jy = fx.chamfer_distance(dx, dy, w1=W1, w2=W2, return_indices=True)
    assert np.array_equal(jx.to_host(), ox) and np.array_equal(jy.to_host(), oy)
    _loss_close(loss, oloss, LOSS_RTOL)
    for _ in range(2):   # the loss-only instantiation (WANT_IDX = false), twice
        assert _same_bits(fx.chamfer_distance(dx, dy, w1=W1, w2=W2), loss)

    sums = chamfer_sums(dx, dy)
    for s, o in zip(sums, osums):
        _loss_close(s, o, 1e-6)

    lg, gx, gy = fx.chamfer_value_and_grad(dx, dy, w1=W1, w2=W2, gout=GOUT)
    assert _same_bits(lg, loss), (lg, loss)
    ogx, ogy = oracle.chamfer_bwd(x, y, ox, oy, W1, W2, GOUT)
    hgx, hgy = gx.to_host(), gy.to_host()
    assert np.array_equal(hgx, ogx, equal_nan=True), _first_diff(hgx, ogx)
    assert np.array_equal(hgy, ogy, equal_nan=True), _first_diff(hgy, ogy)
    return ix, iy


def _seed(kind, *shape):
    return sum(map(ord, kind)) * 7919 + int(np.dot(shape, [131, 17, 3, 1]))


# ------------------------------------------------------------------------------ D = 2: the exact loop by default
@pytest.mark.parametrize("N,M,B,kind", [(*s, k) for s in EXACT_SHAPES for k in _kinds(s[0], s[1])])
def test_exact_loop_d2(gpu_fx, oracle, N, M, B, kind):
    assert_exact_plan(N, M, B, 2)
    x, y = _data(kind, 2, N, M, B, _seed(kind, 2, N, M, B))
    _check(gpu_fx, oracle, x, y)


# ------------------------------------------------------------------------------ D = 3 under nn1_variant = 0
@pytest.mark.parametrize("N,M,B,kind", [(*s, k) for s in EXACT_SHAPES for k in _kinds(s[0], s[1])])
def test_exact_loop_d3_variant0(gpu_fx, oracle, N, M, B, kind):
    x, y = _data(kind, 3, N, M, B, _seed(kind, 3, N, M, B))
    with _lib().option("nn1_variant", 0):
        assert_exact_plan(N, M, B, 3)
        ix, iy = _check(gpu_fx, oracle, x, y)
    assert plan_of(N, M, B, 3)["kernel"] != "small_d"
    fx_, fy_ = gpu_fx.nearest_neighbors(x, y)     # the default path (fp16 filter or tiny kernel)
    assert np.array_equal(fx_.to_host(), ix) and np.array_equal(fy_.to_host(), iy)


# ------------------------------------------------------------------------------ generic D
@pytest.mark.parametrize("D,N,M,B,kind", [(D, *s, k) for D in GENERIC_DIMS for s in GENERIC_SHAPES for k in _kinds(s[0], s[1], D)])
def test_generic_kernel(gpu_fx, oracle, D, N, M, B, kind):
    assert_generic_plan(N, M, B, D)
    x, y = _data(kind, D, N, M, B, _seed(kind, D, N, M, B))
    _check(gpu_fx, oracle, x, y)


@pytest.mark.parametrize("D", [1, 5])
def test_generic_kernel_more_clouds_than_grid_rows(gpu_fx, oracle, D):
    """40 000 clouds of four points: 80 000 (cloud, direction) pairs, more than the 65 536 of a grid's y dimension -- the
    generic kernel's grid is 1-D."""
    N, M, B = 4, 4, 40000
    assert_generic_plan(N, M, B, D)
    for kind in ("uniform", "lattice"):
        x, y = _data(kind, D, N, M, B, _seed(kind, D, N, M, B))
        _check(gpu_fx, oracle, x, y)
