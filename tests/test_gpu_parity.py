"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on identical inputs.

Bar (BASELINE.json north_star): bit-exact indices (and distances, areas, samples -- anything the
oracle defines in unfused Float32); losses within 1e-5 relative.  Edge cases follow the
reference's tests (N != M, B = 2, ragged meshes) plus ragged tile/chunk boundaries, ties, D != 3.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5  # north_star: "Chamfer/Laplacian within 1e-5 relative fp32"


def _rand(shape, seed):
    return np.asfortranarray(np.random.default_rng(seed).random(shape, dtype=np.float32))


def _check_nn(fx, oracle, x, y):
    ix, iy, dx, dy = fx.nearest_neighbors(x, y, return_dist=True)
    ox, oy, odx, ody = oracle.nn1(x, y, want_dist=True)
    assert np.array_equal(ix.to_host(), ox), "idx_x differs from the oracle"
    assert np.array_equal(iy.to_host(), oy), "idx_y differs from the oracle"
    assert np.array_equal(dx.to_host(), odx) and np.array_equal(dy.to_host(), ody)


def _check_chamfer(fx, oracle, x, y, w1=1.0, w2=1.0):
    loss, ix, iy = fx.chamfer_distance(x, y, w1=w1, w2=w2, return_indices=True)
    oloss, ox, oy, _ = oracle.chamfer_distance(x, y, w1, w2, return_all=True)
    assert np.array_equal(ix.to_host(), ox) and np.array_equal(iy.to_host(), oy)
    assert np.isclose(loss, oloss, rtol=LOSS_RTOL, atol=0), (loss, oloss)
    loss2 = fx.chamfer_distance(x, y, w1=w1, w2=w2)  # loss-only kernel variant (no rescan)
    assert loss2 == loss
    return loss


# ------------------------------------------------------------------------------ chamfer / nn1
def test_c1_chamfer_b2_n1024(gpu_fx, oracle):
    """BASELINE config 1: B=2, N=M=1024, the documented synthetic stream."""
    fx = gpu_fx
    x = fx.synth.uniform_cloud(fx.synth.SEED_A, 3, 1024, 2)
    y = fx.synth.uniform_cloud(fx.synth.SEED_B, 3, 1024, 2)
    _check_nn(fx, oracle, x, y)
    _check_chamfer(fx, oracle, x, y)


def test_reference_test_shapes(gpu_fx, oracle):
    """test/metrics.jl:109-114: x (3,1000,2), y (3,500,2) -- N != M -- vs the dense naive formula."""
    fx = gpu_fx
    x, y = _rand((3, 1000, 2), 1), _rand((3, 500, 2), 2)
    loss = _check_chamfer(fx, oracle, x, y)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    naive = 0.0
    for b in range(2):
        P = ((x64[:, :, b] ** 2).sum(0)[:, None] + (y64[:, :, b] ** 2).sum(0)[None, :]
             - 2 * x64[:, :, b].T @ y64[:, :, b])
        naive += P.min(1).mean() / 2 + P.min(0).mean() / 2
    assert np.isclose(loss, naive, rtol=3.45e-4)
    # PointCloud front door, device resident, weights (src/metrics/pcloud.jl:11-12)
    pa, pb = fx.gpu(fx.PointCloud(x)), fx.gpu(fx.PointCloud(y))
    assert pa.on_device
    l2 = fx.chamfer_distance(pa, pb, w1=0.25, w2=2.0)
    assert np.isclose(l2, oracle.chamfer_distance(x, y, 0.25, 2.0), rtol=LOSS_RTOL)
    # rank-2 inputs are lifted to B=1 (src/metrics/pcloud.jl:28-37); Float64 input is cast (:14-19)
    l3 = fx.chamfer_distance(x[:, :, 0].astype(np.float64), y[:, :, 0].astype(np.float64))
    assert np.isclose(l3, oracle.chamfer_distance(x[:, :, :1], y[:, :, :1]), rtol=LOSS_RTOL)


def test_committed_golden_fixture(gpu_fx):
    """HIP vs the committed vectors (no oracle in the loop)."""
    fx = gpu_fx
    g = np.load(os.path.join(GOLDEN, "oracle_vectors.npz"))
    loss, ix, iy = fx.chamfer_distance(g["cx"], g["cy"], return_indices=True)
    assert np.array_equal(ix.to_host(), g["c_ix"]) and np.array_equal(iy.to_host(), g["c_iy"])
    assert np.isclose(loss, g["c_loss"], rtol=LOSS_RTOL)
    idx, dist = fx.knn(g["kx"], 20, drop_first=True)
    assert np.array_equal(idx.to_host(), g["k_idx"]) and np.array_equal(dist.to_host(), g["k_dist"])
    # round 4: one LDS image + an exact tail with a lattice block (ties), a split-plan shape, kNN at C4's size in both spaces
    for tag in ("g", "p"):
        loss, ix, iy = fx.chamfer_distance(g[tag + "_x"], g[tag + "_y"], return_indices=True)
        assert np.array_equal(ix.to_host(), g[tag + "_ix"]) and np.array_equal(iy.to_host(), g[tag + "_iy"]), tag
        assert np.isclose(loss, g[tag + "_loss"], rtol=LOSS_RTOL), tag
    for tag in ("k3", "k64"):
        idx, dist = fx.knn(g[tag + "_x"], 20, drop_first=True)
        assert np.array_equal(idx.to_host(), g[tag + "_idx"]) and np.array_equal(dist.to_host(), g[tag + "_dist"]), tag


@pytest.mark.parametrize("N,M,B", [(1, 1, 1), (1, 77, 3), (33, 4097, 1), (257, 31, 9), (513, 1025, 8),
                                   (2048, 300, 2), (5000, 5000, 2), (4096, 8200, 1), (100, 12289, 2)])
def test_ragged_sizes(gpu_fx, oracle, N, M, B):
    """Tile (32), block (256*R), LDS-chunk (4096) and cloud-count (8 per XCD group) boundaries."""
    x, y = _rand((3, N, B), N + B), _rand((3, M, B), M + 7 * B)
    _check_nn(gpu_fx, oracle, x, y)
    _check_chamfer(gpu_fx, oracle, x, y, 0.5, 1.5)


def test_ties_lowest_index_wins(gpu_fx, oracle):
    """Lattice clouds: many exactly equal distances; the first (lowest) index must win, in every
    tile/chunk position."""
    rng = np.random.default_rng(9)
    x = np.asfortranarray(rng.integers(0, 5, (3, 700, 2)).astype(np.float32))
    y = np.asfortranarray(rng.integers(0, 5, (3, 9000, 2)).astype(np.float32))
    _check_nn(gpu_fx, oracle, x, y)
    # all candidates identical: index 0 everywhere
    y1 = np.asfortranarray(np.ones((3, 4500, 1), np.float32))
    ix, _ = gpu_fx.nearest_neighbors(x[:, :, :1], y1)
    assert np.all(ix.to_host() == 0)


def _shell(rng, n, centre, radius):
    v = rng.standard_normal((3, n)).astype(np.float64)
    v /= np.linalg.norm(v, axis=0)
    return (centre[:, None] + radius * v).astype(np.float32)


@pytest.mark.parametrize("case", ["offset1000", "tiny_extent", "far_apart", "far_apart_swapped", "duplicates",
                                  "shell", "anisotropic", "huge_values", "multi_chunk_offset"])
def test_filter_robustness(gpu_fx, oracle, case):
    """Inputs chosen to stress the 16-bit-split filter + error band + exact re-scan: data far from the
    origin (Float32 spacing comparable to the NN gaps -> many near ties), tiny extents, clouds far from
    each other (fp16 range guard -> exact path), duplicate points, equidistant shells, extreme aspect
    ratios, very large magnitudes.  Indices must stay bit-identical to the oracle."""
    rng = np.random.default_rng(abs(hash(case)) % (2 ** 31))
    N, M, B = 1500, 4200, 2
    x, y = rng.random((3, N, B), dtype=np.float32), rng.random((3, M, B), dtype=np.float32)
    if case == "offset1000":
        x, y = x + np.float32(1000.0), y + np.float32(1000.0)
    elif case == "tiny_extent":
        x, y = x * np.float32(1e-6) + np.float32(5.0), y * np.float32(1e-6) + np.float32(5.0)
    elif case == "far_apart":
        y = y * np.float32(1e-3) + np.float32(1e4)
    elif case == "far_apart_swapped":
        x = x * np.float32(1e-3) - np.float32(3e3)
    elif case == "duplicates":
        y[:, ::2, :] = y[:, 1::2, :]
        x[:, :700, :] = y[:, :700, :]
    elif case == "shell":
        for b in range(B):
            c = rng.random(3) + 2.0
            y[:, :, b] = _shell(rng, M, c, 0.75)
            x[:, :, b] = (c[:, None] + 1e-3 * rng.standard_normal((3, N))).astype(np.float32)
    elif case == "anisotropic":
        sc = np.array([1e3, 1.0, 1e-3], np.float32)[:, None, None]
        x, y = x * sc, y * sc
    elif case == "huge_values":
        x, y = x * np.float32(1e15) + np.float32(3e15), y * np.float32(1e15) + np.float32(3e15)
    elif case == "multi_chunk_offset":
        M2 = 9000
        y = rng.random((3, M2, B), dtype=np.float32) - np.float32(250.0)
        x = x - np.float32(250.0)
    x, y = np.asfortranarray(x), np.asfortranarray(y)
    _check_nn(gpu_fx, oracle, x, y)
    _check_chamfer(gpu_fx, oracle, x, y)


@pytest.mark.parametrize("D", [1, 2, 5, 64])
def test_other_dimensions(gpu_fx, oracle, D):
    """D=2 clouds are allowed (src/rep/pcloud.jl:8-9; the *3 factor is kept);
    D=1 / D>3 take the generic kernel."""
    x, y = _rand((D, 300, 3), D), _rand((D, 411, 3), D + 100)
    _check_nn(gpu_fx, oracle, x, y)
    _check_chamfer(gpu_fx, oracle, x, y)


def test_identical_and_degenerate_clouds(gpu_fx, oracle):
    fx = gpu_fx
    x = _rand((3, 2000, 2), 5)
    assert fx.chamfer_distance(x, x) == 0.0
    ix, iy = fx.nearest_neighbors(x, x)
    assert np.array_equal(ix.to_host(), np.tile(np.arange(2000, dtype=np.int32)[:, None], (1, 2)))
    # the reference harness's input p_i = (i,i,i)/n, A == B (benchmarks/metrics.jl:11-15)
    for n in (64, 1024, 16384):
        p = fx.synth.reference_bench_cloud(n)
        assert fx.chamfer_distance(p, p) == 0.0
        _check_nn(fx, oracle, p[:, : min(n, 2048)], p[:, : min(n, 2048)])


def test_c2_full_size_parity_and_properties(gpu_fx, oracle):
    """BASELINE config 2 at full size (B=32, N=M=4096): indices bit-exact vs the oracle, loss within
    1e-5, plus size-independent properties."""
    fx = gpu_fx
    x = fx.synth.uniform_cloud(fx.synth.SEED_A, 3, 4096, 32)
    y = fx.synth.uniform_cloud(fx.synth.SEED_B, 3, 4096, 32)
    dx_, dy_ = fx.gpu(x), fx.gpu(y)
    loss, ix, iy = fx.chamfer_distance(dx_, dy_, return_indices=True)
    oloss, ox, oy, osums = oracle.chamfer_distance(x, y, return_all=True)
    ixh, iyh = ix.to_host(), iy.to_host()
    assert np.array_equal(ixh, ox) and np.array_equal(iyh, oy)
    assert np.isclose(loss, oloss, rtol=LOSS_RTOL, atol=0)
    # distances returned == distance to the returned index, recomputed in unfused float32
    _, _, dmx, _ = fx.nearest_neighbors(dx_, dy_, return_dist=True)
    b = 17
    d = x[:, :, b] - y[:, ixh[:, b], b]
    ref = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
    assert np.array_equal(dmx.to_host()[:, b], ref.astype(np.float32))
    # linearity in (w1, w2)
    la = fx.chamfer_distance(dx_, dy_, w1=1.0, w2=0.0)
    lb = fx.chamfer_distance(dx_, dy_, w1=0.0, w2=1.0)
    assert np.isclose(la + lb, loss, rtol=1e-6)
    assert np.isclose(fx.chamfer_distance(dx_, dy_, w1=0.3, w2=1.7), 0.3 * la + 1.7 * lb, rtol=1e-6)
    # symmetry: swapping the clouds swaps the two directional terms
    assert np.isclose(fx.chamfer_distance(dy_, dx_, w1=1.0, w2=0.0), lb, rtol=1e-6)
    # permuting the points of y permutes the indices and leaves the loss unchanged
    perm = np.random.default_rng(0).permutation(4096)
    yp = np.asfortranarray(y[:, perm, :])
    lp, ixp, _ = fx.chamfer_distance(dx_, yp, return_indices=True)
    assert np.isclose(lp, loss, rtol=1e-6)
    assert np.array_equal(perm[ixp.to_host()[:, 3]], ixh[:, 3])  # unique minima on random data
    # batch shards reproduce the full result (what the multi-GPU split relies on)
    from flux3d_jl_amd.distributed import chamfer_sums
    s_full = chamfer_sums(dx_, dy_)
    s_parts = sum(chamfer_sums(dx_.slab(s, 8), dy_.slab(s, 8)) for s in range(0, 32, 8))
    assert np.allclose(s_full, s_parts, rtol=1e-12) and np.allclose(s_full, osums, rtol=1e-6)


def test_chamfer_backward(gpu_fx, oracle):
    """Adjoint (test/metrics.jl:112-114 tolerance: atol 1e-2, rtol 1e-3).  Round 5: the gather form accumulates every row in
    the oracle's order -- bit for bit."""
    fx = gpu_fx
    x, y = _rand((3, 1000, 2), 21), _rand((3, 500, 2), 22)
    loss, ix, iy = fx.chamfer_distance(x, y, w1=0.7, w2=1.3, return_indices=True)
    gx, gy = fx.chamfer_distance_grad(x, y, ix, iy, w1=0.7, w2=1.3, gout=2.0)
    ogx, ogy = oracle.chamfer_bwd(x, y, ix.to_host(), iy.to_host(), 0.7, 1.3, 2.0)
    assert np.array_equal(gx.to_host(), ogx)
    assert np.array_equal(gy.to_host(), ogy)


@pytest.mark.parametrize("N,M,B", [(4096, 4096, 3), (700, 5000, 1), (14000, 300, 1), (1, 9, 2), (257, 256, 40), (5000, 5000, 8),
                                   (4097, 9000, 2), (20000, 17000, 1)])
def test_chamfer_backward_shapes(gpu_fx, oracle, fx_option, N, M, B):
    """Atomic-free gather adjoint (inverse lists by an LDS counting sort, every row accumulated in the oracle's
    order; row ranges split over blocks, other sides beyond one 4096-row round) is BIT-IDENTICAL to the oracle's adjoint and
    the same run after run; the global-atomics variant stays within rounding."""
    fx = gpu_fx
    x, y = _rand((3, N, B), N + 1), _rand((3, M, B), M + 2)
    _, ix, iy = fx.chamfer_distance(x, y, return_indices=True)
    ogx, ogy = oracle.chamfer_bwd(x, y, ix.to_host(), iy.to_host(), 1.0, 0.5, 1.5)
    for rep in range(2):
        gx, gy = fx.chamfer_distance_grad(x, y, ix, iy, w1=1.0, w2=0.5, gout=1.5)
        assert np.array_equal(gx.to_host(), ogx), (rep, np.abs(gx.to_host() - ogx).max())
        assert np.array_equal(gy.to_host(), ogy), (rep, np.abs(gy.to_host() - ogy).max())
    fx_option("bwd_global_atomics", "1")
    gx, gy = fx.chamfer_distance_grad(x, y, ix, iy, w1=1.0, w2=0.5, gout=1.5)
    assert np.allclose(gx.to_host(), ogx, rtol=1e-5, atol=1e-9)
    assert np.allclose(gy.to_host(), ogy, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("D", [3, 2, 5, 64])
@pytest.mark.parametrize("kind", ["all_to_one", "clusters", "few_targets", "negative_gout"])
def test_chamfer_backward_long_inverse_lists(gpu_fx, oracle, kind, D):
    """Index maps with LONG inverse lists (one row the neighbour of thousands, tight clusters, lists of 9 .. 64 entries that
    take the wave path; lists of 5 .. 8 that take the 8-network) given directly -- the adjoint takes any index arrays -- over
    more than one 4096-row round; D = 3 (registers) and other D (the row of g is the accumulator): bit-identical to the oracle."""
    fx = gpu_fx
    rng = np.random.default_rng(sum(map(ord, kind)) * 131 + D)
    N, M, B = 6000, 9001, 3
    x = np.asfortranarray(rng.standard_normal((D, N, B)).astype(np.float32))
    y = np.asfortranarray(rng.standard_normal((D, M, B)).astype(np.float32))
    if kind == "all_to_one":
        ix = np.full((N, B), 7, np.int32); iy = np.full((M, B), N - 1, np.int32)
        ix[::3, 1] = 8999
    elif kind == "clusters":
        ix = rng.integers(0, 40, (N, B)).astype(np.int32) * 200
        iy = rng.integers(0, 30, (M, B)).astype(np.int32) * 199
    elif kind == "few_targets":
        ix = (rng.integers(0, M // 6, (N, B)) * 6).astype(np.int32)  # lists of ~ 4 (Poisson): both networks and the wave path
        iy = (rng.integers(0, N // 12, (M, B)) * 12).astype(np.int32)  # ~ 18 per target
    else:
        ix = rng.integers(0, M, (N, B)).astype(np.int32); iy = rng.integers(0, N, (M, B)).astype(np.int32)
        x[:, :50, 0] = y[:, ix[:50, 0], 0]  # exact zeros in the own term: 0 + (-0) is +0
    gout = -1.5 if kind == "negative_gout" else 1.0
    ix, iy = np.asfortranarray(ix), np.asfortranarray(iy)
    ogx, ogy = oracle.chamfer_bwd(x, y, ix, iy, 0.9, 1.1, gout)
    gx, gy = fx.chamfer_distance_grad(x, y, fx.gpu(ix), fx.gpu(iy), w1=0.9, w2=1.1, gout=gout)
    hx, hy = gx.to_host(), gy.to_host()
    assert np.array_equal(hx.view(np.uint32), ogx.view(np.uint32)), np.abs(hx - ogx).max()
    assert np.array_equal(hy.view(np.uint32), ogy.view(np.uint32)), np.abs(hy - ogy).max()


@pytest.mark.parametrize("N,M", [(300, 3600), (300, 7700), (600, 7700)])
def test_chamfer_backward_more_long_rows_than_the_lds_table(gpu_fx, oracle, N, M):
    """More rows with long lists in ONE block than the 256 whose point and index travel through LDS: the wave that takes such a
    row re-reads both from memory.  D = 3, B = 160, iy[j] = j % 300: rows 0 .. 299 of side x each get 12 entries of every
    4096-row round (13 or 14 of a full one) -- all long (> 8); a round has at most 4096 entries in all, and 300 <= the 456 rows
    the list of long rows holds.  They belong to one block: blocks per (cloud, side) = max(1, CUs / (2 B)), = 1 for B = 160 on any device
    below 320 CUs, raised until a block's share of max(N, M) rows is at most 4096 -- so 1 at M = 3600 (one round), and 2 at
    M = 7700 (two rounds: rows past the table also reload their accumulator), where N = 300 leaves a block 150 rows, all in the
    table, and N = 600 gives the first block rows 0 .. 299.  Bit-identical to the oracle."""
    fx = gpu_fx
    B = 160
    rng = np.random.default_rng(7 * N + M)
    x = np.asfortranarray(rng.standard_normal((3, N, B)).astype(np.float32))
    y = np.asfortranarray(rng.standard_normal((3, M, B)).astype(np.float32))
    ix = np.asfortranarray(rng.integers(0, M, (N, B)).astype(np.int32))
    iy = np.asfortranarray(np.repeat((np.arange(M, dtype=np.int32) % 300)[:, None], B, axis=1))
    ogx, ogy = oracle.chamfer_bwd(x, y, ix, iy, 0.9, 1.1, 1.0)
    gx, gy = fx.chamfer_distance_grad(x, y, fx.gpu(ix), fx.gpu(iy), w1=0.9, w2=1.1, gout=1.0)
    hx, hy = gx.to_host(), gy.to_host()
    assert np.array_equal(hx.view(np.uint32), ogx.view(np.uint32)), np.abs(hx - ogx).max()
    assert np.array_equal(hy.view(np.uint32), ogy.view(np.uint32)), np.abs(hy - ogy).max()


@pytest.mark.parametrize("ordered", [True, False])
@pytest.mark.parametrize("kind", ["all_to_one", "clusters"])
def test_chamfer_sampled_adjoint_long_inverse_lists(gpu_fx, kind, ordered):
    """The sampled entry points with index maps GIVEN, so that their lists are long (real nearest-neighbour maps have short
    ones): one row the neighbour of thousands, tight clusters -- the kinds of test_chamfer_backward_long_inverse_lists at
    n = 4200 samples, two rounds.  Against fx3d_chamfer_bwd followed by fx3d_sample_points_bwd on the same draws: the ordered
    form bit for bit; the scatter form (long rows through the accumulators in LDS) up to the order of its float atomics."""
    fx = gpu_fx
    paths = [os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj")]
    ma, mb = fx.gpu(fx.load_trimesh(paths[0], paths[1])), fx.gpu(fx.load_trimesh(paths[1], paths[0]))
    n, nb = 4200, 2
    assert fx.sampling_adjoint_is_ordered(ma, n) and fx.sampling_adjoint_is_ordered(mb, n)
    A, fa, ra1, ra2 = fx.sample_points(ma, n, seed=5, return_draws=True)
    Bp, fb, rb1, rb2 = fx.sample_points(mb, n, seed=6, return_draws=True)
    rng = np.random.default_rng(sum(map(ord, kind)))
    if kind == "all_to_one":
        ix = np.full((n, nb), 7, np.int32); iy = np.full((n, nb), n - 1, np.int32)
        ix[::3, 1] = n - 2
    else:
        ix = rng.integers(0, 40, (n, nb)).astype(np.int32) * (n // 40)
        iy = rng.integers(0, 30, (n, nb)).astype(np.int32) * (n // 30)
    ix, iy = fx.gpu(np.asfortranarray(ix)), fx.gpu(np.asfortranarray(iy))
    gA, gB = fx.chamfer_distance_grad(A, Bp, ix, iy, w1=0.9, w2=1.1, gout=1.5)
    ref_a = fx.sample_points_grad(ma, fa, ra1, ra2, gA).to_host()
    ref_b = fx.sample_points_grad(mb, fb, rb1, rb2, gB).to_host()
    assert np.isfinite(ref_a).all() and np.abs(ref_a).max() > 0
    ga, gb = fx.chamfer_sampled_grad(A, Bp, ix, iy, ma, (fa, ra1, ra2), mb, (fb, rb1, rb2), w1=0.9, w2=1.1, gout=1.5, ordered=ordered)
    ha, hb = ga.to_host(), gb.to_host()
    if ordered:
        assert np.array_equal(ha.view(np.uint32), ref_a.view(np.uint32)), np.abs(ha - ref_a).max()
        assert np.array_equal(hb.view(np.uint32), ref_b.view(np.uint32)), np.abs(hb - ref_b).max()
    else:
        assert np.allclose(ha, ref_a, rtol=2e-4, atol=1e-8) and np.allclose(hb, ref_b, rtol=2e-4, atol=1e-8)


def test_invalid_arguments_raise(gpu_fx):
    fx = gpu_fx
    x = _rand((3, 10, 2), 0)
    with pytest.raises(ValueError):
        fx.chamfer_distance(x, _rand((3, 10, 3), 0))  # batch mismatch (src/metrics/pcloud.jl:57-58)
    with pytest.raises(ValueError):
        fx.chamfer_distance(x, _rand((2, 10, 2), 0))
    fx.knn(x, 10)  # k == M is fine without drop_first
    with pytest.raises(fx.Flux3DHipError):
        fx.knn(x, 10, drop_first=True)  # k+1 > M
    idx, _ = fx.knn(_rand((3, 100, 1), 0), 64, drop_first=True)  # k+1 > 64: the general selection kernel (round 2)
    assert idx.shape == (64, 100, 1)
    from flux3d_jl_amd import _lib
    import ctypes
    d = fx.gpu(x)
    rc = _lib.load().fx3d_chamfer_fwd(d.ptr, 10, d.ptr, 10, 2, 3, 1.0, 1.0, d.ptr, None, None, None, None, 0, None)
    assert rc == -6 and "workspace" in _lib.last_error()


def test_non_default_stream_and_async(gpu_fx, oracle):
    fx = gpu_fx
    x, y = _rand((3, 3000, 4), 31), _rand((3, 2500, 4), 32)
    s = fx.Stream.create()
    with fx.stream(s):
        dx_, dy_ = fx.gpu(x), fx.gpu(y)
        out = fx.chamfer_distance(dx_, dy_, sync=False)  # device scalar, no host sync
        e0, e1 = fx.Event(), fx.Event()
        e0.record()
        for _ in range(3):
            fx.chamfer_distance(dx_, dy_, loss_out=out, sync=False)
        e1.record()
        s.synchronize()
        assert e0.elapsed_ms(e1) > 0
        assert np.isclose(out.item(), oracle.chamfer_distance(x, y), rtol=LOSS_RTOL)


def test_torch_interop_zero_copy(gpu_fx):
    """A torch CUDA tensor's memory is consumed in place (DeviceArray.wrap).  Runs in a fresh
    process that imports torch FIRST, so that one HIP runtime (torch's) serves both -- the same
    order bench.py uses for its multi-GPU path."""
    import subprocess
    import sys
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
assert torch.cuda.is_available()
import flux3d_jl_amd as fx
from oracle import oracle
rng = np.random.default_rng(41)
x = np.asfortranarray(rng.random((3, 600, 2), dtype=np.float32))
y = np.asfortranarray(rng.random((3, 700, 2), dtype=np.float32))
# torch row-major (B,N,3) has the same bytes as Julia's column-major (3,N,B)
tx = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 1, 0))).cuda()
ty = torch.from_numpy(np.ascontiguousarray(y.transpose(2, 1, 0))).cuda()
torch.cuda.synchronize()
loss = fx.chamfer_distance(fx.DeviceArray.wrap(tx), fx.DeviceArray.wrap(ty))
assert np.isclose(loss, oracle.chamfer_distance(x, y), rtol=1e-5), loss
from flux3d_jl_amd.distributed import ShardedChamfer
sc = ShardedChamfer()
l2 = sc(fx.DeviceArray.wrap(tx), fx.DeviceArray.wrap(ty), 2)
assert np.isclose(l2, loss, rtol=1e-6), (l2, loss)
print("TORCH_INTEROP_OK")
""" % (os.path.dirname(GOLDEN).rsplit(os.sep, 1)[0],)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "TORCH_INTEROP_OK" in r.stdout, r.stdout + r.stderr


def test_native_rccl_comm_single_rank(gpu_fx, oracle):
    """fx3d_comm_* / fx3d_chamfer_fwd_sharded with a 1-rank RCCL communicator (fresh process: RCCL is
    dlopen'ed by the library, no torch involved)."""
    import subprocess
    import sys
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import flux3d_jl_amd as fx
from flux3d_jl_amd.distributed import NativeComm, NativeShardedChamfer
from oracle import oracle
x = fx.synth.uniform_cloud(1, 3, 700, 4); y = fx.synth.uniform_cloud(2, 3, 900, 4)
comm = NativeComm(0, 1)
sc = NativeShardedChamfer(comm)
loss = sc(fx.gpu(x), fx.gpu(y), 4, 0.5, 1.5)
assert np.isclose(loss, oracle.chamfer_distance(x, y, 0.5, 1.5), rtol=1e-5), loss
buf = fx.DeviceArray.from_host(np.array([1.5, 2.5], np.float64)); comm.allreduce_sum(buf)
assert list(buf.to_host()) == [1.5, 2.5]
# a shard of the batch with the GLOBAL batch size divides by B_global
l2 = sc(fx.gpu(x[:, :, :2]), fx.gpu(y[:, :, :2]), 4)
s = oracle.chamfer_distance(x[:, :, :2], y[:, :, :2], return_all=True)[3]
from flux3d_jl_amd.distributed import loss_from_sums
assert np.isclose(l2, loss_from_sums(s, 700, 900, 4, 3), rtol=1e-6)
print("NATIVE_COMM_OK")
""" % (os.path.dirname(GOLDEN).rsplit(os.sep, 1)[0],)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "NATIVE_COMM_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ------------------------------------------------------------------------------------------ kNN
@pytest.mark.parametrize("N,B,k,drop", [(1024, 4, 20, True), (200, 2, 1, False), (64, 2, 10, True),
                                        (300, 1, 63, True), (2500, 2, 5, False), (70, 3, 7, False)])
def test_knn_d3(gpu_fx, oracle, N, B, k, drop):
    """BASELINE config 4 shape (k=20 self-graph, drop first) and the K=10 of the example
    (examples/dgcnn_classification.jl:28); chunk boundary (N > 2048); kk = 64."""
    x = _rand((3, N, B), N + k)
    idx, dist = gpu_fx.knn(x, k, drop_first=drop)
    oi, od = oracle.knn(x, k, drop_first=drop)
    assert np.array_equal(idx.to_host(), oi)
    assert np.array_equal(dist.to_host(), od)


def test_knn_ties_and_cross_set(gpu_fx, oracle):
    rng = np.random.default_rng(2)
    x = np.asfortranarray(rng.integers(0, 4, (3, 500, 2)).astype(np.float32))
    y = np.asfortranarray(rng.integers(0, 4, (3, 333, 2)).astype(np.float32))
    idx, dist = gpu_fx.knn(x, 16, y=y)
    oi, od = oracle.knn(x, 16, y=y)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


@pytest.mark.parametrize("D", [2, 16, 64])
def test_knn_feature_space(gpu_fx, oracle, D):
    """Second EdgeConv: kNN in 64-D feature space (src/models/dgcnn.jl:121)."""
    x = np.asfortranarray(np.random.default_rng(D).standard_normal((D, 512, 2)).astype(np.float32))
    idx, dist = gpu_fx.knn(x, 20, drop_first=True)
    oi, od = oracle.knn(x, 20, drop_first=True)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


@pytest.mark.parametrize("D,N,M,B,k,drop,kind", [
    (64, 1024, 1024, 2, 20, True, "normal"),     # second EdgeConv (src/models/dgcnn.jl:121), 3 LDS chunks
    (4, 100, 77, 2, 5, False, "normal"),         # smallest D of the matrix-core path, ragged M
    (5, 130, 200, 1, 31, True, "normal"),        # D % 4 != 0 (scalar staging), kk = 32
    (33, 97, 333, 2, 10, True, "normal"),        # D just above a 32 multiple (zero-padded k-steps)
    (100, 64, 640, 1, 8, False, "normal"),
    (128, 300, 300, 1, 20, True, "scaled"),      # large norms: wide band, still exact
    (120, 50, 90, 1, 3, False, "normal"),        # DK = 4, ragged d padding
    (16, 256, 256, 1, 12, True, "lattice"),      # integer features: masses of exact ties
    (8, 128, 160, 1, 20, False, "same"),         # all candidates identical: list overflow -> brute-force merge
    (64, 96, 1500, 1, 20, False, "offset"),      # far-from-origin cloud (cancellation in the expanded form)
    (128, 64, 160, 1, 20, False, "same"),        # DK = 4: every list overflows -> brute-force merge
    (6, 64, 160, 1, 20, False, "same"),          # the same under the Float32 GEMM (D % 4 != 0)
])
def test_knn_matrix_core_path(gpu_fx, oracle, D, N, M, B, k, drop, kind):
    """knn_mfma_kernel: Float32 GEMM filter + exact re-scan must reproduce the oracle's (distance, index)
    order bit for bit on ragged shapes, ties, degenerate and badly scaled inputs."""
    rng = np.random.default_rng(D * 1000 + M)
    if kind == "lattice":
        gen = lambda n: rng.integers(0, 3, (D, n, B)).astype(np.float32)
    elif kind == "same":
        gen = lambda n: np.ones((D, n, B), np.float32) * np.float32(0.37)
    else:
        gen = lambda n: rng.standard_normal((D, n, B)).astype(np.float32)
    x = np.asfortranarray(gen(N))
    y = x if (N == M and kind != "scaled") else np.asfortranarray(gen(M))
    if kind == "scaled":
        x, y = x * np.float32(1.0e4), y * np.float32(1.0e4)
    if kind == "offset":
        x, y = x + np.float32(300.0), y + np.float32(300.0)
    idx, dist = gpu_fx.knn(x, k, y=None if y is x else y, drop_first=drop)
    oi, od = oracle.knn(x, k, y=None if y is x else y, drop_first=drop)
    assert np.array_equal(idx.to_host(), oi)
    assert np.array_equal(dist.to_host(), od)


def test_knn_float32_filter_variant(gpu_fx, oracle):
    """The Float32 GEMM filter is what feature-space clouds get that the fp16 filter does not take (D % 4 != 0, or more than 4096
    candidates): shapes on both sides of either rule must give the oracle's lists."""
    rng = np.random.default_rng(77)
    for (D, N, M, k) in ((62, 300, 1024, 20), (30, 100, 200, 9), (127, 64, 96, 5), (64, 96, 4160, 20), (6, 200, 333, 7),
                         (128, 64, 4161, 5), (64, 64, 4161, 5)):  # an odd M > 4096 is not sliced: the Float32 GEMM with the vectorised gather
        x = np.asfortranarray(rng.standard_normal((D, N, 2)).astype(np.float32))
        y = np.asfortranarray(rng.standard_normal((D, M, 2)).astype(np.float32))
        idx, dist = gpu_fx.knn(x, k, y=y)
        oi, od = oracle.knn(x, k, y=y)
        assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od), (D, N, M, k)


def test_knn_fp16_filter(gpu_fx, oracle):
    """The default feature-space filter uses the fp16-rounded operands alone (one MFMA per K block, band 2^-10): the oracle's
    lists on centred data and on data with a large common offset (the band grows with |q|^2 + |c|^2: more survivors, and past
    the list capacity the exact fallback)."""
    rng = np.random.default_rng(78)
    for (D, N, M, k, shift) in ((64, 300, 1024, 20, 0.0), (64, 200, 512, 20, 3.0), (32, 100, 200, 9, 0.0),
                                (128, 64, 96, 5, 0.5), (16, 130, 700, 31, 10.0), (64, 96, 1024, 12, 40.0)):
        x = np.asfortranarray((rng.standard_normal((D, N, 2)) + shift).astype(np.float32))
        y = np.asfortranarray((rng.standard_normal((D, M, 2)) + shift).astype(np.float32))
        idx, dist = gpu_fx.knn(x, k, y=y)
        oi, od = oracle.knn(x, k, y=y)
        assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


@pytest.mark.parametrize("D,N,M,B,k,drop", [
    (64, 300, 2048, 2, 20, False),   # 8 row stages of 256
    (64, 257, 2047, 1, 20, True),    # ragged last stage (x is not y: N != M)
    (64, 1024, 1024, 9, 20, True),   # the second EdgeConv's shape, B > 8 (clouds share an XCD)
    (128, 130, 1024, 1, 16, False),  # D > 64: two column halves of 64, stages of 256 half rows
    (128, 1024, 1024, 3, 20, True),  # C4's clouds with 128 features
    (100, 200, 1500, 2, 20, False),  # second half 36 columns wide
    (68, 150, 900, 1, 12, True),     # second half: a single 16-byte piece
    (32, 200, 2000, 2, 31, False),
    (16, 100, 700, 1, 7, False),
    (4, 333, 2048, 1, 32, False),    # smallest row (one 16-byte piece)
    (64, 100, 4096, 1, 20, False),   # one long cloud on an empty grid: 8 candidate slices of 512 rows
    (62, 150, 700, 2, 12, False),    # D % 4 != 0: no staging, every survivor's row gathered from L2
    (128, 100, 2305, 1, 12, False),  # more than 8 stages and an odd M (no candidate slices): the vectorised gather, query pieces re-read
    (64, 100, 2305, 1, 20, False),   # the same at D = 64 and
    (32, 100, 2305, 1, 9, False),    # at D = 32 (query row in registers)
])
def test_knn_staged_exact_phase(gpu_fx, oracle, fx_option, D, N, M, B, k, drop):
    """knn_mfma_kernel's exact phase with the candidate rows staged through LDS (default when D/4 divides the block and
    the cloud makes at most 8 stages) and with the per-survivor gather from L2 (clouds of more than 8 stages, rows that are not
    a multiple of 16 bytes): the oracle's lists bit for bit, distances included."""
    rng = np.random.default_rng(D * 7 + M)
    x = np.asfortranarray(rng.standard_normal((D, N, B)).astype(np.float32))
    y = x if drop else np.asfortranarray(rng.standard_normal((D, M, B)).astype(np.float32))
    if drop:
        x = y = np.asfortranarray(rng.standard_normal((D, M, B)).astype(np.float32))
    oi, od = oracle.knn(x, k, y=None if y is x else y, drop_first=drop)
    # (default: fx3d_knn_ws with the pre-pass image; FX3D_KNN_NO_PREPASS=1: every block builds its own image, as fx3d_knn does)
    for nopre in (False, True):
        fx_option("knn_no_prepass", "1" if nopre else "0")
        idx, dist = gpu_fx.knn(x, k, y=None if y is x else y, drop_first=drop)
        assert np.array_equal(idx.to_host(), oi), f"nopre={nopre}"
        assert np.array_equal(dist.to_host(), od), f"nopre={nopre}"


@pytest.mark.parametrize("D,csize,spread", [(64, 80, 1e-3), (32, 200, 1e-4), (64, 700, 1e-3), (128, 200, 1e-3), (30, 200, 1e-3)])
def test_knn_feature_space_clustered_data(gpu_fx, oracle, D, csize, spread):
    """Tight clusters put more candidates inside a query's band than the fast path's key arrays hold (60): the medium
    path selects exactly among the query's own survivors (up to 512), larger clusters take the full exact merge.  D = 128: the
    widest instantiation; D = 30: the Float32 GEMM's two lane lists per query instead of the pre-pass mode's four."""
    rng = np.random.default_rng(D + csize)
    N = 1024
    centres = rng.standard_normal((D, N // csize + 1, 2)) * 3
    x = centres[:, rng.integers(0, centres.shape[1], N), :] + rng.standard_normal((D, N, 2)) * spread
    x = np.asfortranarray(x.astype(np.float32))
    idx, dist = gpu_fx.knn(x, 20, drop_first=True)
    oi, od = oracle.knn(x, 20, drop_first=True)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


def test_knn_graph_gather(gpu_fx, oracle):
    """create_knn_graph == cat([X[:, knn idx]]...) (src/models/dgcnn.jl:3-7,36): (F,K,N,B)."""
    for F in (3, 64):
        x = np.asfortranarray(np.random.default_rng(F).standard_normal((F, 256, 3)).astype(np.float32))
        g = gpu_fx.create_knn_graph(x, 10)
        assert g.shape == (F, 10, 256, 3)
        oi = oracle.knn(x, 10, drop_first=True, want_dist=False)
        assert np.array_equal(g.to_host(), oracle.knn_gather(x, oi))


# --------------------------------------------------------------------------------------- meshes
def _teapot_sphere(fx):
    return fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj"))


def test_face_areas(gpu_fx, oracle, known):
    """Known answers (test/rep.jl:259-260) and bit parity with the oracle on teapot+sphere."""
    fx = gpu_fx
    k = known["areas_batch"]
    vl = [np.asfortranarray(np.array(v, np.float32).T) for v in k["verts"]]
    fl = [np.asfortranarray(np.array(f, np.int64).T) for f in k["faces"]]
    m = fx.TriMesh(vl, fl)
    a = fx.compute_faces_areas_packed(m).to_host()
    assert np.allclose(a, np.concatenate(k["areas"]), rtol=1e-4, atol=1e-4)
    ap = fx.compute_faces_areas_padded(m).to_host()
    assert ap.shape == (1, 4, 2) and np.all(ap[0, 2:, 1] == 0)
    al = fx.compute_faces_areas_list(m)
    assert [x.shape for x in al] == [(1, 4), (1, 2)]
    for mm in (_teapot_sphere(fx), fx.gpu(_teapot_sphere(fx))):
        got = fx.compute_faces_areas_packed(mm).to_host()
        exp = oracle.faces_areas_packed(mm.get_verts_packed_host(), mm.get_faces_packed().astype(np.int64) - 1)
        assert np.array_equal(got, exp)
        gp = fx.compute_faces_areas_padded(mm).to_host()
        ep = oracle.faces_areas_padded(mm.get_verts_padded_host(), mm.get_faces_padded().astype(np.int64) - 1,
                                       mm._faces_len)
        assert np.array_equal(gp, ep)


def test_mesh_losses(gpu_fx, oracle, known):
    fx = gpu_fx
    t = fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj"))
    # README.md:111-112 known answer, on a device-resident mesh like the README example
    assert abs(float(fx.laplacian_loss(fx.gpu(t))) - known["teapot_laplacian_loss"]["value"]) < 1e-7
    for m in (t, _teapot_sphere(fx), fx.gpu(_teapot_sphere(fx))):
        v = m.get_verts_packed_host()
        e0 = m.get_edges_packed().astype(np.int64) - 1
        rowptr, colind, vals = m.get_laplacian_packed()
        ol = oracle.laplacian_loss(v, rowptr.astype(np.int64), colind.astype(np.int64), vals)
        assert np.isclose(fx.laplacian_loss(m), ol, rtol=LOSS_RTOL, atol=0)
        for target in (0.0, 0.05):
            assert np.isclose(fx.edge_loss(m, target), oracle.edge_loss(v, e0, target), rtol=LOSS_RTOL, atol=0)
        gl = fx.laplacian_loss_grad(m, 1.5).to_host()
        assert np.allclose(gl, oracle.laplacian_loss_bwd(v, rowptr.astype(np.int64), colind.astype(np.int64), vals, 1.5),
                           rtol=1e-4, atol=1e-9)
        ge = fx.edge_loss_grad(m, 0.05, 0.5).to_host()
        assert np.allclose(ge, oracle.edge_loss_bwd(v, e0, 0.05, 0.5), rtol=1e-4, atol=1e-9)


def test_three_mesh_batch_losses(gpu_fx, oracle, known):
    """test/metrics.jl:8-73: laplacian_loss on the hand-written ragged batch == dense construction."""
    fx = gpu_fx
    k = known["three_mesh_batch"]
    vl = [np.asfortranarray(np.array(v, np.float32).T) for v in k["verts"]]
    fl = [np.asfortranarray(np.array(f, np.uint32).T) for f in k["faces"]]
    m = fx.TriMesh(vl, fl)
    Ld = m.laplacian_dense().astype(np.float64)
    vp = m.get_verts_packed_host().astype(np.float64)
    ref = np.sqrt(((Ld @ vp.T) ** 2).sum(1)).mean()
    assert np.isclose(fx.laplacian_loss(m), ref, rtol=3.45e-4)
    e0 = m.get_edges_packed().astype(np.int64) - 1
    d = vp[:, e0[:, 0]] - vp[:, e0[:, 1]]
    assert np.isclose(fx.edge_loss(m), (d ** 2).sum(0).mean(), rtol=1e-6)


def test_degenerate_benchmark_mesh(gpu_fx):
    """generate_trimesh (benchmarks/metrics.jl:17-22): faces (i,i,i) -> both losses are 0."""
    n = 1024
    v = np.asfortranarray((np.cumsum(np.ones((3, n)), axis=1) / n).astype(np.float32))
    f = np.asfortranarray(np.tile(np.arange(1, n + 1), (3, 1)).astype(np.int32))
    m = gpu_fx.TriMesh([v], [f])
    assert gpu_fx.laplacian_loss(m) == 0.0 and gpu_fx.edge_loss(m) == 0.0


# -------------------------------------------------------------------------------------- sampler
def test_sample_points_explicit_draws(gpu_fx, oracle):
    """_sample_points for given (face, r1, r2): bit-exact (src/transforms/mesh_func.jl:60-82)."""
    fx = gpu_fx
    m = _teapot_sphere(fx)
    rng = np.random.default_rng(8)
    n = 3000
    fi = np.asfortranarray(np.stack([rng.integers(0, 2256, n), rng.integers(0, 5120, n)], axis=1).astype(np.int32))
    r1 = np.asfortranarray(rng.random((n, 2), dtype=np.float32))
    r2 = np.asfortranarray(rng.random((n, 2), dtype=np.float32))
    r1[0, 0], r2[0, 0], r1[1, 0] = 0.0, 0.0, np.float32(1.0 - 2 ** -24)
    got = fx.sample_points(m, n, face_idx=fi, r1=r1, r2=r2).to_host()
    exp = oracle.sample_points_explicit(m.get_verts_padded_host(), m.get_faces_padded().astype(np.int64) - 1, fi, r1, r2)
    assert got.shape == (3, n, 2) and np.array_equal(got, exp)


@pytest.mark.parametrize("on_device", [False, True])
def test_sample_points_seeded_parity(gpu_fx, oracle, on_device):
    """Device Philox/CDF draw == oracle restatement, bit for bit, on a ragged batch; the sphere
    samples satisfy the reference's radius test (test/transforms/mesh_func.jl:10-12)."""
    fx = gpu_fx
    m = _teapot_sphere(fx)
    if on_device:
        m = fx.gpu(m)
    out, fi, r1, r2 = fx.sample_points(m, 5000, seed=4242, return_draws=True)
    eo, efi, er1, er2 = oracle.sample_points_seeded(
        m.get_verts_padded_host(), m.get_faces_padded().astype(np.int64) - 1, m._faces_len, 5000, 4242,
        return_draws=True)
    assert np.array_equal(fi.to_host(), efi)
    assert np.array_equal(r1.to_host(), er1) and np.array_equal(r2.to_host(), er2)
    s = out.to_host()
    assert np.array_equal(s, eo)
    r = np.sqrt((s[:, :, 1].astype(np.float64) ** 2).sum(0))
    assert np.allclose(r, 1.0, rtol=1e-2, atol=1e-5)
    assert fi.to_host()[:, 0].max() < 2256  # shorter mesh never samples its padding
    # fresh seed per call, like the reference's global RNG
    a, b = fx.sample_points(m, 100).to_host(), fx.sample_points(m, 100).to_host()
    assert not np.array_equal(a, b)


def test_sample_points_statistics(gpu_fx, oracle):
    fx = gpu_fx
    t = fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj"))
    n = 200000
    _, fi, _, _ = fx.sample_points(t, n, seed=7, return_draws=True)
    area = fx.compute_faces_areas_packed(t).to_host().astype(np.float64)
    p = area / area.sum()
    cnt = np.bincount(fi.to_host()[:, 0], minlength=2256)
    keep = p * n >= 5
    chi2 = (((cnt - p * n) ** 2)[keep] / (p * n)[keep]).sum()
    dof = keep.sum() - 1
    assert abs(chi2 - dof) < 6 * np.sqrt(2 * dof)


def test_sample_points_backward(gpu_fx):
    fx = gpu_fx
    m = _teapot_sphere(fx)
    out, fi, r1, r2 = fx.sample_points(m, 2000, seed=5, return_draws=True)
    gout = _rand((3, 2000, 2), 77)
    g = fx.sample_points_grad(m, fi, r1, r2, gout).to_host()
    # reference: scatter in float64 on the host from the same draws
    fih, r1h, r2h = fi.to_host(), r1.to_host(), r2.to_host()
    fp = m.get_faces_padded().astype(np.int64) - 1
    exp = np.zeros((3, m.V, 2))
    for b in range(2):
        u = np.sqrt(r1h[:, b].astype(np.float32)).astype(np.float64)
        v = r2h[:, b].astype(np.float64)
        w = [1 - u, u * (1 - v), u * v]
        for t in range(3):
            np.add.at(exp[:, :, b].T, fp[t, fih[:, b], b], (w[t][None, :] * gout[:, :, b]).T)
    assert np.allclose(g, exp, rtol=1e-4, atol=1e-6)


def test_trimesh_chamfer(gpu_fx):
    """test/metrics.jl:86-90: chamfer_distance(m, m) ~ 0 (two independent samplings), atol 1e-2;
    config 3 shape: B=8 teapot-class meshes, 5000 samples."""
    fx = gpu_fx
    m = _teapot_sphere(fx)
    assert abs(float(fx.chamfer_distance(m, m))) < 1e-2
    t = os.path.join(GOLDEN, "teapot.obj")
    m8 = fx.gpu(fx.load_trimesh(*[t] * 8))
    l8 = float(fx.chamfer_distance(m8, m8, 5000, seed=11))
    assert 0 < l8 < 1e-2
    assert l8 == float(fx.chamfer_distance(m8, m8, 5000, seed=11))  # deterministic given the seed


# ------------------------------------------------------------------------------- fit_mesh objective
def test_offset_and_converters(gpu_fx):
    """offset(m, x) (src/transforms/mesh_func.jl:409-438) and the device packed<->padded converters
    (src/rep/utils.jl:119-181) against their host definitions."""
    fx = gpu_fx
    m = fx.gpu(_teapot_sphere(fx))
    v = m.get_verts_packed_host()
    off = _rand(v.shape, 3) * np.float32(0.01)
    m2 = fx.offset(m, off)
    assert np.array_equal(m2.get_verts_packed().to_host(), v + off)      # exact Float32 add
    assert np.array_equal(m.get_verts_packed().to_host(), v)              # original untouched (deepcopy semantics)
    pad = m2.get_verts_padded().to_host()
    from flux3d_jl_amd import rep
    assert np.array_equal(pad, rep._packed_to_padded(v + off, m._verts_len, 0))
    back = m2.padded_to_packed_dev(m2.get_verts_padded()).to_host()
    assert np.array_equal(back, v + off)
    assert np.isclose(fx.edge_loss(m2), fx.edge_loss(fx.TriMesh(rep._packed_to_list(v + off, m._verts_len), m.get_faces_list())), rtol=1e-6)
    with pytest.raises(ValueError):
        fx.offset(m, off[:, :-1])


def test_loss_dolphin_gradient(gpu_fx, oracle):
    """examples/fit_mesh.jl:78-84 objective: device gradient == the same chain composed from the oracle's
    adjoints (chamfer_bwd -> barycentric scatter -> padded->packed, laplacian/edge bwd)."""
    fx = gpu_fx
    src = fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "sphere.obj")))
    tgt = fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj")))
    x = fx.gpu(_rand((3, 2562), 5) * np.float32(0.02))
    n, seed = 3000, 77
    loss, g = fx.loss_dolphin(x, src, tgt, n, seed=seed, with_grad=True)
    assert loss == fx.loss_dolphin(x, src, tgt, n, seed=seed)  # deterministic given the seed
    # oracle chain
    m = fx.offset(src, x)
    vp = m.get_verts_padded_host()
    fp = m.get_faces_padded().astype(np.int64) - 1
    A, fa, r1, r2 = oracle.sample_points_seeded(vp, fp, m._faces_len, n, seed, return_draws=True)
    tp = tgt.get_verts_padded_host()
    Bp = oracle.sample_points_seeded(tp, tgt.get_faces_padded().astype(np.int64) - 1, tgt._faces_len, n, seed + 1)
    l1, ix, iy, _ = oracle.chamfer_distance(A, Bp, return_all=True)
    gA, _ = oracle.chamfer_bwd(A, Bp, ix, iy)
    u = np.sqrt(r1[:, 0]); w = [1 - u, u * (1 - r2[:, 0]), u * r2[:, 0]]
    g1 = np.zeros((2562, 3))
    for t in range(3):
        np.add.at(g1, fp[t, fa[:, 0], 0], (w[t][None, :] * gA[:, :, 0]).T)
    v = m.get_verts_packed_host()
    e0 = m.get_edges_packed().astype(np.int64) - 1
    rp, ci, va = m.get_laplacian_packed()
    g2 = oracle.laplacian_loss_bwd(v, rp.astype(np.int64), ci.astype(np.int64), va, 0.1)
    g3 = oracle.edge_loss_bwd(v, e0, 0.0, 1.0)
    ref = g1.T + g2 + g3
    l_ref = np.float32(np.float32(l1 + np.float32(0.1) * oracle.laplacian_loss(v, rp.astype(np.int64), ci.astype(np.int64), va))
                       + oracle.edge_loss(v, e0))
    assert np.isclose(loss, l_ref, rtol=1e-5)
    assert np.allclose(g.to_host(), ref, rtol=1e-3, atol=1e-7)
    # ... and bit for bit the ordered chain: both mesh-loss adjoints added in Float32, the sampling adjoint gathered on top of them
    g0 = np.asfortranarray((g2 + g3).astype(np.float32)).reshape((3, 2562, 1), order="F")
    ordered = oracle.sample_points_bwd(fp, m._faces_len, m.V, fa, r1, r2, gA, base=g0)
    assert np.array_equal(g.to_host(), ordered.reshape((3, 2562), order="F"))


def test_loss_dolphin_async_matches_sync(gpu_fx):
    """sync=False keeps the three loss terms and their sum on the device: same Float32 value, same gradient."""
    fx = gpu_fx
    src = fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "sphere.obj")))
    tgt = fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj")))
    x = fx.DeviceArray.zeros((3, src.get_verts_packed().shape[1]), np.float32)
    l0, g0 = fx.loss_dolphin(x, src, tgt, 2000, seed=11, with_grad=True)
    l1, g1 = fx.loss_dolphin(x, src, tgt, 2000, seed=11, with_grad=True, sync=False)
    assert np.float32(l1.item()) == l0
    # the scatter-adds of the two adjoints use float atomics: order-dependent in the last bit
    assert np.allclose(g0.to_host(), g1.to_host(), rtol=1e-4, atol=1e-8)
    # offset() shares the topology caches: the Laplacian is built once for all derived meshes
    assert fx.offset(src, x)._topo is src._topo and src._topo.get("laplacian_packed") is not None


def test_fit_mesh_loop_decreases_loss(gpu_fx):
    """A short run of the tutorial's optimisation (examples/fit_mesh.jl:99-110) entirely on the device."""
    fx = gpu_fx
    src = fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "sphere.obj")))
    tv, tf = fx.load_obj(os.path.join(GOLDEN, "teapot.obj"))
    tv = (tv - tv.mean(1, keepdims=True)) / tv.std()        # the tutorial normalises both meshes
    tgt = fx.gpu(fx.TriMesh([np.asfortranarray(tv.astype(np.float32))], [tf]))
    x = fx.DeviceArray.zeros((3, 2562), np.float32)
    opt = fx.Momentum(1.0, 0.9)
    first = last = None
    for it in range(60):
        loss, g = fx.loss_dolphin(x, src, tgt, 5000, seed=1000 + 2 * it, with_grad=True)
        opt.update(x, g)
        first = loss if first is None else first
        last = loss
    assert np.isfinite(last) and last < 0.5 * first, (first, last)


def test_fit_step_graph_matches_eager_loop(gpu_fx):
    """The hipGraph recording of one fit_mesh iteration replays to the same trajectory as the eager loop: same
    samples (seed + 2 per iteration through the device counter), same losses, same offsets; the cached target CDF and the
    single-mesh packed/padded alias are on this path.  (The default path is the ordered one and has no float atomics:
    tests/test_gpu_fit_chain.py holds both loops to the host chain bit for bit; the tolerances here are those of the atomic form,
    FitStepGraph(ordered=False).)"""
    fx = gpu_fx
    tv, tf = fx.load_obj(os.path.join(GOLDEN, "teapot.obj"))
    tv = (tv - tv.mean(1, keepdims=True)) / tv.std()
    iters, seed = 8, 4242

    def fresh():
        src = fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "sphere.obj")))
        tgt = fx.gpu(fx.TriMesh([np.asfortranarray(tv.astype(np.float32))], [tf]))
        return src, tgt, fx.DeviceArray.zeros((3, 2562), np.float32), fx.Momentum(1.0, 0.9)

    src, tgt, x0, opt0 = fresh()
    eager = []
    for it in range(iters):
        loss, g = fx.loss_dolphin(x0, src, tgt, 5000, seed=seed + 2 * it, with_grad=True, sync=False)
        opt0.update(x0, g)
        eager.append(float(loss.item()))
    src, tgt, x1, opt1 = fresh()
    step = fx.FitStepGraph(x1, src, tgt, opt1, 5000, seed=seed)
    step.synchronize()
    graph = [float(step.first_loss.item())]
    for it in range(1, iters):
        loss = step.step()
        step.synchronize()
        graph.append(float(loss.item()))
    assert np.allclose(graph, eager, rtol=2e-4), (graph, eager)
    assert graph[-1] < graph[0]
    assert np.allclose(x1.to_host(), x0.to_host(), rtol=1e-3, atol=1e-5)
    # the target's CDF was computed once and kept with its vertex mirrors; replacing the vertices drops it
    assert any(isinstance(k, tuple) and k[0] == "face_cdf" for k in tgt._dev)
    tgt.set_verts_packed(tgt.get_verts_packed().clone())
    assert not any(isinstance(k, tuple) and k[0] == "face_cdf" for k in tgt._dev)


def test_fit_step_graph_beyond_the_ordered_adjoints_capacity(gpu_fx):
    """More draws than the ordered sampling adjoint stages in one CU's LDS (7000 on the 5120-face sphere): FitStepGraph takes the
    float-atomic scatter and a separate optimiser launch by itself, the ordered form stays the default where it fits; both descend."""
    fx = gpu_fx
    tv, tf = fx.load_obj(os.path.join(GOLDEN, "teapot.obj"))
    tv = tv - tv.mean(1, keepdims=True)
    tv = np.asfortranarray((tv / np.abs(tv).max()).astype(np.float32))
    for n in (7000, 3000):
        src = fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "sphere.obj")))
        tgt = fx.gpu(fx.TriMesh([tv], [tf]))
        assert fx.sampling_adjoint_is_ordered(src, n) == (n == 3000)
        x = fx.DeviceArray.zeros((3, src.V), np.float32)
        step = fx.FitStepGraph(x, src, tgt, fx.Momentum(1.0, 0.9), num_samples=n, seed=11)
        first = float(step.first_loss.item())
        for _ in range(30):
            step.step()
        step.synchronize()
        last = float(step.loss.item())
        assert np.isfinite(last) and last < first, (n, first, last)


def test_chamfer_sampled_adjoint_in_one_launch(gpu_fx, oracle):
    """fx3d_chamfer_sampled_bwd = fx3d_chamfer_bwd followed by fx3d_sample_points_bwd (the pullback of
    chamfer_distance(m1::TriMesh, m2::TriMesh, n), src/metrics/mesh.jl:34-44): both meshes, one mesh only, added onto an
    existing buffer; ragged batch.  (Float atomics on both paths: equal up to their order.)"""
    fx = gpu_fx
    ma, mb = fx.gpu(_teapot_sphere(fx)), fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "sphere.obj"), os.path.join(GOLDEN, "teapot.obj")))
    n = 3000
    A, fa, ra1, ra2 = fx.sample_points(ma, n, seed=11, return_draws=True)
    Bp, fb, rb1, rb2 = fx.sample_points(mb, n, seed=12, return_draws=True)
    loss, ix, iy = fx.chamfer_distance(A, Bp, w1=0.7, w2=1.3, return_indices=True)
    gA, gB = fx.chamfer_distance_grad(A, Bp, ix, iy, w1=0.7, w2=1.3, gout=2.0)
    ref_a = fx.sample_points_grad(ma, fa, ra1, ra2, gA).to_host()
    ref_b = fx.sample_points_grad(mb, fb, rb1, rb2, gB).to_host()
    # against the oracle's chain as well
    oga, ogb = oracle.chamfer_bwd(A.to_host(), Bp.to_host(), ix.to_host(), iy.to_host(), 0.7, 1.3, 2.0)
    assert np.allclose(gA.to_host(), oga, rtol=1e-5, atol=1e-9)
    ga, gb = fx.chamfer_sampled_grad(A, Bp, ix, iy, ma, (fa, ra1, ra2), mb, (fb, rb1, rb2), w1=0.7, w2=1.3, gout=2.0)
    assert np.allclose(ga.to_host(), ref_a, rtol=2e-4, atol=1e-8) and np.allclose(gb.to_host(), ref_b, rtol=2e-4, atol=1e-8)
    ga1, none = fx.chamfer_sampled_grad(A, Bp, ix, iy, mesh_a=ma, draws_a=(fa, ra1, ra2), w1=0.7, w2=1.3, gout=2.0)
    assert none is None and np.allclose(ga1.to_host(), ref_a, rtol=2e-4, atol=1e-8)
    base = fx.gpu(np.asfortranarray(np.full(ref_b.shape, 0.25, np.float32)))
    _, gb2 = fx.chamfer_sampled_grad(A, Bp, ix, iy, mesh_b=mb, draws_b=(fb, rb1, rb2), w1=0.7, w2=1.3, gout=2.0, out_b=base)
    assert gb2 is base and np.allclose(base.to_host(), ref_b + 0.25, rtol=2e-4, atol=1e-7)


def test_graph_capture_with_a_forked_stream_releases_without_synchronising(gpu_fx):
    """A capture that forks onto a second stream (ordering-only events) and releases an array allocated under that
    stream while the origin stream is current: the pool must not synchronise (a synchronised capturing stream
    invalidates the capture) -- the block is parked with the graph's pool; the recording replays correctly."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    s1, s2 = fx.Stream.create(), fx.Stream.create()
    a = fx.gpu(np.asfortranarray(np.arange(12, dtype=np.float32).reshape(3, 4)))
    b = fx.gpu(np.asfortranarray(np.ones((3, 4), np.float32)))
    out = fx.DeviceArray.zeros((3, 4), np.float32)
    fx.synchronize()
    g = fx.Graph()
    with g.capture(s1):
        e0, e1 = fx.Event(timing=False), fx.Event(timing=False)
        e0.record(s1)
        _lib.call("fx3d_stream_wait_event", s2.handle, e0.handle)
        with fx.stream(s2):
            t = fx.lincomb(2.0, a, 1.0, b)          # allocated under s2
            e1.record(s2)
        _lib.call("fx3d_stream_wait_event", s1.handle, e1.handle)
        fx.lincomb(1.0, t, 3.0, b, out=out)         # consumed on s1
        del t                                        # released while s1 is current: no synchronisation inside a capture
    for _ in range(3):
        g.launch()
    s1.synchronize()
    assert np.array_equal(out.to_host(), 2.0 * a.to_host() + 4.0)


def test_knn_scratch_paths_replay_in_a_graph(gpu_fx, oracle):
    """The multi-kernel kNN paths of fx3d_knn_ws -- pre-pass + search, candidate slices + merge, interleave + slices + verified
    merge + selection fallback -- recorded into a hipGraph after one eager call (workspaces and kernel attributes in place) and
    replayed: the same neighbour lists as the oracle, replay after replay (the pre-pass meeting words, the flags and the slice
    lists live in the scratch the recording owns)."""
    fx = gpu_fx
    rng = np.random.default_rng(41)
    cases = [(np.asfortranarray(rng.standard_normal((64, 512, 3)).astype(np.float32)), 20),    # pre-pass
             (np.asfortranarray(rng.standard_normal((32, 2048, 1)).astype(np.float32)), 12),   # candidate slices
             (np.asfortranarray(rng.standard_normal((16, 512, 2)).astype(np.float32)), 40),    # verified merge
             (np.asfortranarray(rng.random((3, 700, 2), dtype=np.float32)), 40)]               # compact D = 3 geometry
    s = fx.Stream.create()
    with fx.stream(s):
        devs = [fx.gpu(x) for x, _ in cases]
        outs = [fx.DeviceArray.empty((k, x.shape[1], x.shape[2]), np.int32) for x, k in cases]

        from flux3d_jl_amd import _lib

        def step():
            for d, (x, k), o in zip(devs, cases, outs):
                idx = fx.knn(d, k, drop_first=True, return_dist=False)
                _lib.call("fx3d_memcpy_d2d", o.ptr, idx.ptr, o.nbytes, s.handle)

        step()
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            step()
        for _ in range(3):
            for o in outs:
                _lib.call("fx3d_memset", o.ptr, 0, o.nbytes, s.handle)
            g.launch()
            s.synchronize()
            for (x, k), o in zip(cases, outs):
                assert np.array_equal(o.to_host(), oracle.knn(x, k, drop_first=True, want_dist=False))


# ------------------------------------------------------------------- widened rows: EdgeConv features, voxels
@pytest.mark.parametrize("F,N,B,K", [(3, 256, 3, 10), (64, 128, 2, 20), (6, 70, 2, 5)])
def test_edge_features_parity(gpu_fx, oracle, F, N, B, K):
    """cat(X, KNNGraph - X) in both layouts (src/models/dgcnn.jl:36-51), bit-exact, + the @nograd adjoint."""
    rng = np.random.default_rng(F * 7 + N)
    x = np.asfortranarray(rng.standard_normal((F, N, B)).astype(np.float32))
    dx = gpu_fx.gpu(x)
    idx = gpu_fx.knn(dx, K, drop_first=True, return_dist=False)
    oi = oracle.knn(x, K, drop_first=True, want_dist=False)
    assert np.array_equal(idx.to_host(), oi)
    for layout, lay in (("cat", 0), ("mlp", 1)):
        got = gpu_fx.edge_features(dx, idx, layout=layout).to_host()
        exp = oracle.edge_features(x, oi, layout=lay)
        assert got.shape == exp.shape and np.array_equal(got, exp)
        out, idx2 = gpu_fx.edgeconv_graph(dx, K, layout=layout, return_idx=True)
        assert np.array_equal(idx2.to_host(), oi) and np.array_equal(out.to_host(), exp)
        g = np.asfortranarray(rng.standard_normal(exp.shape).astype(np.float32))
        gx = gpu_fx.edge_features_grad(gpu_fx.gpu(g), F, N, B, K, layout=layout).to_host()
        assert np.array_equal(gx, oracle.edge_features_bwd(g, F, N, B, K, layout=lay))


@pytest.mark.parametrize("N,B,K,kind", [(1024, 3, 20, "uniform"), (200, 2, 10, "uniform"), (333, 2, 7, "lattice"),
                                         (96, 1, 31, "uniform"), (300, 2, 12, "outlier"), (70, 2, 4, "same"),
                                         (1024, 2, 40, "uniform"), (333, 2, 33, "lattice"), (200, 1, 63, "uniform"), (160, 1, 38, "same")])
def test_edgeconv_graph_fused_first_layer(gpu_fx, oracle, N, B, K, kind, fx_option):
    """F = 3: fx3d_edgeconv_graph runs the neighbour search and cat(X, KNN - X) in ONE kernel.  Vector and scalar
    rank stores (K % 4), distance ties re-ranked by the wave (lattice), lists overflowing into the exact fallback
    (outlier / identical points): indices and features bit-identical to the oracle and to the two-kernel path."""
    rng = np.random.default_rng(N * 3 + K)
    x = rng.random((3, N, B), dtype=np.float32)
    if kind == "lattice":
        x = np.round(x * 4) / 4
    elif kind == "outlier":
        x = (x * 1e-3).astype(np.float32)
        x[:, 5, :] = 1.0e6
    elif kind == "same":
        x[:] = 0.25
    x = np.asfortranarray(x.astype(np.float32))
    dx = gpu_fx.gpu(x)
    oi = oracle.knn(x, K, drop_first=True, want_dist=False)
    for layout, lay in (("cat", 0), ("mlp", 1)):
        exp = oracle.edge_features(x, oi, layout=lay)
        out, idx = gpu_fx.edgeconv_graph(dx, K, layout=layout, return_idx=True)
        assert np.array_equal(idx.to_host(), oi) and np.array_equal(out.to_host(), exp)
    fx_option("edgeconv_unfused", "1")
    out2, idx2 = gpu_fx.edgeconv_graph(dx, K, layout="mlp", return_idx=True)
    assert np.array_equal(idx2.to_host(), oi) and np.array_equal(out2.to_host(), exp)


@pytest.mark.parametrize("res,N,B", [(16, 300, 2), (32, 1024, 2), (8, 5, 1)])
def test_pointcloud_to_voxel_parity(gpu_fx, oracle, res, N, B):
    """Occupancy grid of pointcloud_to_voxel (src/conversions.jl:91-131): identical to the oracle's
    brute-force Float64 restatement although the kernel scatters from the points."""
    rng = np.random.default_rng(res + N)
    p = np.asfortranarray((rng.random((3, N, B), dtype=np.float32) * 5 - 2).astype(np.float32))
    vox = gpu_fx.pointcloud_to_voxel(gpu_fx.PointCloud(p), res).to_host()
    exp = oracle.pointcloud_to_voxel(p, res)
    assert vox.shape == (res, res, res, B)
    assert np.array_equal(vox, exp)
    assert 0 < exp.sum() < exp.size


def test_pointcloud_to_voxel_sphere_and_degenerate(gpu_fx, oracle):
    """The reference's own conversion input (test/conversions.jl:8-38: a sphere mesh's vertices) and a
    cloud with zero extent (division by zero -> no voxel set, like the reference's NaN distances)."""
    m = gpu_fx.load_trimesh(os.path.join(GOLDEN, "sphere.obj"))
    p = np.asfortranarray(m.get_verts_packed_host().reshape(3, -1, 1, order="F"))
    vox = gpu_fx.pointcloud_to_voxel(p, 32).to_host()
    assert np.array_equal(vox, oracle.pointcloud_to_voxel(p, 32)) and vox.sum() > 0
    flat = np.ones((3, 16, 1), np.float32, order="F")
    assert gpu_fx.pointcloud_to_voxel(flat, 8).to_host().sum() == 0
    assert oracle.pointcloud_to_voxel(flat, 8).sum() == 0


@pytest.mark.parametrize("N", [2, 85, 86, 257])
def test_pointcloud_to_voxel_range_with_signed_zeros(gpu_fx, oracle, N):
    """The minimum of each cloud is -0.0 and +0.0 occurs too (point 0 is (-0, +0, -0) in one cloud and (+0, -0, +0) in the other;
    the last coordinate of a longer cloud is a zero as well), with 3N either side of the range block's 256 threads and of 768:
    whichever zero the reduction returns, the grid is the oracle's.  (A point with a zero coordinate marks no voxel: the lattice
    starts at 1.5 / res.)"""
    rng = np.random.default_rng(8000 + N)
    p = np.asfortranarray(rng.random((3, N, 2), dtype=np.float32) * 3)
    p[:, 0, 0] = np.array([-0.0, 0.0, -0.0], np.float32)
    p[:, 0, 1] = np.array([0.0, -0.0, 0.0], np.float32)
    if N > 2:
        p[2, N - 1, :] = np.array([0.0, -0.0], np.float32)
    assert p.min() == 0 and np.signbit(p).sum() == (3 if N == 2 else 4)
    vox = gpu_fx.pointcloud_to_voxel(gpu_fx.PointCloud(p), 8).to_host()
    exp = oracle.pointcloud_to_voxel(p, 8)
    assert np.array_equal(vox, exp) and 0 < exp.sum() < exp.size


# ------------------------------------------------------------------------------ randomised shape sweeps
def _sweep_cases(seed, count, lo, hi):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(lo, hi)), int(rng.integers(lo, hi)), int(rng.integers(1, 4)), int(rng.integers(0, 1 << 30)))
            for _ in range(count)]


@pytest.mark.parametrize("N,M,B,seed", _sweep_cases(101, 12, 1, 3000))
def test_chamfer_random_shapes(gpu_fx, oracle, N, M, B, seed):
    """Ragged N != M (1 .. 3000: below one tile, across the 512-query pass and 4096-candidate chunk logic),
    clustered + uniform points: indices bit-exact, loss within 1e-5 relative."""
    rng = np.random.default_rng(seed)
    x = rng.random((3, N, B), dtype=np.float32)
    y = rng.random((3, M, B), dtype=np.float32)
    if seed & 1:  # half of the cases: a tight cluster far from the rest (stresses the centring / scaling)
        y[:, : M // 2, :] = y[:, : M // 2, :] * np.float32(1e-3) + np.float32(7.0)
    x, y = np.asfortranarray(x), np.asfortranarray(y)
    _check_nn(gpu_fx, oracle, x, y)
    _check_chamfer(gpu_fx, oracle, x, y, w1=0.5, w2=2.0)


@pytest.mark.parametrize("N,M,B,seed", _sweep_cases(202, 10, 33, 2600))
def test_knn_random_shapes(gpu_fx, oracle, N, M, B, seed):
    """kNN with y != x over ragged shapes, D = 3 (matrix-core filter for M >= 64, wave kernel below) and a
    random feature dimension: (index, distance) lists bit-exact."""
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, min(31, M - 1)))
    drop = bool(seed & 2)
    x = np.asfortranarray(rng.random((3, N, B), dtype=np.float32))
    y = np.asfortranarray(rng.random((3, M, B), dtype=np.float32))
    idx, dist = gpu_fx.knn(x, k, y=y, drop_first=drop)
    oi, od = oracle.knn(x, k, y=y, drop_first=drop)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)
    D = int(rng.integers(4, 100))
    n2, m2 = min(N, 300), min(M, 700)
    xf = np.asfortranarray(rng.standard_normal((D, n2, B)).astype(np.float32))
    yf = np.asfortranarray(rng.standard_normal((D, m2, B)).astype(np.float32))
    k2 = min(k, m2 - 1)
    idx, dist = gpu_fx.knn(xf, k2, y=yf, drop_first=drop)
    oi, od = oracle.knn(xf, k2, y=yf, drop_first=drop)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


def test_knn_d3_degenerate_inputs(gpu_fx, oracle):
    """D = 3 matrix-core path on inputs that defeat the filter: exact ties everywhere (lattice), all points equal,
    a query far outside the candidates' fp16 range, and NaN-free huge coordinates."""
    rng = np.random.default_rng(9)
    lat = np.asfortranarray(rng.integers(0, 5, (3, 400, 2)).astype(np.float32))
    for x, y, k, drop in ((lat, None, 12, True),
                          (np.full((3, 96, 1), 0.25, np.float32, order="F"), None, 20, False),
                          (np.asfortranarray(rng.random((3, 64, 1), dtype=np.float32) * np.float32(1e9)),
                           np.asfortranarray(rng.random((3, 128, 1), dtype=np.float32)), 7, False),
                          (np.asfortranarray(rng.random((3, 200, 1), dtype=np.float32) * np.float32(3e18)), None, 9, True)):
        idx, dist = gpu_fx.knn(x, k, y=y, drop_first=drop)
        oi, od = oracle.knn(x, k, y=y, drop_first=drop)
        assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


def _random_mesh_batch(rng, nmesh):
    """Ragged batch of random triangle soups with shared vertices (1-based UInt32 faces like the reference),
    including thin and zero-area triangles."""
    vl, fl = [], []
    for _ in range(nmesh):
        V = int(rng.integers(4, 400))
        F = int(rng.integers(2, 900))
        v = rng.standard_normal((3, V)).astype(np.float32) * np.float32(rng.choice([1e-3, 1.0, 50.0]))
        f = np.stack([rng.choice(V, 3, replace=False) for _ in range(F)], axis=1).astype(np.uint32) + 1
        if F > 4:
            v[:, f[1, 0] - 1] = v[:, f[0, 0] - 1]  # one degenerate (zero-area) face
        vl.append(np.asfortranarray(v))
        fl.append(np.asfortranarray(f))
    return vl, fl


@pytest.mark.parametrize("seed", [3, 14, 159, 2653])
def test_mesh_ops_random_batches(gpu_fx, oracle, seed):
    """Areas, both mesh losses with gradients, explicit and seeded sampling on random ragged batches."""
    fx = gpu_fx
    rng = np.random.default_rng(seed)
    vl, fl = _random_mesh_batch(rng, int(rng.integers(1, 5)))
    m = fx.gpu(fx.TriMesh(vl, fl))
    v = m.get_verts_packed_host()
    f0 = m.get_faces_packed().astype(np.int64) - 1
    assert np.array_equal(fx.compute_faces_areas_packed(m).to_host().ravel(), oracle.faces_areas_packed(v, f0))
    e0 = m.get_edges_packed().astype(np.int64) - 1
    assert np.array_equal(e0, oracle.edges_packed(f0, v.shape[1]))
    rowptr, colind, vals = m.get_laplacian_packed()
    r64, c64 = rowptr.astype(np.int64), colind.astype(np.int64)
    assert np.isclose(fx.laplacian_loss(m), oracle.laplacian_loss(v, r64, c64, vals), rtol=LOSS_RTOL, atol=1e-30)
    assert np.isclose(fx.edge_loss(m, 0.1), oracle.edge_loss(v, e0, 0.1), rtol=LOSS_RTOL, atol=1e-30)
    gl, ol = fx.laplacian_loss_grad(m, 0.7).to_host(), oracle.laplacian_loss_bwd(v, r64, c64, vals, 0.7)
    assert np.allclose(gl, ol, rtol=2e-4, atol=1e-7 * max(1.0, float(np.abs(ol).max())))
    ge, oe = fx.edge_loss_grad(m, 0.1, 1.3).to_host(), oracle.edge_loss_bwd(v, e0, 0.1, 1.3)
    assert np.allclose(ge, oe, rtol=2e-4, atol=1e-7 * max(1.0, float(np.abs(oe).max())))
    n = int(rng.integers(1, 700))
    out, fi, r1, r2 = fx.sample_points(m, n, seed=seed, return_draws=True)
    eo, efi, er1, er2 = oracle.sample_points_seeded(m.get_verts_padded_host(), m.get_faces_padded().astype(np.int64) - 1,
                                                    m._faces_len, n, seed, return_draws=True)
    assert np.array_equal(fi.to_host(), efi) and np.array_equal(r1.to_host(), er1) and np.array_equal(r2.to_host(), er2)
    assert np.array_equal(out.to_host(), eo)
    assert (fi.to_host() < np.asarray(m._faces_len)[None, :]).all()  # never a padding face


@pytest.mark.parametrize("seed", [5, 50])
def test_voxel_and_edge_features_random(gpu_fx, oracle, seed):
    rng = np.random.default_rng(seed)
    N, B, res = int(rng.integers(2, 900)), int(rng.integers(1, 4)), int(rng.choice([4, 9, 20]))
    p = np.asfortranarray((rng.standard_normal((3, N, B)) * rng.choice([1e-2, 1.0, 1e3])).astype(np.float32))
    assert np.array_equal(gpu_fx.pointcloud_to_voxel(p, res).to_host(), oracle.pointcloud_to_voxel(p, res))
    F, n2, K = int(rng.integers(1, 40)), int(rng.integers(40, 300)), int(rng.integers(1, 20))
    x = np.asfortranarray(rng.standard_normal((F, n2, B)).astype(np.float32))
    oi = oracle.knn(x, K, drop_first=True, want_dist=False)
    for layout, lay in (("cat", 0), ("mlp", 1)):
        out, idx = gpu_fx.edgeconv_graph(x, K, layout=layout, return_idx=True)
        assert np.array_equal(idx.to_host(), oi)
        assert np.array_equal(out.to_host(), oracle.edge_features(x, oi, layout=lay))


@pytest.mark.parametrize("D", [3, 64])
def test_c4_full_size_knn_properties(gpu_fx, oracle, D):
    """BASELINE config 4 at full size (k = 20 self-graph on B = 32 clouds of 1024 points; D = 3 and the second
    EdgeConv's D = 64): oracle parity on a few batch elements, size-independent properties on all of them."""
    fx = gpu_fx
    if D == 3:
        x = fx.synth.uniform_cloud(0x5EED0004, 3, 1024, 32)
    else:
        x = np.asfortranarray(np.random.default_rng(1).standard_normal((D, 1024, 32)).astype(np.float32))
    idx, dist = fx.knn(x, 20, drop_first=True)
    gi, gd = idx.to_host(), dist.to_host()
    for b in (0, 17, 31):
        oi, od = oracle.knn(x[:, :, b:b + 1], 20, drop_first=True)
        assert np.array_equal(gi[:, :, b], oi[:, :, 0]) and np.array_equal(gd[:, :, b], od[:, :, 0])
    assert (np.diff(gd, axis=0) >= 0).all()                       # ascending distances
    assert (gi != np.arange(1024)[None, :, None]).all()           # self dropped
    assert gi.min() >= 0 and gi.max() < 1024
    srt = np.sort(gi, axis=0)
    assert (np.diff(srt, axis=0) > 0).all()                       # no neighbour twice
    # the recorded distance is the oracle-arithmetic distance of the recorded neighbour
    b, n = 5, np.arange(0, 1024, 97)
    for q in n:
        c = x[:, gi[:, q, b], b]
        d = np.zeros(20, np.float32)
        for dd in range(D):
            t = (x[dd, q, b] - c[dd]).astype(np.float32)
            d = (d + t * t).astype(np.float32)
        assert np.array_equal(d, gd[:, q, b])
    # idempotence
    idx2, dist2 = fx.knn(x, 20, drop_first=True)
    assert np.array_equal(idx2.to_host(), gi) and np.array_equal(dist2.to_host(), gd)


@pytest.mark.parametrize("N,M,B", [(4096, 1024, 32), (1024, 4096, 9), (513, 4000, 2), (3000, 1000, 5), (4096, 64, 3)])
def test_chamfer_clouds_of_different_sizes(gpu_fx, oracle, N, M, B):
    """One-chunk clouds of different sizes: the launch plan picks the query passes per block per DIRECTION (the direction
    whose candidates are the large cloud gets more, lighter blocks).  Indices and loss against the oracle."""
    x, y = _rand((3, N, B), N + 3), _rand((3, M, B), M + 4)
    _check_nn(gpu_fx, oracle, x, y)
    _check_chamfer(gpu_fx, oracle, x, y)


@pytest.mark.parametrize("N,M,B", [(9000, 12000, 1), (5000, 5000, 8), (16384, 700, 2)])
def test_chamfer_split_plans(gpu_fx, oracle, N, M, B):
    """Few large clouds: the launch plan splits the candidates into balanced chunks taken by different blocks
    (each stores its per-query row; the unpack kernel takes the 64-bit minimum over the chunk subsets) and runs several query passes per block; fx3d_nn1 (no scratch) takes
    the serial plan.  Both against the oracle."""
    x, y = _rand((3, N, B), N), _rand((3, M, B), M + 1)
    _check_nn(gpu_fx, oracle, x, y)           # fx3d_nn1: serial chunks
    _check_chamfer(gpu_fx, oracle, x, y)      # fx3d_chamfer_fwd: split run


def test_deferred_sharded_chamfer_single_rank(gpu_fx, oracle):
    """DeferredShardedChamfer (one collective per group of evaluations, RCCL behind the C ABI) at world size 1:
    every evaluation's loss equals the direct call, across group boundaries and a shape change."""
    fx = gpu_fx
    from flux3d_jl_amd.distributed import DeferredShardedChamfer, NativeComm
    comm = NativeComm(0, 1)
    d = DeferredShardedChamfer(comm=comm, group=3)
    clouds = [(_rand((3, 300 + 10 * i, 2), i), _rand((3, 200, 2), 50 + i)) for i in range(5)]
    got = []
    for i, (x, y) in enumerate(clouds):
        d(fx.gpu(x), fx.gpu(y), 2, 0.5, 2.0)
        if d.k == 0:  # a flush just happened (group full, or shape change flushed the previous ones first)
            got.extend(d.losses.to_host()[: d.last_count].tolist())
        elif i > 0 and clouds[i][0].shape != clouds[i - 1][0].shape and d.last_count and len(got) < i:
            got.extend(d.losses.to_host()[: d.last_count].tolist())
    if d.flush():
        got.extend(d.losses.to_host()[: d.last_count].tolist())
    exp = [float(fx.chamfer_distance(x, y, w1=0.5, w2=2.0)) for x, y in clouds]
    assert len(got) == len(exp) and np.allclose(got, exp, rtol=1e-6, atol=0)


@pytest.mark.parametrize("D", [3, 64])
def test_knn_outlier_dynamic_range(gpu_fx, oracle, D):
    """One far outlier sets the fp16 filter's scale, so a tight cluster collapses below its resolution: the band
    admits the whole cluster, the lists overflow and the exact fallback has to deliver the oracle's lists."""
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((D, 300, 1)) * 1e-3).astype(np.float32)
    x[:, 7, 0] = 1.0e6
    x[:, 123, 0] = -3.0e5
    x = np.asfortranarray(x)
    idx, dist = gpu_fx.knn(x, 12, drop_first=True)
    oi, od = oracle.knn(x, 12, drop_first=True)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)
    # and the 1-NN / chamfer path on the same cloud against a shifted copy
    if D == 3:
        y = np.asfortranarray(x + np.float32(1e-4))
        _check_nn(gpu_fx, oracle, x, y)


def test_knn_d3_multi_chunk(gpu_fx, oracle):
    """More candidates than one LDS image (3328): phase A and phase B restage the chunks, the group minima and the
    lane lists run across them."""
    rng = np.random.default_rng(31)
    x = np.asfortranarray(rng.random((3, 333, 2), dtype=np.float32))
    y = np.asfortranarray(rng.random((3, 7777, 2), dtype=np.float32))
    idx, dist = gpu_fx.knn(x, 20, y=y)
    oi, od = oracle.knn(x, 20, y=y)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


@pytest.mark.parametrize("M,k,drop", [(64, 32, False), (64, 31, True), (96, 5, False), (192, 17, True), (200, 32, False),
                                      (1000, 1, False), (3072 + 64 * 3 + 5, 30, True), (6500, 8, False)])
def test_knn_d3_wave_split_cases(gpu_fx, oracle, M, k, drop):
    """The D = 3 kernel splits a query group's tiles over two waves and ranks with four lanes per query: odd and
    single tile pairs (one wave has nothing to do), k + drop at the 32-value limit of the threshold selection,
    k not a multiple of four (scalar output path), exact ties across the four lanes' shares."""
    rng = np.random.default_rng(M * 37 + k)
    x = np.asfortranarray(rng.random((3, 150, 3), dtype=np.float32))
    y = np.asfortranarray(rng.random((3, M, 3), dtype=np.float32))
    x[:, :40, :] = np.round(x[:, :40, :] * 4) / 4  # lattice queries against ...
    y[:, : M // 2, :] = np.round(y[:, : M // 2, :] * 4) / 4  # ... lattice candidates: duplicates and exact distance ties
    idx, dist = gpu_fx.knn(x, k, y=y, drop_first=drop)
    oi, od = oracle.knn(x, k, y=y, drop_first=drop)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


@pytest.mark.parametrize("M,k,drop,kind", [(128, 33, False, "uniform"), (128, 64, False, "uniform"), (129, 63, True, "uniform"),
                                           (200, 40, True, "lattice"), (1024, 40, True, "uniform"), (1024, 64, False, "uniform"),
                                           (1024, 47, False, "lattice"), (3072 + 64 * 3 + 5, 50, True, "uniform"), (7777, 33, False, "uniform"),
                                           (640, 64, False, "equal"), (640, 63, True, "clusters"), (2100, 36, True, "uniform")])
def test_knn_d3_wide_selection(gpu_fx, oracle, M, k, drop, kind):
    """32 < k + drop <= 64 at D = 3 on the matrix-core kernel (round 3: the wide geometry -- 64 queries per block, 128 keys per
    query, tau = the larger of the two waves' ceil(kk/2)-th group minimum): the smallest cloud it takes (two pairs of tiles), odd
    tile counts, several LDS images, k not a multiple of four, exact ties (lattice: the tie re-rank with up to 128 keys), all
    points equal and tight clusters (medium path / exact merge with kk = 64: the FULL64 fallback)."""
    rng = np.random.default_rng(M * 131 + k)
    x = rng.random((3, 150, 3), dtype=np.float32)
    y = rng.random((3, M, 3), dtype=np.float32)
    if kind == "lattice":
        x[:, :60, :] = np.round(x[:, :60, :] * 4) / 4
        y[:, : 2 * M // 3, :] = np.round(y[:, : 2 * M // 3, :] * 4) / 4
    elif kind == "equal":
        y[:] = np.float32(0.25)
    elif kind == "clusters":
        c = rng.random((3, 8, 3), dtype=np.float32)
        y = c[:, rng.integers(0, 8, M), :] + rng.standard_normal((3, M, 3)).astype(np.float32) * np.float32(1e-4)
        y = np.ascontiguousarray(y.astype(np.float32))
    x, y = np.asfortranarray(x), np.asfortranarray(y)
    idx, dist = gpu_fx.knn(x, k, y=y, drop_first=drop)
    oi, od = oracle.knn(x, k, y=y, drop_first=drop)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


@pytest.mark.parametrize("M,k,drop", [(1024, 40, True), (1472, 47, False), (1473, 47, True), (130, 33, False), (1024, 48, True),
                                      (3000, 40, True), (5000, 43, True), (5000, 47, False), (4096, 47, True)])
def test_knn_d3_compact_geometry(gpu_fx, oracle, M, k, drop):
    """32 < k + drop <= 48 runs the compact geometry (two blocks per CU, raw coordinates from L2, no medium path; clouds beyond 1472
    candidates pass through its LDS image in chunks; k + drop > 44 on clouds beyond 4096 stays on the wide one): bit-identical to
    the oracle on both sides of the chunk limit, of k + drop = 44 / 48 and of M = 4096."""
    rng = np.random.default_rng(M + k)
    x = np.asfortranarray(rng.random((3, 200, 2), dtype=np.float32))
    y = rng.random((3, M, 2), dtype=np.float32)
    y[:, ::5, :] = np.round(y[:, ::5, :] * 8) / 8
    y = np.asfortranarray(y)
    oi, od = oracle.knn(x, k, y=y, drop_first=drop)
    idx, dist = gpu_fx.knn(x, k, y=y, drop_first=drop)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


def test_knn_d3_wide_selection_full_shape(gpu_fx, oracle):
    """C4's shape with k = 40 (the segmentation networks' neighbourhood): sampled queries against the oracle."""
    rng = np.random.default_rng(77)
    x = np.asfortranarray(rng.standard_normal((3, 1024, 32)).astype(np.float32))
    idx, dist = gpu_fx.knn(x, 40, drop_first=True)
    for b in (0, 17, 31):
        oi, od = oracle.knn(np.asfortranarray(x[:, :, b:b + 1]), 40, drop_first=True)
        assert np.array_equal(idx.to_host()[:, :, b:b + 1], oi) and np.array_equal(dist.to_host()[:, :, b:b + 1], od)


@pytest.mark.parametrize("D,N,M,B,k,drop,slices", [(64, 300, 2048, 1, 20, True, 0), (64, 257, 4096, 2, 7, False, 2), (16, 200, 4096, 1, 31, True, 8),
                                                    (3, 500, 8192, 1, 20, True, 0), (3, 300, 4096, 2, 40, False, 2), (3, 129, 8192, 1, 63, True, 4),
                                                    (32, 130, 2048, 3, 12, False, 4), (64, 100, 1536, 1, 20, True, 2), (20, 150, 2048, 1, 9, True, 0)])
def test_knn_candidate_slices(gpu_fx, oracle, fx_option, D, N, M, B, k, drop, slices):
    """fx3d_knn_ws on few clouds with many rows: the search runs on S slices of every cloud as B x S virtual clouds, one wave per
    query merges the slices' lists (round 3).  Forced and automatic slice counts, both matrix-core kernels (and the wide D = 3
    geometry), cross sets with exact ties across slice borders (lattice candidates: equal distances in different slices must come
    out in index order), drop_first handled by the merge: bit-identical to the oracle and to the unsliced call."""
    rng = np.random.default_rng(D * 1000 + M + k)
    x = rng.standard_normal((D, N, B)).astype(np.float32)
    y = rng.standard_normal((D, M, B)).astype(np.float32)
    y[:, ::3, :] = np.round(y[:, ::3, :] * 2) / 2          # ties across the whole cloud
    x[:, : N // 2, :] = y[:, rng.integers(0, M, N // 2), :]  # queries that are candidates (distance 0, duplicates of lattice points)
    x, y = np.asfortranarray(x), np.asfortranarray(y)
    fx_option("knn_slices", str(slices))
    idx, dist = gpu_fx.knn(x, k, y=y, drop_first=drop)
    oi, od = oracle.knn(x, k, y=y, drop_first=drop)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)
    fx_option("knn_slices", "1")
    idx1, dist1 = gpu_fx.knn(x, k, y=y, drop_first=drop)
    assert np.array_equal(idx1.to_host(), oi) and np.array_equal(dist1.to_host(), od)


def test_knn_candidate_slices_plan_is_a_function_of_the_shape(gpu_fx):
    """fx3d_knn_workspace_bytes and the call agree: scratch for the slices is asked for exactly when the call would use it; a short
    workspace falls back to the unsliced search (same result)."""
    import ctypes as C
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    nb = C.c_size_t(0)
    lib.fx3d_knn_workspace_bytes(8192, 8192, 1, 64, 20, 1, C.byref(nb))
    assert nb.value > 2 * 21 * 8192 * 4 * 2       # slice lists (indices + distances, S >= 2) + pre-pass slabs
    lib.fx3d_knn_workspace_bytes(1024, 1024, 32, 3, 20, 1, C.byref(nb))
    assert nb.value == 0                           # C4: nothing to slice, no pre-pass at D = 3
    rng = np.random.default_rng(3)
    x = gpu_fx.gpu(np.asfortranarray(rng.standard_normal((64, 2048, 1)).astype(np.float32)))
    ref = gpu_fx.knn(x, 20, drop_first=True, return_dist=False).to_host()
    idx = gpu_fx.DeviceArray.empty((20, 2048, 1), np.int32)
    ws = gpu_fx.DeviceArray.empty((4096,), np.uint8)  # far too short
    _lib.call("fx3d_knn_ws", x.ptr, 2048, x.ptr, 2048, 1, 64, 20, 1, idx.ptr, None, ws.ptr, ws.nbytes, None)
    assert np.array_equal(idx.to_host(), ref)


def test_knn_no_mfma_beyond_the_wave_kernels_tile(gpu_fx, oracle, fx_option):
    """knn_no_mfma = 1 at D = 96, k = 20: without the matrix-core kernel the shape's route is the general selection kernel (the
    wave-per-query kernel's tile of 128 rows x (D + 1) floats passes 64 KiB of LDS from D = 85 on): the oracle's lists bit for bit."""
    rng = np.random.default_rng(96)
    x = np.asfortranarray(rng.standard_normal((96, 200, 2)).astype(np.float32))
    y = np.asfortranarray(rng.standard_normal((96, 700, 2)).astype(np.float32))
    fx_option("knn_no_mfma", "1")
    idx, dist = gpu_fx.knn(x, 20, y=y)
    oi, od = oracle.knn(x, 20, y=y)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


@pytest.mark.parametrize("D,N,M,B,k,drop,kind", [(64, 300, 1024, 2, 40, True, "normal"), (64, 257, 512, 1, 63, True, "normal"), (16, 200, 2048, 2, 33, False, "normal"),
                                                  (128, 130, 256, 1, 64, False, "normal"), (64, 200, 1024, 1, 40, False, "sorted"), (32, 150, 1024, 2, 50, True, "sorted"),
                                                  (8, 300, 768, 1, 36, True, "lattice"), (64, 100, 1024, 1, 48, True, "dupes"), (20, 90, 640, 1, 41, False, "normal"),
                                                  (64, 120, 1024, 1, 40, True, "residue"), (16, 100, 512, 2, 60, False, "residue"),
                                                  (64, 130, 1024, 2, 64, True, "normal"), (32, 90, 2048, 1, 100, False, "normal"), (16, 70, 512, 1, 128, False, "sorted"),
                                                  (64, 60, 1024, 1, 127, True, "residue")])
def test_knn_feature_space_wide_selection(gpu_fx, oracle, D, N, M, B, k, drop, kind):
    """32 < k + drop <= 128 in feature space (round 3): 2 / 4 / 8 candidate slices on the matrix-core kernel (32 nearest per slice), the
    verified merge, and the general selection kernel for the flagged queries.  "sorted": the candidates are ordered along the first
    coordinate (index neighbours are spatial neighbours: the slices are interleaved so that each still samples the whole cloud);
    "residue": the near candidates are exactly the rows with index = 0 mod 8, so ONE interleaved slice holds all of a query's
    neighbours and the verification must flag it (every answer then comes from the fallback); lattice / duplicated candidates:
    ties inside and across slices in index order."""
    rng = np.random.default_rng(D * 77 + M + k)
    x = rng.standard_normal((D, N, B)).astype(np.float32)
    y = rng.standard_normal((D, M, B)).astype(np.float32)
    if kind == "sorted":
        for b in range(B):
            y[:, :, b] = y[:, np.argsort(y[0, :, b]), b]
            y[1:, :, b] *= np.float32(0.05)        # the first coordinate decides: neighbours are index neighbours
        x[1:] *= np.float32(0.05)
    elif kind == "residue":
        y[:, 0::8, :] *= np.float32(0.01)          # a tight blob around the origin in rows 0, 8, 16, ... (one slice for S = 2, 4, 8); the queries sit there too
        x *= np.float32(0.01)
    elif kind == "lattice":
        x, y = np.round(x), np.round(y)
    elif kind == "dupes":
        y[:, M // 2:, :] = y[:, : M // 2, :]       # every candidate twice, the copies in different slices
    x, y = np.asfortranarray(x.astype(np.float32)), np.asfortranarray(y.astype(np.float32))
    idx, dist = gpu_fx.knn(x, k, y=y, drop_first=drop)
    oi, od = oracle.knn(x, k, y=y, drop_first=drop)
    assert np.array_equal(idx.to_host(), oi) and np.array_equal(dist.to_host(), od)


def test_c_abi_harness_runs_on_the_device(gpu_fx, tmp_path):
    """examples/c_abi_harness.c: the reference's metric harness sizes (benchmarks/metrics.jl:17-63, A == B) called from plain C --
    it runs, the losses are the exact zeros of identical clouds, and a forward call costs an FFI caller less than the ctypes path."""
    import json
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path / "c_abi_harness")
    libdir = os.path.dirname(gpu_fx.LIB_PATH)
    subprocess.run([gcc, "-std=c99", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_abi_harness.c"),
                    "-o", exe, "-L", libdir, "-lflux3d_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = json.loads(r.stdout)["rows"]
    assert [row["n"] for row in rows] == [64, 256, 1024, 4096, 16384]
    assert all(row["loss"] == 0 for row in rows)
    assert all(0 < row["forward_us"] < row["value_and_grad_us"] for row in rows) and rows[0]["forward_us"] < 15.0


def test_c_abi_example_runs_on_the_device(gpu_fx, oracle, tmp_path):
    """examples/c_abi_example.c (plain C against the shared library, no Python in the call path) prints the oracle's
    loss for its LCG clouds."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path / "c_abi_example")
    libdir = os.path.dirname(gpu_fx.LIB_PATH)
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_abi_example.c"),
                    "-o", exe, "-L", libdir, "-lflux3d_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = float(r.stdout.split("chamfer_distance(A, B) = ")[1].split()[0])
    s = np.uint32(12345)
    vals = np.empty(2 * 3 * 1024 * 2, np.float32)
    with np.errstate(over="ignore"):
        for i in range(vals.size):
            s = np.uint32(s * np.uint32(1664525) + np.uint32(1013904223))
            vals[i] = np.float32(s >> np.uint32(8)) * np.float32(1.0 / 16777216.0)
    x = np.asfortranarray(vals[: 3 * 1024 * 2].reshape((3, 1024, 2), order="F"))
    y = np.asfortranarray(vals[3 * 1024 * 2:].reshape((3, 1024, 2), order="F"))
    assert np.isclose(got, oracle.chamfer_distance(x, y, 1.0, 1.0), rtol=1e-5)


def test_interleaved_calls_share_state_correctly(gpu_fx, oracle):
    """Many back-to-back calls of different ops and shapes on one stream: the caching allocator, the grow-only
    workspaces, the library's ticket pool (fused finalisation) and the per-device attribute cache must never leak
    state from one call into the next."""
    fx = gpu_fx
    rng = np.random.default_rng(2024)
    pending = []
    for it in range(60):
        N, M, B = int(rng.integers(1, 1500)), int(rng.integers(1, 1500)), int(rng.integers(1, 4))
        x = np.asfortranarray(rng.random((3, N, B), dtype=np.float32))
        y = np.asfortranarray(rng.random((3, M, B), dtype=np.float32))
        kind = it % 3
        if kind == 0:
            out = fx.DeviceArray.empty((1,), np.float32)
            fx.chamfer_distance(fx.gpu(x), fx.gpu(y), loss_out=out, sync=False)   # not synchronised: stays in flight
            pending.append(("ch", out, x, y, None))
        elif kind == 1 and M >= 3:
            k = int(rng.integers(1, min(20, M)))
            idx = fx.knn(fx.gpu(x), k, y=fx.gpu(y), return_dist=False)
            pending.append(("knn", idx, x, y, k))
        else:
            _, ix, iy = fx.chamfer_distance(x, y, return_indices=True)
            pending.append(("nn", (ix, iy), x, y, None))
    fx.synchronize()
    for kind, res, x, y, k in pending:
        if kind == "ch":
            assert np.isclose(res.item(), oracle.chamfer_distance(x, y), rtol=LOSS_RTOL, atol=0)
        elif kind == "knn":
            assert np.array_equal(res.to_host(), oracle.knn(x, k, y=y, want_dist=False))
        else:
            ox, oy = oracle.nn1(x, y)
            assert np.array_equal(res[0].to_host(), ox) and np.array_equal(res[1].to_host(), oy)


@pytest.mark.parametrize("dtype", [np.uint32, np.int64, np.int32])
def test_index_arrays_of_the_reference_types_are_converted_on_the_device(gpu_fx, dtype):
    """VERDICT r4 #7 / SURVEY 8(b): faces / edges cross the ABI as the reference holds them (UInt32 or Int64, 1-based,
    src/rep/mesh.jl:70-98) and become the kernels' int32 0-based form ON THE DEVICE (fx3d_index_upload / fx3d_index_convert):
    values, the padding rule of faces_padded, the range check, and a TriMesh built with either type giving the same areas."""
    import ctypes as C
    fx = gpu_fx
    from flux3d_jl_amd.rep import index_upload
    rng = np.random.default_rng(3)
    a = np.asfortranarray(rng.integers(1, 500, (3, 1000)).astype(dtype))
    a[:, 900:] = 0  # padding
    d = index_upload(a, 1, clamp_pad=True, limit=499)
    want = a.astype(np.int64) - 1
    want[want < 0] = 0
    assert d.dtype == np.int32 and np.array_equal(d.to_host(), want.astype(np.int32))
    assert np.array_equal(index_upload(a[:, :900], 1).to_host(), (a[:, :900].astype(np.int64) - 1).astype(np.int32))
    with pytest.raises(ValueError):
        index_upload(a[:, :900], 1, limit=100)          # out of range: counted on the device
    with pytest.raises(ValueError):
        index_upload(a, 1, clamp_pad=False, limit=499)  # the zeros are -1 without the padding rule
    # device-resident source
    src = fx.DeviceArray.from_host(a)
    out = fx.DeviceArray.empty(a.shape, np.int32)
    t = {np.dtype(np.int32): 0, np.dtype(np.uint32): 1, np.dtype(np.int64): 2}[np.dtype(dtype)]
    fx._lib.call("fx3d_index_convert", src.ptr, t, 1, a.size, 1, 0, out.ptr, None, fx.current_stream().handle)
    assert np.array_equal(out.to_host(), want.astype(np.int32))
    with pytest.raises(fx.Flux3DHipError):
        fx._lib.call("fx3d_index_convert", src.ptr, 7, 1, a.size, 1, 0, out.ptr, None, fx.current_stream().handle)
    # a mesh whose faces are held in this type: same device mirrors, same areas as the reference's known answers path
    v, f = fx.load_obj(os.path.join(GOLDEN, "teapot.obj"))
    m = fx.gpu(fx.TriMesh([v], [f.astype(dtype)], faces_dtype=dtype))
    m64 = fx.gpu(fx.TriMesh([v], [f.astype(np.int64)]))
    assert np.array_equal(m.dev("faces_packed").to_host(), m64.dev("faces_packed").to_host())
    assert np.array_equal(m.dev("faces_padded").to_host(), m64.dev("faces_padded").to_host())
    assert np.array_equal(m.dev("edges").to_host(), m64.dev("edges").to_host())
    assert np.array_equal(fx.laplacian_loss(m), fx.laplacian_loss(m64))
