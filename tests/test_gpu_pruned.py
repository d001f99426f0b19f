"""GPU parity of the spatially pruned nearest-neighbour launch (nn1_f16_kernel<.., PRUNE = true>, csrc/chamfer.hip): the
candidates in a Hilbert-ordered LDS image, a bounding box per 64-row lane tile, waves that skip the tiles which cannot hold a
nearest neighbour.  Only chamfer_forward (csrc/chamfer_host.hip) prunes (fx3d_chamfer_fwd / _sums / _fwd_bwd, with the blocks' scratch in the workspace),
and only at shapes with two or more query passes per block in both directions (prune_rows_per_block): B >= 17 at 4096 points,
B = 128 at 1024.  Every test first checks that its shape still takes the pruned launch, so a plan change fails here instead
of quietly testing the unpruned kernel.

No pruned shape has a candidate cloud below 512 points (4096 / 600 at B = 128 is near the smallest), so the unsorted pruned
form is reached through coordinates that are not `sane` (non-finite, or beyond 1e16).

Each case: indices bit for bit against the oracle's brute force, the loss against the oracle's Float32 restatement, the loss
bit-identical from call to call and with a second workspace, and the same indices and loss bits under nn1_prune = 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_hardening import LOSS_RTOL, _nonfinite_case, _worst_split_values

pytestmark = pytest.mark.gpu

C2 = (4096, 4096, 32)
SHAPES = [C2, (4096, 4096, 17), (4096, 4096, 21),                   # 2B a multiple of 8 or not
          (3009, 3009, 32), (4033, 4033, 32), (4095, 4095, 17),     # ragged: scratch rows between cnt and cnt_pad
          (4096, 3500, 32), (2048, 4096, 64),                       # N != M, both ways round
          (4096, 1024, 128), (1024, 4096, 128), (4096, 600, 128),   # eight passes per block
          (2049, 2049, 64),                                         # four passes + a folded remainder of one query
          (1024, 1024, 128), (1087, 1025, 128)]


def _lib():
    from flux3d_jl_amd import _lib
    return _lib


def _ws_bytes(N, M, B, prune, entry="fx3d_chamfer_workspace_bytes"):
    n = C.c_size_t(0)
    with _lib().option("nn1_prune", prune):
        _lib().call(entry, N, M, B, 3, C.byref(n))
    return n.value


def _assert_pruned(N, M, B):
    """The shape takes the pruned launch: the default option prunes and the workspace holds the blocks' scratch."""
    assert _lib().get_option("nn1_prune") == 1
    full, part = _ws_bytes(N, M, B, 1), _ws_bytes(N, M, B, 0)
    assert full > part, f"N={N} M={M} B={B} no longer takes the pruned launch ({full} vs {part} bytes)"
    return full, part


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _loss_close(loss, ref, rtol):
    if np.isnan(ref) or np.isinf(ref):
        assert (np.isnan(loss) and np.isnan(ref)) or loss == ref, (loss, ref)
    else:
        assert np.isclose(loss, ref, rtol=rtol, atol=0), (loss, ref)


def _fwd(fx, dx, dy, ws, nbytes, w1=0.7, w2=1.3):
    """fx3d_chamfer_fwd with a workspace and a byte count of the caller's: (status, loss, idx_x, idx_y)."""
    D, N, B = dx.shape
    M = dy.shape[1]
    ix, iy = fx.DeviceArray.empty((N, B), np.int32), fx.DeviceArray.empty((M, B), np.int32)
    loss_dev = fx.DeviceArray.empty((1,), np.float32)
    host = C.c_float(0)
    rc = _lib().load().fx3d_chamfer_fwd(dx.ptr, N, dy.ptr, M, B, D, w1, w2, loss_dev.ptr, C.byref(host), ix.ptr, iy.ptr,
                                        ws.ptr, nbytes, fx.current_stream().handle)
    return rc, np.float32(host.value), ix.to_host(), iy.to_host()


def _oracle_nn(oracle, x, y):
    ox, oy, _ = oracle.nn1_allcores(x, y, threads=16)   # the serial brute force per (batch element, direction)
    return ox, oy


def _check_pruned(fx, oracle, x, y, w1=0.7, w2=1.3):
    D, N, B = x.shape
    M = y.shape[1]
    full, _ = _assert_pruned(N, M, B)
    dx, dy = fx.gpu(x), fx.gpu(y)
    loss, ix, iy = fx.chamfer_distance(dx, dy, w1=w1, w2=w2, return_indices=True)
    gix, giy = ix.to_host(), iy.to_host()
    ox, oy = _oracle_nn(oracle, x, y)
    assert np.array_equal(gix, ox), np.argwhere(gix != ox)[:5]
    assert np.array_equal(giy, oy), np.argwhere(giy != oy)[:5]
    with np.errstate(all="ignore"):
        _loss_close(loss, oracle.chamfer_loss_pairwise(x, y, ox, oy, w1, w2), LOSS_RTOL)
    # the query order decides which block and lane sums a term: it must not depend on timing, nor on the scratch's address
    for _ in range(2):
        assert _bits(fx.chamfer_distance(dx, dy, w1=w1, w2=w2)) == _bits(loss)
    ws2 = fx.DeviceArray.empty((full,), np.uint8)
    rc, loss2, ix2, iy2 = _fwd(fx, dx, dy, ws2, full, w1, w2)
    assert rc == 0 and _bits(loss2) == _bits(loss) and np.array_equal(ix2, ox) and np.array_equal(iy2, oy)
    with _lib().option("nn1_prune", 0):
        loss0, ix0, iy0 = fx.chamfer_distance(dx, dy, w1=w1, w2=w2, return_indices=True)
    assert np.array_equal(ix0.to_host(), ox) and np.array_equal(iy0.to_host(), oy)
    # the terms are summed in another order (Float64 sums, one rounding to Float32): bit-equal on every case here
    if np.isfinite(loss0):
        assert _bits(loss0) == _bits(loss), (loss0, loss)
    else:
        _loss_close(loss, loss0, 1e-6)
    return loss, ox, oy


def _f(a):
    return np.asfortranarray(np.asarray(a).astype(np.float32))


# ------------------------------------------------------------------------------ every pruned shape, uniform clouds
@pytest.mark.parametrize("N,M,B", SHAPES)
def test_pruned_shapes_uniform(gpu_fx, oracle, N, M, B):
    _assert_pruned(N, M, B)
    rng = np.random.default_rng(N * 131 + M * 7 + B)
    _check_pruned(gpu_fx, oracle, _f(rng.random((3, N, B))), _f(rng.random((3, M, B))))


def test_no_pruned_shape_has_a_candidate_cloud_below_512_points(fx):
    """(the unsorted pruned form at small candidate clouds is unreachable: it needs two query passes per block both ways)"""
    assert not any(_ws_bytes(4096, m, 128, 1) > _ws_bytes(4096, m, 128, 0) for m in (64, 256, 511))


# ------------------------------------------------------------------------------ data aimed at the pruned kernel's branches
def _sphere(rng, n, B, r=1.0):
    v = rng.standard_normal((3, n, B))
    return v / np.linalg.norm(v, axis=0, keepdims=True) * r


def _crowded_lattice(rng, n, B):
    """Points p of every 64-point wave in 16 distinct cells of the 8 x 8 x 8 grid, runs of four lanes per cell: the crowded
    counting path takes 12 cells by grouped atomics, the other four lane by lane."""
    p = np.arange(n)
    k = (((p // 4) % 16) * 37 + (p // 64) * 5) % 512
    g = np.stack([k % 8, (k // 8) % 8, k // 64]).astype(np.float64)[:, :, None]
    return g + 0.2 * rng.random((3, n, B))


def _data(kind, N, M, B, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((3, N, B))
    y = rng.random((3, M, B))
    if kind == "sphere_shells":
        x, y = _sphere(rng, N, B), _sphere(rng, M, B, 1.02) + rng.standard_normal((3, M, B)) * 1e-3
    elif kind == "plane":            # an axis of zero extent: inv = 0 on it
        y[2] = 0.5
    elif kind == "line":
        y = np.array([0.1, 0.2, 0.3])[:, None, None] + np.array([1.0, -2.0, 0.5])[:, None, None] * y[:1]
    elif kind == "one_point":        # every candidate the same point: index 0 wins every query
        y[:] = np.array([0.25, 0.5, 0.75])[:, None, None]
    elif kind == "cell_and_outlier":
        y = 0.3 + rng.standard_normal((3, M, B)) * 1e-4
        y[:, M // 3, :] = 1e3
    elif kind == "crowded_lattice":
        x, y = rng.random((3, N, B)) * 8.0, _crowded_lattice(rng, M, B)
    elif kind == "scattered_duplicates":   # every candidate twice, at scattered indices: the lower index wins
        h = rng.random((3, (M + 1) // 2, B))
        y = np.concatenate([h, h], 1)[:, rng.permutation(2 * h.shape[1])[:M], :]
    elif kind == "equidistant_lattice":
        x = rng.integers(0, 8, (3, N, B)) * 0.25 + 0.125
        y = rng.integers(0, 8, (3, M, B)) * 0.25
    elif kind == "tight_clusters":
        c = np.random.default_rng(7).standard_normal((3, 40, 1)) * 3
        x = c[:, rng.integers(0, 40, N), :] + rng.standard_normal((3, N, B)) * 1e-3
        y = c[:, rng.integers(0, 40, M), :] + rng.standard_normal((3, M, B)) * 1e-3
    elif kind == "worst_split":
        def half_sym(n):
            h = _worst_split_values(rng, 3 * ((n + 1) // 2) * B, 0, 4).reshape(3, (n + 1) // 2, B)
            return np.concatenate([h, -h], 1)[:, rng.permutation(2 * h.shape[1])[:n], :]
        x, y = half_sym(N), half_sym(M)
    elif kind == "far_candidates":
        y = rng.standard_normal((3, M, B))
        for b in range(B):
            y[:, rng.choice(M, 5, replace=False), b] *= 10.0 ** (4 + b % 4)
        y[:, 0, 1] = x[:, 0, 1] * 1.0000001
    elif kind == "far_queries":
        x = rng.standard_normal((3, N, B))
        for b in range(B):
            x[:, rng.choice(N, 5, replace=False), b] *= 10.0 ** (4 + b % 4)
    elif kind.startswith("extent_"):      # per-query scale; queries far outside the candidates' box clamp into border cells
        ratio, offset = {"extent_30": (30.0, 0.0), "extent_3e4_off": (3e4, 3.0), "extent_3e6": (3e6, 0.0)}[kind]
        y = (y - 0.5) * ratio + offset * ratio
        y[2, : M // 2, :] = 0.25 * ratio
    elif kind == "huge":             # finite, beyond 1e16: not `sane`, the pruned launch runs without a sort
        x, y = 1e20 * (1.0 + 1e-3 * x), 1e20 * (1.0 + 1e-3 * y)
    else:
        raise ValueError(kind)
    return _f(x), _f(y)


KIND_SHAPES = {
    "sphere_shells": [C2, (1087, 1025, 128)],
    "plane": [(4095, 4095, 17), (1024, 4096, 128)],
    "line": [(3009, 3009, 32), (2049, 2049, 64)],
    "one_point": [(4096, 600, 128), (1024, 1024, 128)],
    "cell_and_outlier": [(4033, 4033, 32), (2049, 2049, 64)],
    "crowded_lattice": [(4096, 4096, 17), (1024, 1024, 128)],
    "scattered_duplicates": [(4096, 3500, 32), (1087, 1025, 128)],
    "equidistant_lattice": [(3009, 3009, 32), (4096, 1024, 128)],
    "tight_clusters": [(2048, 4096, 64), (4095, 4095, 17)],
    "worst_split": [(4096, 4096, 21), (1024, 1024, 128)],
    "far_candidates": [(4033, 4033, 32), (4096, 600, 128)],
    "far_queries": [(3009, 3009, 32), (1024, 4096, 128)],
    "extent_30": [(4096, 3500, 32), (1087, 1025, 128)],
    "extent_3e4_off": [(2049, 2049, 64), (4096, 1024, 128)],
    "extent_3e6": [(4095, 4095, 17), (1024, 4096, 128)],
    "huge": [(3009, 3009, 32), (1024, 1024, 128)],
}


@pytest.mark.parametrize("kind,N,M,B", [(k, *s) for k, shapes in KIND_SHAPES.items() for s in shapes])
def test_pruned_data_kinds(gpu_fx, oracle, kind, N, M, B):
    _assert_pruned(N, M, B)
    x, y = _data(kind, N, M, B, N + M + B + len(kind))
    _check_pruned(gpu_fx, oracle, x, y)
    if kind in ("scattered_duplicates", "tight_clusters", "one_point") and N == M:
        _check_pruned(gpu_fx, oracle, x, x)    # A == B: every query's nearest neighbour is itself (or a lower duplicate)


@pytest.mark.parametrize("N,M,B", [C2, (2049, 2049, 64)])
def test_pruned_identical_clouds(gpu_fx, oracle, N, M, B):
    _assert_pruned(N, M, B)
    x = _f(np.random.default_rng(B).standard_normal((3, N, B)))
    _check_pruned(gpu_fx, oracle, x, x)


@pytest.mark.parametrize("case", ["nan_query", "nan_candidate", "inf_query", "neg_inf_candidate", "all_nan_cloud", "mixed_everything",
                                  "overflowing_distances"])
@pytest.mark.parametrize("N,M,B", [(4096, 3500, 32), (1087, 1025, 128)])
def test_pruned_nonfinite(gpu_fx, oracle, case, N, M, B):
    """Non-finite coordinates are not `sane`: the pruned instantiation runs without a sort, and a wave with a non-finite query
    keeps every lane tile."""
    _assert_pruned(N, M, B)
    with np.errstate(all="ignore"):
        x, y = _nonfinite_case(case, N, M, B, N + len(case))
        _check_pruned(gpu_fx, oracle, x, y)


def _normalised(p):
    c = p - p.mean(axis=1, keepdims=True)
    return c / np.abs(c).max(axis=(0, 1), keepdims=True)


@pytest.mark.parametrize("normalise", [False, True])
def test_pruned_sampled_mesh_surfaces(gpu_fx, oracle, normalise):
    """fx.sample_points on the teapot and the sphere (16 of each in a batch), at their own scale and normalised."""
    fx = gpu_fx
    N, M, B = 4096, 3500, 32
    _assert_pruned(N, M, B)
    paths = [os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj")] * (B // 2)
    m = fx.gpu(fx.load_trimesh(*paths))
    x = fx.sample_points(m, N, seed=11).to_host()
    y = fx.sample_points(m, M, seed=12).to_host()[:, :, ::-1]   # teapots against spheres
    if normalise:
        x, y = _normalised(x), _normalised(y)
    _check_pruned(fx, oracle, _f(x), _f(y))


def test_pruned_modelnet_surfaces(gpu_fx, oracle, tmp_path):
    """Points sampled from the ModelNet OFF files of tests/golden (138 ... 27 438 faces; millimetre-scale furniture beside unit
    objects): four copies of the eight meshes against a shifted pairing."""
    import shutil
    fx = gpu_fx
    N, M, B = 4096, 4096, 32
    _assert_pruned(N, M, B)
    for z in ("ModelNet10.zip", "ModelNet40.zip"):
        shutil.copy(os.path.join(GOLDEN, "modelnet", z), tmp_path)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import modelnet_chamfer_eval as ev
    meshes = ev.listing(str(tmp_path))
    assert len(meshes) == 8
    ta = fx.gpu(fx.TriMesh([meshes[k % 8][1] for k in range(B)], [meshes[k % 8][2] for k in range(B)]))
    tb = fx.gpu(fx.TriMesh([meshes[(k + 3) % 8][1] for k in range(B)], [meshes[(k + 3) % 8][2] for k in range(B)]))
    x, y = fx.sample_points(ta, N, seed=5).to_host(), fx.sample_points(tb, M, seed=6).to_host()
    _check_pruned(fx, oracle, _f(x), _f(y))


# ------------------------------------------------------------------------------ the workspace contract
def test_pruned_workspace_sizes_and_poisoned_scratch(gpu_fx, oracle):
    """A workspace of the partials' size (or one byte short of the full size) runs unpruned, the full size and more run pruned;
    all give the oracle's indices.  Scratch rows the pruned kernel reads but masks (the rows between cnt and cnt_pad) hold
    whatever the workspace held: zeros, 0xFF bytes or rows (qx, qy, qz, index 0) of real query points -- a zero-distance match
    if read unmasked -- change neither the indices nor the loss's bits."""
    fx = gpu_fx
    N, M, B = 4033, 4033, 32
    full, part = _assert_pruned(N, M, B)
    rng = np.random.default_rng(4033)
    x, y = _f(rng.random((3, N, B))), _f(rng.random((3, M, B)))
    dx, dy = fx.gpu(x), fx.gpu(y)
    ox, oy = _oracle_nn(oracle, x, y)
    ws = fx.DeviceArray.empty((full + (1 << 20),), np.uint8)
    losses = []
    for nb in (part, full - 1, full, full + (1 << 20)):
        rc, loss, ix, iy = _fwd(fx, dx, dy, ws, nb)
        assert rc == 0, _lib().last_error()
        assert np.array_equal(ix, ox) and np.array_equal(iy, oy), nb
        losses.append(loss)
    assert np.isclose(losses[0], losses[2], rtol=1e-6, atol=0) and _bits(losses[0]) == _bits(losses[1])
    assert _bits(losses[2]) == _bits(losses[3])
    clean = losses[2]
    poff = (part + 255) & ~255
    nscr = full - poff
    st = fx.current_stream().handle
    q = np.concatenate([x[:, :, 0].T, y[:, :, 0].T]).astype(np.float32)
    rows = np.zeros((nscr // 16, 4), np.float32)
    rows[:, :3] = q[np.arange(rows.shape[0]) % q.shape[0]]
    for pattern in (0x00, 0xFF, rows):
        if isinstance(pattern, int):
            _lib().call("fx3d_memset", ws.ptr + poff, pattern, nscr, st)
        else:
            _lib().call("fx3d_memcpy_h2d", ws.ptr + poff, pattern.ctypes.data, pattern.nbytes, st)
        rc, loss, ix, iy = _fwd(fx, dx, dy, ws, full)
        assert rc == 0 and np.array_equal(ix, ox) and np.array_equal(iy, oy)
        assert _bits(loss) == _bits(clean), (pattern if isinstance(pattern, int) else "rows", loss, clean)


# ------------------------------------------------------------------------------ gradients and shard sums at pruned shapes
@pytest.mark.parametrize("kind,N,M,B", [("tight_clusters", 4096, 3500, 32), ("scattered_duplicates", 1087, 1025, 128)])
def test_pruned_value_and_grad(gpu_fx, oracle, kind, N, M, B):
    """fx3d_chamfer_fwd_bwd (its workspace holds the pruned scratch): indices and gradients bit for bit the oracle's."""
    fx = gpu_fx
    _assert_pruned(N, M, B)
    assert _ws_bytes(N, M, B, 1, "fx3d_chamfer_fwd_bwd_workspace_bytes") > _ws_bytes(N, M, B, 0, "fx3d_chamfer_fwd_bwd_workspace_bytes")
    x, y = _data(kind, N, M, B, 99 + B)
    loss, gx, gy, ix, iy = fx.chamfer_value_and_grad(fx.gpu(x), fx.gpu(y), w1=0.7, w2=1.3, gout=2.0, return_indices=True)
    ox, oy = _oracle_nn(oracle, x, y)
    assert np.array_equal(ix.to_host(), ox) and np.array_equal(iy.to_host(), oy)
    ogx, ogy = oracle.chamfer_bwd(x, y, ox, oy, 0.7, 1.3, 2.0)
    assert np.array_equal(gx.to_host(), ogx) and np.array_equal(gy.to_host(), ogy)
    _loss_close(loss, oracle.chamfer_loss_pairwise(x, y, ox, oy, 0.7, 1.3), LOSS_RTOL)


def test_pruned_chamfer_sums(gpu_fx, oracle):
    fx = gpu_fx
    N, M, B = 1024, 1024, 128
    _assert_pruned(N, M, B)
    x, y = _data("tight_clusters", N, M, B, 5)
    _, ox, oy, osums = oracle.chamfer_distance(x, y, return_all=True)
    ix, iy = fx.DeviceArray.empty((N, B), np.int32), fx.DeviceArray.empty((M, B), np.int32)
    from flux3d_jl_amd import distributed
    sums = distributed.chamfer_sums(fx.gpu(x), fx.gpu(y), idx_x=ix, idx_y=iy)
    assert np.array_equal(ix.to_host(), ox) and np.array_equal(iy.to_host(), oy)
    # the oracle adds the squared coordinate differences, the kernel each point's Float32 distance: both in Float64
    assert np.allclose(sums, osums, rtol=1e-6, atol=0), (sums, osums)
    with _lib().option("nn1_prune", 0):
        sums0 = distributed.chamfer_sums(fx.gpu(x), fx.gpu(y))
    assert np.allclose(sums, sums0, rtol=1e-12, atol=0), (sums, sums0)
