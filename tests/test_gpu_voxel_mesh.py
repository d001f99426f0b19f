"""voxel_to_trimesh with algo :Exact on the device (fx3d_voxel_mesh_count / _emit) against the literal restatement of the
reference's _voxel_exact (tests/voxel_mesh_ref.py, src/conversions.jl:209-349): every mesh's vertices and faces bit for
bit, through trimesh_from_voxels (device faces seeded into the mesh) and voxel_to_trimesh (host face lists)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import trimesh_voxel_ref as tvref
import voxel_mesh_ref as ref

pytestmark = pytest.mark.gpu


def _check(fx, vox, thresh=0.5, on_device=True):
    vox = np.asfortranarray(vox, dtype=np.float32)
    if vox.ndim == 3:
        vox = vox[..., None]
    ev, ef = ref.voxel_to_trimesh(vox, np.float32(thresh))
    m = fx.trimesh_from_voxels(fx.gpu(vox) if on_device else vox, thresh, "Exact")
    assert m.on_device and m.N == vox.shape[3]
    K = np.array([f.shape[1] // 12 for f in ef])
    assert np.array_equal(m._verts_len, 8 * K) and np.array_equal(m._faces_len, 12 * K)
    packed = m.get_verts_packed().to_host()
    assert np.array_equal(packed, np.concatenate(ev, axis=1))
    for i, (gv, gf) in enumerate(zip(m.get_verts_list(), m.get_faces_list())):
        assert gv.dtype == np.float32 and gf.dtype == np.uint32
        assert np.array_equal(gv, ev[i]) and np.array_equal(gf, ef[i]), i
    fp = m.dev("faces_padded").to_host()  # what the kernel wrote: 0-based, padded with 0
    for i in range(m.N):
        assert np.array_equal(fp[:, : 12 * K[i], i], ef[i].astype(np.int64) - 1), i
        assert not fp[:, 12 * K[i]:, i].any()
    assert np.array_equal(m.dev("faces_len").to_host(), 12 * K) and np.array_equal(m.dev("nverts").to_host(), 8 * K)
    return m, ev, ef


def test_reference_test_grid(gpu_fx):
    """test/conversions.jl: zeros(32,32,32,2) with [1:15, 2:10, 18:32, :] .= 1 at thresh 0.9: K = 842 per grid."""
    m, ev, _ = _check(gpu_fx, ref.reference_test_grid(), 0.9)
    assert list(m._verts_len) == [6736, 6736] and list(m._faces_len) == [10104, 10104]
    v0 = m.get_verts_list()[0]
    assert np.array_equal(v0[:, 0], np.array([0, 1, 17], np.float32) / np.float32(32))
    assert np.array_equal(v0[:, -1], np.array([15, 10, 32], np.float32) / np.float32(32))


@pytest.mark.parametrize("res,K", [(1, 1), (2, 8), (3, 26), (4, 56), (32, 5768)])
def test_full_grids(gpu_fx, res, K):
    m, _, _ = _check(gpu_fx, np.ones((res, res, res, 1), np.float32))
    assert m._verts_len[0] == 8 * K


@pytest.mark.parametrize("res,K", [(5, 63), (64, 131072)])
def test_checkerboards(gpu_fx, res, K):
    m, _, _ = _check(gpu_fx, ref.checkerboard(res))
    assert m._verts_len[0] == 8 * K


def _random_batch(rng, res, B):
    out = np.empty((res, res, res, B), np.float32, order="F")
    for b in range(B):
        kind = (b + res) % 4
        if kind < 3:  # binary at density 0.05 / 0.5 / 0.95
            out[..., b] = (rng.random((res, res, res)) < (0.05, 0.5, 0.95)[kind]).astype(np.float32)
        else:  # values in [0, 1], a quarter of them exactly Float32(0.5), some 0 and 1
            x = rng.random((res, res, res), dtype=np.float32)
            x[rng.random((res, res, res)) < 0.25] = np.float32(0.5)
            x[rng.random((res, res, res)) < 0.05] = 0
            x[rng.random((res, res, res)) < 0.05] = 1
            out[..., b] = x
        if not (out[..., b] >= 0.5).any():
            out[0, 0, 0, b] = 1
    return out


@pytest.mark.parametrize("res", [1, 2, 3, 5, 17, 64, 128])
def test_random_grids(gpu_fx, res):
    rng = np.random.default_rng(7000 + res)
    for B in ((1, 5) if res <= 64 else (3,)):
        _check(gpu_fx, _random_batch(rng, res, B))


def test_more_tiles_than_one_round_of_the_scan_block(gpu_fx):
    """res 32, B = 65: 16 tiles per grid, 1040 in the batch -- the smallest batch whose tile counts take two rounds of the
    one-block scan's 1024 (launch 3), so the last grid's cubes start at the first round's total."""
    _check(gpu_fx, _random_batch(np.random.default_rng(7065), 32, 65))


@pytest.mark.parametrize("thresh", [0.05, 0.9, 1.0])
def test_random_values_other_thresholds(gpu_fx, thresh):
    rng = np.random.default_rng(int(thresh * 100))
    v = rng.random((33, 33, 33, 2), dtype=np.float32)
    v[rng.random(v.shape) < 0.3] = np.float32(thresh)
    _check(gpu_fx, v, thresh)


@pytest.fixture(scope="module")
def ref_meshes(gpu_fx):
    return [gpu_fx.load_obj(os.path.join(GOLDEN, n)) for n in ("teapot.obj", "sphere.obj")]


@pytest.fixture(scope="module")
def modelnet(gpu_fx):
    return tvref.modelnet_meshes(GOLDEN)


def test_grids_from_trimesh_to_voxel(gpu_fx, ref_meshes, modelnet):
    fx = gpu_fx
    for res in (28, 64):
        _check(fx, fx.trimesh_to_voxel(fx.gpu(fx.TriMesh(*map(list, zip(*ref_meshes)))), res).to_host())
    mn = fx.gpu(fx.TriMesh([v for _, v, _ in modelnet], [f for _, _, f in modelnet]))
    for res in (32, 64, 128):
        grid = fx.trimesh_to_voxel(mn, res)
        ev, ef = ref.voxel_to_trimesh(grid.to_host(), np.float32(0.5))
        m = fx.trimesh_from_voxels(grid, 0.5, "Exact")  # the device grid as it is
        for i, (gv, gf) in enumerate(zip(m.get_verts_list(), m.get_faces_list())):
            assert np.array_equal(gv, ev[i]) and np.array_equal(gf, ef[i]), (res, i)


def test_grids_from_pointcloud_to_voxel(gpu_fx, ref_meshes):
    fx = gpu_fx
    m = fx.gpu(fx.TriMesh(*map(list, zip(*ref_meshes))))
    p = fx.sample_points(m, 3000, seed=5)
    _check(fx, fx.pointcloud_to_voxel(p, 32).to_host())


def test_batch_equals_single_calls_and_host_equals_device(gpu_fx):
    fx = gpu_fx
    v = _random_batch(np.random.default_rng(11), 17, 4)
    mb, _, _ = _check(fx, v)
    mh, _, _ = _check(fx, v, on_device=False)
    assert np.array_equal(mb.get_verts_packed().to_host(), mh.get_verts_packed().to_host())
    singles = [fx.trimesh_from_voxels(fx.gpu(np.asfortranarray(v[..., i:i + 1])), 0.5, "Exact") for i in range(4)]
    assert np.array_equal(mb.get_verts_packed().to_host(),
                          np.concatenate([s.get_verts_packed().to_host() for s in singles], axis=1))
    for i, s in enumerate(singles):
        assert np.array_equal(mb.get_faces_list()[i], s.get_faces_list()[0])


def test_two_calls_agree_and_voxel_to_trimesh_matches(gpu_fx):
    fx = gpu_fx
    v = _random_batch(np.random.default_rng(12), 64, 3)
    a = fx.trimesh_from_voxels(fx.gpu(v), 0.5, ":Exact").get_verts_packed().to_host()
    b = fx.trimesh_from_voxels(fx.gpu(v), 0.5, "Exact").get_verts_packed().to_host()
    assert np.array_equal(a, b)
    ev, ef = ref.voxel_to_trimesh(v, np.float32(0.5))
    dv, df = fx.voxel_to_trimesh(fx.VoxelGrid(fx.gpu(v)), 0.5, "Exact")  # device views
    hv, hf = fx.voxel_to_trimesh(v, 0.5, "Exact")  # host arrays
    for i in range(3):
        assert fx.device.is_device(dv[i]) and isinstance(hv[i], np.ndarray)
        assert np.array_equal(dv[i].to_host(), ev[i]) and np.array_equal(hv[i], ev[i])
        assert np.array_equal(df[i], ef[i]) and np.array_equal(hf[i], ef[i])


@pytest.mark.parametrize("bad", [np.nan, -0.5, np.float32(1.0000001), "empty"])
def test_invalid_or_empty_grid_raises_naming_its_index(gpu_fx, bad):
    fx = gpu_fx
    v = _random_batch(np.random.default_rng(13), 9, 4)
    if bad == "empty":
        v[..., 2] = 0.25
        idx = 2
    else:
        v[3, 4, 5, 1] = bad
        idx = 1
    assert ref.first_bad_grid(v, 0.5) == idx
    with pytest.raises(ValueError, match=f"grid {idx} "):
        fx.trimesh_from_voxels(fx.gpu(v), 0.5, "Exact")
    with pytest.raises(ValueError, match=f"grid {idx} "):
        fx.voxel_to_trimesh(v, 0.5, "Exact")
    # the other grids come out right on their own
    keep = [i for i in range(4) if i != idx]
    _check(fx, np.asfortranarray(v[..., keep]))


def test_pointcloud_from_voxels(gpu_fx):
    fx = gpu_fx
    v = _random_batch(np.random.default_rng(14), 12, 3)
    n = 4000
    p = fx.pointcloud_from_voxels(fx.gpu(v), n, 0.5, "Exact", seed=99)
    assert isinstance(p, fx.PointCloud) and p.on_device
    pts = p.points.to_host()
    assert p.points.shape == (3, n, 3) and pts.dtype == np.float32
    m = fx.trimesh_from_voxels(fx.gpu(v), 0.5, "Exact")
    for b in range(3):
        cells = np.argwhere(ref.surviving_cells(v[..., b], 0.5))  # 0-based lower corners
        scale = np.float64(cells.max() + 1)
        q = pts[:, :, b].astype(np.float64) * scale
        assert np.all(np.abs(q - np.round(q)).min(axis=0) < 1e-4)  # every point on a cube face plane
        lo = cells.astype(np.float64)
        inside = np.zeros(n, bool)
        for c in lo:
            inside |= np.all((q >= c[:, None] - 1e-4) & (q <= c[:, None] + 1 + 1e-4), axis=0)
        assert inside.all()
    # the seeded device face caches equal what uploading the host lists gives
    rebuilt = fx.gpu(fx.TriMesh(m.get_verts_list(), m.get_faces_list()))
    assert np.array_equal(fx.sample_points(rebuilt, n, seed=99).to_host(), pts)
    assert np.array_equal(rebuilt.dev("faces_padded").to_host(), m.dev("faces_padded").to_host())


def test_trimesh_from_pointcloud(gpu_fx, ref_meshes):
    fx = gpu_fx
    m = fx.gpu(fx.TriMesh(*map(list, zip(*ref_meshes))))
    p = fx.PointCloud(fx.sample_points(m, 2000, seed=3))
    grid = fx.pointcloud_to_voxel(p, 28).to_host()
    ev, ef = ref.voxel_to_trimesh(grid, np.float32(0.5))
    t = fx.trimesh_from_pointcloud(p, 28, "Exact")
    for i in range(2):
        assert np.array_equal(t.get_verts_list()[i], ev[i]) and np.array_equal(t.get_faces_list()[i], ef[i])
