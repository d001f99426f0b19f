"""trimesh_to_voxel on the device (fx3d_trimesh_to_voxel) against the literal restatement of the reference's _voxelize
(tests/trimesh_voxel_ref.py, src/conversions.jl:133-207): every grid bit for bit."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import trimesh_voxel_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref_meshes(gpu_fx):
    return [gpu_fx.load_obj(os.path.join(GOLDEN, n)) for n in ("teapot.obj", "sphere.obj")]


@pytest.fixture(scope="module")
def modelnet(gpu_fx):
    return ref.modelnet_meshes(GOLDEN)


def _check(fx, verts, faces, res, on_device=True, faces_dtype=None):
    m = fx.TriMesh(list(verts), list(faces), faces_dtype=faces_dtype)
    if on_device:
        m = fx.gpu(m)
    got = fx.trimesh_to_voxel(m, res)
    assert got.shape == (res, res, res, len(verts)) and got.dtype == np.float32
    g = got.to_host()
    exp = ref.trimesh_to_voxel(verts, faces, res)
    for i in range(len(verts)):
        assert np.array_equal(g[..., i], exp[..., i]), (res, i, int(g[..., i].sum()), int(exp[..., i].sum()))
    return g


def test_reference_case_teapot_and_sphere_res_28(gpu_fx, ref_meshes):
    """test/conversions.jl:5-38: VoxelGrid(load_trimesh(teapot, sphere), 28) -> (28,28,28,2) Float32 in {0, 1}."""
    g = _check(gpu_fx, *zip(*ref_meshes), 28)
    assert set(np.unique(g)) == {0.0, 1.0}
    assert [int(g[..., i].sum()) for i in range(2)] == [1150, 2825]


@pytest.mark.parametrize("res", [1, 2, 3, 32, 64, 128])
def test_teapot_and_sphere_resolutions(gpu_fx, ref_meshes, res):
    _check(gpu_fx, *zip(*ref_meshes), res)


def test_host_mesh_gives_the_same_grid(gpu_fx, ref_meshes):
    _check(gpu_fx, *zip(*ref_meshes), 28, on_device=False)


@pytest.mark.parametrize("res", [32, 64])
def test_modelnet_alone_and_as_one_ragged_batch(gpu_fx, modelnet, res):
    """The 8 committed ModelNet meshes (desk_0001: 602 unreferenced vertices, faces 6-7 levels deep): each alone, then
    all in one ragged batch, which must equal the concatenation of the single calls."""
    singles = [_check(gpu_fx, [v], [f], res)[..., 0] for _, v, f in modelnet]
    batch = _check(gpu_fx, [v for _, v, _ in modelnet], [f for _, _, f in modelnet], res)
    assert np.array_equal(batch, np.stack(singles, axis=-1))


@pytest.mark.parametrize("dtype", [np.uint32, np.int64])
def test_reference_index_types(gpu_fx, ref_meshes, dtype):
    """TriMesh{T,UInt32} and TriMesh{T,Int64}, 1-based, enter through index_upload unchanged."""
    verts, faces = zip(*ref_meshes)
    m = gpu_fx.gpu(gpu_fx.TriMesh(list(verts), [f.astype(dtype) for f in faces]))
    assert m.get_faces_padded().dtype == dtype
    assert np.array_equal(gpu_fx.trimesh_to_voxel(m, 28).to_host(), ref.trimesh_to_voxel(verts, faces, 28))


def _random_mesh(rng, kind):
    if kind == "tiny":  # many small faces in a cloud: few splits, vertices dominate
        V, F = int(rng.integers(3, 400)), int(rng.integers(1, 600))
        v = rng.random((3, V), dtype=np.float32)
    elif kind == "span":  # a few faces spanning the whole unit cube: ~9 levels at res 128
        V, F = int(rng.integers(3, 9)), int(rng.integers(1, 5))
        v = (rng.random((3, V), dtype=np.float32) * 2 - 1).astype(np.float32)
        v[:, :2] = np.array([[-1, 1], [-1, 1], [-1, 1]], np.float32)
    elif kind == "needle":  # needle-thin triangles: one long side, one very short
        F = int(rng.integers(1, 40))
        a = rng.random((3, F), dtype=np.float32)
        b = rng.random((3, F), dtype=np.float32)
        c = (a + np.float32(1e-4) * rng.standard_normal((3, F)).astype(np.float32)).astype(np.float32)
        v = np.concatenate([a, b, c], axis=1)
        V = 3 * F
        f = np.stack([np.arange(F), F + np.arange(F), 2 * F + np.arange(F)]) + 1
        return np.asfortranarray(v), np.asfortranarray(f.astype(np.uint32))
    else:  # "lattice": coordinates on a coarse dyadic grid: sides land exactly on thresholds, points on cell borders
        V, F = int(rng.integers(3, 60)), int(rng.integers(1, 80))
        v = (rng.integers(0, 9, (3, V)) / np.float32(8)).astype(np.float32)
    f = rng.integers(1, V + 1, (3, F)).astype(np.uint32)
    return np.asfortranarray(v.astype(np.float32)), np.asfortranarray(f)


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_random_meshes(gpu_fx, seed):
    rng = np.random.default_rng(9000 + seed)
    kinds = ["tiny", "span", "needle", "lattice"]
    meshes = [_random_mesh(rng, kinds[(seed + i) % 4]) for i in range(int(rng.integers(1, 6)))]
    verts, faces = zip(*meshes)
    for res in (int(rng.integers(1, 20)), (17, 33, 100, 128, 64, 48)[seed]):
        _check(gpu_fx, verts, faces, res)


def test_two_calls_and_a_graph_replay_agree(gpu_fx, modelnet):
    fx = gpu_fx
    verts = [v for _, v, _ in modelnet[:4]]
    faces = [f for _, _, f in modelnet[:4]]
    m = fx.gpu(fx.TriMesh(verts, faces))
    exp = ref.trimesh_to_voxel(verts, faces, 64)
    a = fx.trimesh_to_voxel(m, 64).to_host()
    b = fx.trimesh_to_voxel(m, 64).to_host()
    assert np.array_equal(a, exp) and np.array_equal(b, exp)
    s = fx.Stream.create()
    with fx.stream(s):
        bad = fx.DeviceArray.zeros((1,), np.uint32)
        fx.trimesh_to_voxel(m, 64, bad=bad)  # eager once: workspace and mirrors in place
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            out = fx.trimesh_to_voxel(m, 64, bad=bad)
        for _ in range(2):
            g.launch()
        s.synchronize()
        assert np.array_equal(out.to_host(), exp)
        assert int(bad.to_host()[0]) == 0


@pytest.mark.parametrize("bad", ["flat", "nan", "inf"])
def test_non_finite_mesh_raises_and_the_rest_of_the_batch_is_right(gpu_fx, ref_meshes, bad):
    fx = gpu_fx
    (tv, tf), (sv, sf) = ref_meshes
    v = tv.copy(order="F")
    if bad == "flat":
        v[:] = np.float32(0.5)
    elif bad == "nan":
        v[1, 7] = np.nan
    else:
        v[2, 3] = -np.inf
    m = fx.gpu(fx.TriMesh([sv, v, tv], [sf, tf, tf]))
    with pytest.raises(ValueError):
        fx.trimesh_to_voxel(m, 28)
    cnt = fx.DeviceArray.zeros((1,), np.uint32)
    g = fx.trimesh_to_voxel(m, 28, bad=cnt).to_host()
    assert int(cnt.to_host()[0]) == 1
    assert g[..., 1].sum() == 0
    assert np.array_equal(g[..., 0], ref.voxelize(sv, sf, 28)) and np.array_equal(g[..., 2], ref.voxelize(tv, tf, 28))


def test_more_scan_entries_than_one_round_of_the_scan_block(gpu_fx):
    """600 one-triangle meshes at res 4: B * (chunks + 1) = 1200 entries, two rounds of the one-block scan's 1024 (launch 3),
    so the second round's starts carry the first round's total."""
    rng = np.random.default_rng(4242)
    verts = [np.asfortranarray(rng.random((3, 3), dtype=np.float32)) for _ in range(600)]
    faces = [np.asfortranarray(np.array([[1], [2], [3]], np.uint32)) for _ in range(600)]
    g = _check(gpu_fx, verts, faces, 4)
    assert all(g[..., i].sum() >= 3 for i in (0, 511, 512, 599))  # three distinct corners at least, before and behind the carry


def test_range_with_signed_zeros(gpu_fx):
    """The minimum of the mesh is -0.0 and +0.0 occurs too, in several waves of the range block (1025 vertices: 3075 coordinates
    over 1024 threads): whichever zero the reduction returns, the grid is the restatement's."""
    rng = np.random.default_rng(77)
    v = np.asfortranarray(rng.random((3, 1025), dtype=np.float32))
    flat = v.reshape(-1, order="F")  # a view: element e = coordinate e of the device array
    flat[[0, 70, 1023, 2000, 3074]] = np.float32(-0.0)
    flat[[1, 64, 1024, 2049, 3073]] = np.float32(0.0)
    assert v.min() == 0 and np.signbit(v).sum() == 5 and np.shares_memory(flat, v)
    f = rng.integers(1, 1026, (3, 40)).astype(np.uint32)
    for res in (5, 16):
        _check(gpu_fx, [v], [np.asfortranarray(f)], res)
