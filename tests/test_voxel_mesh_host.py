"""voxel_to_trimesh (algo :Exact) without a GPU: the host restatement (tests/voxel_mesh_ref.py) on the known answers
derived by hand, the C ABI's argument checks (refused before any device call), and the Python layer's checks."""
import ctypes as C

import numpy as np
import pytest

import voxel_mesh_ref as ref


def _k(vox, thresh=0.5):
    return int(ref.surviving_cells(vox, thresh).sum())


def test_reference_test_grid_known_answer():
    """test/conversions.jl's grid at thresh 0.9: 15*9*15 = 2025 cells, 13*7*13 = 1183 interior ones (x = 1 and z = 32
    lie on the grid border), so K = 842 per grid, 6736 vertices, 10104 faces, normaliser 32."""
    v = ref.reference_test_grid()
    verts, faces = ref.voxel_to_trimesh(v, np.float32(0.9))
    assert len(verts) == len(faces) == 2
    for vb, fb in zip(verts, faces):
        assert vb.shape == (3, 6736) and fb.shape == (3, 10104)
        assert vb.dtype == np.float32 and fb.dtype == np.uint32
        raw, _ = ref.voxel_exact(v[..., 0], np.float32(0.9))
        assert raw.max() == 32
        assert np.array_equal(vb, raw / np.float32(32))
        # first cube: cell (1,2,18), its first vertex (0,1,17)/32; last cube: cell (15,10,32), last vertex (15,10,32)/32
        assert np.array_equal(raw[:, 0], [0, 1, 17]) and np.array_equal(raw[:, 7], [1, 2, 18])
        assert np.array_equal(raw[:, -8], [14, 9, 31]) and np.array_equal(raw[:, -1], [15, 10, 32])
        assert np.array_equal(vb[:, 0], np.array([0, 1, 17], np.float32) / np.float32(32))
        assert fb.min() == 1 and fb.max() == 6736
    assert np.array_equal(verts[0], verts[1]) and np.array_equal(faces[0], faces[1])


@pytest.mark.parametrize("res,K", [(1, 1), (2, 8), (3, 26), (4, 56), (32, 32 ** 3 - 30 ** 3)])
def test_full_grids(res, K):
    assert _k(np.ones((res, res, res), np.float32)) == K


def test_checkerboard_keeps_every_set_cell():
    v = ref.checkerboard(64)[..., 0]
    assert _k(v) == int(v.sum()) == 131072


def test_single_voxel_is_exactly_the_two_tables():
    verts, faces = ref.voxel_to_trimesh(np.ones((1, 1, 1), np.float32), 0.5)
    exp_v = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]], np.float32).T
    exp_f = np.array([[1, 7, 5], [1, 3, 7], [1, 4, 3], [1, 2, 4], [3, 8, 7], [3, 4, 8], [5, 7, 8], [5, 8, 6], [1, 5, 6],
                      [1, 6, 2], [2, 6, 8], [2, 8, 4]], np.uint32).T
    assert np.array_equal(verts[0], exp_v) and np.array_equal(faces[0], exp_f)


def test_second_cube_faces_are_offset_by_eight():
    v = np.zeros((2, 2, 2), np.float32)
    v[0, 0, 0] = v[1, 1, 1] = 1
    verts, faces = ref.voxel_to_trimesh(v, 0.5)
    assert np.array_equal(faces[0][:, 12:], faces[0][:, :12] + 8)
    assert np.array_equal(verts[0][:, 8:] * 2, verts[0][:, :8] * 2 + 1)


def test_cell_next_to_the_border_of_an_otherwise_full_grid():
    """res 5, everything set but cell (1,3,3) (1-based), which lies on the x = 1 face: the interior cell (2,3,3) loses its
    x-1 neighbour and survives; every other interior cell is still cleared; border cells are never cleared."""
    v = np.ones((5, 5, 5), np.float32)
    v[0, 2, 2] = 0
    s = ref.surviving_cells(v, 0.5)
    assert not s[0, 2, 2] and s[1, 2, 2]
    assert int(s[1:4, 1:4, 1:4].sum()) == 1
    assert _k(v) == (125 - 27) - 1 + 1
    # an interior hole: its six neighbours survive (they see it in the un-eroded grid), nothing else inside does
    w = np.ones((5, 5, 5), np.float32)
    w[2, 2, 2] = 0
    t = ref.surviving_cells(w, 0.5)
    assert int(t[1:4, 1:4, 1:4].sum()) == 6 and _k(w) == 98 + 6


def test_threshold_equal_value_is_set():
    v = np.full((2, 2, 2), np.float32(0.9), np.float32)
    assert _k(v, np.float32(0.9)) == 8
    assert _k(v, np.nextafter(np.float32(0.9), np.float32(1))) == 0


@pytest.mark.parametrize("bad", [np.nan, -0.5, np.float32(1.0000001)])
def test_restatement_raises_on_invalid_elements(bad):
    v = np.ones((3, 3, 3, 2), np.float32)
    v[1, 0, 2, 1] = bad
    assert not ref.assert_voxel(v)
    with pytest.raises(ValueError):
        ref.voxel_to_trimesh(v, 0.5)
    assert ref.first_bad_grid(v, 0.5) == 1


def test_restatement_raises_on_an_empty_grid():
    v = np.ones((4, 4, 4, 3), np.float32)
    v[..., 2] = 0.25
    with pytest.raises(ValueError):
        ref.voxel_to_trimesh(v, 0.5)
    assert ref.first_bad_grid(v, 0.5) == 2


def test_voxel_mesh_is_exported(fx):
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    for name in ("fx3d_voxel_mesh_workspace_bytes", "fx3d_voxel_mesh_count", "fx3d_voxel_mesh_emit"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    from flux3d_jl_amd import conversions
    for name in ("voxel_to_trimesh", "trimesh_from_voxels", "pointcloud_from_voxels", "trimesh_from_pointcloud"):
        assert getattr(fx, name) is getattr(conversions, name)


def test_workspace_query_and_argument_checks(fx):
    from flux3d_jl_amd import _lib
    n = C.c_size_t(0)
    _lib.call("fx3d_voxel_mesh_workspace_bytes", 128, 8, C.byref(n))
    assert n.value >= 2 * 8 * (128 * 128 * 2) * 8  # occupancy + survivor words
    for res, B in [(0, 1), (1025, 1), (-3, 1), (32, 0), (32, -1)]:
        with pytest.raises(_lib.Flux3DHipError):
            _lib.call("fx3d_voxel_mesh_workspace_bytes", res, B, C.byref(n))
    with pytest.raises(_lib.Flux3DHipError):
        _lib.call("fx3d_voxel_mesh_workspace_bytes", 32, 1, None)
    d = C.c_void_p(256)
    _lib.call("fx3d_voxel_mesh_workspace_bytes", 32, 2, C.byref(n))
    big = n.value
    with pytest.raises(_lib.Flux3DHipError, match="null"):
        _lib.call("fx3d_voxel_mesh_count", None, 32, 2, 0.5, d, d, d, big, None)
    for i in (4, 5, 6):  # cubes_dev, bad_dev, ws
        args = [d, 32, 2, 0.5, d, d, d, big, None]
        args[i] = None
        with pytest.raises(_lib.Flux3DHipError, match="null"):
            _lib.call("fx3d_voxel_mesh_count", *args)
    for res, B in [(0, 2), (1025, 2), (32, 0)]:
        with pytest.raises(_lib.Flux3DHipError, match="bad sizes"):
            _lib.call("fx3d_voxel_mesh_count", d, res, B, 0.5, d, d, d, 1 << 40, None)
    with pytest.raises(_lib.Flux3DHipError, match="workspace"):
        _lib.call("fx3d_voxel_mesh_count", d, 32, 2, 0.5, d, d, d, big - 1, None)
    with pytest.raises(_lib.Flux3DHipError, match="null"):
        _lib.call("fx3d_voxel_mesh_emit", 32, 2, 10, d, None, 0, None, big, None)
    with pytest.raises(_lib.Flux3DHipError, match="null"):
        _lib.call("fx3d_voxel_mesh_emit", 32, 2, 10, None, None, 0, d, big, None)
    for res, B, cap, Fmax in [(0, 2, 10, 0), (1025, 2, 10, 0), (32, 0, 10, 0), (32, 2, -1, 0)]:
        with pytest.raises(_lib.Flux3DHipError, match="bad sizes"):
            _lib.call("fx3d_voxel_mesh_emit", res, B, cap, d, None, Fmax, d, 1 << 40, None)
    with pytest.raises(_lib.Flux3DHipError, match="bad sizes"):  # faces without room
        _lib.call("fx3d_voxel_mesh_emit", 32, 2, 10, d, d, 0, d, big, None)
    with pytest.raises(_lib.Flux3DHipError, match="workspace"):
        _lib.call("fx3d_voxel_mesh_emit", 32, 2, 10, d, d, 120, d, big - 1, None)


def test_voxelgrid_lifts_and_rejects_shapes(fx):
    g = fx.VoxelGrid(np.zeros((4, 4, 4)))
    assert g.voxels.shape == (4, 4, 4, 1) and g.voxels.dtype == np.float32 and g.voxels.flags.f_contiguous
    assert fx.VoxelGrid(np.zeros((3, 3, 3, 5), np.float64)).voxels.shape == (3, 3, 3, 5)
    assert fx.VoxelGrid(g).voxels is g.voxels
    v = np.random.default_rng(0).random((2, 2, 2, 3)).astype(np.float32)
    assert np.array_equal(fx.VoxelGrid(v)[1], v[..., 1])
    assert "Batch size: 3" in repr(fx.VoxelGrid(v)) and "Voxels features: 2" in repr(fx.VoxelGrid(v))
    assert fx.cpu(fx.VoxelGrid(v)).voxels is not None  # a host grid stays as it is
    for shape in [(4, 4, 5), (4, 5, 4, 2), (5, 4, 4, 1), (4, 4), (4, 4, 4, 1, 1)]:
        with pytest.raises(ValueError):
            fx.VoxelGrid(np.zeros(shape, np.float32))


def test_python_layer_checks_before_the_device(fx):
    cube = np.ones((3, 3, 3, 1), np.float32)
    for fn in (fx.voxel_to_trimesh, fx.trimesh_from_voxels):
        with pytest.raises(ValueError):
            fn(np.ones((3, 3, 4, 1), np.float32), 0.5, "Exact")
        with pytest.raises(ValueError, match="not supported"):
            fn(cube, 0.5, "Marching")
        with pytest.raises(ValueError, match="not supported"):
            fn(cube, 0.5, ":exact")
        for algo in ("MarchingCubes", ":MarchingTetrahedra", "NaiveSurfaceNets"):
            with pytest.raises(NotImplementedError, match="Exact"):
                fn(cube, 0.5, algo)
    with pytest.raises(NotImplementedError, match="Exact"):  # the reference's default algo
        fx.voxel_to_trimesh(cube)
    with pytest.raises(NotImplementedError, match="Exact"):
        fx.pointcloud_from_voxels(cube, 100, 0.5, "MarchingCubes")
    with pytest.raises(ValueError, match="not supported"):
        fx.trimesh_from_pointcloud(np.zeros((3, 10), np.float32), 8, "Bogus")
    with pytest.raises(ValueError):
        fx.voxel_to_trimesh(np.ones((2, 2, 3), np.float32), 0.5, "Exact")
