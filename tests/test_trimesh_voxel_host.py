"""trimesh_to_voxel without a GPU: the host restatement (tests/trimesh_voxel_ref.py) on cases derived by hand and on the
reference's own test meshes, and the C ABI / Python entry points of fx3d_trimesh_to_voxel (argument checks run before any
device call)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
import trimesh_voxel_ref as ref

RIGHT_TRIANGLE = (np.array([[0, 1, 0], [0, 0, 1], [0, 0, 0]], np.float32), np.array([[1], [2], [3]], np.uint32))


def _set(vox):
    return sorted(map(tuple, np.argwhere(vox).tolist()))


@pytest.mark.parametrize("res,levels,cells", [
    # res 1: threshold 1.0 < 2 (the hypotenuse^2): one level; every point lands in voxel 0
    (1, 1, [(0, 0, 0)]),
    # res 2: sides^2 2 -> 0.5 -> 0.125 against 0.25: two levels, points on the 1/4 lattice; only x = 1 or y = 1 reach index 1
    (2, 2, [(0, 0, 0), (0, 1, 0), (1, 0, 0)]),
    # res 3: 0.125 > 1/9 -> three levels, the 1/8 lattice; trunc(2p): [0,.5) -> 0, [.5,1) -> 1, 1 -> 2; x + y <= 1
    (3, 3, [(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 0, 0), (1, 1, 0), (2, 0, 0)]),
    # res 4: 0.125 > 1/16 > 0.03125 -> three levels; trunc(3k/8): k 0-2 -> 0, 3-5 -> 1, 6-7 -> 2, 8 -> 3
    (4, 3, [(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0), (1, 0, 0), (1, 1, 0), (2, 0, 0), (3, 0, 0)]),
])
def test_restatement_right_triangle(res, levels, cells):
    vox, L, _ = ref.voxelize(*RIGHT_TRIANGLE, res, return_stats=True)
    assert L == levels
    assert _set(vox) == cells


def test_restatement_axis_order_x_is_the_first_dimension():
    """A triangle in the x = 0 plane only sets voxels with index 0 in the FIRST dimension (the reference's idx[1, :])."""
    v = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    vox = ref.voxelize(v, RIGHT_TRIANGLE[1], 8)
    assert vox[0].sum() == vox.sum() > 10 and vox.flags.f_contiguous


def test_restatement_point_like_mesh_with_an_unreferenced_far_vertex():
    """A tiny face never splits; the vertex no face uses still takes part in the range and is a point of its own."""
    v = np.array([[0, 1e-3, 0, 1], [0, 0, 1e-3, 1], [0, 0, 0, 1]], np.float32)
    f = np.array([[1], [2], [3]], np.int64)
    for res in (1, 2, 32, 128):
        vox, L, P = ref.voxelize(v, f, res, return_stats=True)
        assert (L, P) == (0, 4)
        assert _set(vox) == sorted({(0, 0, 0), (res - 1,) * 3})


def test_restatement_threshold_is_compared_in_double():
    """Sides^2 equal to (1/res)^2 in Float32 but not in Float64: the reference's Float32 > Float64 compare decides."""
    res = 10
    t = np.float32(0.1)  # Float32(0.1)^2 as a Float32 differs from the Float64 0.01
    s = np.float32(t * t)
    v = np.array([[0, t, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1]], np.float32)
    f = np.array([[1], [2], [3]], np.int64)
    _, L, _ = ref.voxelize(v, f, res, return_stats=True)
    assert L == (1 if float(s) > (1.0 / res) ** 2 else 0)
    assert float(s) != (1.0 / res) ** 2


@pytest.mark.parametrize("bad", ["flat", "nan", "inf"])
def test_restatement_raises_on_non_finite_normalisation(bad):
    v = np.ones((3, 3), np.float32) if bad == "flat" else RIGHT_TRIANGLE[0].copy()
    if bad == "nan":
        v[1, 2] = np.nan
    if bad == "inf":
        v[0, 1] = np.inf
    with pytest.raises(ValueError):
        ref.voxelize(v, RIGHT_TRIANGLE[1], 8)


@pytest.mark.parametrize("name,levels,points,voxels", [("teapot.obj", 2, 13130, 1150), ("sphere.obj", 1, 17922, 2825)])
def test_restatement_reference_meshes_at_res_28(fx, name, levels, points, voxels):
    """test/conversions.jl:5-38 voxelises teapot + sphere at res 28."""
    v, f = fx.load_obj(os.path.join(GOLDEN, name))
    vox, L, P = ref.voxelize(v, f, 28, return_stats=True)
    assert (L, P, int(vox.sum())) == (levels, points, voxels)
    assert set(np.unique(vox)) == {0.0, 1.0}


def test_trimesh_to_voxel_is_exported(fx):
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "fx3d_trimesh_to_voxel") and hasattr(lib, "fx3d_trimesh_voxel_workspace_bytes")
    assert "fx3d_trimesh_to_voxel" in _lib.SIGNATURES
    from flux3d_jl_amd.conversions import trimesh_to_voxel
    assert fx.trimesh_to_voxel is trimesh_to_voxel


def test_trimesh_voxel_workspace_query_and_argument_checks(fx):
    from flux3d_jl_amd import _lib
    n = C.c_size_t(0)
    _lib.call("fx3d_trimesh_voxel_workspace_bytes", 12036, 8748, 8, 64, C.byref(n))
    assert n.value >= 8 * 8748 * 8 + 8 * 9  # per-face leaf-slot offsets (int64) + per-mesh offsets
    m = C.c_size_t(0)
    _lib.call("fx3d_trimesh_voxel_workspace_bytes", 12036, 0, 8, 64, C.byref(m))  # meshes without faces
    assert 0 < m.value < n.value
    for args in [(0, 10, 1, 32), (10, 10, 0, 32), (10, 10, 1, 0), (10, 10, 1, 1025), (10, -1, 1, 32)]:
        with pytest.raises(_lib.Flux3DHipError):
            _lib.call("fx3d_trimesh_voxel_workspace_bytes", *args, C.byref(n))
    # null pointers and bad sizes are refused before any device call
    with pytest.raises(_lib.Flux3DHipError, match="null"):
        _lib.call("fx3d_trimesh_to_voxel", None, 3, None, None, 1, None, 1, 32, None, None, None, 0, None)
    dummy = C.c_void_p(16)
    with pytest.raises(_lib.Flux3DHipError, match="bad sizes"):
        _lib.call("fx3d_trimesh_to_voxel", dummy, 3, dummy, dummy, 1, dummy, 1, 2048, dummy, None, dummy, 1 << 20, None)
    with pytest.raises(_lib.Flux3DHipError, match="workspace"):
        _lib.call("fx3d_trimesh_to_voxel", dummy, 3, dummy, dummy, 1, dummy, 1, 32, dummy, None, dummy, 8, None)


def test_python_wrapper_checks_before_the_device(fx):
    m = fx.TriMesh([RIGHT_TRIANGLE[0]], [RIGHT_TRIANGLE[1]])
    with pytest.raises(ValueError):
        fx.trimesh_to_voxel(m, 0)
    with pytest.raises(ValueError):
        fx.trimesh_to_voxel(m, 1025)
    with pytest.raises(TypeError):
        fx.trimesh_to_voxel(RIGHT_TRIANGLE[0], 32)
