"""Literal numpy restatement of the reference's voxel_to_trimesh with algo :Exact, the checker of fx3d_voxel_mesh_*.

``voxel_to_trimesh`` / ``_voxel_exact`` / ``_add_face!`` (src/conversions.jl:209-232, 246-349), grid by grid:
``_assert_voxel`` (src/rep/voxels.jl:53) over the whole batch first, then ``voxel .>= Float32(thresh)``, the interior
removal for ``res >= 3`` with a right-hand side read from the un-eroded grid, one cube per remaining cell in column-major
order (first index x fastest), and ``v ./ maximum(v)`` in Float32.  Where the reference throws (an element outside [0, 1]
or NaN; a grid without a remaining cell, whose ``maximum`` is over an empty array) this raises ``ValueError``.  Test
infrastructure only: the library never calls it.
"""
import numpy as np

# _add_face! (:290-349): the 8 corners of cell (x,y,z) as offsets from (x-1,y-1,z-1), and the 12 faces, 1-based
CUBE_VERTS = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]], np.int64)
CUBE_FACES = np.array([1, 7, 5, 1, 3, 7, 1, 4, 3, 1, 2, 4, 3, 8, 7, 3, 4, 8,
                       5, 7, 8, 5, 8, 6, 1, 5, 6, 1, 6, 2, 2, 6, 8, 2, 8, 4], np.int64)


def assert_voxel(voxels):
    """_assert_voxel: all(0.0 .<= v .<= 1.0) -- NaN fails."""
    v = np.asarray(voxels, dtype=np.float32)
    return bool(np.all((v >= 0.0) & (v <= 1.0)))


def surviving_cells(voxel, thresh):
    """Steps 2-3 of _voxel_exact for one (res,res,res) grid: the boolean grid after the interior removal."""
    v = np.asarray(voxel, dtype=np.float32) >= np.float32(thresh)
    res = v.shape[0]
    if res >= 3:
        i = slice(1, res - 1)
        lo, hi = slice(0, res - 2), slice(2, res)
        interior = (v[lo, i, i] & v[hi, i, i] & v[i, lo, i] & v[i, hi, i] & v[i, i, lo] & v[i, i, hi])
        v = v.copy()
        v[i, i, i] = v[i, i, i] & ~interior  # the right-hand side was computed from the un-eroded grid
    return v


def voxel_exact(voxel, thresh):
    """_voxel_exact(voxel, thresh, :Exact) for one grid: (verts (3, 8K) Float32 un-normalised, faces (3, 12K) UInt32)."""
    v = surviving_cells(voxel, thresh)
    # CartesianIndices order: first index fastest == the F-order flattening; 1-based (x, y, z)
    flat = np.flatnonzero(v.reshape(-1, order="F"))
    x, y, z = np.unravel_index(flat, v.shape, order="F")
    xyz = np.stack([x, y, z], axis=1) + 1
    K = len(flat)
    corners = (xyz[:, None, :] - 1) + CUBE_VERTS[None, :, :]  # (K, 8, 3)
    verts = np.asfortranarray(corners.reshape(8 * K, 3).T.astype(np.float32))
    faces = (CUBE_FACES[None, :] + 8 * np.arange(K, dtype=np.int64)[:, None]).reshape(-1)
    return verts, np.asfortranarray(faces.reshape((3, 12 * K), order="F").astype(np.uint32))


def voxel_to_trimesh(voxels, thresh):
    """voxel_to_trimesh(VoxelGrid(voxels), Float32(thresh), :Exact): (verts_list, faces_list)."""
    vox = np.asarray(voxels, dtype=np.float32)
    if vox.ndim == 3:
        vox = vox[..., None]
    if not assert_voxel(vox):
        raise ValueError("invalid VoxelGrid, found element which is not between [0,1].")
    verts, faces = [], []
    for i in range(vox.shape[3]):
        v, f = voxel_exact(vox[..., i], thresh)
        if v.size == 0:
            raise ValueError(f"grid {i}: maximum of an empty array")
        verts.append(np.asfortranarray(v / v.max()))  # Float32 ./ Float32
        faces.append(f)
    return verts, faces


def first_bad_grid(voxels, thresh):
    """Index of the grid the device path names: the first invalid grid, else the first empty one, else None."""
    vox = np.asarray(voxels, dtype=np.float32)
    for i in range(vox.shape[3]):
        if not assert_voxel(vox[..., i]):
            return i
    for i in range(vox.shape[3]):
        if not surviving_cells(vox[..., i], thresh).any():
            return i
    return None


def reference_test_grid():
    """test/conversions.jl:3-5: zeros(32,32,32,2) with [1:15, 2:10, 18:32, :] .= 1."""
    v = np.zeros((32, 32, 32, 2), np.float32, order="F")
    v[0:15, 1:10, 17:32, :] = 1
    return v


def checkerboard(res, B=1):
    i = np.indices((res, res, res)).sum(axis=0)
    g = ((i % 2) == 0).astype(np.float32)
    return np.asfortranarray(np.repeat(g[..., None], B, axis=3))
