"""Representation conversions on the device: pointcloud_to_voxel and trimesh_to_voxel (src/conversions.jl:91-207)."""
import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, current_stream, workspace
from .metrics import _as_dev_points
from .rep import TriMesh
from .transforms import _verts_padded_dev


def pointcloud_to_voxel(pcloud, resolution=32):
    """`pointcloud_to_voxel(pcloud, resolution)` (src/conversions.jl:91-131): occupancy grid
    (res,res,res,B) Float32 on the device; a voxel is set iff the nearest (min/max-normalised) cloud
    point of its lattice centre is within sqrt(0.6)/res.  Same lattice convention as the reference
    (centres (i+0.5)/res for i = 1..res; first array dimension = the innermost loop variable)."""
    x = _as_dev_points(pcloud)
    D, N, B = x.shape
    if D != 3:
        raise ValueError("pointcloud_to_voxel needs 3-D points")
    res = int(resolution)
    nb = C.c_size_t(0)
    _lib.call("fx3d_voxel_workspace_bytes", B, C.byref(nb))
    ws = workspace(nb.value, tag="voxel")
    out = DeviceArray.empty((res, res, res, B), np.float32)
    _lib.call("fx3d_pointcloud_to_voxel", x.ptr, N, B, res, out.ptr, ws.ptr, ws.nbytes, current_stream().handle)
    return out


def trimesh_to_voxel(m, resolution=32, bad=None):
    """`trimesh_to_voxel(m, res)` / `VoxelGrid(m::TriMesh, res)` (src/conversions.jl:74-77, 133-207): occupancy grid
    (res,res,res,B) Float32 0/1 on the device, bit-identical to the reference's `_voxelize` of every mesh (normalise by one
    scalar min / max, split triangles at their midpoints until no side^2 exceeds (1/res)^2, mark trunc(p * (res-1))).
    The first array dimension is the x coordinate (unlike :func:`pointcloud_to_voxel`).

    A mesh the reference cannot voxelise (zero extent, a NaN / Inf coordinate: it throws) raises ``ValueError``; its grid
    would stay zero.  ``bad``: a caller-zeroed device ``uint32`` counter instead -- such meshes are counted there and
    nothing is read back, so the call can be captured into a :class:`Graph`."""
    if not isinstance(m, TriMesh):
        raise TypeError("trimesh_to_voxel needs a TriMesh")
    res = int(resolution)
    if not 1 <= res <= 1024:
        raise ValueError("trimesh_to_voxel: resolution must lie in [1, 1024]")
    verts = _verts_padded_dev(m)
    faces, flen = (m.dev("faces_padded").ptr, m.dev("faces_len").ptr) if m.F > 0 else (None, None)
    B = m.N
    nb = C.c_size_t(0)
    _lib.call("fx3d_trimesh_voxel_workspace_bytes", m.V, m.F, B, res, C.byref(nb))
    ws = workspace(nb.value, tag="trimesh_voxel")
    out = DeviceArray.empty((res, res, res, B), np.float32)
    counter = DeviceArray.zeros((1,), np.uint32) if bad is None else bad
    _lib.call("fx3d_trimesh_to_voxel", verts.ptr, m.V, m.dev("nverts").ptr, faces, m.F, flen, B, res, out.ptr,
              counter.ptr, ws.ptr, ws.nbytes, current_stream().handle)
    if bad is None:
        nbad = int(counter.to_host()[0])
        if nbad:
            raise ValueError(f"trimesh_to_voxel: {nbad} of {B} meshes have zero extent or a non-finite coordinate "
                             "(the reference throws: round(Int, NaN))")
    return out
