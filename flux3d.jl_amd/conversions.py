"""Representation conversions on the device: pointcloud_to_voxel and trimesh_to_voxel (src/conversions.jl:91-207), and
voxel_to_trimesh with algo :Exact and the constructors built on it (src/conversions.jl:1-67, 209-349)."""
import numpy as np

from . import _lib
from .device import DeviceArray, current_stream, is_device, workspace
from .metrics import _as_dev_points
from .rep import PointCloud, TriMesh, VoxelGrid
from .transforms import _verts_padded_dev, sample_points


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
    nb = _lib.query_bytes("fx3d_voxel_workspace_bytes", B)
    ws = workspace(nb, tag="voxel")
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
    nb = _lib.query_bytes("fx3d_trimesh_voxel_workspace_bytes", m.V, m.F, B, res)
    ws = workspace(nb, tag="trimesh_voxel")
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


_ALGOS = ("Exact", "MarchingCubes", "MarchingTetrahedra", "NaiveSurfaceNets")
# cube_faces (src/conversions.jl:313-349): the 12 faces of one cube, 1-based into its 8 vertices
_CUBE_FACES = np.array([1, 7, 5, 1, 3, 7, 1, 4, 3, 1, 2, 4, 3, 8, 7, 3, 4, 8,
                        5, 7, 8, 5, 8, 6, 1, 5, 6, 1, 6, 2, 2, 6, 8, 2, 8, 4], dtype=np.uint32)


def _check_algo(algo):
    """The reference's algo check (src/conversions.jl:210-212); the Meshing.jl algos are not available on the device."""
    name = str(algo)[1:] if str(algo).startswith(":") else str(algo)
    if name not in _ALGOS:
        raise ValueError(f"given algo: {algo} is not supported. Accepted algo are "
                         "{:Exact,:MarchingCubes, :MarchingTetrahedra, :NaiveSurfaceNets}.")
    if name != "Exact":
        raise NotImplementedError(f"voxel_to_trimesh: algo :{name} runs Meshing.jl's isosurface, which this library "
                                  "does not implement; use algo=\"Exact\"")


def _cube_faces(K):
    """The faces _voxel_exact appends for K cubes: (3, 12K) UInt32, 1-based, cube j's 12 faces + 8j."""
    f = np.tile(_CUBE_FACES, K) + np.repeat(np.arange(K, dtype=np.uint32) * np.uint32(8), 36)
    return np.asfortranarray(f.reshape((3, 12 * K), order="F"))


def _voxel_mesh(v, thresh, faces):
    """fx3d_voxel_mesh_count + _emit on grid(s) v: (verts_packed (3, 8 sum K) device, K (B) int64 host,
    faces_padded (3, 12 max K, B) int32 0-based device or None).  One host synchronisation: the B counts."""
    vg = VoxelGrid(v)  # shape checks (cubic, 3-D / 4-D) before any device call
    vox = vg.voxels if vg.on_device else DeviceArray.from_host(vg.voxels)
    res, B = vox.shape[0], vox.shape[3]
    if not 1 <= res <= 1024:
        raise ValueError("voxel_to_trimesh: resolution must lie in [1, 1024]")
    nb = _lib.query_bytes("fx3d_voxel_mesh_workspace_bytes", res, B)
    ws = workspace(nb, tag="voxel_mesh")
    st = current_stream().handle
    counts = DeviceArray.empty((2 * B,), np.int64)  # K (B int64), then the invalid-element counts (B uint32)
    _lib.call("fx3d_voxel_mesh_count", vox.ptr, res, B, float(np.float32(thresh)), counts.ptr, counts.ptr + 8 * B,
              ws.ptr, ws.nbytes, st)
    h = counts.to_host()
    K, nbad = h[:B].copy(), h[B:].view(np.uint32)[:B]
    for i in range(B):
        if nbad[i]:
            raise ValueError(f"invalid VoxelGrid, found element which is not between [0,1]: grid {i} (0-based) has "
                             f"{int(nbad[i])}")
    for i in range(B):
        if K[i] == 0:
            raise ValueError(f"voxel_to_trimesh: grid {i} (0-based) has no cell >= thresh left (the reference's "
                             "maximum of an empty array throws)")
    if int(K.max()) * 8 >= 2 ** 31:
        raise ValueError("voxel_to_trimesh: more than 2^31 vertices in one grid (face ids are int32 on the device)")
    total = int(K.sum())
    verts = DeviceArray.empty((3, 8 * total), np.float32)
    Fmax = 12 * int(K.max())
    fp = DeviceArray.empty((3, Fmax, B), np.int32) if faces else None
    _lib.call("fx3d_voxel_mesh_emit", res, B, total, verts.ptr, fp.ptr if fp else None, Fmax if fp else 0,
              ws.ptr, ws.nbytes, st)
    return verts, K, fp


def voxel_to_trimesh(v, thresh=0.5, algo="MarchingCubes"):
    """`voxel_to_trimesh(v::VoxelGrid, thresh, algo)` (src/conversions.jl:209-232) with algo ``"Exact"`` (``_voxel_exact``,
    :246-349): ``(verts_list, faces_list)``.  ``v``: a :class:`VoxelGrid` or a host / device (N,N,N[,B]) array.  Every grid
    is binarised at ``Float32(thresh)``, its interior cells are removed, and each remaining cell becomes 8 vertices and 12
    faces; ``verts_list[i]`` is (3, 8K) Float32 divided by the grid's largest coordinate -- device views for a device grid,
    numpy arrays for a host one -- and ``faces_list[i]`` (3, 12K) UInt32 1-based, like the reference.

    The Meshing.jl algos raise ``NotImplementedError``; any other algo ``ValueError``.  A grid with an element outside
    [0, 1] or NaN, or with no cell left (K = 0), raises ``ValueError`` naming its index.  The call reads the B cube counts
    back (one host synchronisation): it is eager only, not graph-capturable."""
    _check_algo(algo)
    on_device = is_device(v.voxels if isinstance(v, VoxelGrid) else v)
    verts, K, _ = _voxel_mesh(v, thresh, faces=False)
    offs = np.concatenate([[0], np.cumsum(K)])
    vl = [DeviceArray(verts.ptr + 96 * int(offs[i]), (3, 8 * int(K[i])), np.float32, keep=verts) for i in range(len(K))]
    if not on_device:
        vl = [a.to_host() for a in vl]
    return vl, [_cube_faces(int(k)) for k in K]


def trimesh_from_voxels(v, thresh=0.5, algo="MarchingCubes"):
    """`TriMesh(v::VoxelGrid; thresh, algo)` (src/conversions.jl:28-31): a device-backed :class:`TriMesh` whose packed
    vertices are the kernel's output (no host round trip) and whose device faces (padded, lengths, vertex counts) are
    written by the same call; the host face lists are built on first use.  Eager only (one host synchronisation for
    the B cube counts); errors as :func:`voxel_to_trimesh`."""
    _check_algo(algo)
    verts, K, fp = _voxel_mesh(v, thresh, faces=True)
    counts = [int(k) for k in K]
    m = TriMesh._from_device(verts, 8 * K, 12 * K, lambda: [_cube_faces(k) for k in counts])
    m._topo_dev["faces_padded"] = fp
    m._topo_dev["faces_len"] = DeviceArray.from_host((12 * K).astype(np.int32))
    m._topo_dev["nverts"] = DeviceArray.from_host((8 * K).astype(np.int32))
    return m


def pointcloud_from_voxels(v, npoints=1000, thresh=0.5, algo="MarchingCubes", seed=None):
    """`PointCloud(v::VoxelGrid, npoints; thresh, algo)` (src/conversions.jl:56-67): :func:`trimesh_from_voxels`, then
    the device :func:`sample_points` (``seed`` as there).  The points are a (3, npoints, B) Float32 device array.
    Eager only (one host synchronisation)."""
    m = trimesh_from_voxels(v, thresh, algo)
    return PointCloud(sample_points(m, npoints, seed=seed))


def trimesh_from_pointcloud(p, resolution=32, algo="MarchingCubes"):
    """`TriMesh(p::PointCloud, res; algo)` (src/conversions.jl:11-15): :func:`pointcloud_to_voxel` at ``resolution``, then
    :func:`trimesh_from_voxels` with the reference's default ``thresh = 0.5``.  Eager only (one host synchronisation)."""
    _check_algo(algo)
    return trimesh_from_voxels(pointcloud_to_voxel(p, resolution), 0.5, algo)
