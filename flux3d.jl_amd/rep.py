"""PointCloud / TriMesh: host-side mirror of the reference's types for the hot path.

* ``PointCloud``  -- src/rep/pcloud.jl:25-84: ``points`` is ``(D, N, B)`` Float32 (column-major,
  i.e. an F-ordered numpy array or a :class:`DeviceArray`), optional ``normals``.
* ``TriMesh``     -- src/rep/mesh.jl:70-231, 344-567, 838-1002: batched heterogeneous triangle
  meshes in list / packed ``(3, sumV)`` / padded ``(3, Vmax, B)`` form with the same lazy validity
  flags; faces are integer and stay on the host in the reference (:87-97) -- here they also get a
  cached int32 0-based device mirror because the kernels gather through them.
* ``VoxelGrid``    -- src/rep/voxels.jl:21-55: ``voxels`` is ``(N, N, N, B)`` Float32 (a 3-D grid is lifted to B = 1).

Faces keep the reference's 1-based numbering at this level (``index_base=1``), so fixtures copied
from the reference's tests read the same; the C ABI takes 0-based int32.
"""
import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, current_stream, is_device


def _f32(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float32))


class PointCloud:
    """PointCloud(points, normals=None) -- src/rep/pcloud.jl:25-55."""

    def __init__(self, points, normals=None):
        if isinstance(points, PointCloud):
            points, normals = points.points, points.normals
        self.points = self._lift(points)
        self.normals = None if normals is None else self._lift(normals)
        if self.normals is not None and self.normals.shape[1] != self.points.shape[1]:
            raise ValueError("number of points and normals must match in PointCloud.")

    @staticmethod
    def _lift(a):
        if is_device(a):
            if a.dtype != np.float32:
                raise TypeError("PointCloud device storage must be Float32")
            return a.reshape(a.shape + (1,)) if a.ndim == 2 else a
        a = _f32(a)
        if a.ndim == 2:  # (D,N) -> (D,N,1), src/rep/pcloud.jl:30-44
            a = a.reshape(a.shape[0], a.shape[1], 1, order="F")
        if a.ndim != 3:
            raise ValueError("points must be (D,N) or (D,N,B)")
        return a

    def __getitem__(self, index):  # p[i] -> points[:, :, i]  (:66), 0-based here
        pts = self.points.to_host() if is_device(self.points) else self.points
        return pts[:, :, index]

    @property
    def on_device(self):
        return is_device(self.points)

    def _to_device(self):
        if self.on_device:
            return self
        return PointCloud(DeviceArray.from_host(self.points),
                          None if self.normals is None else DeviceArray.from_host(self.normals))

    def _to_host(self):
        if not self.on_device:
            return self
        return PointCloud(self.points.to_host(),
                          None if self.normals is None else self.normals.to_host())

    def __repr__(self):
        D, N, B = self.points.shape
        return (f"PointCloud{{Float32}} Structure:\n    Batch size: {B}\n    Points: {N}\n"
                f"    Normals {0 if self.normals is None else self.normals.shape[1]}\n"
                f"    Storage type: {type(self.points).__name__}")


def npoints(p):
    """npoints(p::PointCloud), src/rep/pcloud.jl:84."""
    return p.points.shape[1]


class VoxelGrid:
    """VoxelGrid(voxels) -- src/rep/voxels.jl:21-55: ``voxels`` is ``(N, N, N, B)`` Float32 (column-major, an F-ordered
    numpy array or a :class:`DeviceArray`); a 3-D array is lifted to ``B = 1``.  Unlike the reference, a grid that is not
    cubic or not 3-D / 4-D is refused here (every consumer of the reference's grids assumes res^3)."""

    def __init__(self, voxels):
        if isinstance(voxels, VoxelGrid):
            voxels = voxels.voxels
        if is_device(voxels):
            if voxels.dtype != np.float32:
                raise TypeError("VoxelGrid device storage must be Float32")
            v = voxels.reshape(voxels.shape + (1,)) if voxels.ndim == 3 else voxels
        else:
            v = _f32(voxels)
            if v.ndim == 3:  # (N,N,N) -> (N,N,N,1), src/rep/voxels.jl:34-37
                v = v.reshape(v.shape + (1,), order="F")
        if v.ndim != 4 or not v.shape[0] == v.shape[1] == v.shape[2]:
            raise ValueError(f"VoxelGrid needs (N,N,N) or (N,N,N,B) voxels, got shape {tuple(voxels.shape)}")
        self.voxels = v

    def __getitem__(self, index):  # v[i] -> voxels[:, :, :, i]  (:43), 0-based here
        vox = self.voxels.to_host() if is_device(self.voxels) else self.voxels
        return vox[:, :, :, index]

    @property
    def on_device(self):
        return is_device(self.voxels)

    def _to_device(self):
        return self if self.on_device else VoxelGrid(DeviceArray.from_host(self.voxels))

    def _to_host(self):
        return VoxelGrid(self.voxels.to_host()) if self.on_device else self

    def __repr__(self):
        return (f"VoxelGrid{{Float32}} Structure:\n    Batch size: {self.voxels.shape[3]}\n"
                f"    Voxels features: {self.voxels.shape[0]}\n    Storage type: {type(self.voxels).__name__}")


# ------------------------------------------------------------------------------------ converters
def _list_to_packed(lst):
    """src/rep/utils.jl:95-101."""
    return np.asfortranarray(np.concatenate(lst, axis=1))


def _list_to_padded(lst, pad_value=0, pad_size=None):
    """src/rep/utils.jl:51-93."""
    if pad_size is None:
        pad_size = (max(x.shape[0] for x in lst), max(x.shape[1] for x in lst))
    out = np.full((pad_size[0], pad_size[1], len(lst)), pad_value, dtype=lst[0].dtype, order="F")
    for i, x in enumerate(lst):
        out[: x.shape[0], : x.shape[1], i] = x
    return out


def _packed_to_padded(packed, items_len, pad_value=0):
    """src/rep/utils.jl:119-139."""
    M = int(max(items_len))
    out = np.full((packed.shape[0], M, len(items_len)), pad_value, dtype=packed.dtype, order="F")
    cur = 0
    for i, n in enumerate(items_len):
        out[:, :n, i] = packed[:, cur:cur + n]
        cur += n
    return out


def _packed_to_list(packed, items_len):
    """src/rep/utils.jl:141-157."""
    out, cur = [], 0
    for n in items_len:
        out.append(np.asfortranarray(packed[:, cur:cur + n]))
        cur += n
    return out


def _padded_to_packed(padded, items_len):
    """src/rep/utils.jl:159-181."""
    return np.asfortranarray(np.concatenate([padded[:, :n, i] for i, n in enumerate(items_len)], axis=1))


def _padded_to_list(padded, items_len):
    """src/rep/utils.jl:183-206."""
    return [np.asfortranarray(padded[:, :n, i]) for i, n in enumerate(items_len)]


def _auxiliary_mesh(lst):
    """src/rep/utils.jl:31-49 (1-based first indices, like the reference)."""
    items_len = np.array([x.shape[1] for x in lst], dtype=np.int64)
    first = np.concatenate([[1], 1 + np.cumsum(items_len)[:-1]]).astype(np.int64)
    to_list = np.repeat(np.arange(1, len(lst) + 1), items_len).astype(np.int64)
    return items_len, first, to_list


# ---------------------------------------------------------------------------------------- TriMesh
_IDX_TYPES = {np.dtype(np.int32): 0, np.dtype(np.uint32): 1, np.dtype(np.int64): 2}


def index_upload(arr, index_base, clamp_pad=False, limit=0):
    """Host index array of one of the reference's types (UInt32 / Int64, or Int32; src/rep/mesh.jl:70-98) -> device int32
    0-based of the same (column-major) shape through fx3d_index_upload: the conversion runs on the device.  ``limit`` > 0:
    values outside [0, limit) raise (counted on the device)."""
    a = np.asfortranarray(arr)
    if a.dtype not in _IDX_TYPES:
        a = a.astype(np.int64)
    t = _IDX_TYPES[a.dtype]
    out = DeviceArray.empty(a.shape, np.int32)
    if a.size == 0:
        return out
    n = _lib.query_bytes("fx3d_index_upload_workspace_bytes", t, int(a.size))
    ws = DeviceArray.empty((n,), np.uint8)
    bad = DeviceArray.zeros((1,), np.uint32)
    _lib.call("fx3d_index_upload", a.ctypes.data, t, int(index_base), int(a.size), int(bool(clamp_pad)), int(limit), out.ptr, bad.ptr,
              ws.ptr, ws.nbytes, current_stream().handle)
    nbad = int(bad.to_host()[0])
    if nbad:
        raise ValueError(f"index_upload: {nbad} indices outside [0, {limit}) after subtracting index_base={index_base}")
    return out


class _Deferred:
    """Host cache entry of a table that was built on the device: ``fetch()`` downloads it in the host form."""

    def __init__(self, fetch):
        self.fetch = fetch


class TriMesh:
    """TriMesh(verts_list, faces_list; offset=-1) -- src/rep/mesh.jl:70-187.

    ``verts_list[i]`` is ``(3, V_i)`` float (numpy or DeviceArray), ``faces_list[i]`` is
    ``(3, F_i)`` integer, 1-based mesh-local vertex ids (``index_base=1``) like the reference.
    """

    def __init__(self, verts_list, faces_list, offset=-1, index_base=1, faces_dtype=None):
        if len(verts_list) != len(faces_list):
            raise ValueError(
                f"batch size of verts and faces should match, {len(verts_list)} != {len(faces_list)}")
        self._device = any(is_device(v) for v in verts_list)
        host_verts = [_f32(v.to_host() if is_device(v) else v) for v in verts_list]
        for v in host_verts:
            if v.ndim != 2 or v.shape[0] != 3:
                raise ValueError("each verts array must be (3, V)")
        R = faces_dtype or np.asarray(faces_list[0]).dtype
        if not np.issubdtype(R, np.integer):
            R = np.int64
        self.R = np.dtype(R)
        self.index_base = int(index_base)
        self._faces_list = [np.asfortranarray(np.asarray(f, dtype=self.R)) for f in faces_list]
        self._verts_len = np.array([v.shape[1] for v in host_verts], dtype=np.int64)
        self._faces_len = np.array([f.shape[1] for f in self._faces_list], dtype=np.int64)
        for f, nv in zip(self._faces_list, self._verts_len):
            if f.ndim != 2 or f.shape[0] != 3:
                raise ValueError("each faces array must be (3, F)")
            if f.size and (f.min() < self.index_base or f.max() >= nv + self.index_base):
                raise ValueError("face index outside the mesh's vertex range")
        self.N = len(host_verts)
        self.V = int(self._verts_len.max())
        self.F = int(self._faces_len.max())
        self.equalised = bool(np.all(self._verts_len == self.V) and np.all(self._faces_len == self.F))
        # padded (3,Vmax,B) and packed (3,sumV) vertex arrays are the same bytes (one mesh, or equal vertex counts): no copy between them
        self.verts_aliased = bool(np.all(self._verts_len == self.V))
        self.valid = self._faces_len > 0
        self.offset = int(offset)

        # verts: list is the primary host form (always valid, src/rep/mesh.jl:208-231)
        self._verts_list = host_verts
        self._verts_packed = None
        self._verts_padded = None
        self._verts_packed_valid = False
        self._verts_padded_valid = False
        self._verts_list_valid = True
        # topology caches (never invalidated: faces are immutable, :87-97).  They live in dicts SHARED by every
        # TriMesh derived from this one (gpu/cpu, offset): `offset(m, x)` is deepcopy + offset! upstream
        # (src/transforms/mesh_func.jl:435-438) and must not rebuild edges / Laplacian per optimiser step
        self._topo = {}       # faces_packed, faces_padded, edges_packed, faces_to_edges_packed, laplacian_packed
        self._topo_dev = {}   # int32 0-based device mirrors of the integer data
        # device mirrors of the vertex positions (per mesh)
        self._dev = {}
        if self._device:
            self._dev["verts_packed"] = DeviceArray.from_host(self.get_verts_packed_host())

    @property
    def _faces_list(self):
        """Host face lists; a mesh born on the device (:meth:`_from_device`) builds them on first use."""
        fl = self.__dict__.get("_faces_list_")
        if fl is None:
            fl = self.__dict__["_faces_list_"] = self._faces_builder()
        return fl

    @_faces_list.setter
    def _faces_list(self, value):
        self.__dict__["_faces_list_"] = value

    @classmethod
    def _from_device(cls, verts_packed, verts_len, faces_len, faces_builder, faces_dtype=np.uint32):
        """A device mesh whose vertices were written by a kernel: ``verts_packed`` (3, sum(verts_len)) Float32 device
        array becomes the mesh's packed vertices as it is (no host round trip).  ``faces_builder()`` returns the host face
        lists (1-based, ``faces_dtype``) when they are first needed."""
        m = cls.__new__(cls)
        m._device = True
        m.R = np.dtype(faces_dtype)
        m.index_base = 1
        m._faces_builder = faces_builder
        m._verts_len = np.asarray(verts_len, dtype=np.int64)
        m._faces_len = np.asarray(faces_len, dtype=np.int64)
        m.N = len(m._verts_len)
        m.V = int(m._verts_len.max())
        m.F = int(m._faces_len.max())
        m.equalised = bool(np.all(m._verts_len == m.V) and np.all(m._faces_len == m.F))
        m.verts_aliased = bool(np.all(m._verts_len == m.V))
        m.valid = m._faces_len > 0
        m.offset = -1
        m._verts_list, m._verts_packed, m._verts_padded = None, None, None
        m._verts_packed_valid = m._verts_padded_valid = m._verts_list_valid = False
        m._topo, m._topo_dev = {}, {}
        m._dev = {"verts_packed": verts_packed}
        return m

    def _topo_prop(name):  # noqa: N805  (attribute backed by the shared topology dict)
        def get(self):
            v = self._topo.get(name)
            if isinstance(v, _Deferred):  # built on the device: downloaded when the host first reads it
                v = self._topo[name] = v.fetch()
            return v
        return property(get, lambda self, v: self._topo.__setitem__(name, v))

    _faces_packed = _topo_prop("faces_packed")
    _faces_padded = _topo_prop("faces_padded")
    _edges_packed = _topo_prop("edges_packed")
    _faces_to_edges_packed = _topo_prop("faces_to_edges_packed")
    _laplacian_packed = _topo_prop("laplacian_packed")  # (rowptr, colind, vals) host CSR, 0-based
    del _topo_prop

    # ---- verts -----------------------------------------------------------------------------
    def get_verts_list(self):
        if self._device and not self._verts_list_valid:
            self._verts_list = _packed_to_list(self._dev["verts_packed"].to_host(), self._verts_len)
            self._verts_list_valid = True
        return self._verts_list

    def get_verts_packed_host(self):
        if self._device and "verts_packed" in self._dev and not self._verts_list_valid:
            return self._dev["verts_packed"].to_host()
        if not self._verts_packed_valid:
            self._verts_packed = _list_to_packed(self.get_verts_list())
            self._verts_packed_valid = True
        return self._verts_packed

    def get_verts_padded_host(self):
        if not self._verts_padded_valid or self._device:
            self._verts_padded = _packed_to_padded(self.get_verts_packed_host(), self._verts_len, 0)
            self._verts_padded_valid = True
        return self._verts_padded

    def get_verts_packed(self):
        """get_verts_packed (src/rep/mesh.jl:344-347): (3, sumV), storage type of the mesh."""
        return self._dev["verts_packed"] if self._device else self.get_verts_packed_host()

    def get_verts_padded(self):
        """get_verts_padded (src/rep/mesh.jl:366-369): (3, Vmax, B) zero padded."""
        if not self._device:
            return self.get_verts_padded_host()
        if "verts_padded" not in self._dev:
            if self.verts_aliased:  # one mesh, or equal vertex counts: (3,sumV) and (3,V,B) are the same bytes
                self._dev["verts_padded"] = self._dev["verts_packed"].reshape(3, self.V, self.N)
            else:
                self._dev["verts_padded"] = self._packed_to_padded_dev(self._dev["verts_packed"])
        return self._dev["verts_padded"]

    def _packed_to_padded_dev(self, packed):
        """_packed_to_padded (src/rep/utils.jl:119-139) without leaving the device."""
        out = DeviceArray.empty((3, self.V, self.N), np.float32)
        _lib.call("fx3d_packed_to_padded", packed.ptr, self._verts_len.ctypes.data, self.N, self.V, out.ptr,
                  current_stream().handle)
        return out

    def padded_to_packed_dev(self, padded):
        """_padded_to_packed (src/rep/utils.jl:159-181) on the device: (3,Vmax,B) -> (3,sumV)."""
        if self.verts_aliased:
            return padded.reshape(3, self.V * self.N)
        out = DeviceArray.empty((3, int(self._verts_len.sum())), np.float32)
        _lib.call("fx3d_padded_to_packed", padded.ptr, self._verts_len.ctypes.data, self.N, self.V, out.ptr,
                  current_stream().handle)
        return out

    def with_verts_packed(self, new_packed):
        """A TriMesh with the same topology (shared caches and device mirrors) and new device vertex
        positions -- what `offset(m, x)` (deepcopy + offset!, src/transforms/mesh_func.jl:409-438) needs."""
        m = TriMesh.__new__(TriMesh)
        m.__dict__.update(self.__dict__)
        m._dev = {}  # vertex mirrors are per mesh; _topo / _topo_dev stay shared
        m._device = True
        m._dev["verts_packed"] = new_packed
        m._verts_list_valid = False
        m._verts_packed_valid = False
        m._verts_padded_valid = False
        return m

    def set_verts_packed(self, new):
        """`m._verts_packed = v` (setproperty!, src/rep/mesh.jl:208-231): replaces the vertex
        positions and invalidates the other forms.  Topology caches are kept."""
        if is_device(new):
            assert new.shape == (3, int(self._verts_len.sum())) and new.dtype == np.float32
            self._device = True
            self._dev = {"verts_packed": new}  # every vertex-derived mirror (padded form, sampling CDF) is stale
            self._verts_list_valid = False
            self._verts_packed_valid = False
            self._verts_padded_valid = False
        else:
            new = _f32(new)
            assert new.shape == (3, int(self._verts_len.sum()))
            self._verts_list = _packed_to_list(new, self._verts_len)
            self._verts_list_valid = True
            self._verts_packed, self._verts_packed_valid = new, True
            self._verts_padded_valid = False
            if self._device:
                self._dev = {"verts_packed": DeviceArray.from_host(new)}

    # ---- faces (host, reference numbering) ------------------------------------------------------
    def get_faces_list(self):
        return self._faces_list

    def get_faces_packed(self):
        """get_faces_packed (src/rep/mesh.jl:413-416, _compute_faces_packed :884-896): (3, sumF),
        ids offset by the cumulative vertex count of the preceding meshes."""
        if self._faces_packed is None:
            offs = np.concatenate([[0], np.cumsum(self._verts_len)[:-1]])
            self._faces_packed = np.asfortranarray(np.concatenate(
                [f.astype(np.int64) + o for f, o in zip(self._faces_list, offs)], axis=1).astype(self.R))
        return self._faces_packed

    def get_faces_padded(self):
        """get_faces_padded (src/rep/mesh.jl:435-438): (3, Fmax, B), pad value 0."""
        if self._faces_padded is None:
            self._faces_padded = _list_to_padded(self._faces_list, 0, (3, self.F))
        return self._faces_padded

    # ---- topology (host builders of the C ABI; cached forever like the reference) ---------------
    def _device_born(self):
        """A device mesh without host face lists (:meth:`_from_device`, until something asks for them): its topology is
        built on the device and the host getters download it."""
        return self._device and self.__dict__.get("_faces_list_") is None

    def _index_download(self, arr):
        """Device int32 0-based index array -> the reference's type and numbering (the inverse of :func:`index_upload`)."""
        return np.asfortranarray((arr.to_host().astype(np.int64) + self.index_base).astype(self.R))

    def _build_edges(self):
        if self._device_born():  # (the device build leaves the host entries behind as deferred downloads)
            self.dev("edges"), self.dev("faces_to_edges")
            return
        faces = np.asfortranarray(self.get_faces_packed(), dtype=np.int64)
        F = faces.shape[1]
        V = int(self._verts_len.sum())
        f2e = np.zeros((F, 3), np.int64, order="F")
        E = C.c_int64(0)
        buf = np.zeros(6 * F, np.int64)  # capacity 3F rows; written densely as (E,2) column-major
        _lib.call("fx3d_build_edges_packed", faces.ctypes.data, F, V, self.index_base,
                  buf.ctypes.data, f2e.ctypes.data, C.byref(E))
        E = E.value
        edges = np.asfortranarray(buf[: 2 * E].reshape((E, 2), order="F")).astype(self.R)
        self._edges_packed = edges
        self._faces_to_edges_packed = f2e.astype(self.R)

    def get_edges_packed(self):
        """get_edges_packed (src/rep/mesh.jl:482-485): (E,2) sorted unique, reference numbering."""
        if self._edges_packed is None:
            self._build_edges()
        return self._edges_packed

    def get_faces_to_edges_packed(self):
        if self._faces_to_edges_packed is None:
            self._build_edges()
        return self._faces_to_edges_packed

    def get_edges_to_key(self):
        """get_edges_to_key: Dict edge tuple -> key (src/rep/mesh.jl:939-940), key in reference numbering."""
        e = self.get_edges_packed()
        return {(int(a), int(b)): i + self.index_base for i, (a, b) in enumerate(e)}

    def get_laplacian_packed(self):
        """get_laplacian_packed (src/rep/mesh.jl:559-565) as 0-based CSR (rowptr, colind, vals)."""
        if self._laplacian_packed is None and self._device_born():
            self.dev("lap_rowptr")
        if self._laplacian_packed is None:
            e = np.asfortranarray(self.get_edges_packed(), dtype=np.int64)
            E, V = e.shape[0], int(self._verts_len.sum())
            rowptr = np.zeros(V + 1, np.int32)
            colind = np.zeros(2 * E + V, np.int32)
            vals = np.zeros(2 * E + V, np.float32)
            nnz = C.c_int64(0)
            _lib.call("fx3d_build_laplacian_csr", e.ctypes.data, E, V, self.index_base,
                      rowptr.ctypes.data, colind.ctypes.data, vals.ctypes.data, C.byref(nnz))
            self._laplacian_packed = (rowptr, colind[: nnz.value].copy(), vals[: nnz.value].copy())
        return self._laplacian_packed

    def laplacian_dense(self):
        rowptr, colind, vals = self.get_laplacian_packed()
        V = len(rowptr) - 1
        L = np.zeros((V, V), np.float32)
        for i in range(V):
            L[i, colind[rowptr[i]:rowptr[i + 1]]] = vals[rowptr[i]:rowptr[i + 1]]
        return L

    # ---- device mirrors of the integer data ---------------------------------------------------------
    def dev(self, name):
        """Cached device copies: faces_packed / faces_padded / faces_len / nverts (int32 0-based), edges
        (E,2) int32 0-based, lap_rowptr / lap_colind / lap_vals, the vertex -> (face, corner) tables vf_rowptr / vf_ent
        (padded batch) and vf_packed_rowptr / vf_packed_ent (packed faces), and verts_* float32.

        One rule for edges, faces_to_edges, lap_*, vf_*, vf_packed_* and faces_packed: an item whose host form is already
        cached is uploaded; otherwise a device mesh builds it on the device from its device faces (csrc/topology_dev.hip:
        the same bits as the host builders), and a host mesh builds it on the host and uploads it.  A device build is
        eager -- it reads one count back to size its output -- so, like the host build, it has to run before a graph
        capture begins: touch the mesh's losses (or ``dev(name)``) once outside the capture.  The host form of a table
        built on the device is downloaded when a host getter first reads it."""
        store = self._dev if name.startswith("verts") else self._topo_dev
        if name in store:
            return store[name]
        b = self.index_base
        if name == "verts_packed":
            arr = DeviceArray.from_host(self.get_verts_packed_host())
        elif name == "verts_padded":
            arr = DeviceArray.from_host(self.get_verts_padded_host())
        elif name == "faces_packed" and self._faces_packed is None and self._device_born() and "faces_padded" in store:
            arr = self._pack_faces_dev()
        elif name == "faces_packed":   # the reference's own arrays (UInt32 / Int64, 1-based) cross the ABI untouched: the
            arr = index_upload(self.get_faces_packed(), b, limit=int(np.sum(self._verts_len)))   # library converts on the device
        elif name == "faces_padded":    # (pad entries -- value 0 in the reference -- become 0: never dereferenced)
            arr = index_upload(self.get_faces_padded(), b, clamp_pad=True, limit=int(self.V))
        elif name == "faces_len":
            arr = DeviceArray.from_host(self._faces_len.astype(np.int32))
        elif name == "nverts":  # per-mesh vertex counts (B) int32 (not "verts_len": names starting with "verts" are vertex mirrors)
            arr = DeviceArray.from_host(self._verts_len.astype(np.int32))
        elif name in ("edges", "faces_to_edges") and self._device and self._topo.get(name + "_packed") is None:
            self._build_edges_dev(name)
            return store[name]
        elif name == "edges":
            arr = index_upload(self.get_edges_packed(), b, limit=int(np.sum(self._verts_len)))
        elif name == "faces_to_edges":
            arr = index_upload(self.get_faces_to_edges_packed(), b)
        elif name in ("vf_rowptr", "vf_ent", "vf_packed_rowptr", "vf_packed_ent") and self._device:
            self._build_vertex_faces_dev(packed="packed" in name)
            return store[name]
        elif name in ("vf_rowptr", "vf_ent"):  # vertex -> (face, corner) table of the ordered sampling adjoint (padded batch)
            fp = np.asfortranarray(self.get_faces_padded().astype(np.int64) - b).astype(np.int32)
            fp[fp < 0] = 0  # (padding faces: never read, faces_len bounds the walk)
            fp = np.asfortranarray(fp)
            fl = np.ascontiguousarray(self._faces_len, dtype=np.int32)
            rowptr = np.zeros((self.V + 1, self.N), np.int32, order="F")
            ent = np.zeros((3 * self.F, self.N), np.int32, order="F")
            _lib.call("fx3d_build_vertex_faces", fp.ctypes.data, fl.ctypes.data, int(self.V), int(self.F), int(self.N),
                      rowptr.ctypes.data, ent.ctypes.data)
            store["vf_rowptr"] = DeviceArray.from_host(rowptr)
            store["vf_ent"] = DeviceArray.from_host(ent)
            return store[name]
        elif name in ("vf_packed_rowptr", "vf_packed_ent"):  # the same table over the PACKED faces, for the normals
            fp = np.asfortranarray(self.get_faces_packed().astype(np.int64) - b).astype(np.int32)  # one mesh, sum V / sum F
            V, F = int(np.sum(self._verts_len)), fp.shape[1]
            rowptr = np.zeros(V + 1, np.int32)
            ent = np.zeros(3 * F, np.int32)
            fl = np.array([F], np.int32)
            _lib.call("fx3d_build_vertex_faces", fp.ctypes.data, fl.ctypes.data, V, F, 1, rowptr.ctypes.data, ent.ctypes.data)
            store["vf_packed_rowptr"] = DeviceArray.from_host(rowptr)
            store["vf_packed_ent"] = DeviceArray.from_host(ent)
            return store[name]
        elif name in ("lap_rowptr", "lap_colind", "lap_vals") and self._device and self._laplacian_packed is None:
            self._build_laplacian_dev()
            return store[name]
        elif name in ("lap_rowptr", "lap_colind", "lap_vals"):
            rowptr, colind, vals = self.get_laplacian_packed()
            store["lap_rowptr"] = DeviceArray.from_host(rowptr)
            store["lap_colind"] = DeviceArray.from_host(colind)
            store["lap_vals"] = DeviceArray.from_host(vals)
            return store[name]
        else:
            raise KeyError(name)
        if name.startswith("verts") and not self._device:
            return arr  # host mesh: do not cache vertex uploads (verts may change)
        store[name] = arr
        return arr

    # ---- topology built on the device (csrc/topology_dev.hip); each leaves its tables in the shared _topo_dev ----------
    @staticmethod
    def _check_ids(what, bad):
        nbad = int(bad.to_host()[0])
        if nbad:
            raise ValueError(f"{what}: {nbad} vertex ids outside the mesh's vertex range")

    def _pack_faces_dev(self):
        fp = self.dev("faces_padded")
        out = DeviceArray.empty((3, int(self._faces_len.sum())), np.int32)
        ws = DeviceArray.empty((_lib.query_bytes("fx3d_faces_padded_to_packed_dev_workspace_bytes", self.N),), np.uint8)
        _lib.call("fx3d_faces_padded_to_packed_dev", fp.ptr, self.dev("faces_len").ptr, self.dev("nverts").ptr, int(self.F),
                  int(self.N), out.shape[1], out.ptr, ws.ptr, ws.nbytes, current_stream().handle)
        return out

    def _build_edges_dev(self, name):
        faces, store, s = self.dev("faces_packed"), self._topo_dev, current_stream().handle
        F, V = int(faces.shape[1]), int(np.sum(self._verts_len))
        ws = DeviceArray.empty((_lib.query_bytes("fx3d_edges_dev_workspace_bytes", F, V),), np.uint8)
        count, bad = DeviceArray.empty((1,), np.int64), DeviceArray.empty((1,), np.uint32)
        _lib.call("fx3d_edges_dev_count", faces.ptr, F, V, count.ptr, bad.ptr, ws.ptr, ws.nbytes, s)
        E = int(count.to_host()[0])  # the one synchronisation of the build: E sizes the edge list
        self._check_ids("edges", bad)
        edges = DeviceArray.empty((E, 2), np.int32)
        f2e = DeviceArray.empty((F, 3), np.int32) if name == "faces_to_edges" else None  # no kernel reads it: on request only
        _lib.call("fx3d_edges_dev_emit", faces.ptr, F, V, E, edges.ptr, f2e.ptr if f2e is not None else None, ws.ptr, ws.nbytes, s)
        edges = store.setdefault("edges", edges)
        self._topo.setdefault("edges_packed", _Deferred(lambda: self._index_download(edges)))
        if f2e is not None:
            store["faces_to_edges"] = f2e
            self._topo["faces_to_edges_packed"] = _Deferred(lambda: self._index_download(f2e))

    def _build_laplacian_dev(self):
        edges, store = self.dev("edges"), self._topo_dev
        E, V = int(edges.shape[0]), int(np.sum(self._verts_len))
        ws = DeviceArray.empty((_lib.query_bytes("fx3d_laplacian_dev_workspace_bytes", E, V),), np.uint8)
        rowptr, colind, vals = (DeviceArray.empty((n,), t) for n, t in ((V + 1, np.int32), (2 * E + V, np.int32), (2 * E + V, np.float32)))
        count, bad = DeviceArray.empty((1,), np.int64), DeviceArray.empty((1,), np.uint32)
        _lib.call("fx3d_laplacian_dev_csr", edges.ptr, E, V, rowptr.ptr, colind.ptr, vals.ptr, count.ptr, bad.ptr, ws.ptr, ws.nbytes,
                  current_stream().handle)
        nnz = int(count.to_host()[0])  # 2E + V less two per self-edge: the arrays are handed out at that length
        self._check_ids("laplacian", bad)
        store["lap_rowptr"] = rowptr
        store["lap_colind"] = DeviceArray(colind.ptr, (nnz,), np.int32, keep=colind)
        store["lap_vals"] = DeviceArray(vals.ptr, (nnz,), np.float32, keep=vals)
        self._topo["laplacian_packed"] = _Deferred(lambda: tuple(store[n].to_host() for n in ("lap_rowptr", "lap_colind", "lap_vals")))

    def _build_vertex_faces_dev(self, packed):
        """The padded batch's tables, or (``packed``) the B = 1 table over the packed faces."""
        store = self._topo_dev
        if packed:
            faces = self.dev("faces_packed")
            V, F, B, pre = int(np.sum(self._verts_len)), int(faces.shape[1]), 1, "vf_packed_"
            flen = None  # (every face is live)
            shapes = ((V + 1,), (3 * F,))
        else:
            faces, flen = self.dev("faces_padded"), self.dev("faces_len")
            V, F, B, pre = int(self.V), int(self.F), int(self.N), "vf_"
            shapes = ((V + 1, B), (3 * F, B))
        ws = DeviceArray.empty((_lib.query_bytes("fx3d_vertex_faces_dev_workspace_bytes", V, F, B),), np.uint8)
        rowptr, ent = DeviceArray.empty(shapes[0], np.int32), DeviceArray.empty(shapes[1], np.int32)
        bad = DeviceArray.empty((1,), np.uint32)
        _lib.call("fx3d_vertex_faces_dev", faces.ptr, flen.ptr if flen is not None else None, V, F, B, rowptr.ptr, ent.ptr, bad.ptr, ws.ptr, ws.nbytes,
                  current_stream().handle)
        self._check_ids("vertex tables", bad)
        store[pre + "rowptr"], store[pre + "ent"] = rowptr, ent

    # ---- gpu / cpu (functor(::TriMesh) moves only the verts, src/rep/mesh.jl:189-190) ---------------
    @property
    def on_device(self):
        return self._device

    def _to_device(self):
        if self._device:
            return self
        m = TriMesh(self.get_verts_list(), self._faces_list, offset=self.offset,
                    index_base=self.index_base, faces_dtype=self.R)
        m._share_topology(self)
        m._device = True
        m._dev["verts_packed"] = DeviceArray.from_host(m.get_verts_packed_host())
        return m

    def _to_host(self):
        if not self._device:
            return self
        m = TriMesh(self.get_verts_list(), self._faces_list, offset=self.offset,
                    index_base=self.index_base, faces_dtype=self.R)
        m._share_topology(self)
        return m

    def _share_topology(self, other):
        self._topo, self._topo_dev = other._topo, other._topo_dev

    def __getitem__(self, i):
        return self.get_verts_list()[i], self._faces_list[i]

    def __repr__(self):
        return (f"TriMesh{{Float32, {self.R}, {'DeviceArray' if self._device else 'Array'}}} Structure:\n"
                f"    Batch size: {self.N}\n    Max verts: {self.V}\n    Max faces: {self.F}\n"
                f"    offset: {self.offset}\n    Storage type: {'DeviceArray' if self._device else 'Array'}")


# accessor functions with the reference's names
def get_verts_packed(m): return m.get_verts_packed()
def get_verts_padded(m): return m.get_verts_padded()
def get_verts_list(m): return m.get_verts_list()
def get_faces_packed(m): return m.get_faces_packed()
def get_faces_padded(m): return m.get_faces_padded()
def get_faces_list(m): return m.get_faces_list()
def get_edges_packed(m): return m.get_edges_packed()
def get_faces_to_edges_packed(m): return m.get_faces_to_edges_packed()
def get_edges_to_key(m): return m.get_edges_to_key()
def get_laplacian_packed(m): return m.get_laplacian_packed()


def load_obj(path):
    """Minimal Wavefront OBJ reader (``v`` and triangular ``f`` records, ``a/b/c`` index forms).
    Stands in for MeshIO behind load_trimesh (src/rep/mesh.jl:244-262) for the test assets."""
    verts, faces = [], []
    with open(path) as fh:
        for line in fh:
            if line.startswith("v "):
                verts.append([float(t) for t in line.split()[1:4]])
            elif line.startswith("f "):
                ids = [int(t.split("/")[0]) for t in line.split()[1:]]
                for k in range(1, len(ids) - 1):  # fan-triangulate polygons
                    faces.append([ids[0], ids[k], ids[k + 1]])
    v = np.asfortranarray(np.array(verts, dtype=np.float32).T)
    f = np.asfortranarray(np.array(faces, dtype=np.uint32).T)
    return v, f


def load_off(path):
    """Minimal OFF reader (the ModelNet on-disk format read by load_trimesh at
    src/datasets/modelnet/base.jl:100-101): header ``OFF`` (ModelNet also ships files with the counts glued
    to it, ``OFF490 518 0``), ``nv nf ne``, nv vertex lines, nf face lines ``k i0 .. ik-1`` (0-based;
    polygons are fan-triangulated).  Returns the same (verts (3,V) Float32, faces (3,F) UInt32 1-based)."""
    with open(path) as fh:
        toks = fh.read().split()
    if not toks or not toks[0].upper().startswith("OFF"):
        raise ValueError(f"{path}: not an OFF file")
    head = toks[0][3:]
    toks = ([head] if head else []) + toks[1:]
    nv, nf = int(toks[0]), int(toks[1])
    pos = 3
    v = np.array(toks[pos:pos + 3 * nv], dtype=np.float32).reshape(nv, 3)
    pos += 3 * nv
    faces = []
    for _ in range(nf):
        k = int(toks[pos])
        ids = [int(t) + 1 for t in toks[pos + 1:pos + 1 + k]]
        pos += 1 + k
        for j in range(1, k - 1):
            faces.append([ids[0], ids[j], ids[j + 1]])
    return (np.asfortranarray(v.T), np.asfortranarray(np.array(faces, dtype=np.uint32).reshape(-1, 3).T))


def load_trimesh(*paths):
    """load_trimesh(fn...) (src/rep/mesh.jl:244-262) for .obj / .off files: one batched TriMesh."""
    flat = []
    for p in paths:
        flat.extend(p if isinstance(p, (list, tuple)) else [p])
    vs, fs = zip(*[(load_off(p) if str(p).lower().endswith(".off") else load_obj(p)) for p in flat])
    return TriMesh(list(vs), list(fs))
