"""Vertex and face normals of a TriMesh on the device, and their adjoints (src/rep/mesh.jl:569-746).

The vertex normals are what the reference computes on the CPU, not what its docstring says: per corner row, the cross
product of the LAST face that has the vertex in that row (include/flux3d_hip.h states the definition).  Every result is the
same bits on every run: no float atomics."""
import numpy as np

from . import _lib
from .device import DeviceArray, current_stream, workspace, is_device
from .rep import TriMesh


def _check_mesh(m, fn):
    if not isinstance(m, TriMesh):
        raise TypeError(f"{fn}: expected a TriMesh, got {type(m).__name__}")


def _sizes(m):
    return int(np.sum(m._verts_len)), int(np.sum(m._faces_len))


def _verts_normals(m, mask=None):
    verts, faces = m.dev("verts_packed"), m.dev("faces_packed")
    V, F = _sizes(m)
    out = DeviceArray.empty((3, V), np.float32)
    _lib.call("fx3d_verts_normals_packed", verts.ptr, V, faces.ptr, F, m.dev("vf_packed_rowptr").ptr,
              m.dev("vf_packed_ent").ptr, out.ptr, mask.ptr if mask is not None else None, current_stream().handle)
    return out


def _winner_mask(m):
    """(3, sum F) uint8: "(f, r) is the winner of vertex faces[r, f]" -- topology only, so built once and kept with the topology."""
    mask = m._topo_dev.get("vn_winner_mask")
    if mask is None:
        mask = DeviceArray.empty((3, _sizes(m)[1]), np.uint8)
        _verts_normals(m, mask)
        m._topo_dev["vn_winner_mask"] = mask
    return mask


def compute_verts_normals_packed(m):
    """compute_verts_normals_packed (src/rep/mesh.jl:589-621): device (3, sumV) Float32."""
    _check_mesh(m, "compute_verts_normals_packed")
    return _verts_normals(m)


def compute_faces_normals_packed(m):
    """compute_faces_normals_packed (src/rep/mesh.jl:689-699): device (3, sumF) Float32."""
    _check_mesh(m, "compute_faces_normals_packed")
    verts, faces = m.dev("verts_packed"), m.dev("faces_packed")
    V, F = _sizes(m)
    out = DeviceArray.empty((3, F), np.float32)
    _lib.call("fx3d_faces_normals_packed", verts.ptr, V, faces.ptr, F, out.ptr, current_stream().handle)
    return out


def _to_padded(m, packed, lens, width):
    out = DeviceArray.empty((3, width, m.N), np.float32)
    lens = np.ascontiguousarray(lens, dtype=np.int64)
    _lib.call("fx3d_packed_to_padded", packed.ptr, lens.ctypes.data, m.N, width, out.ptr, current_stream().handle)
    return out


def _to_list(packed, lens):
    a = packed.to_host()
    out, cur = [], 0
    for n in lens:
        out.append(np.asfortranarray(a[:, cur:cur + int(n)]))
        cur += int(n)
    return out


def compute_verts_normals_padded(m):
    """compute_verts_normals_padded (src/rep/mesh.jl:640-644): device (3, Vmax, B), zero padded."""
    _check_mesh(m, "compute_verts_normals_padded")
    return _to_padded(m, _verts_normals(m), m._verts_len, m.V)


def compute_verts_normals_list(m):
    """compute_verts_normals_list (src/rep/mesh.jl:666-670): list of host (3, V_i) arrays."""
    _check_mesh(m, "compute_verts_normals_list")
    return _to_list(_verts_normals(m), m._verts_len)


def compute_faces_normals_padded(m):
    """compute_faces_normals_padded (src/rep/mesh.jl:719-723): device (3, Fmax, B), zero padded."""
    return _to_padded(m, compute_faces_normals_packed(m), m._faces_len, m.F)


def compute_faces_normals_list(m):
    """compute_faces_normals_list (src/rep/mesh.jl:742-746): list of host (3, F_i) arrays."""
    return _to_list(compute_faces_normals_packed(m), m._faces_len)


def _grad_args(m, gout, out, accumulate, per_face, fn):
    """Checks everything before any device work; returns (gout, g) as device arrays."""
    _check_mesh(m, fn)
    V, F = _sizes(m)
    n_out = F if per_face else V
    if is_device(gout):
        if gout.dtype != np.float32:
            raise TypeError(f"{fn}: gout must be Float32, got {gout.dtype}")
    else:
        gout = np.asarray(gout)
        if gout.dtype != np.float32:
            raise TypeError(f"{fn}: gout must be Float32, got {gout.dtype}")
    if tuple(gout.shape) != (3, n_out):
        raise ValueError(f"{fn}: gout must be (3, {n_out}), got {tuple(gout.shape)}")
    if out is not None:
        if not is_device(out) or out.dtype != np.float32 or tuple(out.shape) != (3, V):
            raise ValueError(f"{fn}: out must be a (3, {V}) Float32 device array")
    elif accumulate:
        raise ValueError(f"{fn}: accumulate needs `out`")
    if not is_device(gout):
        gout = DeviceArray.from_host(np.asfortranarray(gout))
    return gout, (out if out is not None else DeviceArray.empty((3, V), np.float32))


def compute_verts_normals_grad(m, gout, out=None, accumulate=False):
    """Adjoint of compute_verts_normals_packed w.r.t. the packed vertices: device (3, sumV).  ``gout`` (3, sumV) Float32.
    ``out``: write into this (3, sumV) device array; with ``accumulate`` add to what it holds."""
    gout, g = _grad_args(m, gout, out, accumulate, False, "compute_verts_normals_grad")
    verts, faces = m.dev("verts_packed"), m.dev("faces_packed")
    V, F = _sizes(m)
    mask = _winner_mask(m)
    nb = _lib.query_bytes("fx3d_normals_workspace_bytes", V, F)
    ws = workspace(nb, tag="normals")
    _lib.call("fx3d_verts_normals_bwd", verts.ptr, V, faces.ptr, F, m.dev("vf_packed_rowptr").ptr, m.dev("vf_packed_ent").ptr,
              mask.ptr, gout.ptr, g.ptr, int(bool(accumulate)), ws.ptr, ws.nbytes, current_stream().handle)
    return g


def compute_faces_normals_grad(m, gout, out=None, accumulate=False):
    """Adjoint of compute_faces_normals_packed w.r.t. the packed vertices: device (3, sumV).  ``gout`` (3, sumF) Float32.
    ``out`` / ``accumulate`` as compute_verts_normals_grad."""
    gout, g = _grad_args(m, gout, out, accumulate, True, "compute_faces_normals_grad")
    verts, faces = m.dev("verts_packed"), m.dev("faces_packed")
    V, F = _sizes(m)
    nb = _lib.query_bytes("fx3d_normals_workspace_bytes", V, F)
    ws = workspace(nb, tag="normals")
    _lib.call("fx3d_faces_normals_bwd", verts.ptr, V, faces.ptr, F, m.dev("vf_packed_rowptr").ptr, m.dev("vf_packed_ent").ptr,
              gout.ptr, g.ptr, int(bool(accumulate)), ws.ptr, ws.nbytes, current_stream().handle)
    return g
