"""Mesh and point-cloud transforms: lincomb / offset (src/transforms/mesh_func.jl:435-438) and normalize / scale / rotate /
realign / translate (src/transforms/pcloud_func.jl, src/transforms/mesh_func.jl:99-399).  Sampling and face areas live in
:mod:`.sampling`; their names are re-exported here, where they used to be defined."""
import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, current_stream, is_device, workspace
from .sampling import (EPS, _face_cdf, _verts_padded_dev, compute_faces_areas_list, compute_faces_areas_packed,  # noqa: F401
                       compute_faces_areas_padded, sample_points, sample_points_grad, sample_points_pair)


def lincomb(a, x, b, y, c=0.0, z=None, out=None):
    """out = a*x + b*y (+ c*z): Float32 device arrays of equal size (fx3d_lincomb)."""
    out = out if out is not None else DeviceArray.empty(x.shape, np.float32)
    _lib.call("fx3d_lincomb", x.size, float(a), x.ptr, float(b), y.ptr, float(c), z.ptr if z is not None else None,
              out.ptr, current_stream().handle)
    return out


def offset(m, offset_verts_packed):
    """offset(m::TriMesh, offset_verts_packed) (src/transforms/mesh_func.jl:435-438): a new mesh whose
    packed vertices are `verts + offset`; stays on the device, topology caches are shared."""
    verts = m.dev("verts_packed")
    off = offset_verts_packed if isinstance(offset_verts_packed, DeviceArray) else \
        DeviceArray.from_host(np.asarray(offset_verts_packed, np.float32))
    if off.shape != verts.shape:
        raise ValueError("mesh and offset_verts size mismatch")
    return m.with_verts_packed(lincomb(1.0, verts, 1.0, off))


# ---- normalize / scale / rotate / realign / translate (src/transforms/pcloud_func.jl, src/transforms/mesh_func.jl:99-399) ----
# Every argument check runs here, on the host, before any launch (the reference's errors: ValueError for `error(...)`, TypeError
# where Julia raises one).  The transforms move the points / vertices only: normals are left as they are.  In-place forms
# (trailing underscore) mutate and return the same object; the others leave their input unchanged.  A host object is uploaded,
# transformed on the device and returned in host storage.

def _transform_ws(D, n_max, B):
    nb = _lib.query_bytes("fx3d_transform_workspace_bytes", int(D), int(n_max), int(B))
    return workspace(nb, tag="transforms") if nb else None


def transform_plan(D, n_max, B):
    """fx3d_transform_plan_describe: the launch plan of normalize / segment_minmax for B segments of at most n_max
    columns of D rows, as text ("plan=fused ..." or "plan=two_launch ...").  A function of the shape alone."""
    buf = C.create_string_buffer(256)
    _lib.call("fx3d_transform_plan_describe", int(D), int(n_max), int(B), buf, 256)
    return buf.value.decode()


def _rep():
    from .rep import PointCloud, TriMesh
    return PointCloud, TriMesh


class _Seg:
    """The device (D, ncols) stream of a PointCloud (dense (D, N, B)) or a TriMesh (packed (3, sum V)) and its segments."""

    def __init__(self, obj):
        PointCloud, TriMesh = _rep()
        self.obj = obj
        if isinstance(obj, PointCloud):
            pts = obj.points
            self.host = not is_device(pts)
            self.x = DeviceArray.from_host(pts) if self.host else pts
            self.D, self.n_max, self.B = self.x.shape
            self.ncols, self.seg_off, self.mesh = self.n_max * self.B, None, False
        elif isinstance(obj, TriMesh):
            self.host = not obj.on_device
            self.x = obj.dev("verts_packed")
            self.D, self.n_max, self.B = 3, int(obj.V), int(obj.N)
            self.ncols, self.mesh = int(np.sum(obj._verts_len)), True
            self.seg_off = obj._topo_dev.get("seg_off")
            if self.seg_off is None:  # the vertex-count prefix sums: topology, uploaded once
                off = np.concatenate([[0], np.cumsum(obj._verts_len)]).astype(np.int64)
                self.seg_off = obj._topo_dev["seg_off"] = DeviceArray.from_host(off)
        else:
            raise TypeError(f"expected a PointCloud or a TriMesh, got {type(obj).__name__}")

    @property
    def off_ptr(self):
        return self.seg_off.ptr if self.seg_off is not None else None

    def empty_like(self):
        return DeviceArray.empty(self.x.shape, np.float32)

    def finish(self, y, inplace):
        """Put y (device, the input's shape) back: in place, or as a new object (the input unchanged)."""
        PointCloud, _ = _rep()
        obj = self.obj
        if not self.mesh:
            pts = y.to_host() if self.host else y
            if inplace:
                obj.points = pts
                return obj
            return PointCloud(pts, obj.normals)
        if inplace:
            obj.set_verts_packed(y.to_host() if self.host else y)
            return obj
        m = obj.with_verts_packed(y)
        return m._to_host() if self.host else m


def _f32_scalar(v, what):
    try:
        return np.float32(v)
    except (TypeError, ValueError):
        raise TypeError(f"{what} must be a number or an array of numbers") from None


def _check_factor(factor):
    f = _f32_scalar(factor, "factor")
    if not f > 0.0:  # `(factor > 0.0) || error(...)`: NaN fails too
        raise ValueError("factor must be greater than 0.0")
    return f


def _scale_translate(sg, mode, vec, inplace):
    y = sg.empty_like()
    v = np.ascontiguousarray(np.resize(np.asarray(vec, np.float32), 3))
    _lib.call("fx3d_scale_translate", sg.x.ptr, sg.x.size, int(mode), v.ctypes.data, y.ptr, current_stream().handle)
    return sg.finish(y, inplace)


def _scale(obj, factor, inplace):
    _, TriMesh = _rep()
    if isinstance(obj, TriMesh) and np.ndim(factor) > 0:
        f = np.asarray(factor)
        if f.shape != (3,):
            raise ValueError(f"factor must be (3, ), but instead got {f.shape} array")
        # `(factor .> 0.0) || error(...)` with a BitVector in `||` (src/transforms/mesh_func.jl:162-169): always a TypeError
        raise TypeError("non-boolean (BitVector) used in boolean context: scale!(m::TriMesh, factor::AbstractArray) always "
                        "throws in the reference (src/transforms/mesh_func.jl:165)")
    f = _check_factor(factor)
    sg = _Seg(obj)
    return _scale_translate(sg, 0, [f, 0.0, 0.0], inplace)


def scale(obj, factor):
    """scale(p::PointCloud, factor) / scale(m::TriMesh, factor) (pcloud_func.jl:84-91, mesh_func.jl:194-200):
    factor * x.  factor must be > 0 (NaN is rejected).  A (3,) factor on a TriMesh raises TypeError, as the reference does."""
    return _scale(obj, factor, False)


def scale_(obj, factor):
    """scale!(p, factor) / scale!(m, factor) (pcloud_func.jl:62-68, mesh_func.jl:154-170), in place."""
    return _scale(obj, factor, True)


def _translate(m, vector, inplace):
    _, TriMesh = _rep()
    if not isinstance(m, TriMesh):
        raise TypeError(f"translate needs a TriMesh, got {type(m).__name__}")
    if np.ndim(vector) == 0:
        vec = np.full(3, _f32_scalar(vector, "vector"), np.float32)  # translate!(m, ::Float32) = fill(vector, (3,))
    else:
        vec = np.asarray(vector)
        if vec.shape != (3,):
            raise ValueError(f"vector must be (3, ), but instead got {vec.shape} array")
        vec = vec.astype(np.float32)
    return _scale_translate(_Seg(m), 1, vec, inplace)


def translate(m, vector):
    """translate(m::TriMesh, vector) (src/transforms/mesh_func.jl:368-371): x + t[d]; a scalar t is fill(t, 3)."""
    return _translate(m, vector, False)


def translate_(m, vector):
    """translate!(m::TriMesh, vector) (src/transforms/mesh_func.jl:331-341), in place."""
    return _translate(m, vector, True)


def _rotate(obj, rotmat, inplace):
    PointCloud, TriMesh = _rep()
    if not isinstance(obj, (PointCloud, TriMesh)):
        raise TypeError(f"expected a PointCloud or a TriMesh, got {type(obj).__name__}")
    R = rotmat.to_host() if is_device(rotmat) else np.asarray(rotmat)
    if R.ndim not in (2, 3):
        raise TypeError(f"no method matching rotate!(::{type(obj).__name__}, ::Array{{Float32,{R.ndim}}})")
    B = obj.N if isinstance(obj, TriMesh) else obj.points.shape[2]
    if R.ndim == 2 and R.shape != (3, 3):
        raise ValueError(f"rotmat must be (3, 3) array, but instead got {R.shape} array")
    if R.ndim == 3 and R.shape != (3, 3, B):
        raise ValueError(f"rotmat must be (3, 3, {B}) array, but instead got {R.shape} array")
    if isinstance(obj, PointCloud) and obj.points.shape[0] != 3:
        raise ValueError("dimension of points in PointCloud must be 3")
    sg = _Seg(obj)
    y = sg.empty_like()
    st = current_stream().handle
    if R.ndim == 2:
        host = np.asfortranarray(R, dtype=np.float32).reshape(-1, order="F").copy()
        _lib.call("fx3d_rotate", sg.x.ptr, sg.ncols, sg.n_max, sg.B, sg.off_ptr, host.ctypes.data, None, y.ptr, st)
    else:
        rd = rotmat if (is_device(rotmat) and rotmat.dtype == np.float32) else DeviceArray.from_host(np.asfortranarray(R, np.float32))
        _lib.call("fx3d_rotate", sg.x.ptr, sg.ncols, sg.n_max, sg.B, sg.off_ptr, None, rd.ptr, y.ptr, st)
    return sg.finish(y, inplace)


def rotate(obj, rotmat):
    """rotate(p, rotmat) / rotate(m, rotmat) (pcloud_func.jl:155-159, mesh_func.jl:252-256): transpose(R) * X, one (3,3)
    matrix for the batch or a (3,3,B) one per cloud / mesh.  Definition and order: fx3d_rotate (include/flux3d_hip.h)."""
    return _rotate(obj, rotmat, False)


def rotate_(obj, rotmat):
    """rotate!(p, rotmat) / rotate!(m, rotmat) (pcloud_func.jl:120-139, mesh_func.jl:221-237), in place."""
    return _rotate(obj, rotmat, True)


def _normalize(obj, inplace, stats=False):
    sg = _Seg(obj)
    y = sg.empty_like()
    c = DeviceArray.empty((sg.D, sg.B), np.float32) if stats else None
    s = DeviceArray.empty((sg.D, sg.B), np.float32) if stats else None
    ws = _transform_ws(sg.D, sg.n_max, sg.B)
    _lib.call("fx3d_normalize", sg.x.ptr, sg.D, sg.n_max, sg.B, sg.off_ptr, 1 if sg.mesh else 0, y.ptr,
              c.ptr if stats else None, s.ptr if stats else None, ws.ptr if ws else None, ws.nbytes if ws else 0,
              current_stream().handle)
    out = sg.finish(y, inplace)
    return (out, c, s) if stats else out


def normalize(obj, return_stats=False):
    """normalize(p::PointCloud) / normalize(m::TriMesh) (pcloud_func.jl:25-43, mesh_func.jl:115-133): (x - c) / (s + EPS)
    for a cloud, (x - c) / max(s, EPS) for a mesh, c and s per cloud / mesh and row (statistics contract:
    include/flux3d_hip.h).  ``return_stats``: also the (D, B) device centroid and scale."""
    return _normalize(obj, False, return_stats)


def normalize_(obj, return_stats=False):
    """normalize!(p) / normalize!(m) (pcloud_func.jl:16-22, mesh_func.jl:99-113), in place."""
    return _normalize(obj, True, return_stats)


def segment_minmax(sg_or_obj, pad_zero=False):
    """(min, max) per row and cloud / mesh with Julia's min / max: (D, B) device arrays (fx3d_segment_minmax)."""
    sg = sg_or_obj if isinstance(sg_or_obj, _Seg) else _Seg(sg_or_obj)
    if sg.n_max == 0:
        raise ValueError("reducing over an empty collection is not allowed")
    mn = DeviceArray.empty((sg.D, sg.B), np.float32)
    mx = DeviceArray.empty((sg.D, sg.B), np.float32)
    ws = _transform_ws(sg.D, sg.n_max, sg.B)
    _lib.call("fx3d_segment_minmax", sg.x.ptr, sg.D, sg.n_max, sg.B, sg.off_ptr, int(bool(pad_zero)), mn.ptr, mx.ptr,
              ws.ptr if ws else None, ws.nbytes if ws else 0, current_stream().handle)
    return mn, mx


def _bounds_of_columns(x, D, n):
    """minimum / maximum(points, dims = 2) of one (D, n) device column block: (D, 1) device arrays."""
    if n == 0:
        raise ValueError("reducing over an empty collection is not allowed")
    mn = DeviceArray.empty((D, 1), np.float32)
    mx = DeviceArray.empty((D, 1), np.float32)
    ws = _transform_ws(D, n, 1)
    _lib.call("fx3d_segment_minmax", x.ptr, D, n, 1, None, 0, mn.ptr, mx.ptr, ws.ptr if ws else None,
              ws.nbytes if ws else 0, current_stream().handle)
    return mn, mx


def target_bounds(tgt, index=0):
    """(tgt_min, tgt_max) (D, 1) device of tgt[index] (PointCloud, pcloud_func.jl:221-227) or get_verts_list(tgt)[index]
    (TriMesh, mesh_func.jl:297-298), or of a (D, V) array (mesh_func.jl:291-296).  0-based index."""
    PointCloud, TriMesh = _rep()
    D, n = _target_rows(tgt, index)
    if n == 0:
        raise ValueError("reducing over an empty collection is not allowed")
    if isinstance(tgt, PointCloud):
        pts = tgt.points if is_device(tgt.points) else DeviceArray.from_host(tgt.points)
        D, N, B = pts.shape
        i = int(index)
        if not -B <= i < B:
            raise IndexError(f"index {index} out of range for a batch of {B}")
        return _bounds_of_columns(pts.slab(i % B, 1), D, N)
    if isinstance(tgt, TriMesh):
        i = int(index)
        if not -tgt.N <= i < tgt.N:
            raise IndexError(f"index {index} out of range for a batch of {tgt.N}")
        i %= tgt.N
        n = int(tgt._verts_len[i])
        off = int(np.sum(tgt._verts_len[:i]))
        v = tgt.dev("verts_packed")
        blk = DeviceArray(v.ptr + 12 * off, (3, n), np.float32, keep=v)
        return _bounds_of_columns(blk, 3, n)
    a = tgt if is_device(tgt) else DeviceArray.from_host(np.asfortranarray(np.asarray(tgt, np.float32)))
    if a.ndim != 2:
        raise TypeError("a target array must be 2-D (D, V)")
    return _bounds_of_columns(a, a.shape[0], a.shape[1])


def _as_bound(b):
    if is_device(b):
        return b
    return DeviceArray.from_host(np.asfortranarray(np.asarray(b, np.float32)))


def _target_rows(tgt, index):
    """(D, n) of the target block realign! reduces over, from host metadata only (no device work)."""
    PointCloud, TriMesh = _rep()
    if isinstance(tgt, PointCloud):
        D, N, B = tgt.points.shape
        if not -B <= int(index) < B:
            raise IndexError(f"index {index} out of range for a batch of {B}")
        return D, N
    if isinstance(tgt, TriMesh):
        if not -tgt.N <= int(index) < tgt.N:
            raise IndexError(f"index {index} out of range for a batch of {tgt.N}")
        return 3, int(tgt._verts_len[int(index) % tgt.N])
    shape = tgt.shape if is_device(tgt) else np.shape(tgt)
    if len(shape) != 2:
        raise TypeError("a target array must be 2-D (D, V)")
    return shape


def _realign(src, a, b, index, inplace):
    PointCloud, TriMesh = _rep()
    if not isinstance(src, (PointCloud, TriMesh)):
        raise TypeError(f"expected a PointCloud or a TriMesh, got {type(src).__name__}")
    D = src.points.shape[0] if isinstance(src, PointCloud) else 3
    # every check first, on host metadata; the reference's order: target bounds, then D, then the source's own bounds
    if b is None:  # realign!(src, tgt[, index])
        if isinstance(src, PointCloud) and not isinstance(a, PointCloud):
            raise TypeError("realign!(::PointCloud, tgt) needs a PointCloud target, or tgt_min and tgt_max")
        if isinstance(src, TriMesh) and isinstance(a, PointCloud):
            raise TypeError("realign!(::TriMesh, tgt) needs a TriMesh or a (3, V) array target")
        tD, tn = _target_rows(a, index)
        if tn == 0:
            raise ValueError("reducing over an empty collection is not allowed")
        tshape = (tD, 1)
    else:
        sa = a.shape if is_device(a) else np.shape(a)
        sb = b.shape if is_device(b) else np.shape(b)
        if len(sa) != 2 or len(sb) != 2:
            raise TypeError("tgt_min and tgt_max must be 2-D (D, 1) arrays")
        if tuple(sa) != tuple(sb):
            raise ValueError(f"DimensionMismatch: tgt_min {tuple(sa)} and tgt_max {tuple(sb)}")
        tshape = tuple(sb)
    if tshape[0] != D or tshape[1] != 1:
        if isinstance(src, PointCloud) and tshape[0] != D:
            raise ValueError("source and target pointcloud dimension mismatch")
        raise ValueError(f"DimensionMismatch: a (D, 1) target box is needed, got {tshape} for D = {D}")
    if (src.points.shape[1] if isinstance(src, PointCloud) else src.V) == 0:
        raise ValueError("reducing over an empty collection is not allowed")
    tmin, tmax = target_bounds(a, index) if b is None else (_as_bound(a), _as_bound(b))
    sg = _Seg(src)
    smin, smax = segment_minmax(sg, pad_zero=sg.mesh)  # realign!(::TriMesh) reduces over verts_padded
    y = sg.empty_like()
    _lib.call("fx3d_realign", sg.x.ptr, sg.D, sg.n_max, sg.B, sg.off_ptr, smin.ptr, smax.ptr, tmin.ptr, tmax.ptr, y.ptr,
              current_stream().handle)
    return sg.finish(y, inplace)


def realign(src, tgt_or_min, tgt_max=None, index=0):
    """realign(src, tgt[, index]) / realign(src, tgt_min, tgt_max) (pcloud_func.jl:250-262, mesh_func.jl:318-330):
    ((x - smin) / ((smax - smin) + EPS)) * (tmax - tmin) + tmin.  A TriMesh's smin / smax come from verts_padded: a mesh
    shorter than the batch's longest also takes +0.0 (mesh_func.jl:281-283).  ``index`` is 0-based."""
    return _realign(src, tgt_or_min, tgt_max, index, False)


def realign_(src, tgt_or_min, tgt_max=None, index=0):
    """realign!(src, ...) (pcloud_func.jl:206-228, mesh_func.jl:276-298), in place."""
    return _realign(src, tgt_or_min, tgt_max, index, True)


# ---- the transform structs (src/transforms/transforms.jl) ----------------------------------------------------------------

def _jl_f32(v):
    """Julia's `string(::Float32)`: 2.0f0, 0.5f0, 1.0f-6."""
    v = np.float32(v)
    if not np.isfinite(v):
        return {True: "NaN32"}.get(bool(np.isnan(v)), "Inf32" if v > 0 else "-Inf32")
    a = abs(float(v))
    if a == 0.0 or 1e-5 <= a < 1e6:
        t = np.format_float_positional(v, unique=True, trim="0")
        return t + "f0"
    m, e = np.format_float_scientific(v, unique=True, trim="0").split("e")
    return f"{m}f{int(e)}"


def _jl_bool(b):
    return "true" if b else "false"


class AbstractTransform:
    def __repr__(self):
        return f"{type(self).__name__}(...)"


class ScalePointCloud(AbstractTransform):
    def __init__(self, factor, inplace=True):
        self.factor, self.inplace = _check_factor(factor), bool(inplace)

    def __call__(self, p):
        return (scale_ if self.inplace else scale)(p, self.factor)

    def __repr__(self):
        return f"ScalePointCloud(factor={_jl_f32(self.factor)}; inplace={_jl_bool(self.inplace)})"


class RotatePointCloud(AbstractTransform):
    def __init__(self, rotmat, inplace=True):
        R = np.asarray(rotmat)
        if R.shape != (3, 3):
            raise ValueError(f"rotmat must be (3,3) array, but instead got {R.shape} array")
        self.rotmat, self.inplace = R.astype(np.float32), bool(inplace)

    def __call__(self, p):
        return (rotate_ if self.inplace else rotate)(p, self.rotmat)

    def __repr__(self):
        return f"RotatePointCloud(rotmat; inplace={_jl_bool(self.inplace)})"


class ReAlignPointCloud(AbstractTransform):
    """ReAlignPointCloud(target[, index]; inplace) with a PointCloud or a (D, N) / (D, N, B) array target."""

    def __init__(self, target, index=0, inplace=True):
        PointCloud, _ = _rep()
        if not isinstance(target, PointCloud):
            target = PointCloud(target)
        self.t_min, self.t_max = target_bounds(target, index)
        self.inplace = bool(inplace)

    def __call__(self, p):
        return (realign_ if self.inplace else realign)(p, self.t_min, self.t_max)

    def __repr__(self):
        return f"ReAlignPointCloud(target=PointCloud(...); inplace={_jl_bool(self.inplace)})"


class NormalizePointCloud(AbstractTransform):
    def __init__(self, inplace=True):
        self.inplace = bool(inplace)

    def __call__(self, p):
        return (normalize_ if self.inplace else normalize)(p)

    def __repr__(self):
        return f"NormalizePointCloud(;inplace={_jl_bool(self.inplace)})"


class ScaleTriMesh(ScalePointCloud):
    def __repr__(self):
        return f"ScaleTriMesh(factor={_jl_f32(self.factor)}; inplace={_jl_bool(self.inplace)})"


class RotateTriMesh(RotatePointCloud):
    def __repr__(self):
        return f"RotateTriMesh(rotmat; inplace={_jl_bool(self.inplace)})"


class ReAlignTriMesh(AbstractTransform):
    def __init__(self, target, index=0, inplace=True):
        self.t_min, self.t_max = target_bounds(target, index)
        self.inplace = bool(inplace)

    def __call__(self, m):
        return (realign_ if self.inplace else realign)(m, self.t_min, self.t_max)

    def __repr__(self):
        return f"ReAlignTriMesh(target=TriMesh(...); inplace={_jl_bool(self.inplace)})"


class NormalizeTriMesh(NormalizePointCloud):
    def __repr__(self):
        return f"NormalizeTriMesh(;inplace={_jl_bool(self.inplace)})"


class TranslateTriMesh(AbstractTransform):
    def __init__(self, vector, inplace=True):
        if np.ndim(vector) == 0:
            vector = np.full(3, vector)
        v = np.asarray(vector)
        if v.shape != (3,):
            raise ValueError(f"vector must be (3, ), but instead got {v.shape} array")
        self.vector, self.inplace = v.astype(np.float32), bool(inplace)

    def __call__(self, m):
        return (translate_ if self.inplace else translate)(m, self.vector)

    def __repr__(self):
        elems = ", ".join(_jl_f32(x).replace("f0", "").replace("f", "e") for x in self.vector)  # Float32[1.0, 2.0, 3.0]
        return f"TranslateTriMesh(vector=Float32[{elems}];inplace={_jl_bool(self.inplace)})"


class OffsetTriMesh(AbstractTransform):
    def __init__(self, offset_verts, inplace=True):
        self.offset_verts = offset_verts if is_device(offset_verts) else np.asfortranarray(np.asarray(offset_verts, np.float32))
        self.inplace = bool(inplace)

    def __call__(self, m):
        out = offset(m if m.on_device else m._to_device(), self.offset_verts)
        if not m.on_device:
            out = out._to_host()
        if self.inplace:
            m.set_verts_packed(out.get_verts_packed())
            return m
        return out

    def __repr__(self):
        return f"OffsetTriMesh(offset_verts; inplace={_jl_bool(self.inplace)})"


_CONV_ALGOS = ("Exact", "MarchingCubes", "MarchingTetrahedra", "NaiveSurfaceNets")


def _conv_algo(algo):
    algo = str(algo).lstrip(":")
    if algo not in _CONV_ALGOS:
        raise ValueError(f"given algo={algo} is not supported. Accepted algos are "
                         "{:Exact,:MarchingCubes, :MarchingTetrahedra, :NaiveSurfaceNets}.")
    return algo


def _conv_thresh(thresh):
    if not 0 <= thresh <= 1:
        raise ValueError(f"given threshold={thresh} is not between [0,1]")
    return np.float32(thresh)


class TriMeshToVoxelGrid(AbstractTransform):
    def __init__(self, resolution=32):
        self.resolution = int(resolution)

    def __call__(self, m):
        from .conversions import trimesh_to_voxel
        from .rep import VoxelGrid
        return VoxelGrid(trimesh_to_voxel(m, self.resolution))

    def __repr__(self):
        return f"TriMeshToVoxelGrid(resolution={self.resolution})"


class PointCloudToVoxelGrid(AbstractTransform):
    def __init__(self, resolution=32):
        self.resolution = int(resolution)

    def __call__(self, p):
        from .conversions import pointcloud_to_voxel
        from .rep import VoxelGrid
        return VoxelGrid(pointcloud_to_voxel(p, self.resolution))

    def __repr__(self):
        return f"PointCloudToVoxelGrid(resolution={self.resolution})"


class VoxelGridToTriMesh(AbstractTransform):
    def __init__(self, thresh=0.5, algo="MarchingCubes"):
        self.algo = _conv_algo(algo)
        self.threshold = _conv_thresh(thresh)

    def __call__(self, v):
        from .conversions import trimesh_from_voxels
        return trimesh_from_voxels(v, float(self.threshold), self.algo)

    def __repr__(self):
        return f"VoxelGridToTriMesh((threshold={_jl_f32(self.threshold)}, algo={self.algo})"


class PointCloudToTriMesh(AbstractTransform):
    def __init__(self, resolution=32, algo="MarchingCubes"):
        self.algo = _conv_algo(algo)
        self.resolution = int(resolution)

    def __call__(self, p):
        from .conversions import trimesh_from_pointcloud
        return trimesh_from_pointcloud(p, self.resolution)  # TriMesh(p, t.resolution): the default algo (transforms.jl:427)

    def __repr__(self):
        return f"PointCloudToTriMesh(resolution={self.resolution})"


class TriMeshToPointCloud(AbstractTransform):
    def __init__(self, npoints=1024):
        if int(npoints) < 0:
            raise ValueError("npoints cannot be less than 0")
        self.npoints = int(npoints)

    def __call__(self, m, seed=None):
        from .rep import PointCloud
        return PointCloud(sample_points(m, self.npoints, seed=seed))

    def __repr__(self):
        return f"TriMeshToPointCloud(npoints={self.npoints})"


class VoxelGridToPointCloud(AbstractTransform):
    def __init__(self, npoints=1024, thresh=0.5, algo="MarchingCubes"):
        if int(npoints) < 0:
            raise ValueError("npoints cannot be less than 0")
        self.npoints = int(npoints)
        self.algo = _conv_algo(algo)
        self.threshold = _conv_thresh(thresh)

    def __call__(self, v, seed=None):
        from .conversions import pointcloud_from_voxels
        return pointcloud_from_voxels(v, self.npoints, float(self.threshold), self.algo, seed=seed)

    def __repr__(self):
        return f"VoxelGridToPointCloud(npoints={self.npoints}, threshold={_jl_f32(self.threshold)}, algo={self.algo})"


class Chain:
    """Chain(t1, t2, ...): applies the transforms in order (Flux.Chain, as the reference's examples compose them)."""

    def __init__(self, *ts):
        self.transforms = tuple(ts)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x

    def __getitem__(self, i):
        return self.transforms[i]

    def __len__(self):
        return len(self.transforms)

    def __repr__(self):
        return "Chain(" + ", ".join(repr(t) for t in self.transforms) + ")"
