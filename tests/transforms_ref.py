"""numpy restatement of the PointCloud / TriMesh transforms (src/transforms/pcloud_func.jl, src/transforms/mesh_func.jl:99-399,
src/transforms/transforms.jl) -- the contract the device must meet (include/flux3d_hip.h).

Clouds are (D, N, B) Float32 arrays, meshes are packed (3, sum V) Float32 arrays with their per-mesh vertex counts.  Every map
is Float32, unfused, bracketed as the reference's broadcast; numpy evaluates each binary operation with one IEEE rounding, so
the device must match these results bit for bit.  The reference's rotate goes through BLAS (`*`, `batched_mul`), whose
summation order nobody can pin: the order below is this project's definition, checked against the reference's own tests at
their tolerance (rtol = atol = 1e-5, test/transforms/mesh_func.jl:80-117).

Edge cases, each from the reference source:
* empty cloud (N = 0): normalize / scale / rotate return an empty cloud (`mean` of nothing is 0/0, never used; `lmul!` and
  `*` of a (3, 0) block are empty); realign throws: `minimum(points, dims = 2)` reduces over an empty collection
  (pcloud_func.jl:215-216) -- and so does an empty realign TARGET (pcloud_func.jl:222-224, mesh_func.jl:292-294).
* factor <= 0 or NaN: `(factor > 0.0) || error("factor must be greater than 0.0")` (pcloud_func.jl:63, mesh_func.jl:155).
* scale!(m::TriMesh, ::AbstractArray) with a (3,) factor: `(factor .> 0.0) || error(...)` puts a BitVector in `||`, a
  TypeError whatever the values (mesh_func.jl:165).  Another size: "factor must be (3, ), ..." first (:163-164).
* rotmat of the wrong size: "rotmat must be (3, 3) array, ..." (pcloud_func.jl:121-122, mesh_func.jl:222-223) or
  "rotmat must be (3, 3, B) array, ..." (pcloud_func.jl:132-133, mesh_func.jl:230-231); then a cloud with D != 3:
  "dimension of points in PointCloud must be 3" (pcloud_func.jl:123, 134).
* realign of a cloud whose D differs from the target's: "source and target pointcloud dimension mismatch"
  (pcloud_func.jl:211-212), checked before the source's min / max.
* translate with a vector that is not (3,): "vector must be (3, ), ..." (mesh_func.jl:332-333).
* n = 1: normalize gives NaN in both forms (std of one point is 0/0 with the corrected estimator).
"""
import math

import numpy as np

EPS = np.float32(1e-6)  # src/transforms/utils.jl:4
f32 = np.float32


# ---- Julia's min / max (base/math.jl): NaN propagates, -0.0 < +0.0 -----------------------------------------------------------
def jmin(a, axis):
    """minimum(a; dims = axis) with Julia's min."""
    a = np.asarray(a, np.float32)
    m = np.min(np.where(np.isnan(a), np.inf, a), axis=axis, keepdims=True)
    neg0 = np.any((a == 0) & np.signbit(a), axis=axis, keepdims=True)
    m = np.where((m == 0) & neg0, f32(-0.0), m)
    return np.where(np.any(np.isnan(a), axis=axis, keepdims=True), f32(np.nan), m).astype(np.float32)


def jmax(a, axis):
    """maximum(a; dims = axis) with Julia's max."""
    a = np.asarray(a, np.float32)
    m = np.max(np.where(np.isnan(a), -np.inf, a), axis=axis, keepdims=True)
    pos0 = np.any((a == 0) & ~np.signbit(a), axis=axis, keepdims=True)
    m = np.where((m == 0) & pos0, f32(0.0), m)
    return np.where(np.any(np.isnan(a), axis=axis, keepdims=True), f32(np.nan), m).astype(np.float32)


def jmax2(x, y):
    """Julia's max(x, y) elementwise (max.(_std, EPS), mesh_func.jl:111)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    out = np.where((y > x) | (~np.signbit(y) & np.signbit(x)), np.where(np.isnan(x), x, y), np.where(np.isnan(y), y, x))
    return out.astype(np.float32)


# ---- the statistics contract (include/flux3d_hip.h) --------------------------------------------------------------------------
def stats(cols):
    """(c, s) of one (D, n) block: c = Float32(sum x / n) with the sum in Float64, s = Float32(sqrt(sum (x - c)^2 / (n - 1)))
    in Float64 with the Float32 c.  math.fsum: the correctly rounded Float64 truth."""
    cols = np.asarray(cols, np.float32)
    D, n = cols.shape
    c = np.empty(D, np.float32)
    s = np.empty(D, np.float32)
    with np.errstate(all="ignore"):
        for d in range(D):
            row = cols[d].astype(np.float64)
            tot = math.fsum(row) if np.all(np.isfinite(row)) else float(np.sum(row))
            c[d] = f32(tot / n) if n else f32(np.nan)
            if np.all(np.isfinite(row)) and n > 1:
                s[d] = f32(math.sqrt(math.fsum((row - float(c[d])) ** 2) / (n - 1)))
            else:
                q = np.sum((row - float(c[d])) ** 2)
                s[d] = f32(np.sqrt(q / (n - 1))) if n != 1 else f32(np.nan)
    return c, s


def _segments(lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [(int(off[i]), int(off[i + 1])) for i in range(len(lens))]


# ---- PointCloud (pcloud_func.jl) ---------------------------------------------------------------------------------------------
def pcloud_stats(points):
    D, N, B = points.shape
    cs = [stats(points[:, :, b]) for b in range(B)]
    return np.stack([c for c, _ in cs], 1), np.stack([s for _, s in cs], 1)


def pcloud_normalize(points, c=None, s=None):
    """normalize!(pcloud) (pcloud_func.jl:16-22): (x - c) ./ (s .+ EPS), given the statistics (default: the contract's)."""
    if c is None:
        c, s = pcloud_stats(points)
    c, s = c[:, None, :], s[:, None, :]
    with np.errstate(all="ignore"):
        return ((points - c) / (s + EPS)).astype(np.float32)


def check_factor(factor):
    f = f32(factor)
    if not f > 0.0:
        raise ValueError("factor must be greater than 0.0")
    return f


def pcloud_scale(points, factor):
    """scale!(pcloud, factor) (pcloud_func.jl:62-66): lmul!(factor, points) = factor * x."""
    return (check_factor(factor) * points).astype(np.float32)


def _rot(R, x):
    """transpose(R) * x, y_i = (R[0,i] x0 + R[1,i] x1) + R[2,i] x2 in Float32, unfused, in that order."""
    R = np.asarray(R, np.float32)
    x = np.asarray(x, np.float32)
    out = np.empty_like(x)
    for i in range(3):
        out[i] = (R[0, i] * x[0] + R[1, i] * x[1]) + R[2, i] * x[2]
    return out


def check_rotmat(rotmat, B, D):
    R = np.asarray(rotmat)
    if R.ndim == 2 and R.shape != (3, 3):
        raise ValueError(f"rotmat must be (3, 3) array, but instead got {R.shape} array")
    if R.ndim == 3 and R.shape != (3, 3, B):
        raise ValueError(f"rotmat must be (3, 3, {B}) array, but instead got {R.shape} array")
    if R.ndim not in (2, 3):
        raise TypeError("no method matching rotate!")
    if D != 3:
        raise ValueError("dimension of points in PointCloud must be 3")
    return R.astype(np.float32)


def pcloud_rotate(points, rotmat):
    """rotate!(pcloud, rotmat) (pcloud_func.jl:120-137)."""
    D, N, B = points.shape
    R = check_rotmat(rotmat, B, D)
    out = np.empty_like(points)
    for b in range(B):
        out[:, :, b] = _rot(R if R.ndim == 2 else R[:, :, b], points[:, :, b])
    return out


def realign_map(x, smin, smax, tmin, tmax):
    """((x .- smin) ./ (smax - smin .+ EPS)) .* (tmax - tmin) .+ tmin (pcloud_func.jl:213-217, mesh_func.jl:284-288)."""
    with np.errstate(all="ignore"):
        return (((x - smin) / ((smax - smin) + EPS)) * (tmax - tmin) + tmin).astype(np.float32)


def bounds(cols):
    """minimum / maximum(cols, dims = 2) of a (D, n) block; an empty block throws like Julia."""
    if cols.shape[1] == 0:
        raise ValueError("reducing over an empty collection is not allowed")
    return jmin(cols, 1), jmax(cols, 1)


def pcloud_realign(points, tmin, tmax):
    """realign!(src, tgt_min, tgt_max) (pcloud_func.jl:206-218)."""
    tmin, tmax = np.asarray(tmin, np.float32), np.asarray(tmax, np.float32)
    if points.shape[0] != tmax.shape[0]:
        raise ValueError("source and target pointcloud dimension mismatch")
    if points.shape[1] == 0:
        raise ValueError("reducing over an empty collection is not allowed")
    smin, smax = jmin(points, 1), jmax(points, 1)
    return realign_map(points, smin, smax, tmin[:, :, None], tmax[:, :, None])


# ---- TriMesh (mesh_func.jl:99-399) over packed (3, sum V) ---------------------------------------------------------------------
def mesh_stats(packed, lens):
    cs = [stats(packed[:, a:b]) for a, b in _segments(lens)]
    return np.stack([c for c, _ in cs], 1), np.stack([s for _, s in cs], 1)


def mesh_normalize(packed, lens, c=None, s=None):
    """normalize!(m) (mesh_func.jl:99-113): (x - c) ./ max.(s, EPS) per mesh (Julia's max: NaN wins)."""
    if c is None:
        c, s = mesh_stats(packed, lens)
    out = np.empty_like(packed)
    with np.errstate(all="ignore"):
        for i, (a, b) in enumerate(_segments(lens)):
            out[:, a:b] = (packed[:, a:b] - c[:, i:i + 1]) / jmax2(s[:, i:i + 1], EPS)
    return out.astype(np.float32)


def mesh_scale(packed, factor):
    """scale!(m, factor) (mesh_func.jl:154-160 scalar; :162-169 a (3,) array always throws TypeError)."""
    if np.ndim(factor) > 0:
        f = np.asarray(factor)
        if f.shape != (3,):
            raise ValueError(f"factor must be (3, ), but instead got {f.shape} array")
        raise TypeError("non-boolean (BitVector) used in boolean context (src/transforms/mesh_func.jl:165)")
    return (check_factor(factor) * packed).astype(np.float32)


def mesh_translate(packed, vector):
    """translate!(m, vector) (mesh_func.jl:329-339): x .+ reshape(vector, :, 1); a scalar is fill(t, 3)."""
    if np.ndim(vector) == 0:
        vector = np.full(3, f32(vector))
    v = np.asarray(vector)
    if v.shape != (3,):
        raise ValueError(f"vector must be (3, ), but instead got {v.shape} array")
    return (packed + v.astype(np.float32)[:, None]).astype(np.float32)


def mesh_rotate(packed, lens, rotmat):
    """rotate!(m, rotmat) (mesh_func.jl:221-235): one (3,3) matrix over the packed verts, or (3,3,B) per mesh."""
    R = np.asarray(rotmat)
    if R.ndim == 2 and R.shape != (3, 3):
        raise ValueError(f"rotmat must be (3, 3) array, but instead got {R.shape} array")
    if R.ndim == 3 and R.shape != (3, 3, len(lens)):
        raise ValueError(f"rotmat must be (3, 3, {len(lens)}) array, but instead got {R.shape} array")
    R = R.astype(np.float32)
    if R.ndim == 2:
        return _rot(R, packed)
    out = np.empty_like(packed)
    for i, (a, b) in enumerate(_segments(lens)):
        out[:, a:b] = _rot(R[:, :, i], packed[:, a:b])
    return out


def mesh_bounds_padded(packed, lens):
    """minimum / maximum(verts_padded, dims = 2) (mesh_func.jl:281-283): a mesh shorter than the longest gets the +0.0 padding."""
    V = int(max(lens))
    mins, maxs = [], []
    for a, b in _segments(lens):
        blk = packed[:, a:b]
        if b - a < V:
            blk = np.concatenate([blk, np.zeros((3, 1), np.float32)], 1)
        lo, hi = bounds(blk)
        mins.append(lo[:, 0])
        maxs.append(hi[:, 0])
    return np.stack(mins, 1), np.stack(maxs, 1)


def mesh_realign(packed, lens, tmin, tmax):
    """realign!(src::TriMesh, tgt_min, tgt_max) (mesh_func.jl:276-289)."""
    tmin, tmax = np.asarray(tmin, np.float32), np.asarray(tmax, np.float32)
    smin, smax = mesh_bounds_padded(packed, lens)
    out = np.empty_like(packed)
    for i, (a, b) in enumerate(_segments(lens)):
        out[:, a:b] = realign_map(packed[:, a:b], smin[:, i:i + 1], smax[:, i:i + 1], tmin, tmax)
    return out


# ---- comparison helpers ------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """Equal uint32 views where not NaN, and NaN in the same places."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def within_ulp(a, b, ulps=1):
    """|a - b| <= ulps units in the last place of Float32 (NaN in the same places)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    ia, ib = a[~na].view(np.int32).astype(np.int64), b[~nb].view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return bool(np.all(np.abs(ia - ib) <= ulps))
