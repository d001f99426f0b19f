"""The transforms' numpy restatement (tests/transforms_ref.py) against the reference's own tests (test/transforms/*.jl), the
statistics against a math.fsum truth, Julia's min / max rules, the padded-realign quirk, every argument error (raised on the
host, before any launch) and the plan rule.  CPU only."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
import transforms_ref as ref


def _close(a, b):  # isapprox.(a, b, rtol = 1e-5, atol = 1e-5) (test/transforms/*.jl)
    return bool(np.all(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
                       <= 1e-5 + 1e-5 * np.abs(np.asarray(b, np.float64))))


def _rand(shape, seed=0):
    return np.asfortranarray(np.random.default_rng(seed).random(shape, dtype=np.float32))


def test_reference_cases_pointcloud():
    """test/transforms/pcloud_func.jl: normalize's mean ~ 0 and std ~ 1, scale 2 then 0.5, rotate by 2I then its inverse (one
    matrix and one per cloud), realign inside the target's box."""
    p = _rand((3, 8, 2))
    q = ref.pcloud_normalize(p)
    assert _close(q.mean(1), 0) and _close(q.std(1, ddof=1), 1)
    assert _close(ref.pcloud_scale(ref.pcloud_scale(p, 2.0), 0.5), p)
    R = 2 * np.eye(3, dtype=np.float32)
    Ri = np.linalg.inv(R).astype(np.float32)
    assert _close(ref.pcloud_rotate(ref.pcloud_rotate(p, R), Ri), p)
    Rb, Rib = np.stack([R, R], 2), np.stack([Ri, Ri], 2)
    assert _close(ref.pcloud_rotate(ref.pcloud_rotate(p, Rb), Rib), p)
    src, tgt = _rand((8, 3, 2), 1), _rand((8, 3, 1), 2)
    tmin, tmax = ref.bounds(tgt[:, :, 0])
    out = ref.pcloud_realign(src, tmin, tmax)
    assert np.all(out >= tmin[:, :, None]) and np.all(out <= tmax[:, :, None])


def _teapot_sphere():
    from flux3d_jl_amd import load_trimesh
    return load_trimesh(os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj"))


def test_reference_cases_trimesh():
    """test/transforms/mesh_func.jl: the same identities on a batched TriMesh, translate there and back."""
    m = _teapot_sphere()
    v, lens = m.get_verts_packed_host(), m._verts_len
    n = ref.mesh_normalize(v, lens)
    for a, b in ref._segments(lens):
        assert _close(n[:, a:b].mean(1), 0) and _close(n[:, a:b].std(1, ddof=1), 1)
    assert _close(ref.mesh_scale(ref.mesh_scale(v, 2.0), 0.5), v)
    R = 2 * np.eye(3, dtype=np.float32)
    Ri = np.linalg.inv(R).astype(np.float32)
    assert _close(ref.mesh_rotate(ref.mesh_rotate(v, lens, R), lens, Ri), v)
    assert _close(ref.mesh_rotate(ref.mesh_rotate(v, lens, np.stack([R, R], 2)), lens, np.stack([Ri, Ri], 2)), v)
    assert _close(ref.mesh_translate(ref.mesh_translate(v, [1, 2, 3]), [-1, -2, -3]), v)
    tgt = ref.mesh_scale(v, 2.0)
    tmin, tmax = ref.bounds(tgt[:, :int(lens[0])])
    out = ref.mesh_realign(v, lens, tmin, tmax)
    assert np.all(out >= tmin - 1e-5) and np.all(out <= tmax + 1e-5)


def test_rotation_order_is_the_stated_one():
    rng = np.random.default_rng(3)
    R = rng.standard_normal((3, 3)).astype(np.float32)
    x = rng.standard_normal((3, 50)).astype(np.float32)
    y = ref._rot(R, x)
    for i in range(3):
        want = np.float32(np.float32(R[0, i] * x[0]) + np.float32(R[1, i] * x[1])) + np.float32(R[2, i] * x[2])
        assert ref.same_bits(y[i], want)
    assert _close(y, (R.T.astype(np.float64) @ x.astype(np.float64)))


def test_statistics_against_fsum():
    rng = np.random.default_rng(11)
    for n, off in ((2, 0.0), (1000, 0.0), (5000, 1e4), (77, -3.5)):
        x = (rng.standard_normal((2, n)) + off).astype(np.float32)
        c, s = ref.stats(x)
        for d in range(2):
            row = [float(t) for t in x[d]]
            tc = math.fsum(row) / n
            assert c[d] == np.float32(tc)
            ts = math.sqrt(math.fsum((t - float(c[d])) ** 2 for t in row) / (n - 1))
            assert s[d] == np.float32(ts)
    c, s = ref.stats(np.ones((3, 1), np.float32))
    assert np.all(c == 1) and np.all(np.isnan(s))  # n = 1: 0/0
    assert np.all(np.isnan(ref.pcloud_normalize(np.ones((3, 1, 1), np.float32))))
    assert np.all(np.isnan(ref.mesh_normalize(np.ones((3, 1), np.float32), [1])))


def test_ulp_helper():
    a = np.array([1.0, -2.0, 0.0, np.nan], np.float32)
    b = np.nextafter(a, np.float32(np.inf))
    b[3] = np.nan
    assert ref.within_ulp(a, b) and not ref.within_ulp(a, np.nextafter(b, np.float32(np.inf)))
    assert ref.within_ulp(np.float32([-0.0]), np.float32([0.0]))


def test_julia_min_max_rules():
    z = np.array([[0.0, -0.0, 1.0]], np.float32)
    assert np.signbit(ref.jmin(z, 1)[0, 0]) and not np.signbit(ref.jmax(z, 1)[0, 0])
    allneg = np.array([[-0.0, -0.0]], np.float32)
    assert np.signbit(ref.jmax(allneg, 1)[0, 0])
    n = np.array([[1.0, np.nan, -5.0]], np.float32)
    assert np.isnan(ref.jmin(n, 1)[0, 0]) and np.isnan(ref.jmax(n, 1)[0, 0])
    assert np.isnan(ref.jmax2(np.float32(np.nan), ref.EPS)) and ref.jmax2(np.float32(0.0), ref.EPS) == ref.EPS
    assert not np.signbit(ref.jmax2(np.float32(-0.0), np.float32(0.0)))


def test_padded_realign_quirk_teapot_sphere():
    """realign!(::TriMesh) takes min / max over verts_padded (mesh_func.jl:281-283): the shorter mesh's bounds take +0.0."""
    m = _teapot_sphere()
    v, lens = ref.mesh_translate(m.get_verts_packed_host(), 5.0), m._verts_len  # moved off the origin: the quirk shows
    short = int(np.argmin(lens))
    a, b = ref._segments(lens)[short]
    mn, mx = ref.mesh_bounds_padded(v, lens)
    plain_mn, plain_mx = ref.bounds(v[:, a:b])
    want_mn = np.minimum(plain_mn[:, 0], 0)
    want_mx = np.maximum(plain_mx[:, 0], 0)
    assert np.array_equal(mn[:, short], want_mn) and np.array_equal(mx[:, short], want_mx)
    assert not (np.array_equal(plain_mn[:, 0], want_mn) and np.array_equal(plain_mx[:, 0], want_mx)), \
        "fixture must show the quirk: the shorter mesh's box does not contain the origin"
    long_ = 1 - short
    a, b = ref._segments(lens)[long_]
    lmn, lmx = ref.bounds(v[:, a:b])
    assert np.array_equal(mn[:, long_], lmn[:, 0]) and np.array_equal(mx[:, long_], lmx[:, 0])


# ---- argument errors: the restatement and the package raise the same, before any device work -------------------------------
@pytest.fixture(scope="module")
def fxp():
    import flux3d_jl_amd
    return flux3d_jl_amd


def test_argument_errors_restatement():
    p = _rand((3, 4, 2))
    for f in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="factor must be greater than 0.0"):
            ref.pcloud_scale(p, f)
    with pytest.raises(TypeError):
        ref.mesh_scale(p[:, :, 0], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match=r"factor must be \(3, \)"):
        ref.mesh_scale(p[:, :, 0], [1.0, 2.0])
    with pytest.raises(ValueError, match=r"rotmat must be \(3, 3\) array"):
        ref.pcloud_rotate(p, np.eye(4))
    with pytest.raises(ValueError, match=r"rotmat must be \(3, 3, 2\) array"):
        ref.pcloud_rotate(p, np.ones((3, 3, 3)))
    with pytest.raises(ValueError, match="dimension of points in PointCloud must be 3"):
        ref.pcloud_rotate(_rand((4, 4, 2)), np.eye(3))
    with pytest.raises(ValueError, match="dimension mismatch"):
        ref.pcloud_realign(p, np.zeros((2, 1)), np.ones((2, 1)))
    with pytest.raises(ValueError, match="empty collection"):
        ref.pcloud_realign(np.zeros((3, 0, 1), np.float32), np.zeros((3, 1)), np.ones((3, 1)))
    with pytest.raises(ValueError, match="empty collection"):
        ref.bounds(np.zeros((3, 0), np.float32))
    with pytest.raises(ValueError, match=r"vector must be \(3, \)"):
        ref.mesh_translate(p[:, :, 0], [1.0, 2.0])


def test_argument_errors_package(fxp):
    """Every error is raised on the host: these run without a GPU (no launch is reached)."""
    fx = fxp
    p = fx.PointCloud(_rand((3, 4, 2)))
    m = _teapot_sphere()
    for f in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="factor must be greater than 0.0"):
            fx.scale(p, f)
        with pytest.raises(ValueError, match="factor must be greater than 0.0"):
            fx.scale_(m, f)
        with pytest.raises(ValueError, match="factor must be greater than 0.0"):
            fx.ScalePointCloud(f)
    with pytest.raises(TypeError, match="mesh_func.jl:165"):
        fx.scale(m, [2.0, 2.0, 2.0])
    with pytest.raises(ValueError, match=r"factor must be \(3, \)"):
        fx.scale(m, [2.0, 2.0])
    with pytest.raises(ValueError, match=r"rotmat must be \(3, 3\) array"):
        fx.rotate(p, np.eye(4))
    with pytest.raises(ValueError, match=r"rotmat must be \(3, 3, 2\) array"):
        fx.rotate(m, np.ones((3, 3, 3)))
    with pytest.raises(TypeError):
        fx.rotate(p, np.ones(3))
    with pytest.raises(ValueError, match="dimension of points in PointCloud must be 3"):
        fx.rotate(fx.PointCloud(_rand((4, 4, 2))), np.eye(3))
    with pytest.raises(ValueError, match=r"rotmat must be \(3,3\) array"):
        fx.RotatePointCloud(np.eye(2))
    with pytest.raises(ValueError, match="source and target pointcloud dimension mismatch"):
        fx.realign(p, np.zeros((2, 1)), np.ones((2, 1)))
    with pytest.raises(ValueError, match="empty collection"):
        fx.realign(p, fx.PointCloud(np.zeros((3, 0, 1), np.float32)))
    with pytest.raises(ValueError, match=r"vector must be \(3, \)"):
        fx.translate(m, [1.0, 2.0])
    with pytest.raises(ValueError, match=r"vector must be \(3, \)"):
        fx.TranslateTriMesh(np.ones(4))
    with pytest.raises(TypeError):
        fx.translate(p, 1.0)
    with pytest.raises(ValueError, match="not supported"):
        fx.VoxelGridToTriMesh(algo="Nope")
    with pytest.raises(ValueError, match="not between"):
        fx.VoxelGridToPointCloud(thresh=2)
    with pytest.raises(ValueError, match="npoints cannot be less than 0"):
        fx.TriMeshToPointCloud(-1)


def test_transform_reprs(fxp):
    fx = fxp
    assert repr(fx.ScalePointCloud(2.0)) == "ScalePointCloud(factor=2.0f0; inplace=true)"
    assert repr(fx.ScaleTriMesh(0.5, inplace=False)) == "ScaleTriMesh(factor=0.5f0; inplace=false)"
    assert repr(fx.RotatePointCloud(np.eye(3))) == "RotatePointCloud(rotmat; inplace=true)"
    assert repr(fx.NormalizeTriMesh()) == "NormalizeTriMesh(;inplace=true)"
    assert repr(fx.TranslateTriMesh(1.0)) == "TranslateTriMesh(vector=Float32[1.0, 1.0, 1.0];inplace=true)"
    assert repr(fx.VoxelGridToTriMesh(algo="Exact")) == "VoxelGridToTriMesh((threshold=0.5f0, algo=Exact)"
    assert repr(fx.VoxelGridToPointCloud()) == "VoxelGridToPointCloud(npoints=1024, threshold=0.5f0, algo=MarchingCubes)"
    assert repr(fx.TriMeshToPointCloud()) == "TriMeshToPointCloud(npoints=1024)"
    c = fx.Chain(fx.NormalizePointCloud(), fx.PointCloudToVoxelGrid(16))
    assert repr(c) == "Chain(NormalizePointCloud(;inplace=true), PointCloudToVoxelGrid(resolution=16))" and len(c) == 2


def test_chain_applies_in_order(fxp):
    calls = []
    c = fxp.Chain(lambda x: calls.append(1) or x + 1, lambda x: calls.append(2) or x * 3)
    assert c(1) == 6 and calls == [1, 2]


def test_plan_rule(fxp):
    """chunk = 16384 // D columns; fused iff the longest segment fits one chunk; the workspace is one (sum, M2) pair of
    Float64 per (chunk, segment, row).  A pure function of (D, n_max, B)."""
    fx = fxp
    for D in (1, 3, 4, 7, 1024):
        cc = max(1, 16384 // D)
        for n, B in ((1, 1), (cc, 32), (cc + 1, 2), (2_000_000, 1), (0, 3)):
            plan = fx.transform_plan(D, n, B)
            nk = (n + cc - 1) // cc
            assert f"chunk_cols={cc} " in plan and f"nchunks={nk} " in plan
            assert plan.startswith("plan=fused" if nk <= 1 else "plan=two_launch")
            want = 0 if nk <= 1 else nk * B * D * 16
            assert plan.endswith(f"ws={want}")
            assert fx.transform_plan(D, n, B) == plan
    assert fx.transform_plan(3, 1024, 32).startswith("plan=fused")
    assert fx.transform_plan(3, 1_962_801, 1).startswith("plan=two_launch")
