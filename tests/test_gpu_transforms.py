"""PointCloud and TriMesh transforms on the device (fx3d_normalize, fx3d_segment_minmax, fx3d_realign, fx3d_rotate,
fx3d_scale_translate) against the numpy restatement tests/transforms_ref.py: every map bit for bit (uint32 views, NaN in the
same places), the statistics within 1 ulp of the Float64 truth and the same bits on every call, both layouts, both plans,
both forms of every function, the transform structs, a Chain and a captured graph."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import normals_ref
import transforms_ref as ref

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    got = got.to_host() if hasattr(got, "to_host") else np.asarray(got)
    assert got.shape == np.asarray(want).shape, (what, got.shape, np.asarray(want).shape)
    assert ref.same_bits(got, want), (what, got.ravel()[:6], np.asarray(want).ravel()[:6])


def _cloud(rng, D, N, B, offset=0.0):
    x = rng.standard_normal((D, N, B)).astype(np.float32) + np.float32(offset)
    return np.asfortranarray(x)


def _meshes(fx):
    return fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj"))


def _rotmat(rng, B=None):
    shape = (3, 3) if B is None else (3, 3, B)
    return np.asfortranarray(rng.standard_normal(shape).astype(np.float32))


def _check_normalize_cloud(fx, x):
    p = fx.PointCloud(fx.gpu(x))
    out, c, s = fx.normalize(p, return_stats=True)
    wc, ws = ref.pcloud_stats(x)
    c, s = c.to_host(), s.to_host()
    assert ref.within_ulp(c, wc) and ref.within_ulp(s, ws), (c.ravel()[:4], wc.ravel()[:4], s.ravel()[:4], ws.ravel()[:4])
    _same(out.points, ref.pcloud_normalize(x, c, s), f"normalize {x.shape}")
    out2, c2, s2 = fx.normalize(p, return_stats=True)
    assert ref.same_bits(c2.to_host(), c) and ref.same_bits(s2.to_host(), s)
    _same(out2.points, out.points.to_host(), "normalize repeat")
    return c, s


@pytest.mark.parametrize("D", [1, 3, 7])
@pytest.mark.parametrize("N,B", [(1, 1), (2, 32), (1023, 1), (1024, 32), (1025, 2), (70000, 1)])
def test_cloud_maps_all_shapes(gpu_fx, D, N, B):
    fx = gpu_fx
    rng = np.random.default_rng(D * 100003 + N + B)
    x = _cloud(rng, D, N, B)
    _check_normalize_cloud(fx, x)
    p = fx.PointCloud(fx.gpu(x))
    _same(fx.scale(p, 1.7).points, ref.pcloud_scale(x, 1.7), "scale")
    tmin, tmax = np.full((D, 1), -2.0, np.float32), np.linspace(1, 3, D, dtype=np.float32).reshape(D, 1)
    if N > 0:
        _same(fx.realign(p, tmin, tmax).points, ref.pcloud_realign(x, tmin, tmax), "realign")
    if D == 3:
        R = _rotmat(rng)
        _same(fx.rotate(p, R).points, ref.pcloud_rotate(x, R), "rotate (3,3)")
        Rb = _rotmat(rng, B)
        _same(fx.rotate(p, Rb).points, ref.pcloud_rotate(x, Rb), "rotate (3,3,B)")
    _same(p.points, x, "input unchanged")


def test_plans_forced_at_their_boundary(gpu_fx):
    """chunk = 16384 // D columns: n_max = chunk is the fused plan, chunk + 1 the two-launch plan; both meet the contract."""
    fx = gpu_fx
    rng = np.random.default_rng(5)
    for D in (3, 4, 7):
        cc = 16384 // D
        assert fx.transform_plan(D, cc, 2).startswith("plan=fused")
        assert fx.transform_plan(D, cc + 1, 2).startswith("plan=two_launch")
        for N in (cc, cc + 1, 3 * cc + 5):
            x = _cloud(rng, D, N, 2, offset=1e4)
            _check_normalize_cloud(fx, x)
            p = fx.PointCloud(fx.gpu(x))
            mn, mx = fx.segment_minmax(p)
            _same(mn, ref.jmin(x, 1)[:, 0, :], "min")
            _same(mx, ref.jmax(x, 1)[:, 0, :], "max")


def test_special_values(gpu_fx):
    """+-0, NaN, Inf and a 1e4 offset: Julia's min / max rules, NaN propagation through the statistics, bits of the maps."""
    fx = gpu_fx
    rng = np.random.default_rng(9)
    for N in (100, 20000):
        x = _cloud(rng, 3, N, 4, offset=1e4)
        x[0, :, 1] = 0.0
        x[0, 3, 1] = -0.0              # min -0.0, max +0.0
        x[1, :, 1] = -0.0              # all -0.0: min and max -0.0
        x[2, 7, 2] = np.nan            # NaN row
        x[1, 5, 3] = np.inf            # Inf row
        x[2, 9, 3] = -np.inf
        p = fx.PointCloud(fx.gpu(x))
        mn, mx = fx.segment_minmax(p)
        _same(mn, ref.jmin(x, 1)[:, 0, :], "min")
        _same(mx, ref.jmax(x, 1)[:, 0, :], "max")
        assert np.signbit(mn.to_host()[0, 1]) and not np.signbit(mx.to_host()[0, 1])
        assert np.signbit(mx.to_host()[1, 1])
        _check_normalize_cloud(fx, x)
        tmin, tmax = np.zeros((3, 1), np.float32), np.ones((3, 1), np.float32)
        _same(fx.realign(p, tmin, tmax).points, ref.pcloud_realign(x, tmin, tmax), "realign special")
        _same(fx.scale(p, 3.0).points, ref.pcloud_scale(x, 3.0), "scale special")
        R = _rotmat(rng)
        _same(fx.rotate(p, R).points, ref.pcloud_rotate(x, R), "rotate special")


def test_single_point_gives_nan(gpu_fx):
    fx = gpu_fx
    x = np.asfortranarray(np.array([[[1.0]], [[2.0]], [[3.0]]], np.float32))
    assert np.all(np.isnan(fx.normalize(fx.PointCloud(fx.gpu(x))).points.to_host()))
    m = fx.gpu(fx.TriMesh([np.ones((3, 1), np.float32)], [np.array([[1], [1], [1]])]))
    assert np.all(np.isnan(fx.normalize(m).get_verts_packed().to_host()))


def test_empty_cloud(gpu_fx):
    fx = gpu_fx
    p = fx.PointCloud(fx.gpu(np.zeros((3, 0, 2), np.float32, order="F")))
    for f in (fx.normalize, lambda q: fx.scale(q, 2.0), lambda q: fx.rotate(q, np.eye(3))):
        assert f(p).points.shape == (3, 0, 2)
    with pytest.raises(ValueError, match="empty collection"):
        fx.realign(p, np.zeros((3, 1)), np.ones((3, 1)))


def _mesh_checks(fx, m, seed=0):
    rng = np.random.default_rng(seed)
    v = m.get_verts_packed().to_host() if m.on_device else m.get_verts_packed_host()
    lens = m._verts_len
    out, c, s = fx.normalize(m, return_stats=True)
    wc, ws = ref.mesh_stats(v, lens)
    assert ref.within_ulp(c.to_host(), wc) and ref.within_ulp(s.to_host(), ws)
    _same(out.get_verts_packed(), ref.mesh_normalize(v, lens, c.to_host(), s.to_host()), "mesh normalize")
    _same(fx.scale(m, 0.25).get_verts_packed(), ref.mesh_scale(v, 0.25), "mesh scale")
    _same(fx.translate(m, [1.0, -2.0, 1e4]).get_verts_packed(), ref.mesh_translate(v, [1.0, -2.0, 1e4]), "mesh translate")
    _same(fx.translate(m, 0.5).get_verts_packed(), ref.mesh_translate(v, 0.5), "mesh translate scalar")
    R, Rb = _rotmat(rng), _rotmat(rng, m.N)
    _same(fx.rotate(m, R).get_verts_packed(), ref.mesh_rotate(v, lens, R), "mesh rotate")
    _same(fx.rotate(m, Rb).get_verts_packed(), ref.mesh_rotate(v, lens, Rb), "mesh rotate batched")
    tmin, tmax = np.array([[-1.0], [0.0], [2.0]], np.float32), np.array([[1.0], [3.0], [2.5]], np.float32)
    _same(fx.realign(m, tmin, tmax).get_verts_packed(), ref.mesh_realign(v, lens, tmin, tmax), "mesh realign")
    _same(m.get_verts_packed().to_host() if m.on_device else m.get_verts_packed_host(), v, "mesh input unchanged")


def test_teapot_and_sphere_batched(gpu_fx):
    fx = gpu_fx
    h = _meshes(fx)
    assert h._verts_len[0] != h._verts_len[1]
    _mesh_checks(fx, fx.gpu(h))
    _mesh_checks(fx, h, seed=1)  # host storage: uploaded, transformed, returned on the host
    assert not fx.scale(h, 2.0).on_device
    # the padded-realign quirk: the shorter mesh takes +0.0 into its bounds
    d = fx.gpu(h)
    mn, mx = fx.segment_minmax(d, pad_zero=True)
    wmn, wmx = ref.mesh_bounds_padded(h.get_verts_packed_host(), h._verts_len)
    _same(mn, wmn, "padded min")
    _same(mx, wmx, "padded max")
    # realign onto a target mesh's box, index 1 (0-based): get_verts_list(tgt)[index]
    tgt = fx.gpu(fx.scale(h, 3.0))
    tl = tgt.get_verts_list()[1]
    _same(fx.realign(d, tgt, index=1).get_verts_packed(),
          ref.mesh_realign(h.get_verts_packed_host(), h._verts_len, ref.jmin(tl, 1), ref.jmax(tl, 1)), "realign onto mesh")


def test_two_million_vertex_sheet(gpu_fx):
    """1.96 M vertices in one mesh: the two-launch plan on the packed layout."""
    fx = gpu_fx
    v, f = normals_ref.sheet(1400, 1400)
    m = fx.gpu(fx.TriMesh([v], [f], index_base=0))
    assert fx.transform_plan(3, m.V, 1).startswith("plan=two_launch")
    _mesh_checks(fx, m, seed=3)


def test_inplace_forms_return_the_same_object(gpu_fx):
    fx = gpu_fx
    rng = np.random.default_rng(4)
    x = _cloud(rng, 3, 500, 3)
    n = _cloud(rng, 3, 500, 3)
    p = fx.PointCloud(fx.gpu(x), fx.gpu(n))
    _, c, s = fx.normalize(p, return_stats=True)
    assert fx.normalize_(p) is p
    _same(p.points, ref.pcloud_normalize(x, c.to_host(), s.to_host()), "normalize_")
    _same(p.normals, n, "normals untouched")
    y = p.points.to_host()
    R = _rotmat(rng)
    assert fx.rotate_(p, R) is p
    _same(p.points, ref.pcloud_rotate(y, R), "rotate_")
    _same(p.normals, n, "normals untouched by rotate")
    y = p.points.to_host()
    assert fx.scale_(p, 2.0) is p
    _same(p.points, ref.pcloud_scale(y, 2.0), "scale_")
    y = p.points.to_host()
    assert fx.realign_(p, np.zeros((3, 1)), np.ones((3, 1))) is p
    _same(p.points, ref.pcloud_realign(y, np.zeros((3, 1)), np.ones((3, 1))), "realign_")
    h = _meshes(fx)
    for m in (fx.gpu(h), h):
        v = m.get_verts_packed_host()
        assert fx.translate_(m, [1, 2, 3]) is m
        _same(m.get_verts_packed_host(), ref.mesh_translate(v, [1, 2, 3]), "translate_")
        for f in (fx.normalize_, lambda q: fx.scale_(q, 0.5), lambda q: fx.rotate_(q, np.eye(3)),
                  lambda q: fx.realign_(q, np.zeros((3, 1)), np.ones((3, 1)))):
            assert f(m) is m
        assert m.on_device == (m is not h)


def test_mesh_mirrors_are_dropped(gpu_fx):
    """sample_points and chamfer_distance on a mesh normalised in place equal those of a fresh device mesh of the same verts."""
    fx = gpu_fx
    m = fx.gpu(_meshes(fx))
    fx.sample_points(m, 300, seed=2)          # builds the CDF and the padded mirror
    m.get_verts_padded()
    fx.normalize_(m)
    fresh = fx.gpu(fx.TriMesh(m.get_verts_list(), m.get_faces_list()))
    a, b = fx.sample_points(m, 400, seed=7).to_host(), fx.sample_points(fresh, 400, seed=7).to_host()
    assert ref.same_bits(a, b)
    _same(m.get_verts_padded(), fresh.get_verts_padded().to_host(), "padded mirror")
    y = fx.gpu(_cloud(np.random.default_rng(1), 3, 400, 2))
    assert float(fx.chamfer_distance(fx.sample_points(m, 400, seed=3), y)) == \
        float(fx.chamfer_distance(fx.sample_points(fresh, 400, seed=3), y))


def test_transform_structs_and_chain(gpu_fx):
    fx = gpu_fx
    rng = np.random.default_rng(8)
    x = _cloud(rng, 3, 1024, 4)
    R = _rotmat(rng)
    tgt = fx.PointCloud(_cloud(rng, 3, 64, 2))
    p = fx.PointCloud(fx.gpu(x))
    q = fx.Chain(fx.NormalizePointCloud(inplace=False), fx.ScalePointCloud(2.0, inplace=False),
                 fx.RotatePointCloud(R, inplace=False), fx.ReAlignPointCloud(tgt, 1, inplace=False))(p)
    assert q is not p
    _same(p.points, x, "chain input unchanged")
    _, c, s = fx.normalize(p, return_stats=True)
    y = ref.pcloud_normalize(x, c.to_host(), s.to_host())
    y = ref.pcloud_rotate(ref.pcloud_scale(y, 2.0), R)
    tp = tgt.points[:, :, 1]
    _same(q.points, ref.pcloud_realign(y, ref.jmin(tp, 1), ref.jmax(tp, 1)), "chain")
    assert fx.NormalizePointCloud()(p) is p
    h = fx.gpu(_meshes(fx))
    v = h.get_verts_packed().to_host()
    out = fx.Chain(fx.ScaleTriMesh(2.0, inplace=False), fx.TranslateTriMesh(1.0, inplace=False),
                   fx.RotateTriMesh(R, inplace=False))(h)
    _same(out.get_verts_packed(), ref.mesh_rotate(ref.mesh_translate(ref.mesh_scale(v, 2.0), 1.0), h._verts_len, R), "mesh chain")
    o = fx.OffsetTriMesh(np.ones_like(v), inplace=False)(h)
    _same(o.get_verts_packed(), v + np.float32(1), "offset")
    nm = fx.NormalizeTriMesh(inplace=False)(h)
    _same(nm.get_verts_packed(), fx.normalize(h).get_verts_packed().to_host(), "NormalizeTriMesh")
    ra = fx.ReAlignTriMesh(fx.scale(h, 2.0), 0, inplace=False)(h)
    t0 = fx.scale(h, 2.0).get_verts_list()[0]
    _same(ra.get_verts_packed(), ref.mesh_realign(v, h._verts_len, ref.jmin(t0, 1), ref.jmax(t0, 1)), "ReAlignTriMesh")
    vg = fx.TriMeshToVoxelGrid(16)(h)
    assert vg.voxels.shape == (16, 16, 16, 2)
    assert fx.PointCloudToVoxelGrid(8)(p).voxels.shape == (8, 8, 8, 4)
    assert fx.TriMeshToPointCloud(100)(h, seed=1).points.shape == (3, 100, 2)
    m2 = fx.VoxelGridToTriMesh(algo="Exact")(vg)
    assert m2.N == 2
    assert fx.VoxelGridToPointCloud(50, algo="Exact")(vg, seed=1).points.shape == (3, 50, 2)
    assert fx.PointCloudToTriMesh(8, algo="Exact").resolution == 8


def test_graph_replay_matches_eager(gpu_fx):
    """A captured NormalizePointCloud followed by RotatePointCloud replays to the same bits as the eager calls."""
    fx = gpu_fx
    rng = np.random.default_rng(6)
    R = _rotmat(rng)
    chain = fx.Chain(fx.NormalizePointCloud(inplace=False), fx.RotatePointCloud(R, inplace=False))
    for N in (1024, 20000):   # fused and two-launch plans
        x = fx.gpu(_cloud(rng, 3, N, 8, offset=3.0))
        p = fx.PointCloud(x)
        s = fx.Stream.create()
        with fx.stream(s):
            e1 = chain(p).points.to_host()
            e2 = chain(p).points.to_host()
            s.synchronize()
            graph = fx.Graph()
            with graph.capture(s):
                out = chain(p)
            for _ in range(2):
                graph.launch()
                s.synchronize()
                assert ref.same_bits(out.points.to_host(), e1)
        assert ref.same_bits(e1, e2)
