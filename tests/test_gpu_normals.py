"""Vertex and face normals on the device (fx3d_verts_normals_packed / _bwd, fx3d_faces_normals_packed / _bwd) against the
numpy restatement of the reference's CPU semantics (tests/normals_ref.py): bit for bit through a uint32 view, NaN in the same
places, forward and both adjoints, for the reference's known answers, real meshes, every index type, degenerate input, a
2 M-vertex sheet, device-born meshes and a captured graph."""
import json
import os
import zipfile

import numpy as np
import pytest

from conftest import GOLDEN
import normals_ref as ref

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want, np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), what
    bad = np.nonzero(got.view(np.uint32)[~gn] != want.view(np.uint32)[~wn])[0]
    assert bad.size == 0, (what, bad.size, got[~gn][bad[:4]], want[~wn][bad[:4]])


def _packed_host(m):
    return m.get_verts_packed_host(), np.asfortranarray(m.get_faces_packed().astype(np.int64) - m.index_base)


def _check_all(fx, m, grads=True, seed=0):
    """Every form of both normals and both adjoints (with and without accumulate) against the restatement."""
    v, f = _packed_host(m)
    vn, fn = ref.verts_normals(v, f), ref.faces_normals(v, f)
    _same(fx.compute_verts_normals_packed(m).to_host(), vn, "verts packed")
    _same(fx.compute_faces_normals_packed(m).to_host(), fn, "faces packed")
    for kind, want, lens, width in (("verts", vn, m._verts_len, m.V), ("faces", fn, m._faces_len, m.F)):
        pad = getattr(fx, f"compute_{kind}_normals_padded")(m).to_host()
        lst = getattr(fx, f"compute_{kind}_normals_list")(m)
        assert pad.shape == (3, width, m.N) and len(lst) == m.N
        cur = 0
        for b, n in enumerate(lens):
            _same(pad[:, :n, b], want[:, cur:cur + n], f"{kind} padded {b}")
            assert not pad[:, n:, b].any()
            _same(lst[b], want[:, cur:cur + n], f"{kind} list {b}")
            cur += int(n)
    if grads:
        rng = np.random.default_rng(seed)
        for kind, n_out in (("verts", v.shape[1]), ("faces", f.shape[1])):
            bwd = getattr(ref, f"{kind}_normals_bwd")
            grad = getattr(fx, f"compute_{kind}_normals_grad")
            g = np.asfortranarray(rng.standard_normal((3, n_out)).astype(np.float32))
            base = np.asfortranarray(rng.standard_normal(v.shape).astype(np.float32))
            _same(grad(m, g).to_host(), bwd(v, f, g), f"{kind} adjoint")
            out = fx.gpu(base)
            r = grad(m, fx.gpu(g), out=out, accumulate=True)
            assert r is out
            _same(out.to_host(), bwd(v, f, g, base=base), f"{kind} adjoint, accumulate")
            out = fx.gpu(base)
            grad(m, g, out=out)
            _same(out.to_host(), bwd(v, f, g), f"{kind} adjoint, overwrite")
    return vn, fn


def _known_batch(fx, faces_dtype=np.int64, index_base=1):
    k = json.load(open(os.path.join(GOLDEN, "ref_known_answers.json")))["areas_batch"]
    verts = [np.asfortranarray(np.array(v, np.float32).T) for v in k["verts"]]
    faces = [np.asfortranarray((np.array(f, np.int64).T - 1 + index_base).astype(faces_dtype)) for f in k["faces"]]
    return fx.TriMesh(verts, faces, index_base=index_base)


@pytest.mark.parametrize("faces_dtype,index_base", [(np.int64, 1), (np.uint32, 1), (np.int32, 0), (np.int64, 0)])
def test_known_answer_batch_all_forms(gpu_fx, faces_dtype, index_base):
    """test/rep.jl:224-330's batch in the six forms; the reference's UInt32 / Int64 1-based indices and 0-based ones."""
    fx = gpu_fx
    m = fx.gpu(_known_batch(fx, faces_dtype, index_base))
    vn, fn = _check_all(fx, m)
    ka = json.load(open(os.path.join(GOLDEN, "normals_known_answers.json")))
    assert np.allclose(vn, np.concatenate([np.array(a, np.float32).T for a in ka["verts_normals"]], 1), rtol=1e-4, atol=1e-4)
    assert np.allclose(fn, np.concatenate([np.array(a, np.float32).T for a in ka["faces_normals"]], 1), rtol=1e-4, atol=1e-4)
    assert np.signbit(fx.compute_faces_normals_packed(m).to_host()[0, 0])  # _fnormal1's -0.0


def test_host_mesh_uploads(gpu_fx):
    """A host-backed TriMesh goes through the same kernels (its vertices uploaded per call)."""
    _check_all(gpu_fx, _known_batch(gpu_fx), grads=False)


def _modelnet(tmp_path):
    out = []
    for z in ("ModelNet10.zip", "ModelNet40.zip"):
        with zipfile.ZipFile(os.path.join(GOLDEN, "modelnet", z)) as zf:
            for name in sorted(n for n in zf.namelist() if n.endswith(".off")):
                zf.extract(name, tmp_path)
                out.append(os.path.join(tmp_path, name))
    return out


def test_teapot_sphere_modelnet_alone_and_ragged(gpu_fx, tmp_path):
    fx = gpu_fx
    paths = [os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj")] + _modelnet(tmp_path)
    assert len(paths) == 10
    for i, p in enumerate(paths):
        _check_all(fx, fx.gpu(fx.load_trimesh(p)), seed=i)
    _check_all(fx, fx.gpu(fx.load_trimesh(*paths)), seed=99)


def test_last_write_wins_on_the_device(gpu_fx):
    """Vertex 0 is corner 1 of two faces with different normals: the later face's normal alone."""
    fx = gpu_fx
    v = np.asfortranarray(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32).T)
    f = np.asfortranarray(np.array([[1, 2, 3], [1, 4, 2]], np.int64).T)
    m = fx.gpu(fx.TriMesh([v], [f]))
    assert np.array_equal(fx.compute_verts_normals_packed(m).to_host()[:, 0], [0, 1, 0])
    _check_all(fx, m)


def test_degenerate_unused_and_nan(gpu_fx):
    """Degenerate faces (repeated and collinear vertices), vertices no face uses (normal 0), a NaN and an Inf coordinate."""
    fx = gpu_fx
    rng = np.random.default_rng(3)
    v, f = ref.sheet(6, 5, seed=1)
    V = v.shape[1]
    v = np.asfortranarray(np.concatenate([v, rng.standard_normal((3, 4)).astype(np.float32)], 1))  # 4 unused vertices
    f = np.asfortranarray(np.concatenate([f, [[0, 1], [0, 2], [3, 1]]], 1))                          # (0,0,3) and (1,2,1)
    cases = [v]
    vn = v.copy(); vn[1, 7] = np.nan; cases.append(vn)
    vi = v.copy(); vi[0, 20] = np.inf; cases.append(vi)
    vc = v.copy(); vc[:, 10] = vc[:, 9]; cases.append(vc)                                            # coincident vertices
    for i, vv in enumerate(cases):
        m = fx.gpu(fx.TriMesh([np.asfortranarray(vv)], [f], index_base=0))
        vnorm, _ = _check_all(fx, m, seed=i)
        assert np.all(vnorm[:, V:] == 0) and not np.signbit(vnorm[:, V:]).any()
    assert np.isnan(ref.verts_normals(cases[1], f)).any()


def test_launch_grid_does_not_change_the_bits(gpu_fx, fx_option):
    """Grid-stride tails: every kernel capped at a few blocks gives the bits of the default grids."""
    fx = gpu_fx
    m = fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj")))
    g = np.asfortranarray(np.random.default_rng(5).standard_normal((3, int(m._verts_len.sum()))).astype(np.float32))
    gf = np.asfortranarray(np.random.default_rng(6).standard_normal((3, int(m._faces_len.sum()))).astype(np.float32))
    runs = []
    for cap in (0, 3, 7):
        fx_option("mesh_max_blocks", cap)
        runs.append([fx.compute_verts_normals_packed(m).to_host(), fx.compute_faces_normals_packed(m).to_host(),
                     fx.compute_verts_normals_grad(m, g).to_host(), fx.compute_faces_normals_grad(m, gf).to_host()])
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_two_million_vertex_sheet(gpu_fx):
    """The 1400 x 1400-cell sheet: 1.96 M vertices, 3.92 M faces -- thousands of blocks, face kernels grid-striding."""
    fx = gpu_fx
    v, f = ref.sheet(1400, 1400)
    m = fx.gpu(fx.TriMesh([v], [f], index_base=0))
    w = ref.winners(f, v.shape[1])
    _same(fx.compute_verts_normals_packed(m).to_host(), ref.verts_normals(v, f, w), "sheet verts")
    _same(fx.compute_faces_normals_packed(m).to_host(), ref.faces_normals(v, f), "sheet faces")
    rng = np.random.default_rng(8)
    g = np.asfortranarray(rng.standard_normal(v.shape).astype(np.float32))
    _same(fx.compute_verts_normals_grad(m, g).to_host(), ref.verts_normals_bwd(v, f, g), "sheet verts adjoint")
    gf = np.asfortranarray(rng.standard_normal(f.shape).astype(np.float32))
    _same(fx.compute_faces_normals_grad(m, gf).to_host(), ref.faces_normals_bwd(v, f, gf), "sheet faces adjoint")


def test_mesh_born_on_the_device(gpu_fx):
    """trimesh_from_voxels: vertices written by a kernel, host faces built lazily."""
    fx = gpu_fx
    vox = np.zeros((12, 12, 12, 2), np.float32)
    vox[2:9, 3:7, 1:10, 0] = 1
    vox[::2, ::3, 1::2, 1] = 1
    m = fx.trimesh_from_voxels(fx.gpu(np.asfortranarray(vox)), 0.5, "Exact")
    assert m.on_device
    _check_all(fx, m)


def test_eager_calls_and_graph_replay_are_identical(gpu_fx):
    """Two eager calls and a captured graph of forward + adjoint (both kinds) replayed twice: the same bits every time."""
    fx = gpu_fx
    m = fx.gpu(fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj")))
    rng = np.random.default_rng(12)
    g = fx.gpu(np.asfortranarray(rng.standard_normal((3, int(m._verts_len.sum()))).astype(np.float32)))
    gf = fx.gpu(np.asfortranarray(rng.standard_normal((3, int(m._faces_len.sum()))).astype(np.float32)))
    s = fx.Stream.create()

    def step(out):
        res = [fx.compute_verts_normals_packed(m), fx.compute_faces_normals_packed(m)]
        fx.compute_verts_normals_grad(m, g, out=out)
        fx.compute_faces_normals_grad(m, gf, out=out, accumulate=True)
        return res

    with fx.stream(s):
        o1, o2 = fx.DeviceArray.empty(g.shape, np.float32), fx.DeviceArray.empty(g.shape, np.float32)
        e1 = [a.to_host() for a in step(o1)] + [o1.to_host()]
        e2 = [a.to_host() for a in step(o2)] + [o2.to_host()]
        og = fx.DeviceArray.zeros(g.shape, np.float32)
        s.synchronize()
        graph = fx.Graph()
        with graph.capture(s):
            res = step(og)
        for _ in range(2):
            graph.launch()
            s.synchronize()
            rep = [a.to_host() for a in res] + [og.to_host()]
            for a, b, c in zip(e1, e2, rep):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
                assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    v, f = _packed_host(m)
    _same(e1[2], ref.faces_normals_bwd(v, f, gf.to_host(), base=ref.verts_normals_bwd(v, f, g.to_host())), "verts + faces adjoint")
