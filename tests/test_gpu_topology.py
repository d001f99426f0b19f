"""Mesh topology built on the device (csrc/topology_dev.hip) against the host builders of csrc/topology.cpp.

Every comparison is np.array_equal on integers and on the uint32 view of the Laplacian's values, against fx3d_build_*
called directly on the same faces: the outputs are integers except `vals`, whose expression is IEEE-exact on both sides, so
there is no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from normals_ref import sheet

pytestmark = pytest.mark.gpu


# ---- the host builders, called directly (0-based int arrays in, int32 out) -------------------------------------------
def host_edges(lib, faces, V):
    faces = np.asfortranarray(faces, dtype=np.int64)
    F = faces.shape[1]
    buf, f2e, E = np.zeros(6 * F, np.int64), np.zeros((F, 3), np.int64, order="F"), C.c_int64(0)
    lib.call("fx3d_build_edges_packed", faces.ctypes.data, F, V, 0, buf.ctypes.data, f2e.ctypes.data, C.byref(E))
    E = E.value
    return np.asfortranarray(buf[:2 * E].reshape((E, 2), order="F").astype(np.int32)), np.asfortranarray(f2e.astype(np.int32))


def host_laplacian(lib, edges, V):
    e = np.asfortranarray(edges, dtype=np.int64)
    E = e.shape[0]
    rowptr, colind, vals = np.zeros(V + 1, np.int32), np.zeros(2 * E + V, np.int32), np.zeros(2 * E + V, np.float32)
    nnz = C.c_int64(0)
    lib.call("fx3d_build_laplacian_csr", e.ctypes.data, E, V, 0, rowptr.ctypes.data, colind.ctypes.data, vals.ctypes.data,
             C.byref(nnz))
    return rowptr, colind[:nnz.value].copy(), vals[:nnz.value].copy()


def host_vertex_faces(lib, faces_padded, faces_len, Vmax):
    fp = np.asfortranarray(faces_padded, dtype=np.int32)
    Fmax, B = fp.shape[1], fp.shape[2]
    fl = np.ascontiguousarray(faces_len, dtype=np.int32)
    rowptr, ent = np.zeros((Vmax + 1, B), np.int32, order="F"), np.zeros((3 * Fmax, B), np.int32, order="F")
    lib.call("fx3d_build_vertex_faces", fp.ctypes.data, fl.ctypes.data, Vmax, Fmax, B, rowptr.ctypes.data, ent.ctypes.data)
    return rowptr, ent


# ---- the device entry points through the raw ABI ---------------------------------------------------------------------
class Dev:
    def __init__(self, fx):
        self.fx, self.lib, self.A = fx, fx._lib, fx.DeviceArray

    def _ws(self, query, *sizes):
        return self.A.empty((self.lib.query_bytes(query, *sizes),), np.uint8)

    def edges(self, faces, V, want_bad=False):
        fx, A = self.fx, self.A
        f = A.from_host(np.asfortranarray(faces, dtype=np.int32))
        F, s = f.shape[1], fx.current_stream().handle
        ws = self._ws("fx3d_edges_dev_workspace_bytes", F, V)
        cnt, bad = A.empty((1,), np.int64), A.empty((1,), np.uint32)
        self.lib.call("fx3d_edges_dev_count", f.ptr, F, V, cnt.ptr, bad.ptr, ws.ptr, ws.nbytes, s)
        E, nbad = int(cnt.to_host()[0]), int(bad.to_host()[0])
        edges, f2e = A.empty((E, 2), np.int32), A.empty((F, 3), np.int32)
        self.lib.call("fx3d_edges_dev_emit", f.ptr, F, V, E, edges.ptr, f2e.ptr, ws.ptr, ws.nbytes, s)
        out = (edges.to_host(), f2e.to_host())
        return out + (nbad,) if want_bad else out

    def laplacian(self, edges, V):
        A = self.A
        e = A.from_host(np.asfortranarray(edges, dtype=np.int32))
        E = e.shape[0]
        ws = self._ws("fx3d_laplacian_dev_workspace_bytes", E, V)
        rowptr, colind, vals = A.empty((V + 1,), np.int32), A.zeros((2 * E + V,), np.int32), A.zeros((2 * E + V,), np.float32)
        cnt, bad = A.empty((1,), np.int64), A.empty((1,), np.uint32)
        self.lib.call("fx3d_laplacian_dev_csr", e.ptr, E, V, rowptr.ptr, colind.ptr, vals.ptr, cnt.ptr, bad.ptr, ws.ptr, ws.nbytes,
                      self.fx.current_stream().handle)
        nnz = int(cnt.to_host()[0])
        assert int(bad.to_host()[0]) == 0
        return rowptr.to_host(), colind.to_host()[:nnz], vals.to_host()[:nnz]

    def vertex_faces(self, faces_padded, faces_len, Vmax):
        A = self.A
        fp = A.from_host(np.asfortranarray(faces_padded, dtype=np.int32))
        Fmax, B = fp.shape[1], fp.shape[2]
        fl = A.from_host(np.ascontiguousarray(faces_len, dtype=np.int32))
        ws = self._ws("fx3d_vertex_faces_dev_workspace_bytes", Vmax, Fmax, B)
        rowptr, ent, bad = A.empty((Vmax + 1, B), np.int32), A.empty((3 * Fmax, B), np.int32), A.empty((1,), np.uint32)
        self.lib.call("fx3d_vertex_faces_dev", fp.ptr, fl.ptr, Vmax, Fmax, B, rowptr.ptr, ent.ptr, bad.ptr, ws.ptr, ws.nbytes,
                      self.fx.current_stream().handle)
        assert int(bad.to_host()[0]) == 0
        return rowptr.to_host(), ent.to_host()

    def pack(self, faces_padded, faces_len, nverts):
        A = self.A
        fp = A.from_host(np.asfortranarray(faces_padded, dtype=np.int32))
        Fmax, B, sumF = fp.shape[1], fp.shape[2], int(np.sum(faces_len))
        fl, nv = A.from_host(np.asarray(faces_len, np.int32)), A.from_host(np.asarray(nverts, np.int32))
        ws = self._ws("fx3d_faces_padded_to_packed_dev_workspace_bytes", B)
        out = A.empty((3, sumF), np.int32)
        self.lib.call("fx3d_faces_padded_to_packed_dev", fp.ptr, fl.ptr, nv.ptr, Fmax, B, sumF, out.ptr, ws.ptr, ws.nbytes,
                      self.fx.current_stream().handle)
        return out.to_host()


@pytest.fixture(scope="module")
def dev(gpu_fx):
    return Dev(gpu_fx)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), np.asarray(b, np.float32).view(np.uint32)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def batch_forms(faces_list, verts_len):
    """0-based mesh-local face lists -> (faces_packed int64, faces_padded int32 with pad 0, faces_len)."""
    offs = np.concatenate([[0], np.cumsum(verts_len)[:-1]])
    packed = np.asfortranarray(np.concatenate([np.asarray(f, np.int64) + o for f, o in zip(faces_list, offs)], axis=1))
    flen = np.array([f.shape[1] for f in faces_list], np.int32)
    padded = np.zeros((3, int(flen.max()), len(faces_list)), np.int32, order="F")
    for i, f in enumerate(faces_list):
        padded[:, :f.shape[1], i] = f
    return packed, padded, flen


def check_raw(dev, faces_list, verts_len):
    """Every device table of a batch against the host builders on the same faces; returns the host tables."""
    lib = dev.lib
    verts_len = np.asarray(verts_len, np.int64)
    packed, padded, flen = batch_forms(faces_list, verts_len)
    V, Vmax = int(verts_len.sum()), int(verts_len.max())
    assert same(dev.pack(padded, flen, verts_len), packed.astype(np.int32))
    he, hf2e = host_edges(lib, packed, V)
    de, df2e = dev.edges(packed, V)
    assert same(de, he) and same(df2e, hf2e)
    hl, dl = host_laplacian(lib, he, V), dev.laplacian(he, V)
    assert all(same(d, h) for d, h in zip(dl, hl))
    hvf, dvf = host_vertex_faces(lib, padded, flen, Vmax), dev.vertex_faces(padded, flen, Vmax)
    assert same(dvf[0], hvf[0]) and same(dvf[1], hvf[1])
    p1 = np.asfortranarray(packed.astype(np.int32).reshape(3, -1, 1))  # the packed table: the B = 1 call over faces_packed
    hvp, dvp = host_vertex_faces(lib, p1, [packed.shape[1]], V), dev.vertex_faces(p1, [packed.shape[1]], V)
    assert same(dvp[0], hvp[0]) and same(dvp[1], hvp[1])
    return he, hf2e, hl, hvf, hvp


def check_mesh(fx, m, faces_list, verts_len):
    """The tables TriMesh.dev() hands out against the host builders on the same (0-based) faces."""
    lib = fx._lib
    verts_len = np.asarray(verts_len, np.int64)
    packed, padded, flen = batch_forms(faces_list, verts_len)
    V, Vmax = int(verts_len.sum()), int(verts_len.max())
    he, hf2e = host_edges(lib, packed, V)
    hl = host_laplacian(lib, he, V)
    hvf = host_vertex_faces(lib, padded, flen, Vmax)
    hvp = host_vertex_faces(lib, packed.astype(np.int32).reshape(3, -1, 1), [packed.shape[1]], V)
    assert same(m.dev("faces_packed").to_host(), packed.astype(np.int32))
    assert same(m.dev("edges").to_host(), he) and same(m.dev("faces_to_edges").to_host(), hf2e)
    assert all(same(m.dev(n).to_host(), h) for n, h in zip(("lap_rowptr", "lap_colind", "lap_vals"), hl))
    assert same(m.dev("vf_rowptr").to_host(), hvf[0]) and same(m.dev("vf_ent").to_host(), hvf[1])
    assert same(m.dev("vf_packed_rowptr").to_host(), hvp[0].reshape(-1)) and same(m.dev("vf_packed_ent").to_host(), hvp[1].reshape(-1))
    return he, hl


# ---- 1. the reference's own three-mesh batch ---------------------------------------------------------------------
def test_reference_three_mesh_batch(dev, known):
    """3 / 4 / 5 vertices and 1 / 2 / 7 faces (test/rep.jl).  The file records the batch's vertices and faces and no
    topology array, so the known answers here are its sizes; the tables are held to the host builders."""
    k = known["three_mesh_batch"]
    faces = [np.asfortranarray(np.array(f, np.int64).T - 1) for f in k["faces"]]  # (rows are 1-based triangles / points)
    verts = [np.asfortranarray(np.array(v, np.float32).T) for v in k["verts"]]
    vlen = [v.shape[1] for v in verts]
    assert vlen == [3, 4, 5] and [f.shape[1] for f in faces] == [1, 2, 7]
    check_raw(dev, faces, vlen)
    fx = dev.fx
    m = fx.gpu(fx.TriMesh(verts, [f + 1 for f in faces]))
    check_mesh(fx, m, faces, vlen)


# ---- 2. teapot and sphere ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def assets(gpu_fx):
    out = {}
    for name in ("teapot", "sphere"):
        v, f = gpu_fx.load_obj(os.path.join(GOLDEN, name + ".obj"))
        out[name] = (np.asfortranarray(v, dtype=np.float32), np.asfortranarray(np.asarray(f, np.int64) - 1))
    return out


@pytest.mark.parametrize("names", [("teapot",), ("sphere",), ("teapot", "sphere", "teapot")])
def test_assets_raw(dev, assets, names):
    check_raw(dev, [assets[n][1] for n in names], [assets[n][0].shape[1] for n in names])


@pytest.mark.parametrize("index_base", [0, 1])
@pytest.mark.parametrize("dtype", [np.uint32, np.int64])
def test_assets_mesh(dev, assets, index_base, dtype):
    fx, names = dev.fx, ("teapot", "sphere", "teapot")
    verts, faces = [assets[n][0] for n in names], [assets[n][1] for n in names]
    m = fx.gpu(fx.TriMesh(verts, [(f + index_base).astype(dtype) for f in faces], index_base=index_base, faces_dtype=dtype))
    check_mesh(fx, m, faces, [v.shape[1] for v in verts])


# ---- 3. degenerate inputs ------------------------------------------------------------------------------------------
def test_degenerate_faces(dev):
    """6 vertices: a face (a, a, b) (a self-edge, the summed duplicate on the diagonal, nnz two short of 2E + V), the same
    face twice, a face repeated with its corners rotated, and vertex 5 isolated (its row is the diagonal alone)."""
    faces = np.asfortranarray(np.array([[0, 1, 2], [0, 1, 2], [1, 2, 0], [3, 3, 4], [2, 3, 4]], np.int64).T)
    he, _, (rowptr, colind, vals), _, _ = check_raw(dev, [faces], [6])
    E = he.shape[0]
    assert [3, 3] in he.tolist() and len(colind) == 2 * E + 6 - 2
    assert rowptr[6] - rowptr[5] == 1 and colind[rowptr[5]] == 5 and vals[rowptr[5]] == np.float32(-1)
    k = rowptr[3] + list(colind[rowptr[3]:rowptr[4]]).index(3)
    deg3 = 2 + 2  # the self-edge counts both ends; (2,3) and (3,4)
    inv = np.float32(1.0 / deg3)
    assert vals[k] == np.float32(np.float32(inv + inv) + np.float32(-1))


# ---- 4. high valence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfaces", [5000, 70000])
@pytest.mark.parametrize("hub_last", [False, True])
def test_fan(dev, nfaces, hub_last):
    """A fan around one hub: the hub's edge bucket and face list hold every face (70 000: more than a block's LDS)."""
    V = nfaces + 2
    rim = np.arange(nfaces, dtype=np.int64)
    hub = V - 1 if hub_last else 0
    off = 0 if hub_last else 1
    faces = np.asfortranarray(np.stack([np.full(nfaces, hub), rim + off, rim + off + 1]))
    check_raw(dev, [faces], [V])


# ---- 5. grid striding ----------------------------------------------------------------------------------------------
def shuffled_sheet(nx, ny, seed):
    _, f = sheet(nx, ny)
    return np.asfortranarray(f[:, np.random.default_rng(seed).permutation(f.shape[1])])


@pytest.mark.parametrize("nx,ny", [(6, 5), (400, 400)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_sheet(dev, nx, ny, shuffle):
    f = shuffled_sheet(nx, ny, 11) if shuffle else sheet(nx, ny)[1]
    check_raw(dev, [f], [(nx + 1) * (ny + 1)])


def test_sheet_padded_batch(dev):
    """Two sheets of unequal size in one padded batch: padding faces and unequal V in the padded tables."""
    a, b = shuffled_sheet(60, 50, 3), sheet(6, 5)[1]
    check_raw(dev, [a, b, a], [61 * 51, 7 * 6, 61 * 51])


def test_more_meshes_than_one_round_of_the_offset_scan(dev):
    """B = 1025 ragged meshes of one to three faces over three to five vertices: the face and vertex offsets of faces_packed take
    two rounds of the one-block scan's 1024 (td_pack_offsets_kernel), so mesh 1024 is placed by the first round's totals."""
    rng = np.random.default_rng(1025)
    vlen = rng.integers(3, 6, 1025)
    faces = [np.asfortranarray(rng.integers(0, v, (3, int(rng.integers(1, 4)))).astype(np.int64)) for v in vlen]
    assert {f.shape[1] for f in faces} == {1, 2, 3}
    check_raw(dev, faces, vlen)


# ---- 6. device-born meshes -------------------------------------------------------------------------------------------
def test_device_born_mesh_never_builds_host_faces(dev):
    fx = dev.fx
    from flux3d_jl_amd import conversions
    from flux3d_jl_amd.sampling import sampling_adjoint_is_ordered
    rng = np.random.default_rng(5)
    vox = np.asfortranarray(rng.uniform(0, 1, (8, 8, 8, 3)).astype(np.float32))
    vox[..., 1] *= 0.8
    vox[..., 2] *= 0.65
    m = fx.trimesh_from_voxels(fx.gpu(vox), 0.5, "Exact")
    K = (m._faces_len // 12).astype(int)
    assert len(set(K.tolist())) == 3
    calls = []
    builder = m._faces_builder
    m._faces_builder = lambda: calls.append(1) or builder()

    n = 500
    assert sampling_adjoint_is_ordered(m, n)
    fi = fx.DeviceArray.from_host(np.asfortranarray(np.stack([rng.integers(0, 12 * k, n) for k in K], 1).astype(np.int32)))
    r1, r2 = (fx.DeviceArray.from_host(np.asfortranarray(rng.uniform(0, 1, (n, 3)).astype(np.float32))) for _ in range(2))
    gout = np.asfortranarray(rng.standard_normal((3, n, 3)).astype(np.float32))

    def results(mesh):
        return (np.float32(fx.laplacian_loss(mesh)), np.float32(fx.edge_loss(mesh, 0.05)),
                fx.compute_verts_normals_packed(mesh).to_host(), fx.sample_points_grad(mesh, fi, r1, r2, gout).to_host())

    got = results(m)
    assert not calls
    faces = [np.asfortranarray(conversions._cube_faces(int(k)).astype(np.int64) - 1) for k in K]
    he, hl = check_mesh(fx, m, faces, 8 * K)
    assert not calls

    # the same mesh from host lists, its topology built on the host and uploaded
    vl = fx.rep._packed_to_list(m.get_verts_packed().to_host(), m._verts_len)
    ref = fx.gpu(fx.TriMesh(vl, [conversions._cube_faces(int(k)) for k in K]))
    ref.get_edges_packed(), ref.get_laplacian_packed()
    exp = results(ref)
    for g, e in zip(got, exp):
        assert same(np.atleast_1d(g), np.atleast_1d(e))

    # the host getters download the device result in the reference's type and numbering
    e, (rowptr, colind, vals) = m.get_edges_packed(), m.get_laplacian_packed()
    assert e.dtype == m.R == np.uint32 and np.array_equal(e, he.astype(np.int64) + 1) and e.flags.f_contiguous
    assert same(rowptr, hl[0]) and same(colind, hl[1]) and same(vals, hl[2])
    assert same(m.get_edges_packed(), ref.get_edges_packed()) and same(m.get_faces_to_edges_packed(), ref.get_faces_to_edges_packed())
    assert not calls


# ---- 7. reproducibility --------------------------------------------------------------------------------------------
def test_two_builds_same_bytes(dev):
    fx = dev.fx
    v, _ = sheet(400, 400)
    f = shuffled_sheet(400, 400, 11) + 1
    names = ("edges", "faces_to_edges", "lap_rowptr", "lap_colind", "lap_vals", "vf_rowptr", "vf_ent", "vf_packed_rowptr", "vf_packed_ent")
    tables = []
    for _ in range(2):
        m = fx.gpu(fx.TriMesh([v], [f]))
        tables.append([m.dev(n).to_host().tobytes() for n in names])
    assert tables[0] == tables[1]


# ---- 8. bad ids ----------------------------------------------------------------------------------------------------
def test_bad_ids_are_counted_not_dereferenced(dev):
    fx, V = dev.fx, 6
    faces = np.asfortranarray(np.array([[0, 1, 2], [2, 3, V], [3, 4, 5], [-1, 4, 5]], np.int32).T)
    _, _, nbad = dev.edges(faces, V, want_bad=True)
    assert nbad == 2
    # the Python path: a device-born mesh whose device faces carry the same ids
    verts = fx.DeviceArray.from_host(np.zeros((3, V), np.float32, order="F"))
    m = fx.TriMesh._from_device(verts, [V], [4], lambda: [])
    m._topo_dev["faces_padded"] = fx.DeviceArray.from_host(faces.reshape(3, 4, 1))
    m._topo_dev["faces_len"] = fx.DeviceArray.from_host(np.array([4], np.int32))
    m._topo_dev["nverts"] = fx.DeviceArray.from_host(np.array([V], np.int32))
    with pytest.raises(ValueError, match="2 vertex ids"):
        m.dev("edges")
    with pytest.raises(ValueError, match="2 vertex ids"):
        m.dev("vf_rowptr")
    # no later launch fails
    check_raw(dev, [np.asfortranarray(np.array([[0, 1, 2], [2, 3, 4]], np.int64).T)], [V])
    fx.synchronize()


# ---- 9. limits -----------------------------------------------------------------------------------------------------
def test_limits_are_error_statuses(dev):
    fx, lib = dev.fx, dev.lib.load()
    d = fx.DeviceArray.zeros((64,), np.int64)  # stands in for every pointer: the sizes are refused before any launch
    F = (1 << 31) // 3 + 1
    p, n = d.ptr, C.c_size_t(0)
    assert lib.fx3d_edges_dev_workspace_bytes(F, 10, C.byref(n)) != 0
    assert lib.fx3d_edges_dev_count(p, F, 10, p, p, p, d.nbytes, None) != 0
    assert lib.fx3d_edges_dev_emit(p, F, 10, 5, p, p, p, d.nbytes, None) != 0
    assert lib.fx3d_laplacian_dev_csr(p, 1 << 30, 10, p, p, p, p, p, p, d.nbytes, None) != 0
    assert lib.fx3d_vertex_faces_dev_workspace_bytes(10, 1 << 29, 1, C.byref(n)) != 0
    assert lib.fx3d_vertex_faces_dev(p, p, 10, 1 << 29, 1, p, p, p, p, d.nbytes, None) != 0
    assert lib.fx3d_faces_padded_to_packed_dev(p, p, p, 1 << 29, 1, 5, p, p, d.nbytes, None) != 0
    for F0, V0 in ((0, 5), (5, 0)):
        assert lib.fx3d_edges_dev_count(p, F0, V0, p, p, p, d.nbytes, None) != 0
    assert lib.fx3d_laplacian_dev_csr(p, 3, 0, p, p, p, p, p, p, d.nbytes, None) != 0
    fx.synchronize()
    assert np.all(d.to_host() == 0)
