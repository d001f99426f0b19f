"""Vertex / face normals without a GPU: the host restatement (tests/normals_ref.py) against the reference's known answers, the
last-write-wins rule on a hand-built fan, the restated adjoints against float64 torch.autograd of an independent formulation,
the exported symbols, and the Python layer's argument checks (refused before any device call)."""
import json
import os

import numpy as np
import pytest

import normals_ref as ref
from conftest import GOLDEN


def _known_mesh():
    k = json.load(open(os.path.join(GOLDEN, "ref_known_answers.json")))["areas_batch"]
    verts = [np.asfortranarray(np.array(v, np.float32).T) for v in k["verts"]]
    faces = [np.asfortranarray(np.array(f, np.int64).T) for f in k["faces"]]  # 1-based, mesh-local
    return verts, faces


def _packed(verts, faces):
    offs = np.concatenate([[0], np.cumsum([v.shape[1] for v in verts])[:-1]])
    return (np.asfortranarray(np.concatenate(verts, 1)),
            np.asfortranarray(np.concatenate([f - 1 + o for f, o in zip(faces, offs)], 1)))


def _padded(packed, lens):
    out = np.zeros((3, max(lens), len(lens)), np.float32)
    cur = 0
    for b, n in enumerate(lens):
        out[:, :n, b] = packed[:, cur:cur + n]
        cur += n
    return out


@pytest.mark.parametrize("kind", ["verts", "faces"])
def test_known_answers_packed_padded_list(kind):
    """test/rep.jl:270-330: packed, padded (zeros beyond each length) and list forms at rtol = atol = 1e-4."""
    verts, faces = _known_mesh()
    v, f = _packed(verts, faces)
    ka = json.load(open(os.path.join(GOLDEN, "normals_known_answers.json")))
    want = [np.array(a, np.float32).T for a in ka[f"{kind}_normals"]]
    got = ref.verts_normals(v, f) if kind == "verts" else ref.faces_normals(v, f)
    lens = [a.shape[1] for a in want]
    assert got.shape == (3, sum(lens)) and got.dtype == np.float32
    assert np.allclose(got, np.concatenate(want, 1), rtol=ka["tol"], atol=ka["tol"])
    pad = _padded(got, lens)
    cur = 0
    for b, w in enumerate(want):
        assert np.allclose(pad[:, :lens[b], b], w, rtol=ka["tol"], atol=ka["tol"])
        assert np.all(pad[:, lens[b]:, b] == 0)
        assert np.allclose(got[:, cur:cur + lens[b]], w, rtol=ka["tol"], atol=ka["tol"])
        cur += lens[b]


def test_known_answers_signed_zeros():
    """The reference's _fnormal1 shows -0.0 for face 1: face normals keep it; vertex normals start from +0 and never do."""
    verts, faces = _known_mesh()
    v, f = _packed(verts, faces)
    fn, vn = ref.faces_normals(v, f), ref.verts_normals(v, f)
    assert np.signbit(fn[0, 0])
    assert not np.any(np.signbit(vn) & (vn == 0))
    assert np.all(vn[:, 9:12] == 0) and np.all(fn[:, 3] == 0)  # the degenerate face (three equal vertices): 0 / 1f-6


def test_last_write_wins_fan():
    """Vertex 0 is corner 1 of two faces with different normals: its normal is the LATER face's alone, not the sum."""
    v = np.asfortranarray(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32).T)
    f = np.asfortranarray(np.array([[0, 1, 2], [0, 3, 1]], np.int64).T)  # normals +z, then +y (times area)
    got = ref.verts_normals(v, f)
    assert np.array_equal(got[:, 0], np.array([0, 1, 0], np.float32))
    summed = np.array([0, 1, 1], np.float32) / np.sqrt(np.float32(2))
    assert not np.allclose(got[:, 0], summed)
    # the reversed face order makes the other face win
    got_r = ref.verts_normals(v, np.asfortranarray(f[:, ::-1]))
    assert np.array_equal(got_r[:, 0], np.array([0, 0, 1], np.float32))
    assert np.array_equal(ref.winners(f, 4)[:, 0], [1, -1, -1])


def test_vertex_faces_matches_the_library_table(fx):
    """The restatement's table is fx3d_build_vertex_faces' (entries face * 4 + corner ascending per vertex)."""
    from flux3d_jl_amd import _lib
    v, f = ref.sheet(5, 4, seed=3)
    V, F = v.shape[1], f.shape[1]
    rowptr = np.zeros(V + 1, np.int32)
    ent = np.zeros(3 * F, np.int32)
    fp = np.asfortranarray(f.astype(np.int32))
    fl = np.array([F], np.int32)
    _lib.call("fx3d_build_vertex_faces", fp.ctypes.data, fl.ctypes.data, V, F, 1, rowptr.ctypes.data, ent.ctypes.data)
    rp, ef, et = ref.vertex_faces(f, V)
    assert np.array_equal(rowptr, rp) and np.array_equal(ent, ef * 4 + et)


def _teapot_sphere(fx, name):
    m = fx.load_trimesh(os.path.join(GOLDEN, name))
    return m.get_verts_packed_host(), np.asfortranarray(m.get_faces_packed().astype(np.int64) - m.index_base)


# The independent formulation, in a child process: torch for ROCm brings HIP / RCCL libraries of its own, and the library's
# RCCL loaded in this process beside them (test_distributed_cpu.py) aborts the interpreter at exit.
_TORCH_CHILD = r"""
import sys
import numpy as np
import torch

def normals(verts, faces, which):
    # winners by np.maximum.at, gathered, crossed and normalised in float64 autograd
    V, F = verts.shape[1], faces.shape[1]
    x = torch.tensor(verts.astype(np.float64), requires_grad=True)
    p = [x[:, torch.tensor(faces[k])] for k in range(3)]
    cross = lambda r: torch.linalg.cross(p[(r + 1) % 3] - p[r], p[(r + 2) % 3] - p[r], dim=0)
    if which == "faces":
        raw = cross(0)
    else:
        raw = torch.zeros((3, V), dtype=torch.float64)
        for r in range(3):
            w = np.full(V, -1, np.int64)
            np.maximum.at(w, faces[r], np.arange(F))
            idx = torch.tensor(np.where(w >= 0, w, 0))
            raw = raw + torch.where(torch.tensor(w >= 0), cross(r)[:, idx], torch.zeros((), dtype=torch.float64))
    s = torch.sqrt((raw * raw).sum(0))
    return x, raw / torch.clamp(s, min=1e-6)

d = np.load(sys.argv[1])
out = {}
for i in range(int(d["n"])):
    for which in ("verts", "faces"):
        x, n = normals(d[f"v{i}"], d[f"f{i}"], which)
        (n * torch.tensor(d[f"g{which}{i}"].astype(np.float64))).sum().backward()
        out[f"grad{which}{i}"], out[f"fwd{which}{i}"] = x.grad.numpy(), n.detach().numpy()
np.savez(sys.argv[2], **out)
"""


def _meshes(fx):
    rng = np.random.default_rng(7)
    v, f = ref.sheet(12, 9, seed=5)
    perm = rng.permutation(f.shape[1])  # a jittered random mesh: faces shuffled, corners rotated at random
    f = f[:, perm]
    rot = rng.integers(0, 3, f.shape[1])
    f = np.asfortranarray(np.stack([f[(k + rot) % 3, np.arange(f.shape[1])] for k in range(3)]))
    return [_teapot_sphere(fx, "teapot.obj"), _teapot_sphere(fx, "sphere.obj"), (v, f)]


def test_restated_adjoints_match_float64_autograd(fx, tmp_path):
    import importlib.util
    import subprocess
    import sys
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    rng = np.random.default_rng(11)
    meshes = _meshes(fx)
    data = {"n": len(meshes)}
    for i, (v, f) in enumerate(meshes):
        data[f"v{i}"], data[f"f{i}"] = v, f
        data[f"gverts{i}"] = rng.standard_normal((3, v.shape[1])).astype(np.float32)
        data[f"gfaces{i}"] = rng.standard_normal((3, f.shape[1])).astype(np.float32)
    np.savez(tmp_path / "in.npz", **data)
    subprocess.run([sys.executable, "-c", _TORCH_CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], check=True,
                   timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1"))
    res = np.load(tmp_path / "out.npz")
    for i, (verts, faces) in enumerate(meshes):
        for which in ("verts", "faces"):
            g, want = data[f"g{which}{i}"], res[f"grad{which}{i}"]
            bwd = ref.verts_normals_bwd if which == "verts" else ref.faces_normals_bwd
            got = bwd(verts, faces, g)
            assert got.dtype == np.float32
            assert np.max(np.abs(got - want)) <= 1e-4 * np.max(np.abs(want)), (i, which)
            # the forward of the independent formulation agrees too
            fwd = ref.verts_normals(verts, faces) if which == "verts" else ref.faces_normals(verts, faces)
            assert np.allclose(fwd, res[f"fwd{which}{i}"], atol=1e-5), (i, which)
            # accumulate: the base is the first term of every vertex's sum
            base = rng.standard_normal(verts.shape).astype(np.float32)
            acc = bwd(verts, faces, g, base=base)
            assert np.allclose(acc, base + got, atol=1e-4 * np.max(np.abs(want))), (i, which)


def test_new_symbols_are_exported(fx):
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    for name in ("fx3d_normals_workspace_bytes", "fx3d_verts_normals_packed", "fx3d_verts_normals_bwd",
                 "fx3d_faces_normals_packed", "fx3d_faces_normals_bwd"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_workspace_query_and_abi_checks(fx):
    import ctypes as C
    from flux3d_jl_amd import _lib
    nb = C.c_size_t(0)
    _lib.call("fx3d_normals_workspace_bytes", 1000, 3000, C.byref(nb))
    assert nb.value >= 12 * 3000
    lib = _lib.load()
    assert lib.fx3d_normals_workspace_bytes(0, 10, C.byref(nb)) != 0
    assert lib.fx3d_verts_normals_packed(None, 10, None, 10, None, None, None, None, None) != 0
    assert lib.fx3d_faces_normals_bwd(None, 10, None, 10, None, None, None, None, 0, None, 0, None) != 0


def test_python_entry_points_reject_bad_input_before_the_device(fx):
    m = fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj"))
    V, F = int(np.sum(m._verts_len)), int(np.sum(m._faces_len))
    for fn in (fx.compute_verts_normals_packed, fx.compute_verts_normals_padded, fx.compute_verts_normals_list,
               fx.compute_faces_normals_packed, fx.compute_faces_normals_padded, fx.compute_faces_normals_list):
        with pytest.raises(TypeError):
            fn(np.zeros((3, 4), np.float32))
    with pytest.raises(TypeError):
        fx.compute_verts_normals_grad("mesh", np.zeros((3, V), np.float32))
    with pytest.raises(ValueError):
        fx.compute_verts_normals_grad(m, np.zeros((3, V + 1), np.float32))
    with pytest.raises(TypeError):
        fx.compute_verts_normals_grad(m, np.zeros((3, V), np.float64))
    with pytest.raises(ValueError):
        fx.compute_faces_normals_grad(m, np.zeros((3, V), np.float32))  # faces' gout is (3, F)
    with pytest.raises(TypeError):
        fx.compute_faces_normals_grad(m, np.zeros((3, F), np.int32))
    with pytest.raises(ValueError):
        fx.compute_faces_normals_grad(m, np.zeros((3, F), np.float32), accumulate=True)  # nothing to add into
