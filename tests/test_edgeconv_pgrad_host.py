"""The EdgeConv parameter adjoint, the part that needs no GPU: the host restatement tests/edgeconv_pgrad_ref.py is the gradient
(each of the four families held against torch float64 autograd with the neighbours given and constant, for one layer and for
DGCNN's two-stage composition), its gx is the input adjoint's restatement bit for bit, and every refusal of
fx3d_edgeconv_grad_workspace_bytes, fx3d_edgeconv_grad and EdgeConv.grad comes before any device work."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dgcnn_ref
import edgeconv_bwd_ref as bref
import edgeconv_pgrad_ref as pref
import edgeconv_ref as ref

F32 = np.float32
INVALID, UNSUPPORTED = -1, -5   # FX3D_ERR_INVALID_ARG, FX3D_ERR_UNSUPPORTED (include/flux3d_hip.h)
HERE = os.path.dirname(os.path.abspath(__file__))


def _arr(layers):
    return (ctypes.c_int32 * len(layers))(*layers), len(layers)


def _lib():
    from flux3d_jl_amd import _lib
    return _lib


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _against_torch(tmp_path, X, gout, stages, mine):
    """stages: a list of (P, layers, idx); mine: the restatement's grads, one dict per stage.  The siblings' bound
    (test_edgeconv_bwd_host.py), for each of the four families on its own: the restatement and a float32 autograd are both
    Float32 sums in some order, so the restatement's error against float64, relative to the family's largest float64
    magnitude, may be at most 8 x torch-float32's."""
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    case = {"X": X, "gout": gout, "nstages": np.array(len(stages))}
    for s, (P, layers, idx) in enumerate(stages):
        case[f"s{s}.layers"], case[f"s{s}.idx"] = np.array(layers), idx
        case.update({f"s{s}.{k}": v for k, v in P.items()})
    np.savez(src, **case)
    subprocess.run([sys.executable, os.path.join(HERE, "edgeconv_pgrad_torch_eval.py"), src, dst], check=True, timeout=600)
    t = np.load(dst)
    failed = []
    for fam, pattern in pref.FAMILIES.items():
        def gather(get):
            return np.concatenate([np.asarray(get(s, pattern.format(i)), np.float64).ravel()
                                   for s, (_, layers, _) in enumerate(stages) for i in range(1, len(layers))])
        m = gather(lambda s, n: mine[s][n])
        t64, t32 = gather(lambda s, n: t[f"g64.s{s}.{n}"]), gather(lambda s, n: t[f"g32.s{s}.{n}"])
        assert m.shape == t64.shape
        scale = float(np.max(np.abs(t64)))
        err_ref, err_t32 = float(np.max(np.abs(m - t64))) / scale, float(np.max(np.abs(t32 - t64))) / scale
        print(f"{fam}: {m.size} elements, non-zero share {np.count_nonzero(m) / m.size:.2f}; relative error of the restatement "
              f"{err_ref:.3e}, of torch float32 {err_t32:.3e}, ratio {err_ref / err_t32:.2f}")
        if not (err_t32 > 0 and err_ref <= 8 * err_t32):
            failed.append((fam, err_ref, err_t32))
    assert not failed, failed


def test_the_restatement_is_the_gradient(tmp_path):
    """[5, 33, 70], N = 65, B = 2, K = 6 against torch float64 autograd, both torch runs with the restatement's neighbours; gx is
    the input adjoint's restatement, bit for bit, and mu / sigma2 get zeros."""
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    rng = np.random.default_rng(310)
    X = rng.standard_normal((5, N, B)).astype(F32)
    gout = rng.standard_normal((70, N, B)).astype(F32)
    P = ref.random_params(layers, seed=1)
    idx, out = ref.forward(X, P, layers, K)
    ref.check_draw(out)
    G, gx = pref.grad(X, P, layers, K, gout, idx, out)
    pref.check_draw(G, layers)
    assert set(G) == set(ref.param_shapes(layers)) and all(G[n].shape == s for n, s in ref.param_shapes(layers).items())
    assert all(not _bits(G[f"bn{i}.{f}"]).any() for i in (1, 2) for f in ("mu", "sigma2"))
    assert np.array_equal(_bits(gx), _bits(bref.input_grad(X, P, layers, K, gout, idx, out)))
    again, gx2 = pref.grad(X, P, layers, K, gout)  # idx and out computed by the restatement itself
    assert all(np.array_equal(_bits(G[n]), _bits(again[n])) for n in G) and np.array_equal(_bits(gx), _bits(gx2))
    assert pref.flat(G, layers).size == sum(int(np.prod(s)) for s in ref.param_shapes(layers).values())
    _against_torch(tmp_path, X, gout, [(P, layers, idx)], [G])


def test_the_two_stage_composition_is_dgcnns_gradient(tmp_path):
    """The parameter gradients of sum(g x2) for DGCNN's two EdgeConv stages at N = 64, B = 2, K = 10 with
    dgcnn_ref.random_params: stage 2 from grad(x1, g), stage 1 from grad(X, stage 2's gx)."""
    N, B, K = 64, 2, 10
    L1, L2 = [3, 32, 64, 64], [64, 128, 256]
    P = dgcnn_ref.random_params(10, seed=3)
    P1 = {k[4:]: v for k, v in P.items() if k.startswith("ec1.")}
    P2 = {k[4:]: v for k, v in P.items() if k.startswith("ec2.")}
    rng = np.random.default_rng(311)
    X = rng.standard_normal((3, N, B)).astype(F32)
    gout = rng.standard_normal((256, N, B)).astype(F32)
    idx1, x1 = ref.forward(X, P1, L1, K)
    idx2, x2 = ref.forward(x1, P2, L2, K)
    ref.check_draw(x1)
    ref.check_draw(x2)
    G2, g1 = pref.grad(x1, P2, L2, K, gout, idx2, x2)
    G1, gx = pref.grad(X, P1, L1, K, g1, idx1, x1)
    pref.check_draw(G2, L2)
    pref.check_draw(G1, L1)
    assert np.array_equal(_bits(g1), _bits(bref.input_grad(x1, P2, L2, K, gout, idx2, x2)))
    assert np.array_equal(_bits(gx), _bits(bref.input_grad(X, P1, L1, K, g1, idx1, x1)))
    _against_torch(tmp_path, X, gout, [(P1, L1, idx1), (P2, L2, idx2)], [G1, G2])


def test_the_order_of_the_chunks():
    """Three chunks with a tail of one point: the rows of a chunk come tile by tile, k by k, in the header's permutation, and
    no row of a point beyond the cloud's last appears."""
    ks, ns, half = pref.chunk_rows(257, 2, 256)
    assert ns.tolist() == [256, 256] and ks.tolist() == [0, 1] and half.tolist() == [0, 0]
    ks, ns, half = pref.chunk_rows(257, 2, 0)
    assert ns.size == 2 * 128 and ns[:4].tolist() == [0, 4, 1, 5] and half[:4].tolist() == [0, 1, 0, 1]
    assert ns[32:36].tolist() == [0, 4, 1, 5] and ks[31] == 0 and ks[32] == 1 and ns[64] == 32
    assert sorted(ns[:32].tolist()) == list(range(32))


def test_both_symbols_are_exported(fx):
    lib_mod = _lib()
    lib = lib_mod.load()
    for name in ("fx3d_edgeconv_grad_workspace_bytes", "fx3d_edgeconv_grad"):
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES, name
    assert callable(fx.EdgeConv.grad) and callable(fx.EdgeConv.flat_grad)


def test_the_c_entry_points_refuse_before_any_device_work(fx):
    """The refusals of fx3d_edgeconv_bwd, code for code and value for value.  No call here has arguments that would pass the
    check: the dummy pointers are never dereferenced."""
    lib_mod = _lib()
    lib = lib_mod.load()
    dummy = ctypes.c_void_p(4096)
    good, ngood = _arr([5, 33, 70])
    nb = ctypes.c_size_t(0)

    def grad(layers=(5, 33, 70), nl=None, K=6, N=65, B=2, params=dummy, x=dummy, idx=None, out=None, gout=dummy, gparams=dummy,
             gx=None, ws=dummy, ws_bytes=1 << 40, arr=True):
        la, n = _arr(list(layers))
        return lib.fx3d_edgeconv_grad(params, la if arr else None, n if nl is None else nl, K, x, N, B, idx, out, gout, gparams,
                                      gx, ws, ws_bytes, None)

    def says(*words):
        msg = lib_mod.last_error()
        return all(w in msg for w in words)

    # NULL pointers (idx, out and gx are optional)
    assert lib.fx3d_edgeconv_grad_workspace_bytes(good, ngood, 6, 65, 2, None) == INVALID and says("NULL")
    assert lib.fx3d_edgeconv_grad_workspace_bytes(None, 3, 6, 65, 2, ctypes.byref(nb)) == INVALID and says("NULL")
    for k in ("params", "x", "gout", "gparams", "ws"):
        assert grad(**{k: None}) == INVALID and says("NULL"), k
    assert grad(arr=False) == INVALID and says("NULL")
    # depth: nlayers < 2 or > 5
    for layers in ([5], [5, 8, 8, 8, 8, 8]):
        la, n = _arr(layers)
        assert lib.fx3d_edgeconv_grad_workspace_bytes(la, n, 6, 65, 2, ctypes.byref(nb)) == UNSUPPORTED and says(str(n))
        assert grad(layers=layers) == UNSUPPORTED and says(str(n))
    assert grad(nl=0) == UNSUPPORTED and grad(nl=-1) == UNSUPPORTED
    # widths of 0 and 257, F = 129 and 0
    for layers, value in (([5, 0, 70], "0"), ([5, 33, 257], "257"), ([129, 8], "129"), ([0, 8], "0"), ([5, -4], "-4")):
        la, n = _arr(layers)
        assert lib.fx3d_edgeconv_grad_workspace_bytes(la, n, 6, 65, 2, ctypes.byref(nb)) == UNSUPPORTED and says(value), layers
        assert grad(layers=layers) == UNSUPPORTED and says(value), layers
    # the envelope's corners are taken: nothing inside it is refused
    for layers in ([128, 256, 256, 256, 256], [1, 1], [128, 1], [1, 256, 1, 256, 1]):
        la, n = _arr(layers)
        assert lib.fx3d_edgeconv_grad_workspace_bytes(la, n, 6, 65, 2, ctypes.byref(nb)) == 0 and nb.value > 0, layers
    # K = 0, K + 1 > N, N = 36865, B
    for kw, words in ((dict(K=0), ("K", "0")), (dict(K=-2), ("K", "-2")), (dict(K=65), ("K + 1", "66")), (dict(N=36865), ("36865",)),
                      (dict(N=0), ("N=0",)), (dict(B=0), ("B=0",)), (dict(B=65536, N=8), ("65536",)),
                      (dict(N=36864, B=65535, K=1), ("2^31",))):
        assert grad(**kw) == INVALID and says(*words), kw
        a = dict(K=6, N=65, B=2)
        a.update(kw)
        assert lib.fx3d_edgeconv_grad_workspace_bytes(good, ngood, a["K"], a["N"], a["B"], ctypes.byref(nb)) == INVALID and says(*words), kw
    # the workspace: short, misaligned; it holds the chunk partials and the sums besides the input adjoint's
    bwd = ctypes.c_size_t(0)
    count = ctypes.c_int64(0)
    assert lib.fx3d_edgeconv_param_count(good, ngood, ctypes.byref(count)) == 0
    assert lib.fx3d_edgeconv_bwd_workspace_bytes(good, ngood, 6, 65, 2, ctypes.byref(bwd)) == 0
    assert lib.fx3d_edgeconv_grad_workspace_bytes(good, ngood, 6, 65, 2, ctypes.byref(nb)) == 0
    assert nb.value >= bwd.value + 4 * count.value * (1 * 2 + 1) and nb.value % 256 == 0   # one chunk per cloud at N = 65
    assert grad(ws_bytes=nb.value - 1) == INVALID and says("workspace", str(nb.value))
    assert grad(ws=ctypes.c_void_p(4096 + 16)) == INVALID and says("aligned")


def test_python_errors_before_any_launch(fx):
    layers, K, N, B = [5, 33, 70], 6, 65, 2
    m = fx.EdgeConv(layers, K)
    X = np.zeros((5, N, B), F32)
    g = np.zeros((70, N, B), F32)
    for call in (m.grad, m.flat_grad):
        with pytest.raises(ValueError, match="5 channels"):
            call(np.zeros((3, N, B), F32), g)
        with pytest.raises(ValueError, match="K"):
            call(np.zeros((5, 6, B), F32), np.zeros((70, 6, B), F32))  # K + 1 > N
        with pytest.raises(ValueError, match="PointCloud"):
            call(fx.PointCloud(np.zeros((3, N, B), F32)), g)
        with pytest.raises(fx.Flux3DHipError, match="36865"):
            call(np.zeros((5, 36865), F32), np.zeros((70, 36865), F32))
        for bad in (g[:69], g[:, :64], g[:, :, :1], np.zeros((70, N, B, 1), F32), np.zeros((5, N, B), F32)):
            with pytest.raises(ValueError, match="gout must be"):
                call(X, bad)
            with pytest.raises(ValueError, match="out must be"):
                call(X, g, out=bad)
        with pytest.raises(TypeError, match="gout"):
            call(X, g.astype(np.complex64))
        with pytest.raises(TypeError, match="out"):
            call(X, g, out=np.zeros((70, N, B), bool))
        ok = np.zeros((K, N, B), np.int64)
        with pytest.raises(ValueError, match="idx must be"):
            call(X, g, idx=ok[:, :, :1])
        with pytest.raises(ValueError, match="idx must be"):
            call(X, g, idx=ok[:5])
        with pytest.raises(TypeError, match="integers"):
            call(X, g, idx=ok.astype(F32))
        lists = ok.copy()
        lists[2, 7, 1] = N
        with pytest.raises(ValueError, match="0-based"):
            call(X, g, idx=lists, input_grad=False)
