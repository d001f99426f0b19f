"""The PointNet adjoint, the part that needs no GPU: the host restatement tests/pointnet_grad_ref.py is the gradient of the whole
network (each of the four families over all parameterised layers, and X, held against torch float64 autograd), the equalities
the header states hold, and every refusal of fx3d_pointnet_grad_workspace_bytes, fx3d_pointnet_grad and PointNet.grad /
flat_grad / crossentropy_grad comes before any device work."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pointnet_grad_ref as gref
import pointnet_ref as ref

F32 = np.float32
INVALID = -1   # FX3D_ERR_INVALID_ARG (include/flux3d_hip.h)
HERE = os.path.dirname(os.path.abspath(__file__))
N, B, NC = 65, 2, 10
# X is np.random.default_rng(SEED_X).standard_normal, glogits SEED_G's; the parameters pointnet_ref.random_params(10, seed=10)
SEED_X, SEED_G = 710, 711


def _lib():
    from flux3d_jl_amd import _lib
    return _lib


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


@pytest.fixture(scope="module")
def case():
    """One draw and one restatement for the tests of this module; nothing here changes them."""
    P = ref.random_params(NC, seed=10)
    X = np.asfortranarray(np.random.default_rng(SEED_X).standard_normal((3, N, B)).astype(F32))
    glogits = np.asfortranarray(np.random.default_rng(SEED_G).standard_normal((NC, B)).astype(F32))
    keep = {}
    G, gx, mid = gref.grad(X, P, glogits, keep)
    return dict(P=P, X=X, glogits=glogits, G=G, gx=gx, mid=mid, **keep)


def test_the_draw_means_something(case):
    """In each of the three rounds no maximum that passes a gradient is tied and the winners are spread over more than N / 2
    points per cloud; every family is finite, most of dW is non-zero, gx, gstn and gfstn are non-zero."""
    r = case["forward"]
    # (the BatchNorm's output, the cloud's maximum, the relu's output under it or None): a maximum passes a gradient to the
    # convolution where the relu's output at the winner is positive (feat.conv2 has no relu: everywhere)
    rounds = {"stn": (r["stn_stage"]["a3"], r["stn_stage"]["max"], r["stn_stage"]["relu3"]),
              "fstn": (r["fstn_stage"]["a3"], r["fstn_stage"]["max"], r["fstn_stage"]["relu3"]),
              "feat": (r["feat_a2"], np.ascontiguousarray(r["pooled"].T), None)}
    for name, (a3, pooled, relu3) in rounds.items():
        nstar = case["nstar"][name]
        assert np.array_equal(nstar, gref.winners(a3, pooled)) and np.all(nstar >= 0)   # no NaN: every channel has a winner
        passes = np.ones(nstar.shape, bool) if relu3 is None else relu3.max(axis=1) > 0
        tied = (a3 == pooled[:, None, :]).sum(axis=1) > 1
        ties = int(np.count_nonzero(tied & passes))
        distinct = [len(set(nstar[b].tolist())) for b in range(B)]
        print(f"{name}: maxima that pass a gradient {int(passes.sum())} of {passes.size}, tied among them {ties}, tied dead channels "
              f"{int(np.count_nonzero(tied & ~passes))}; distinct winning points per cloud {distinct}")
        assert ties == 0 and 2 * passes.sum() > passes.size and min(distinct) > N // 2
    for fam in gref.FAMILIES:
        assert np.all(np.isfinite(gref.family(case["G"], fam))), fam
    dW = gref.family(case["G"], "dW")
    assert 2 * np.count_nonzero(dW) >= dW.size and np.all(np.isfinite(case["gx"])) and np.count_nonzero(case["gx"]) > 0
    assert np.count_nonzero(case["mid"]["gstn"]) > 0 and np.count_nonzero(case["mid"]["gfstn"]) > 0


def test_the_restatement_is_the_gradient(case, tmp_path):
    """Against torch float64 autograd of the whole network from X.  The siblings' bound (test_dgcnn_grad_host.py), per family
    over all parameterised layers and for X on its own: the restatement and a float32 autograd are both Float32 sums in some
    order, so the restatement's error against float64, relative to the family's largest float64 magnitude, may be at most 8 x
    torch-float32's."""
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    np.savez(src, X=case["X"], glogits=case["glogits"], **case["P"])
    subprocess.run([sys.executable, os.path.join(HERE, "pointnet_grad_torch_eval.py"), src, dst], check=True, timeout=600)
    t = np.load(dst)
    G = case["G"]
    groups = {fam: [n for n in G if n.endswith(suffix)] for fam, suffix in gref.FAMILIES.items()}
    assert [len(v) for v in groups.values()] == [18, 18, 13, 13]   # 9 convs and 9 dense layers; 13 BatchNorms
    failed = []
    for fam, names in list(groups.items()) + [("X", None)]:
        def gather(get):
            return np.concatenate([np.asarray(get(n), np.float64).ravel() for n in names])
        if names is None:
            m, t64, t32 = (np.asarray(v, np.float64).ravel() for v in (case["gx"], t["g64.X"], t["g32.X"]))
        else:
            m, t64, t32 = gather(lambda n: G[n]), gather(lambda n: t["g64." + n]), gather(lambda n: t["g32." + n])
        assert m.shape == t64.shape
        scale = float(np.max(np.abs(t64)))
        err_ref, err_t32 = float(np.max(np.abs(m - t64))) / scale, float(np.max(np.abs(t32 - t64))) / scale
        print(f"{fam}: {m.size} elements, non-zero share {np.count_nonzero(m) / m.size:.2f}; relative error of the restatement "
              f"{err_ref:.3e}, of torch float32 {err_t32:.3e}, ratio {err_ref / err_t32:.2f}")
        if not (err_t32 > 0 and err_ref <= 8 * err_t32):
            failed.append((fam, err_ref, err_t32))
    assert not failed, failed


def test_the_stated_equalities(case):
    """mu and sigma2 get zeros; names and shapes are param_shapes'; flat has param_count elements; the gradient at dense3's
    output of both transform nets is gstn / gfstn re-indexed (dense3's bias gradient is the sum over the clouds of exactly
    that)."""
    G, mid = case["G"], case["mid"]
    shapes = ref.param_shapes(NC)
    assert list(G) == list(shapes) and all(G[n].shape == s and G[n].dtype == F32 for n, s in shapes.items())
    assert gref.flat(G).size == sum(int(np.prod(s)) for s in shapes.values())
    stats = [n for n in G if n.endswith((".mu", ".sigma2"))]
    assert len(stats) == 26 and all(not _bits(G[n]).any() for n in stats)
    assert case["gx"].shape == (3, N, B) and mid["gh"].shape == (64, N, B) and mid["gxt"].shape == (3, N, B)
    for name, key, K in (("stn", "gstn", 3), ("fstn", "gfstn", 64)):
        gd3 = np.ascontiguousarray(np.transpose(mid[key], (2, 0, 1))).reshape(B, K * K)   # gd3[b, K i + j] = gT[i, j, b]
        acc = np.zeros(K * K, F32)
        for b in range(B):
            acc = (acc + gd3[b]).astype(F32)
        assert np.array_equal(_bits(G[f"{name}.dense3.bias"]), _bits(acc)), name
        assert mid[key].shape == (K, K, B)


def test_both_symbols_are_exported(fx):
    lib_mod = _lib()
    lib = lib_mod.load()
    for name in ("fx3d_pointnet_grad_workspace_bytes", "fx3d_pointnet_grad"):
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES, name
    assert callable(fx.PointNet.grad) and callable(fx.PointNet.flat_grad) and callable(fx.PointNet.crossentropy_grad)


def test_the_c_entry_points_refuse_before_any_device_work(fx):
    """The refusals of fx3d_pointnet_forward, code for code.  No call here has arguments that would pass the check: the dummy
    pointers are never dereferenced."""
    lib_mod = _lib()
    lib = lib_mod.load()
    dummy = ctypes.c_void_p(4096)
    nb = ctypes.c_size_t(0)

    def grad(nc=NC, N_=N, B_=B, params=dummy, x=dummy, glogits=dummy, gparams=dummy, gx=None, gstn=None, gfstn=None, gh=None,
             gxt=None, ws=dummy, ws_bytes=1 << 40):
        return lib.fx3d_pointnet_grad(params, nc, x, N_, B_, glogits, gparams, gx, gstn, gfstn, gh, gxt, ws, ws_bytes, None)

    def says(*words):
        msg = lib_mod.last_error()
        return all(w in msg for w in words)

    def size(N_=N, B_=B, nc=NC, out=ctypes.byref(nb)):
        return lib.fx3d_pointnet_grad_workspace_bytes(N_, B_, nc, out)

    assert size(out=None) == INVALID and says("NULL")
    for k in ("params", "x", "glogits", "gparams", "ws"):
        assert grad(**{k: None}) == INVALID and says("NULL"), k
    for kw, words in ((dict(nc=0), ("num_classes", "0")), (dict(nc=(1 << 20) + 1), ("num_classes", "1048577")),
                      (dict(N_=0), ("N=0",)), (dict(B_=0), ("B=0",)), (dict(N_=-4), ("N=-4",)),
                      (dict(B_=65536, N_=8), ("65536",)), (dict(N_=1 << 20, B_=4096), ("2^31",))):
        assert grad(**kw) == INVALID and says("fx3d_pointnet_grad", *words), kw
        assert grad(**kw, gx=dummy, gstn=dummy, gfstn=dummy, gh=dummy, gxt=dummy) == INVALID and says(*words), kw
        assert size(**kw) == INVALID and says("fx3d_pointnet_grad_workspace_bytes", *words), kw
    # the workspace holds the forward's besides the adjoint's own arrays
    fwd = ctypes.c_size_t(0)
    assert size() == 0 and nb.value % 256 == 0
    assert lib.fx3d_pointnet_workspace_bytes(N, B, NC, ctypes.byref(fwd)) == 0 and nb.value > fwd.value
    assert grad(ws_bytes=nb.value - 1) == INVALID and says("workspace", str(nb.value))
    assert grad(ws=ctypes.c_void_p(4096 + 16)) == INVALID and says("256-byte aligned")


def test_python_errors_before_any_launch(fx):
    m = fx.PointNet(NC)
    X = np.zeros((3, N, B), F32)
    g = np.zeros((NC, B), F32)
    for call in (m.grad, m.flat_grad):
        with pytest.raises(ValueError, match="3 channels"):
            call(np.zeros((4, N, B), F32), g)
        with pytest.raises(ValueError, match="at least one point"):
            call(np.zeros((3, 0, B), F32), g)
        for bad in (g[:NC - 1], g[:, :1], np.zeros((NC, B, 1), F32), np.zeros((B, NC), F32)):
            with pytest.raises(ValueError, match="glogits must be"):
                call(X, bad)
        with pytest.raises(TypeError, match="glogits"):
            call(X, g.astype(np.complex64), input_grad=False)
        with pytest.raises(ValueError, match="glogits must be"):
            call(X[:, :, 0], g, intermediates=True)   # one cloud, glogits of two
    # crossentropy_grad: the labels are checked on the host, before the forward
    for bad in ([0, NC], [-1, 0]):
        with pytest.raises(ValueError, match=r"labels must be in \[0, 10\)"):
            m.crossentropy_grad(X, np.array(bad))
    with pytest.raises(ValueError, match="labels must be"):
        m.crossentropy_grad(X, np.array([0, 1, 2]))
    with pytest.raises(TypeError, match="integers"):
        m.crossentropy_grad(X, np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="3 channels"):
        m.crossentropy_grad(np.zeros((2, N, B), F32), np.array([0, 1]))
