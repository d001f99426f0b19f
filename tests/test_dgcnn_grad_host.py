"""The DGCNN adjoint, the part that needs no GPU: the host restatement tests/dgcnn_grad_ref.py is the gradient of the whole
network (each of the four families over all 8 parameterised layers, and X, held against torch float64 autograd with the
neighbours given and constant), its EdgeConv slices are tests/edgeconv_pgrad_ref.py's bit for bit, and every refusal of
fx3d_dgcnn_grad_workspace_bytes, fx3d_dgcnn_grad and DGCNN.grad / flat_grad / crossentropy_grad comes before any device work."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dgcnn_grad_ref as gref
import dgcnn_ref
import edgeconv_pgrad_ref as pref

F32 = np.float32
INVALID = -1   # FX3D_ERR_INVALID_ARG (include/flux3d_hip.h)
HERE = os.path.dirname(os.path.abspath(__file__))
N, B, K, NC = 65, 2, 3, 10
# X is np.random.default_rng(SEED_X).standard_normal, glogits SEED_G's; the parameters dgcnn_ref.random_params(10, seed=3)
SEED_X, SEED_G = 410, 411


def _lib():
    from flux3d_jl_amd import _lib
    return _lib


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


@pytest.fixture(scope="module")
def case():
    """One draw, one forward and one restatement for the tests of this module; nothing here changes them."""
    P = dgcnn_ref.random_params(NC, seed=3)
    X = np.asfortranarray(np.random.default_rng(SEED_X).standard_normal((3, N, B)).astype(F32))
    glogits = np.asfortranarray(np.random.default_rng(SEED_G).standard_normal((NC, B)).astype(F32))
    fwd = dgcnn_ref.forward(X, P, K)
    dgcnn_ref.check_draw(fwd)
    G, gx, gx2, gx1 = gref.grad(X, P, K, glogits, fwd)
    return dict(P=P, X=X, glogits=glogits, fwd=fwd, G=G, gx=gx, gx2=gx2, gx1=gx1)


def test_the_draw_means_something(case):
    """Most pooled channels are positive, no positive maximum is tied, the winners are spread over the cloud, and the
    restatement's gradients are finite with most of dW non-zero."""
    fwd, P = case["fwd"], case["P"]
    a3 = gref.conv3(P, fwd["x2"])
    assert np.array_equal(_bits(gref.pool(a3)), _bits(fwd["pooled"]))
    pooled = fwd["pooled"].T[:, None, :]
    share = np.count_nonzero(fwd["pooled"] > 0) / fwd["pooled"].size
    ties = int(np.count_nonzero((((a3 == pooled) & (pooled > 0)).sum(axis=1)) > 1))
    nstar = gref.winners(a3, fwd["pooled"])
    distinct = [len(set(nstar[b][nstar[b] >= 0].tolist())) for b in range(B)]
    print(f"share of pooled > 0: {share:.2f}; tied positive maxima: {ties}; distinct winning points per cloud: {distinct}")
    assert share > 0.5 and ties == 0 and min(distinct) > N // 2
    for fam in gref.FAMILIES:
        assert np.all(np.isfinite(gref.family(case["G"], fam))), fam
    dW = gref.family(case["G"], "dW")
    assert 2 * np.count_nonzero(dW) >= dW.size and np.all(np.isfinite(case["gx"])) and np.count_nonzero(case["gx"]) > 0


def test_the_restatement_is_the_gradient(case, tmp_path):
    """N = npoints = 65, B = 2, K = 3, num_classes = 10 against torch float64 autograd of the whole network, with the
    restatement's neighbour lists.  The siblings' bound (test_edgeconv_pgrad_host.py), per family over all 8 parameterised
    layers and for X on its own: the restatement and a float32 autograd are both Float32 sums in some order, so the
    restatement's error against float64, relative to the family's largest float64 magnitude, may be at most 8 x
    torch-float32's."""
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    np.savez(src, X=case["X"], glogits=case["glogits"], idx1=case["fwd"]["idx1"], idx2=case["fwd"]["idx2"], **case["P"])
    subprocess.run([sys.executable, os.path.join(HERE, "dgcnn_grad_torch_eval.py"), src, dst], check=True, timeout=600)
    t = np.load(dst)
    G = case["G"]
    groups = {fam: [n for n in G if n.endswith(suffix)] for fam, suffix in gref.FAMILIES.items()}
    assert [len(v) for v in groups.values()] == [9, 9, 8, 8]   # 8 layers with BatchNorm, and fc6
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


def test_the_stages_are_the_edgeconv_adjoints_and_the_statistics_get_zeros(case):
    """The ec2 / ec1 slices and gx1 / gx equal edgeconv_pgrad_ref.grad fed with the restatement's gx2 / gx1, bit for bit; a
    restatement that computes the forward itself gives the same bits; mu and sigma2 get zeros; names and shapes are the
    parameters'."""
    P, X, fwd, G = case["P"], case["X"], case["fwd"], case["G"]
    shapes = dgcnn_ref.param_shapes(NC)
    assert list(G) == list(shapes) and all(G[n].shape == s and G[n].dtype == F32 for n, s in shapes.items())
    assert gref.flat(G).size == sum(int(np.prod(s)) for s in shapes.values())
    G2, g1 = pref.grad(fwd["x1"], gref.stage_params(P, "ec2"), gref.L2, K, case["gx2"], fwd["idx2"], fwd["x2"])
    G1, gx = pref.grad(X, gref.stage_params(P, "ec1"), gref.L1, K, case["gx1"], fwd["idx1"], fwd["x1"])
    assert np.array_equal(_bits(g1), _bits(case["gx1"])) and np.array_equal(_bits(gx), _bits(case["gx"]))
    for pre, Gs in (("ec1.", G1), ("ec2.", G2)):
        assert all(np.array_equal(_bits(G[pre + n]), _bits(v)) for n, v in Gs.items()), pre
    stats = [n for n in G if n.endswith((".mu", ".sigma2"))]
    assert len(stats) == 16 and all(not _bits(G[n]).any() for n in stats)
    again, gx_, gx2_, gx1_ = gref.grad(X, P, K, case["glogits"])  # the forward computed by the restatement itself
    assert all(np.array_equal(_bits(G[n]), _bits(again[n])) for n in G)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in ((gx_, case["gx"]), (gx2_, case["gx2"]), (gx1_, case["gx1"])))


def test_the_gather_is_the_dense_product_for_finite_weights(case):
    """gx2 as the header's gather equals, bit for bit, the dense chain over ALL 1024 channels with dz3 = (+0 gamma) / sd away from
    the winning point: the terms left out are zeros times finite weights, which leave a chain that began at +0 as it is."""
    from pointnet_ref import contract
    P, fwd = case["P"], case["fwd"]
    kept = {}
    _, gx2, nstar = gref.tail(P, fwd["x2"], fwd["pooled"], case["glogits"], kept)
    assert np.array_equal(_bits(gx2), _bits(case["gx2"]))
    W3 = np.asarray(P["conv3.conv.weight"], F32)[0]
    zero = ((np.zeros(1024, F32) * P["conv3.bn.gamma"]) / np.sqrt(P["conv3.bn.sigma2"] + F32(1e-5))).astype(F32)
    dense = np.broadcast_to(zero, (B, N, 1024)).copy()
    for b in range(B):
        c = np.flatnonzero(nstar[b] >= 0)
        dense[b, nstar[b, c], c] = kept["dz3"][b, c]
    full = contract(dense, np.ascontiguousarray(W3.T))  # (B, N, 256): the chain over all c
    assert np.array_equal(_bits(np.transpose(full, (2, 1, 0))), _bits(gx2))


def test_both_symbols_are_exported(fx):
    lib_mod = _lib()
    lib = lib_mod.load()
    for name in ("fx3d_dgcnn_grad_workspace_bytes", "fx3d_dgcnn_grad"):
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES, name
    assert callable(fx.DGCNN.grad) and callable(fx.DGCNN.flat_grad) and callable(fx.DGCNN.crossentropy_grad)


def test_the_c_entry_points_refuse_before_any_device_work(fx):
    """The refusals of fx3d_dgcnn_forward, code for code, and the five-or-none rule.  No call here has arguments that would pass
    the check: the dummy pointers are never dereferenced."""
    lib_mod = _lib()
    lib = lib_mod.load()
    dummy = ctypes.c_void_p(4096)
    nb = ctypes.c_size_t(0)
    FIVE = ("idx1", "x1", "idx2", "x2", "pooled")

    def grad(nc=NC, K_=K, N_=N, B_=B, params=dummy, x=dummy, glogits=dummy, gparams=dummy, gx=None, gx2=None, gx1=None, ws=dummy,
             ws_bytes=1 << 40, **five):
        return lib.fx3d_dgcnn_grad(params, nc, K_, x, N_, B_, *(five.get(k) for k in FIVE), glogits, gparams, gx, gx2, gx1, ws,
                                   ws_bytes, None)

    def says(*words):
        msg = lib_mod.last_error()
        return all(w in msg for w in words)

    def size(N_=N, B_=B, K_=K, nc=NC, out=ctypes.byref(nb)):
        return lib.fx3d_dgcnn_grad_workspace_bytes(N_, B_, K_, nc, out)

    # NULL pointers (the intermediates, gx, gx2 and gx1 are optional)
    assert size(out=None) == INVALID and says("NULL")
    for k in ("params", "x", "glogits", "gparams", "ws"):
        assert grad(**{k: None}) == INVALID and says("NULL"), k
    # some but not all of the five intermediates: each one missing, and one alone
    for k in FIVE:
        assert grad(**{j: dummy for j in FIVE if j != k}) == INVALID and says("all five or none", "4"), k
        assert grad(**{k: dummy}) == INVALID and says("all five or none", "1"), k
    # num_classes, K, N, B
    for kw, words in ((dict(nc=0), ("num_classes", "0")), (dict(nc=(1 << 20) + 1), ("num_classes", "1048577")),
                      (dict(K_=0), ("K", "0")), (dict(K_=-2), ("K", "-2")), (dict(K_=65), ("K + 1", "66")),
                      (dict(N_=36865), ("36865",)), (dict(N_=0), ("N=0",)), (dict(B_=0), ("B=0",)),
                      (dict(B_=65536, N_=8), ("65536",)), (dict(N_=36864, B_=65535, K_=1), ("2^31",))):
        assert grad(**kw) == INVALID and says("fx3d_dgcnn_grad", *words), kw
        assert grad(**kw, **{j: dummy for j in FIVE}) == INVALID and says(*words), kw
        assert size(**kw) == INVALID and says("fx3d_dgcnn_grad_workspace_bytes", *words), kw
    # the workspace: it holds the forward's and both stages' adjoint workspaces' largest besides its own arrays
    fwd, ec = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert size() == 0 and nb.value % 256 == 0
    assert lib.fx3d_dgcnn_workspace_bytes(N, B, K, NC, ctypes.byref(fwd)) == 0
    la = (ctypes.c_int32 * 3)(64, 128, 256)
    assert lib.fx3d_edgeconv_grad_workspace_bytes(la, 3, K, N, B, ctypes.byref(ec)) == 0
    own = 4 * N * B * (2 * K + 2 * (64 + 256)) + 4 * B * (1024 * (4 + 2) + 2 * (512 + 256) + NC)   # 2 tiles at N = 65
    assert nb.value >= max(fwd.value, ec.value) + own
    assert grad(ws_bytes=nb.value - 1) == INVALID and says("workspace", str(nb.value))
    assert grad(ws_bytes=nb.value - 1, **{j: dummy for j in FIVE}) == INVALID and says("workspace", str(nb.value))
    assert grad(ws=ctypes.c_void_p(4096 + 16)) == INVALID and says("aligned")


def test_python_errors_before_any_launch(fx):
    m = fx.DGCNN(NC, K, N)
    X = np.zeros((3, N, B), F32)
    g = np.zeros((NC, B), F32)
    i32 = np.int32
    fwd = {"idx1": np.zeros((K, N, B), i32), "x1": np.zeros((64, N, B), F32), "idx2": np.zeros((K, N, B), i32),
           "x2": np.zeros((256, N, B), F32), "pooled": np.zeros((1024, B), F32)}
    for call in (m.grad, m.flat_grad):
        with pytest.raises(ValueError, match="npoints"):
            call(np.zeros((3, N - 1, B), F32), g)            # N != npoints
        with pytest.raises(ValueError, match="3 channels"):
            call(np.zeros((4, N, B), F32), g)
        for bad in (g[:NC - 1], g[:, :1], np.zeros((NC, B, 1), F32), np.zeros((B, NC), F32)):
            with pytest.raises(ValueError, match="glogits must be"):
                call(X, bad)
        with pytest.raises(TypeError, match="glogits"):
            call(X, g.astype(np.complex64))
        for k in fwd:
            with pytest.raises(ValueError, match=k):
                call(X, g, fwd={j: v for j, v in fwd.items() if j != k})   # fwd missing a key
        with pytest.raises(ValueError, match="x2'. must be"):
            call(X, g, fwd=dict(fwd, x2=np.zeros((255, N, B), F32)))
        with pytest.raises(ValueError, match="pooled'. must be"):
            call(X, g, fwd=dict(fwd, pooled=np.zeros((1024, B + 1), F32)))
        with pytest.raises(TypeError, match="integers"):
            call(X, g, fwd=dict(fwd, idx2=np.zeros((K, N, B), F32)))
        lists = np.zeros((K, N, B), i32)
        lists[1, 7, 1] = N
        with pytest.raises(ValueError, match="0-based"):
            call(X, g, fwd=dict(fwd, idx1=lists), input_grad=False)
    # crossentropy_grad: the labels are checked on the host, before the forward
    for bad in ([0, NC], [-1, 0]):
        with pytest.raises(ValueError, match=r"labels must be in \[0, 10\)"):
            m.crossentropy_grad(X, np.array(bad))
    with pytest.raises(ValueError, match="labels must be"):
        m.crossentropy_grad(X, np.array([0, 1, 2]))
    with pytest.raises(TypeError, match="integers"):
        m.crossentropy_grad(X, np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="npoints"):
        m.crossentropy_grad(np.zeros((3, N + 1, B), F32), np.array([0, 1]))
