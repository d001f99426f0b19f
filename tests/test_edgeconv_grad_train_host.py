"""The EdgeConv training-mode adjoint, the part that needs no GPU: the host restatement tests/edgeconv_grad_train_ref.py is the
gradient of the training-mode forward (each of the four families and gx held against torch float64 autograd through
batch_norm(training=True), the neighbours given and constant, for one layer and for DGCNN's two-stage composition), the cut at
every BatchNorm is there, the running statistics do not enter, the Float64 sums run in the header's order, and every refusal of
fx3d_edgeconv_grad_train_workspace_bytes, fx3d_edgeconv_grad_train and EdgeConv.grad_train comes before any device work."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dgcnn_ref
import dgcnn_train_ref as tref
import edgeconv_grad_train_ref as gref
import edgeconv_pgrad_ref as pref
import edgeconv_ref as ref

F32, F64 = np.float32, np.float64
INVALID, UNSUPPORTED = -1, -5   # FX3D_ERR_INVALID_ARG, FX3D_ERR_UNSUPPORTED (include/flux3d_hip.h)
HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 8.0
# Every EdgeConv bias sits directly under a batch-statistic BatchNorm: its true gradient is 0, and both the restatement's db and
# torch-float32's are the rounding noise of a sum of gv whose terms cancel.  The scale cancels in the ratio of the two errors, so db
# is held to the same bound; the ratios measured on three draws of each case are in the two tests' docstrings
# (`python tests/test_edgeconv_grad_train_host.py` prints them).


def _arr(layers):
    return (ctypes.c_int32 * len(layers))(*layers), len(layers)


def _lib():
    from flux3d_jl_amd import _lib
    return _lib


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _torch_ratios(tmp, X, gout, stages, mine, gx):
    """stages: a list of (P, layers, idx); mine: the restatement's grads, one dict per stage; gx: its input gradient.  Per family
    (and "gx"): (the restatement's error against torch float64, torch float32's), both relative to the family's largest float64
    magnitude."""
    src, dst = os.path.join(str(tmp), "case.npz"), os.path.join(str(tmp), "torch.npz")
    case = {"X": X, "gout": gout, "nstages": np.array(len(stages))}
    for s, (P, layers, idx) in enumerate(stages):
        case[f"s{s}.layers"], case[f"s{s}.idx"] = np.array(layers), idx
        case.update({f"s{s}.{k}": v for k, v in P.items()})
    np.savez(src, **case)
    subprocess.run([sys.executable, os.path.join(HERE, "edgeconv_grad_train_torch_eval.py"), src, dst], check=True, timeout=600)
    t = np.load(dst)
    res = {}
    for fam, pattern in list(pref.FAMILIES.items()) + [("gx", None)]:
        def gather(get):
            if pattern is None:
                return np.asarray(get(None, "X"), F64).ravel()
            return np.concatenate([np.asarray(get(s, pattern.format(i)), F64).ravel()
                                   for s, (_, layers, _) in enumerate(stages) for i in range(1, len(layers))])
        m = gather(lambda s, n: gx if s is None else mine[s][n])
        t64 = gather(lambda s, n: t["g64.X" if s is None else f"g64.s{s}.{n}"])
        t32 = gather(lambda s, n: t["g32.X" if s is None else f"g32.s{s}.{n}"])
        assert m.shape == t64.shape
        scale = float(np.max(np.abs(t64)))
        res[fam] = (float(np.max(np.abs(m - t64))) / scale, float(np.max(np.abs(t32 - t64))) / scale, m.size)
    return res


def _hold(res):
    failed = []
    for fam, (err_ref, err_t32, size) in res.items():
        bound = BOUND
        print(f"{fam}: {size} elements; relative error of the restatement {err_ref:.3e}, of torch float32 {err_t32:.3e}, "
              f"ratio {err_ref / err_t32:.2f} (bound {bound})")
        if not (err_t32 > 0 and err_ref <= bound * err_t32):
            failed.append((fam, err_ref, err_t32))
    assert not failed, failed


def _single(seed=310):
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((5, N, B)).astype(F32)
    gout = rng.standard_normal((70, N, B)).astype(F32)
    P = ref.random_params(layers, seed=1)
    fwd = tref.edgeconv_forward_train(X, P, layers, K)
    ref.check_draw(fwd["out"])
    return layers, K, X, gout, P, fwd


def _composed(seed=311):
    N, B, K = 64, 2, 10
    L1, L2 = [3, 32, 64, 64], [64, 128, 256]
    P = dgcnn_ref.random_params(10, seed=3)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3, N, B)).astype(F32)
    gout = rng.standard_normal((256, N, B)).astype(F32)
    fwd = tref.forward_train(X, P, K)
    ref.check_draw(fwd["x1"])
    ref.check_draw(fwd["x2"])
    stages = []
    for pre, layers, idx in (("ec1.", L1, fwd["idx1"]), ("ec2.", L2, fwd["idx2"])):
        Ps = {k[4:]: v for k, v in P.items() if k.startswith(pre)}
        st = {k[4:]: v for k, v in fwd["batch_stats"].items() if k.startswith(pre)}
        stages.append((Ps, layers, idx, st))
    return K, X, gout, stages, fwd


def _composed_grads(K, X, gout, stages, fwd):
    (P1, L1, idx1, st1), (P2, L2, idx2, st2) = stages
    G2, g1 = gref.grad(fwd["x1"], P2, L2, K, gout, st2, idx2, fwd["x2"])
    G1, gx = gref.grad(X, P1, L1, K, g1, st1, idx1, fwd["x1"])
    return G1, G2, g1, gx


def test_the_restatement_is_the_gradient(tmp_path):
    """[5, 33, 70], N = 65, B = 2, K = 6 against torch float64 autograd through batch_norm(training=True), both torch runs with
    the restatement's neighbours.  The cut is there: dW differs from the test-mode adjoint's at the batch statistics, and gv of
    every layer is orthogonal to 1 and to xh over the edge rows, the projection BatchNorm's adjoint performs.  The running
    statistics do not enter: other mu / sigma2 in the parameters change no bit, and their slots are all-zero bits.
    The ratio of db's error to torch-float32's on the data seeds 310, 312, 313: 0.50, 1.00, 0.66 (dW: 1.38, 1.48, 1.82)."""
    layers, K, X, gout, P, fwd = _single()
    stats, idx, out = fwd["batch_stats"], fwd["idx"], fwd["out"]
    keep = {}
    G, gx = gref.grad(X, P, layers, K, gout, stats, idx, out, keep=keep)
    gref.check_draw(G, layers)
    assert list(G) == list(ref.param_shapes(layers)) and all(G[n].shape == s for n, s in ref.param_shapes(layers).items())
    assert all(not _bits(G[f"bn{i}.{f}"]).any() for i in (1, 2) for f in ("mu", "sigma2"))
    again, gx2 = gref.grad(X, P, layers, K, gout, stats)  # idx and out computed by the restatement itself
    assert all(np.array_equal(_bits(G[n]), _bits(again[n])) for n in G) and np.array_equal(_bits(gx), _bits(gx2))
    # the running statistics are not read
    other = dict(P)
    for i in (1, 2):
        other[f"bn{i}.mu"], other[f"bn{i}.sigma2"] = (P[f"bn{i}.mu"] + F32(3.0)).astype(F32), (P[f"bn{i}.sigma2"] * F32(7.0)).astype(F32)
    moved, gx3 = gref.grad(X, other, layers, K, gout, stats, idx, out)
    assert all(np.array_equal(_bits(G[n]), _bits(moved[n])) for n in G) and np.array_equal(_bits(gx), _bits(gx3))
    # the cut: the test-mode adjoint at the same statistics is another function
    frozen, _ = pref.grad(X, gref.at_stats(P, stats), layers, K, gout, idx, out)
    for i in (1, 2):
        assert not np.array_equal(_bits(G[f"conv{i}.weight"]), _bits(frozen[f"conv{i}.weight"])), i
    for i, (gv, xh) in enumerate(zip(keep["gv"], keep["xh"]), 1):
        gv64, xh64 = gv.astype(F64).reshape(-1, gv.shape[-1]), xh.astype(F64).reshape(-1, gv.shape[-1])
        size = np.abs(gv64).sum(axis=0)
        assert np.all(size > 0), i
        assert np.all(np.abs(gv64.sum(axis=0)) < 1e-4 * size), (i, float(np.max(np.abs(gv64.sum(axis=0)) / size)))
        assert np.all(np.abs((gv64 * xh64).sum(axis=0)) < 1e-4 * size), (i, float(np.max(np.abs((gv64 * xh64).sum(axis=0)) / size)))
    _hold(_torch_ratios(tmp_path, X, gout, [(P, layers, idx)], [G], gx))


def test_the_two_stage_composition_is_dgcnns_gradient(tmp_path):
    """The gradients of sum(g x2) for DGCNN's two EdgeConv stages in training mode at N = 64, B = 2, K = 10 with
    dgcnn_ref.random_params, idx2 and the statistics from dgcnn_train_ref.forward_train: stage 2 from grad(x1, g), stage 1 from
    grad(X, stage 2's gx).  The ratio of db's error to torch-float32's on the data seeds 311, 314, 315: 1.14, 0.97, 1.88 (dW: below 0.01, 1.68, 1.93)."""
    K, X, gout, stages, fwd = _composed()
    G1, G2, g1, gx = _composed_grads(K, X, gout, stages, fwd)
    gref.check_draw(G2, stages[1][1])
    gref.check_draw(G1, stages[0][1])
    _hold(_torch_ratios(tmp_path, X, gout, [s[:3] for s in stages], [G1, G2], gx))


def test_the_order_of_the_half_tile_rows():
    """N = 65: a third half-tile of one point.  Chain h of a half-tile holds the points whose position has bit 2 equal to h,
    k by k, in ascending position, and no row of a point beyond the cloud's last appears."""
    (k0, n0), (k1, n1) = gref.half_rows(65, 2, 0)
    assert n0[:16].tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27] and k0[:16].tolist() == [0] * 16
    assert n1[:16].tolist() == [4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 28, 29, 30, 31]
    assert n0[16:].tolist() == n0[:16].tolist() and k0[16:].tolist() == [1] * 16 and n0.size == n1.size == 32
    (k0, n0), (k1, n1) = gref.half_rows(65, 2, 1)
    assert n0[:4].tolist() == [32, 33, 34, 35] and n1[:4].tolist() == [36, 37, 38, 39]
    (k0, n0), (k1, n1) = gref.half_rows(65, 2, 2)
    assert n0.tolist() == [64, 64] and k0.tolist() == [0, 1] and n1.size == 0 and k1.size == 0
    # half_sums adds exactly these rows in exactly this order
    rng = np.random.default_rng(5)
    gy = (rng.standard_normal((2, 2, 65, 3)) * 10.0 ** rng.integers(-3, 4, (2, 2, 65, 3))).astype(F32)
    xh = rng.standard_normal((2, 2, 65, 3)).astype(F32)
    s1, s2 = gref.half_sums(gy, xh)
    t1, t2 = np.zeros((2, 3, 3), F64), np.zeros((2, 3, 3), F64)
    for b in range(2):
        for t in range(3):
            c1, c2 = [], []
            for ks, ns in gref.half_rows(65, 2, t):
                a1, a2 = np.zeros(3, F64), np.zeros(3, F64)
                for k, n in zip(ks, ns):
                    a1 = a1 + gy[b, k, n].astype(F64)
                    a2 = a2 + gy[b, k, n].astype(F64) * xh[b, k, n].astype(F64)
                c1.append(a1)
                c2.append(a2)
            t1[b, t], t2[b, t] = c1[0] + c1[1], c2[0] + c2[1]
    assert np.array_equal(s1.view(np.uint64), tref.fold_tiles(t1).view(np.uint64))
    assert np.array_equal(s2.view(np.uint64), tref.fold_tiles(t2).view(np.uint64))


def test_the_fold_past_its_groups():
    """34 half-tiles of one cloud (N = 1057) and 17 of each of three: the half-tile values t = half-tile + nhalf b go into
    FX3D_POINTNET_STAT_GROUPS = 32 interleaved chains, t = 32 and 33 onto chains 0 and 1, and the chains are added in ascending
    order -- not one chain over t."""
    assert tref.GROUPS == 32
    rng = np.random.default_rng(6)
    for B, N in ((1, 1057), (3, 17 * 32 - 5)):
        nh = (N + 31) // 32
        gy = (rng.standard_normal((B, 1, N, 2)) * 10.0 ** rng.integers(-4, 5, (B, 1, N, 2))).astype(F32)
        xh = rng.standard_normal((B, 1, N, 2)).astype(F32)
        s1, s2 = gref.half_sums(gy, xh)
        vals = np.zeros((B * nh, 2, 2), F64)
        for b in range(B):
            for t in range(nh):
                for h, (ks, ns) in enumerate(gref.half_rows(N, 1, t)):
                    a = np.zeros((2, 2), F64)
                    for k, n in zip(ks, ns):
                        g = gy[b, k, n].astype(F64)
                        a = a + np.stack([g, g * xh[b, k, n].astype(F64)])
                    vals[t + nh * b] = a if h == 0 else vals[t + nh * b] + a
        chains = np.zeros((32, 2, 2), F64)
        for t in range(B * nh):
            chains[t % 32] = chains[t % 32] + vals[t]
        total = np.zeros((2, 2), F64)
        for g in range(32):
            total = total + chains[g]
        assert np.array_equal(s1.view(np.uint64), total[0].view(np.uint64)) and np.array_equal(s2.view(np.uint64), total[1].view(np.uint64))
        one = np.zeros((2, 2), F64)
        for t in range(B * nh):
            one = one + vals[t]
        assert not np.array_equal(total.view(np.uint64), one.view(np.uint64))  # (the draw tells the two orders apart)


def test_both_symbols_are_exported(fx):
    lib_mod = _lib()
    lib = lib_mod.load()
    for name in ("fx3d_edgeconv_grad_train_workspace_bytes", "fx3d_edgeconv_grad_train"):
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES, name
    assert len(lib_mod.SIGNATURES["fx3d_edgeconv_grad_train"]) == 16 and len(lib_mod.SIGNATURES["fx3d_edgeconv_grad_train_workspace_bytes"]) == 6
    assert callable(fx.EdgeConv.grad_train) and callable(fx.EdgeConv.flat_grad_train)


def test_the_c_entry_points_refuse_before_any_device_work(fx):
    """The refusals of fx3d_edgeconv_grad, code for code and value for value, with batch_stats among the required pointers.  No
    call here has arguments that would pass the check: the dummy pointers are never dereferenced."""
    lib_mod = _lib()
    lib = lib_mod.load()
    dummy = ctypes.c_void_p(4096)
    good, ngood = _arr([5, 33, 70])
    nb = ctypes.c_size_t(0)
    size = lib.fx3d_edgeconv_grad_train_workspace_bytes

    def grad(layers=(5, 33, 70), nl=None, K=6, N=65, B=2, params=dummy, x=dummy, idx=None, out=None, stats=dummy, gout=dummy,
             gparams=dummy, gx=None, ws=dummy, ws_bytes=1 << 40, arr=True):
        la, n = _arr(list(layers))
        return lib.fx3d_edgeconv_grad_train(params, la if arr else None, n if nl is None else nl, K, x, N, B, idx, out, stats, gout,
                                            gparams, gx, ws, ws_bytes, None)

    def says(*words):
        msg = lib_mod.last_error()
        return all(w in msg for w in words)

    # NULL pointers (idx, out and gx are optional)
    assert size(good, ngood, 6, 65, 2, None) == INVALID and says("NULL")
    assert size(None, 3, 6, 65, 2, ctypes.byref(nb)) == INVALID and says("NULL")
    for k in ("params", "x", "stats", "gout", "gparams", "ws"):
        assert grad(**{k: None}) == INVALID and says("fx3d_edgeconv_grad_train", "batch_stats", "NULL"), k
    assert grad(arr=False) == INVALID and says("NULL")
    # depth: nlayers < 2 or > 5
    for layers in ([5], [5, 8, 8, 8, 8, 8]):
        la, n = _arr(layers)
        assert size(la, n, 6, 65, 2, ctypes.byref(nb)) == UNSUPPORTED and says(str(n))
        assert grad(layers=layers) == UNSUPPORTED and says(str(n))
    assert grad(nl=0) == UNSUPPORTED and grad(nl=-1) == UNSUPPORTED
    # widths of 0 and 257, F = 129 and 0
    for layers, value in (([5, 0, 70], "0"), ([5, 33, 257], "257"), ([129, 8], "129"), ([0, 8], "0"), ([5, -4], "-4")):
        la, n = _arr(layers)
        assert size(la, n, 6, 65, 2, ctypes.byref(nb)) == UNSUPPORTED and says(value), layers
        assert grad(layers=layers) == UNSUPPORTED and says(value), layers
    # the envelope's corners are taken: nothing inside it is refused; B = 1 is allowed
    for layers in ([128, 256, 256, 256, 256], [1, 1], [128, 1], [1, 256, 1, 256, 1]):
        la, n = _arr(layers)
        assert size(la, n, 6, 65, 2, ctypes.byref(nb)) == 0 and nb.value > 0, layers
        assert size(la, n, 6, 65, 1, ctypes.byref(nb)) == 0 and nb.value > 0, layers
    # K = 0, K + 1 > N, N = 36865, B
    for kw, words in ((dict(K=0), ("K", "0")), (dict(K=-2), ("K", "-2")), (dict(K=65), ("K + 1", "66")), (dict(N=36865), ("36865",)),
                      (dict(N=0), ("N=0",)), (dict(B=0), ("B=0",)), (dict(B=65536, N=8), ("65536",)),
                      (dict(N=36864, B=65535, K=1), ("2^31",))):
        assert grad(**kw) == INVALID and says(*words), kw
        a = dict(K=6, N=65, B=2)
        a.update(kw)
        assert size(good, ngood, a["K"], a["N"], a["B"], ctypes.byref(nb)) == INVALID and says(*words), kw
    # the workspace: short, misaligned; besides the input adjoint's it holds the chunk partials, the Float64 half-tile sums of the
    # widest layer and the means
    bwd = ctypes.c_size_t(0)
    count = ctypes.c_int64(0)
    assert lib.fx3d_edgeconv_param_count(good, ngood, ctypes.byref(count)) == 0
    assert lib.fx3d_edgeconv_bwd_workspace_bytes(good, ngood, 6, 65, 2, ctypes.byref(bwd)) == 0
    assert size(good, ngood, 6, 65, 2, ctypes.byref(nb)) == 0
    assert nb.value >= bwd.value + 4 * count.value * (1 * 2) + 8 * 2 * 70 * 3 * 2 + 4 * 2 * (33 + 70) and nb.value % 256 == 0
    assert grad(ws_bytes=nb.value - 1) == INVALID and says("workspace", str(nb.value))
    assert grad(ws=ctypes.c_void_p(4096 + 16)) == INVALID and says("aligned")


def test_python_errors_before_any_launch(fx):
    layers, K, N, B = [5, 33, 70], 6, 65, 2
    m = fx.EdgeConv(layers, K)
    X = np.zeros((5, N, B), F32)
    g = np.zeros((70, N, B), F32)
    stats = {f"bn{i}.{f}": np.zeros(c, F32) for i, c in ((1, 33), (2, 70)) for f in ("mu", "sigma2")}
    good = {"out": g, "idx": np.zeros((K, N, B), np.int64), "batch_stats": stats}
    for call in (m.grad_train, m.flat_grad_train):
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
                call(X, bad, fwd=good)
            with pytest.raises(ValueError, match="out'\\] must be"):
                call(X, g, fwd=dict(good, out=bad))
        with pytest.raises(TypeError, match="gout"):
            call(X, g.astype(np.complex64), fwd=good)
        with pytest.raises(TypeError, match="forward_train"):
            call(X, g, fwd=(g, stats))
        with pytest.raises(TypeError, match="forward_train"):
            call(X, g, fwd={"out": g, "idx": good["idx"]})
        with pytest.raises(ValueError, match="2 BatchNorms"):
            call(X, g, fwd=dict(good, batch_stats={k: stats[k] for k in list(stats)[:2]}))
        with pytest.raises(ValueError, match="bn2.mu"):
            call(X, g, fwd=dict(good, batch_stats=dict(stats, **{"bn2.mu": np.zeros(69, F32)})))
        with pytest.raises(ValueError, match="bn1.sigma2"):
            call(X, g, fwd=dict(good, batch_stats=dict(stats, **{"bn1.sigma2": np.zeros(33, F64)})))
        ok = np.zeros((K, N, B), np.int64)
        with pytest.raises(ValueError, match="idx must be"):
            call(X, g, idx=ok[:, :, :1], fwd=good)
        with pytest.raises(ValueError, match="idx must be"):
            call(X, g, fwd=dict(good, idx=ok[:5]))
        with pytest.raises(TypeError, match="integers"):
            call(X, g, idx=ok.astype(F32), fwd=good)
        lists = ok.copy()
        lists[2, 7, 1] = N
        with pytest.raises(ValueError, match="0-based"):
            call(X, g, idx=lists, fwd=good, input_grad=False)


if __name__ == "__main__":   # the figures of the docstrings
    import tempfile
    for name, seeds in (("single", (310, 312, 313)), ("composed", (311, 314, 315))):
        for seed in seeds:
            with tempfile.TemporaryDirectory() as tmp:
                if name == "single":
                    layers, K, X, gout, P, fwd = _single(seed)
                    G, gx = gref.grad(X, P, layers, K, gout, fwd["batch_stats"], fwd["idx"], fwd["out"])
                    res = _torch_ratios(tmp, X, gout, [(P, layers, fwd["idx"])], [G], gx)
                else:
                    K, X, gout, stages, fwd = _composed(seed)
                    G1, G2, g1, gx = _composed_grads(K, X, gout, stages, fwd)
                    res = _torch_ratios(tmp, X, gout, [s[:3] for s in stages], [G1, G2], gx)
            print(name, seed, {fam: round(e / t, 2) for fam, (e, t, _) in res.items()}, flush=True)
