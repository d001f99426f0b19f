"""The DGCNN / EdgeConv training-mode forward, the part that needs no GPU: the restatement tests/dgcnn_train_ref.py is a DGCNN
(and an EdgeConv of any widths) in training mode (against torch in float64, tests/dgcnn_train_torch_eval.py), its one-pass
Float64 variance agrees with a two-pass one, and the library's host-side contract: the statistics layout and counts, the
exported symbols, the refusals before any device work, the dropout masks and the Python argument errors."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dgcnn_ref as ref
import dgcnn_train_ref as tref
import edgeconv_ref as eref

F32 = np.float32
INVALID, UNSUPPORTED = -1, -5  # FX3D_ERR_INVALID_ARG, FX3D_ERR_UNSUPPORTED
HERE = os.path.dirname(os.path.abspath(__file__))
N, B, K = 64, 4, 10
MOMENTUM = 0.1
GENERIC = [5, 33, 70]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


_CASES = {}


def _restated(key):
    """The restatement's run of a case, computed once and shared (never modified).  key: the number of classes of a DGCNN, or
    "edgeconv" for EdgeConv(GENERIC, K)."""
    if key in _CASES:
        return _CASES[key]
    if key == "edgeconv":
        X = np.random.default_rng(301).standard_normal((GENERIC[0], N, B)).astype(F32)
        P = eref.random_params(GENERIC, seed=302)
        mine = tref.edgeconv_forward_train(X, P, GENERIC, K, momentum=MOMENTUM)
        eref.check_draw(mine["out"])
        case = dict(X=X, momentum=MOMENTUM, layers=np.asarray(GENERIC), idx=mine["idx"], **P)
        order = [f"bn{i}" for i in range(1, len(GENERIC))]
        result = mine["out"]
    else:
        from flux3d_jl_amd import models
        X = np.random.default_rng(300 + key).standard_normal((3, N, B)).astype(F32)
        P = ref.random_params(key, seed=key)
        m4, m5 = models.DGCNN.dropout_masks(B, seed=key)
        mine = tref.forward_train(X, P, K, dropout=(m4, m5), momentum=MOMENTUM)
        ref.check_draw(mine)
        case = dict(X=X, momentum=MOMENTUM, idx1=mine["idx1"], idx2=mine["idx2"], dropout4=m4, dropout5=m5, **P)
        order = tref.BN_ORDER
        result = mine["logits"]
    _CASES[key] = (case, order, mine, result)
    return _CASES[key]


def _split(flat, widths):
    """A flat statistics buffer as (all means, all variances)."""
    mu, var, at = [], [], 0
    for C in widths:
        mu.append(flat[at:at + C])
        var.append(flat[at + C:at + 2 * C])
        at += 2 * C
    assert at == flat.size
    return np.concatenate(mu), np.concatenate(var)


@pytest.mark.parametrize("key", [10, 40, "edgeconv"])
def test_the_restatement_is_the_network_in_training_mode(key, tmp_path):
    """Against torch (BatchNorm with training=True over all B K N columns, the masks applied as given, the neighbours given from
    the restatement) in float64, with the bound of test_dgcnn_host.py / test_pointnet_train_host.py: the restatement's relative
    error is at most 8 x torch-float32's, for the result (the logits; the generic layer's output), the batch means, the batch
    variances and the updated running means and variances."""
    case, order, mine, result = _restated(key)
    widths = [mine["batch_stats"][bn + ".mu"].size for bn in order]
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    np.savez(src, **case)
    subprocess.run([sys.executable, os.path.join(HERE, "dgcnn_train_torch_eval.py"), src, dst], check=True, timeout=600)
    t = np.load(dst)
    assert result.shape == t["result64"].shape
    got = {"result": result}
    got["batch means"], got["batch variances"] = _split(tref.flat_stats(mine["batch_stats"], order), widths)
    got["running means"], got["running variances"] = _split(tref.flat_stats(mine["running"], order), widths)
    t64, t32 = {"result": t["result64"]}, {"result": t["result32"]}
    for d, tag in ((t64, "64"), (t32, "32")):
        d["batch means"], d["batch variances"] = _split(t["stats" + tag], widths)
        d["running means"], d["running variances"] = _split(t["running" + tag], widths)
    bad = []
    for name in got:
        scale = float(np.max(np.abs(t64[name])))
        err_ref = float(np.max(np.abs(got[name].astype(np.float64) - t64[name]))) / scale
        err_t32 = float(np.max(np.abs(t32[name].astype(np.float64) - t64[name]))) / scale
        print(f"  {key} {name}: relative error of the restatement {err_ref:.3e}, of torch float32 {err_t32:.3e}, "
              f"ratio {err_ref / err_t32:.2f}")
        if not (err_t32 > 0 and err_ref <= 8 * err_t32):
            bad.append((name, err_ref, err_t32))
    assert not bad, bad


def test_one_pass_variance_agrees_with_two_pass():
    """var = S2 / m - mu^2 from the Float64 sums against numpy's two-pass Float64 variance of the same Float32 values, both
    rounded to Float32 once, for every channel of the three cases.  The one-pass form loses about log2(1 + mu^2 / var) of
    Float64's 53 bits; with that ratio below 2^20 its error stays far below half a Float32 ulp (2^-25), so the two Float32
    results can differ only where the Float64 values straddle a rounding boundary: by one ulp at most."""
    for key in (10, 40, "edgeconv"):
        _, order, mine, _ = _restated(key)
        worst, cond = 0, 0.0
        for name in order:
            v = mine["bn_inputs"][name].astype(np.float64)
            axes = tuple(range(v.ndim - 1))
            var64 = np.var(v, axis=axes)
            two = var64.astype(F32)
            one = mine["batch_stats"][name + ".sigma2"]
            mean = np.mean(v, axis=axes)
            live = two > 0
            assert np.array_equal(one[~live], two[~live]), name  # a constant channel: both are +0.0
            ulps = np.abs(_bits(one[live]).astype(np.int64) - _bits(two[live]).astype(np.int64))
            worst = max(worst, int(ulps.max(initial=0)))
            cond = max(cond, float(np.max(mean[live] ** 2 / var64[live], initial=0.0)))
        print(f"{key}: one-pass against two-pass variance at most {worst} Float32 ulp apart; largest mu^2/var {cond:.3g}")
        assert cond < 2.0 ** 20, cond
        assert worst <= 1, worst


def test_edge_sums_order_is_the_stated_one():
    """edge_sums against a scalar walk of the header's sentence, chain by chain, on a partial second tile."""
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((2, 3, 70, 2)) * 10.0 ** rng.integers(-3, 4, (2, 3, 70, 2))).astype(F32)
    s1, s2 = tref.edge_sums(v)
    for c in range(2):
        tiles = []
        for b in range(2):
            for tile in range(2):
                ch = {}
                for q in (0, 1):
                    for h in (0, 1):
                        a1 = a2 = np.float64(0)
                        for k in range(3):
                            for p in range(64):
                                n = 64 * tile + p
                                if p // 32 == q and (p >> 2) & 1 == h and n < 70:
                                    d = np.float64(v[b, k, n, c])
                                    a1, a2 = a1 + d, a2 + d * d
                        ch[q, h] = (a1, a2)
                tiles.append([(ch[0, 0][i] + ch[0, 1][i]) + (ch[1, 0][i] + ch[1, 1][i]) for i in (0, 1)])
        for i, s in ((0, s1), (1, s2)):
            total = np.float64(0)
            for t in tiles:  # fewer tiles than groups: every chain holds one tile sum, added in ascending g from +0.0
                total = total + (np.float64(0) + t[i])
            assert total == s[c], (c, i)


def test_stat_layout_and_counts(fx):
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    count = ctypes.c_int64(0)
    _lib.call("fx3d_dgcnn_stat_count", ctypes.byref(count))
    assert count.value == 2 * 2336 == 2 * sum(tref.BN_WIDTH)
    assert lib.fx3d_dgcnn_stat_count(None) == INVALID and "NULL" in _lib.last_error()
    for nc in (10, 40):
        shapes = ref.param_shapes(nc)
        names = [n for n in shapes if n.endswith((".mu", ".sigma2"))]   # the order of the slots in the flat parameter buffer
        assert names == [f"{bn}.{f}" for bn in tref.BN_ORDER for f in ("mu", "sigma2")]
        assert [shapes[bn + ".mu"][0] for bn in tref.BN_ORDER] == tref.BN_WIDTH
        m = fx.DGCNN(nc, K, N)
        at, flat = 0, 0
        slots = {name: (C, s, p) for name, C, s, p in m._stat_slots()}
        for name, shape in shapes.items():   # offsets in both buffers, derived here from the shapes alone
            if name.endswith(".mu"):
                assert slots[name[:-3]] == (shape[0], at, flat), name
                at += 2 * shape[0]
            flat += int(np.prod(shape))
        assert at == count.value and flat == m.param_count
    for layers in ([3, 32, 64, 64], [64, 128, 256], GENERIC, [1, 1], [128, 256, 256, 256, 256]):
        arr = (ctypes.c_int32 * len(layers))(*layers)
        _lib.call("fx3d_edgeconv_stat_count", arr, len(layers), ctypes.byref(count))
        assert count.value == 2 * sum(layers[1:]), layers
        assert [s[0] for s in fx.EdgeConv(layers, 2)._stat_slots()] == [f"bn{i}" for i in range(1, len(layers))]
    arr = (ctypes.c_int32 * 3)(3, 8, 8)
    assert lib.fx3d_edgeconv_stat_count(arr, 3, None) == INVALID and "NULL" in _lib.last_error()
    assert lib.fx3d_edgeconv_stat_count(None, 3, ctypes.byref(count)) == INVALID
    assert lib.fx3d_edgeconv_stat_count((ctypes.c_int32 * 3)(3, 8, 257), 3, ctypes.byref(count)) == UNSUPPORTED
    assert lib.fx3d_edgeconv_stat_count((ctypes.c_int32 * 6)(3, 8, 8, 8, 8, 8), 6, ctypes.byref(count)) == UNSUPPORTED


def test_the_six_symbols_are_exported_with_the_header_arity(fx):
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "flux3d_hip.h")).read()
    assert "DGCNN / EdgeConv training-mode forward" in hdr
    for name in ("fx3d_dgcnn_stat_count", "fx3d_dgcnn_train_workspace_bytes", "fx3d_dgcnn_forward_train",
                 "fx3d_edgeconv_stat_count", "fx3d_edgeconv_train_workspace_bytes", "fx3d_edgeconv_forward_train"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        args = re.search(r"FX3D_API\s+fx3d_status\s+" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(_lib.SIGNATURES[name]) == len(args.split(",")), name
    assert len(_lib.SIGNATURES["fx3d_dgcnn_forward_train"]) == 21 and len(_lib.SIGNATURES["fx3d_edgeconv_forward_train"]) == 16
    assert callable(fx.DGCNN.forward_train) and callable(fx.DGCNN.dropout_masks) and callable(fx.EdgeConv.forward_train)


def _says(*words):
    from flux3d_jl_amd import _lib
    msg = _lib.last_error()
    return all(w in msg for w in words)


def test_dgcnn_entry_points_refuse_before_any_device_work(fx):
    """No call here has arguments that would pass the checks: the dummy pointers are never dereferenced."""
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(4096)
    nb = ctypes.c_size_t(0)

    def train(nc=10, K_=3, N_=64, B_=2, params=dummy, x=dummy, d4=None, d5=None, momentum=0.1, probs=dummy, stats=dummy,
              running=None, ws=dummy, ws_bytes=1 << 40):
        return lib.fx3d_dgcnn_forward_train(params, nc, K_, x, N_, B_, d4, d5, momentum, probs, None, None, None, None, None, None,
                                            stats, running, ws, ws_bytes, None)

    def size(N_=64, B_=2, K_=3, nc=10, out=ctypes.byref(nb)):
        return lib.fx3d_dgcnn_train_workspace_bytes(N_, B_, K_, nc, out)

    assert size(out=None) == INVALID and _says("NULL")
    for k in ("params", "x", "probs", "stats", "ws"):
        assert train(**{k: None}) == INVALID and _says("NULL"), k
    for kw, words in ((dict(N_=0), ("N=0",)), (dict(B_=0), ("B=0",)), (dict(nc=0), ("num_classes",)), (dict(K_=0), ("K",)),
                      (dict(K_=64), ("K + 1",)), (dict(N_=36865), ("36864",)), (dict(B_=65536, N_=8), ("65536",)),
                      (dict(B_=1), ("B >= 2", "got 1"))):
        assert train(**kw) == INVALID and _says("fx3d_dgcnn_forward_train", *words), kw
        assert train(**kw, d4=dummy, d5=dummy, running=dummy) == INVALID and _says(*words), kw
        assert size(**kw) == INVALID and _says("fx3d_dgcnn_train_workspace_bytes", *words), kw
    for mtm in (-0.1, 1.5, float("nan"), float("inf")):
        assert train(momentum=mtm) == INVALID and _says("momentum"), mtm
    fwd = ctypes.c_size_t(0)
    assert size() == 0 and nb.value % 256 == 0
    assert lib.fx3d_dgcnn_workspace_bytes(64, 2, 3, 10, ctypes.byref(fwd)) == 0
    assert nb.value >= fwd.value + 2 * 1024 * 1 * 2 * 8 + (512 + 256) * 2 * 4  # the forward's, the tile sums, the head's activations
    assert train(ws_bytes=nb.value - 1) == INVALID and _says("workspace", str(nb.value))
    assert train(ws=ctypes.c_void_p(4096 + 16), ws_bytes=nb.value) == INVALID and _says("256-byte aligned")
    # no (K N, C, B) activation array (335 MB at 64 channels): at 32 x 1024, K = 20 the workspace grows by conv_3's tile sums,
    # 8 MiB, and the head's activations over the forward's
    assert size(N_=1024, B_=32, K_=20, nc=40) == 0
    assert lib.fx3d_dgcnn_workspace_bytes(1024, 32, 20, 40, ctypes.byref(fwd)) == 0
    assert nb.value - fwd.value < 9 << 20, (nb.value, fwd.value)


def test_edgeconv_entry_points_refuse_before_any_device_work(fx):
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(4096)
    nb = ctypes.c_size_t(0)
    good = [3, 16, 16]

    def train(layers=good, K_=3, N_=64, B_=1, params=dummy, x=dummy, idx=None, momentum=0.1, out=dummy, stats=dummy, running=None,
              ws=dummy, ws_bytes=1 << 40):
        arr = None if layers is None else (ctypes.c_int32 * len(layers))(*layers)
        return lib.fx3d_edgeconv_forward_train(params, arr, 0 if layers is None else len(layers), K_, x, N_, B_, idx, momentum, out,
                                               None, stats, running, ws, ws_bytes, None)

    def size(layers=good, K_=3, N_=64, B_=1, out=ctypes.byref(nb)):
        arr = (ctypes.c_int32 * len(layers))(*layers)
        return lib.fx3d_edgeconv_train_workspace_bytes(arr, len(layers), K_, N_, B_, out)

    assert size(out=None) == INVALID and _says("NULL")
    for k in ("params", "x", "out", "stats", "ws", "layers"):
        assert train(**{k: None}) == INVALID and _says("NULL"), k
    for layers in ([3], [3, 8, 8, 8, 8, 8], [129, 8], [0, 8], [3, 257], [3, 8, 0]):
        assert train(layers=layers) == UNSUPPORTED and _says("fx3d_edgeconv_forward_train"), layers
        assert size(layers=layers) == UNSUPPORTED, layers
    for kw, words in ((dict(N_=0), ("N=0",)), (dict(B_=0), ("B=0",)), (dict(K_=0), ("K",)), (dict(K_=64), ("K + 1",)),
                      (dict(N_=36865), ("36864",)), (dict(B_=65536, N_=8, K_=1), ("65536",))):
        assert train(**kw) == INVALID and _says("fx3d_edgeconv_forward_train", *words), kw
        assert train(**kw, idx=dummy, running=dummy) == INVALID and _says(*words), kw
        assert size(**kw) == INVALID and _says("fx3d_edgeconv_train_workspace_bytes", *words), kw
    for mtm in (-0.1, 1.5, float("nan"), float("inf")):
        assert train(momentum=mtm) == INVALID and _says("momentum"), mtm
    fwd = ctypes.c_size_t(0)
    assert size() == 0 and nb.value % 256 == 0  # one cloud is enough: m = K N >= 2
    arr = (ctypes.c_int32 * 3)(*good)
    assert lib.fx3d_edgeconv_workspace_bytes(arr, 3, 3, 64, 1, ctypes.byref(fwd)) == 0
    assert nb.value >= fwd.value + 2 * 16 * 1 * 1 * 8
    assert train(ws_bytes=nb.value - 1) == INVALID and _says("workspace", str(nb.value))
    assert train(ws=ctypes.c_void_p(4096 + 16), ws_bytes=nb.value) == INVALID and _says("256-byte aligned")


def test_dropout_masks_values_and_bits(fx):
    m4, m5 = fx.DGCNN.dropout_masks(7, seed=3)
    assert m4.shape == (512, 7) and m5.shape == (256, 7)
    for mask in (m4, m5):
        assert mask.dtype == F32 and mask.flags.f_contiguous
        assert set(np.unique(_bits(mask)).tolist()) == {0, 0x40000000}  # 0 or Float32(2)
        assert set(np.unique(mask).tolist()) == {0.0, float(np.float32(2.0))}
        kept = float(np.mean(mask != 0))
        assert abs(kept - 0.5) < 4 * math.sqrt(0.25 / mask.size), kept  # four standard deviations of the binomial share
    again = fx.DGCNN.dropout_masks(7, seed=3)
    other = fx.DGCNN.dropout_masks(7, seed=4)
    assert np.array_equal(m4, again[0]) and np.array_equal(m5, again[1]) and not np.array_equal(m4, other[0])
    assert not np.array_equal(m4[:256], m5)  # the second mask is drawn after the first, not a copy of it
    third = fx.DGCNN.dropout_masks(5, seed=1, p=0.75)[0]
    assert set(np.unique(third).tolist()) == {0.0, 4.0}
    assert all(np.all(m == 1.0) for m in fx.DGCNN.dropout_masks(3, seed=0, p=0.0))
    for p in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            fx.DGCNN.dropout_masks(4, seed=0, p=p)
    with pytest.raises(ValueError):
        fx.DGCNN.dropout_masks(0, seed=0)


def test_forward_train_argument_errors_before_any_launch(fx):
    m = fx.DGCNN(10, 3, 8)
    X = np.zeros((3, 8, 2), F32)
    with pytest.raises(ValueError, match="at least two clouds"):
        m.forward_train(np.zeros((3, 8, 1), F32))
    with pytest.raises(ValueError, match="at least two clouds"):
        m.forward_train(np.zeros((3, 8), F32))
    with pytest.raises(ValueError, match="npoints"):
        m.forward_train(np.zeros((3, 9, 2), F32))
    ok4, ok5 = np.ones((512, 2), F32), np.ones((256, 2), F32)
    for bad in ((np.ones((512, 3), F32), ok5), (ok4, np.ones((255, 2), F32)), (ok5, ok4), (np.ones((512,), F32), ok5)):
        with pytest.raises(ValueError, match=r"dropout\[[01]\] must be"):
            m.forward_train(X, dropout=bad)
    for bad in (ok4, (ok4,), (ok4, ok5, ok5), 0.5, "seed"):
        with pytest.raises(TypeError, match="dropout must be"):
            m.forward_train(X, dropout=bad)
    with pytest.raises(TypeError, match="dropout"):
        m.forward_train(X, dropout=(ok4.astype(np.complex64), ok5))
    for mtm in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            m.forward_train(X, momentum=mtm)
    with pytest.raises(ValueError, match="3 channels"):
        m.forward_train(np.zeros((4, 8, 2), F32))
    e = fx.EdgeConv([5, 8], 3)
    Xe = np.zeros((5, 8, 1), F32)
    for mtm in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            e.forward_train(Xe, momentum=mtm)
    with pytest.raises(ValueError, match="5 channels"):
        e.forward_train(np.zeros((4, 8, 1), F32))
    with pytest.raises(ValueError, match="K"):
        e.forward_train(np.zeros((5, 3, 1), F32))
    with pytest.raises(ValueError, match="idx must"):
        e.forward_train(Xe, idx=np.zeros((2, 8, 1), np.int32))
    with pytest.raises(ValueError, match="0-based"):
        e.forward_train(Xe, idx=np.full((3, 8, 1), 8, np.int32))
