"""The PointNet training-mode forward, the part that needs no GPU: the restatement tests/pointnet_train_ref.py is a PointNet in
training mode (against torch in float64, tests/pointnet_train_torch_eval.py), its one-pass Float64 variance agrees with a two-pass
one, and the library's host-side contract: the statistics layout, the exported symbols, the refusals before any device work,
the dropout mask and the Python argument errors."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pointnet_ref as ref
import pointnet_train_ref as tref

F32 = np.float32
INVALID = -1  # FX3D_ERR_INVALID_ARG
HERE = os.path.dirname(os.path.abspath(__file__))
N, B = 64, 4
MOMENTUM = 0.1


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _case(num_classes):
    from flux3d_jl_amd import models
    rng = np.random.default_rng(200 + num_classes)
    X = rng.standard_normal((3, N, B)).astype(F32)
    P = ref.random_params(num_classes, seed=num_classes)
    mask = models.PointNet.dropout_mask(B, seed=num_classes)
    return X, P, mask


_CASES = {}


def _restated(num_classes):
    """The restatement's run of the case, computed once and shared (never modified)."""
    if num_classes not in _CASES:
        X, P, mask = _case(num_classes)
        _CASES[num_classes] = (X, P, mask, tref.forward_train(X, P, dropout=mask, momentum=MOMENTUM))
    return _CASES[num_classes]


def _split(flat):
    """A flat statistics buffer as (all means, all variances)."""
    mu, var, at = [], [], 0
    for name in tref.BN_ORDER:
        C = ref.param_shapes(10)[name + ".mu"][0]
        mu.append(flat[at:at + C])
        var.append(flat[at + C:at + 2 * C])
        at += 2 * C
    assert at == flat.size
    return np.concatenate(mu), np.concatenate(var)


@pytest.mark.parametrize("num_classes", [10, 40])
def test_the_restatement_is_a_pointnet_in_training_mode(num_classes, tmp_path):
    """Against torch (BatchNorm with training=True, the mask applied as given) in float64, with the bound of
    test_pointnet_host.py::test_the_restatement_is_a_pointnet: the restatement's relative error is at most 8 x torch-float32's,
    for the logits, the batch means, the batch variances and the updated running means and variances."""
    X, P, mask, mine = _restated(num_classes)
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    np.savez(src, X=X, momentum=MOMENTUM, dropout=mask, **P)
    subprocess.run([sys.executable, os.path.join(HERE, "pointnet_train_torch_eval.py"), src, dst], check=True, timeout=600)
    t = np.load(dst)
    assert mine["logits"].shape == t["logits64"].shape == (num_classes, B)
    alive = int(np.count_nonzero(t["logits64"] > 0))
    print(f"num_classes={num_classes}: {alive} of {t['logits64'].size} logits survive the relu")
    assert alive * 8 >= t["logits64"].size, f"only {alive} of {t['logits64'].size} logits survive the relu: the draw proves nothing"
    got = {"logits": mine["logits"]}
    got["batch means"], got["batch variances"] = _split(tref.flat_stats(mine["batch_stats"]))
    got["running means"], got["running variances"] = _split(tref.flat_stats(mine["running"]))
    t64, t32 = {"logits": t["logits64"]}, {"logits": t["logits32"]}
    for d, tag in ((t64, "64"), (t32, "32")):
        d["batch means"], d["batch variances"] = _split(t["stats" + tag])
        d["running means"], d["running variances"] = _split(t["running" + tag])
    bad = []
    for key in got:
        scale = float(np.max(np.abs(t64[key])))
        err_ref = float(np.max(np.abs(got[key].astype(np.float64) - t64[key]))) / scale
        err_t32 = float(np.max(np.abs(t32[key].astype(np.float64) - t64[key]))) / scale
        print(f"  {key}: relative error of the restatement {err_ref:.3e}, of torch float32 {err_t32:.3e}, "
              f"ratio {err_ref / err_t32:.2f}")
        if not (err_t32 > 0 and err_ref <= 8 * err_t32):
            bad.append((key, err_ref, err_t32))
    assert not bad, bad


def test_one_pass_variance_agrees_with_two_pass():
    """var = S2 / m - mu^2 from the Float64 sums against numpy's two-pass Float64 variance of the same Float32 values, both
    rounded to Float32 once, for all 4928 channels of both cases.  The one-pass form loses about log2(1 + mu^2 / var) of
    Float64's 53 bits; with that ratio below 2^20 on these draws its error stays far below half a Float32 ulp (2^-25), so the
    two Float32 results can differ only where the Float64 values straddle a rounding boundary: by one ulp at most.
    Measured: the largest difference is 0 ulp; the largest mu^2 / var is 1.08e3 (10 classes) and 406 (40 classes)."""
    for nc in (10, 40):
        _, _, _, mine = _restated(nc)
        worst, cond = 0, 0.0
        for name in tref.BN_ORDER:
            v = mine["bn_inputs"][name].astype(np.float64)
            axes = tuple(range(v.ndim - 1))
            two = np.var(v, axis=axes).astype(F32)
            one = mine["batch_stats"][name + ".sigma2"]
            mean = np.mean(v, axis=axes)
            live = two > 0
            assert np.array_equal(one[~live], two[~live]), name  # a constant channel: both are +0.0
            ulps = np.abs(_bits(one[live]).astype(np.int64) - _bits(two[live]).astype(np.int64))
            worst = max(worst, int(ulps.max(initial=0)))
            cond = max(cond, float(np.max(mean[live] ** 2 / np.var(v, axis=axes)[live], initial=0.0)))
        print(f"num_classes={nc}: one-pass against two-pass variance at most {worst} Float32 ulp apart; largest mu^2/var {cond:.3g}")
        assert cond < 2.0 ** 20, cond
        assert worst <= 1, worst


def test_stat_layout_and_count(fx):
    from flux3d_jl_amd import _lib
    count = ctypes.c_int64(0)
    _lib.call("fx3d_pointnet_stat_count", ctypes.byref(count))
    assert count.value == 2 * 4928
    assert _lib.load().fx3d_pointnet_stat_count(None) == INVALID and "NULL" in _lib.last_error()
    for nc in (10, 40):
        shapes = ref.param_shapes(nc)
        names = [n for n in shapes if n.endswith((".mu", ".sigma2"))]   # the order of the slots in the flat parameter buffer
        assert names == [f"{bn}.{f}" for bn in tref.BN_ORDER for f in ("mu", "sigma2")]
        assert sum(shapes[n][0] for n in names) == count.value
        m = fx.PointNet(nc)
        at, flat = 0, 0
        slots = {name: (C, s, p) for name, C, s, p in m._stat_slots()}
        for name, shape in shapes.items():   # offsets in both buffers, derived here from the shapes alone
            if name.endswith(".mu"):
                assert slots[name[:-3]] == (shape[0], at, flat), name
                at += 2 * shape[0]
            flat += int(np.prod(shape))
        assert at == count.value and flat == m.param_count


def test_the_three_symbols_are_exported_with_the_header_arity(fx):
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "flux3d_hip.h")).read()
    assert "PointNet training-mode forward" in hdr
    for name in ("fx3d_pointnet_stat_count", "fx3d_pointnet_train_workspace_bytes", "fx3d_pointnet_forward_train"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        args = re.search(r"FX3D_API\s+fx3d_status\s+" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(_lib.SIGNATURES[name]) == len(args.split(",")), name
    assert len(_lib.SIGNATURES["fx3d_pointnet_forward_train"]) == 17
    assert callable(fx.PointNet.forward_train) and callable(fx.PointNet.dropout_mask)


def test_the_c_entry_points_refuse_before_any_device_work(fx):
    """No call here has arguments that would pass the checks: the dummy pointers are never dereferenced."""
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(4096)
    nb = ctypes.c_size_t(0)

    def train(nc=10, N_=64, B_=2, params=dummy, x=dummy, dropout=None, momentum=0.1, probs=dummy, stats=dummy, running=None,
              ws=dummy, ws_bytes=1 << 40):
        return lib.fx3d_pointnet_forward_train(params, nc, x, N_, B_, dropout, momentum, probs, None, None, None, None, stats,
                                               running, ws, ws_bytes, None)

    def says(*words):
        msg = _lib.last_error()
        return all(w in msg for w in words)

    def size(N_=64, B_=2, nc=10, out=ctypes.byref(nb)):
        return lib.fx3d_pointnet_train_workspace_bytes(N_, B_, nc, out)

    assert size(out=None) == INVALID and says("NULL")
    for k in ("params", "x", "probs", "stats", "ws"):
        assert train(**{k: None}) == INVALID and says("NULL"), k
    for kw, words in ((dict(N_=0), ("N=0",)), (dict(B_=0), ("B=0",)), (dict(nc=0), ("num_classes",)),
                      (dict(B_=65536, N_=8), ("65536",)), (dict(B_=1), ("B >= 2", "got 1"))):
        assert train(**kw) == INVALID and says("fx3d_pointnet_forward_train", *words), kw
        assert train(**kw, dropout=dummy, running=dummy) == INVALID and says(*words), kw
        assert size(**kw) == INVALID and says("fx3d_pointnet_train_workspace_bytes", *words), kw
    for mtm in (-0.1, 1.5, float("nan"), float("inf")):
        assert train(momentum=mtm) == INVALID and says("momentum"), mtm
    fwd = ctypes.c_size_t(0)
    assert size() == 0 and nb.value % 256 == 0
    assert lib.fx3d_pointnet_workspace_bytes(64, 2, 10, ctypes.byref(fwd)) == 0
    assert nb.value >= fwd.value + 2 * 1024 * 1 * 2 * 8 + (512 + 256) * 2 * 4  # the forward's, the tile sums, the heads' activations
    assert train(ws_bytes=nb.value - 1) == INVALID and says("workspace", str(nb.value))
    assert train(ws=ctypes.c_void_p(4096 + 8), ws_bytes=nb.value) == INVALID and says("16-byte aligned")
    # no (1024, N, B) activation array: at 32 x 1024 the workspace stays below one
    assert size(N_=1024, B_=32, nc=40) == 0 and nb.value < 4 * 1024 * 1024 * 32, nb.value


def test_dropout_mask_values_and_bits(fx):
    mask = fx.PointNet.dropout_mask(7, seed=3)
    assert mask.shape == (256, 7) and mask.dtype == F32 and mask.flags.f_contiguous
    assert set(np.unique(_bits(mask)).tolist()) == {0, 0x3FD55555}  # 0 or Float32(1 / 0.6)
    kept = float(np.mean(mask != 0))
    assert abs(kept - 0.6) < 4 * math.sqrt(0.24 / mask.size), kept  # four standard deviations of the binomial share
    assert np.array_equal(mask, fx.PointNet.dropout_mask(7, seed=3)) and not np.array_equal(mask, fx.PointNet.dropout_mask(7, seed=4))
    half = fx.PointNet.dropout_mask(5, seed=1, p=0.5)
    assert set(np.unique(half).tolist()) == {0.0, 2.0}
    assert np.all(fx.PointNet.dropout_mask(3, seed=0, p=0.0) == 1.0)
    for p in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            fx.PointNet.dropout_mask(4, seed=0, p=p)


def test_forward_train_argument_errors_before_any_launch(fx):
    m = fx.PointNet(10)
    X = np.zeros((3, 8, 2), F32)
    with pytest.raises(ValueError, match="at least two clouds"):
        m.forward_train(np.zeros((3, 8, 1), F32))
    with pytest.raises(ValueError, match="at least two clouds"):
        m.forward_train(np.zeros((3, 8), F32))
    for bad in (np.ones((256, 3), F32), np.ones((255, 2), F32), np.ones((2, 256), F32), np.ones((256,), F32)):
        with pytest.raises(ValueError, match="dropout must be"):
            m.forward_train(X, dropout=bad)
    with pytest.raises(TypeError, match="dropout"):
        m.forward_train(X, dropout=np.ones((256, 2), np.complex64))
    for mtm in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            m.forward_train(X, momentum=mtm)
    with pytest.raises(ValueError, match="3 channels"):
        m.forward_train(np.zeros((4, 8, 2), F32))
