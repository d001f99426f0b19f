"""PointNet inference, the part that needs no GPU: the host restatement tests/pointnet_ref.py is what it claims to be (its
fma32 is libm's fmaf; its network is a PointNet, cross-checked against an independent evaluation by torch.nn.functional),
and the library's host-side contract (parameter count and shapes, workspace cap, argument errors)."""
import ctypes
import ctypes.util
import os
import subprocess
import sys

import numpy as np
import pytest

import pointnet_ref as ref

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _libm_fmaf(a, b, c):
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    libm.fmaf.restype = ctypes.c_float
    return np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)


def _double_rounding_triples():
    """a b + c lies 2^-70 (relative to c) BELOW a Float32 tie above an odd c: Float64 rounds the sum onto the tie, the second
    rounding then goes to even -- up -- while fmaf stays at c.  Scaled by powers of two and mirrored."""
    a, b, c = [], [], []
    for e in range(-20, 21, 4):
        for sign in (1.0, -1.0):
            s = 2.0 ** e
            a.append(1.0 + 2.0 ** -23)
            b.append(sign * s * 2.0 ** -24 * (1.0 - 2.0 ** -23))
            c.append(sign * s * (1.0 + 2.0 ** -23))
    return np.array(a, F32), np.array(b, F32), np.array(c, F32)


def test_fma32_is_libm_fmaf():
    rng = np.random.default_rng(20240)
    n = 40000
    # random triples over many binades
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(F32)
    # near ties: c = t, a b = half an ulp of t up to the rounding of b
    t = (rng.standard_normal(n) * 2.0 ** rng.integers(-10, 10, n)).astype(F32)
    half_ulp = (np.spacing(np.abs(t)).astype(np.float64) / 2) * rng.choice([-1.0, 1.0], n)
    a2 = rng.uniform(0.5, 2.0, n).astype(F32)
    b2 = (half_ulp / a2.astype(np.float64)).astype(F32)
    da, db, dc = _double_rounding_triples()
    naive = (da.astype(np.float64) * db.astype(np.float64) + dc.astype(np.float64)).astype(F32)
    want_d = _libm_fmaf(da, db, dc)
    assert np.all(_bits(naive) != _bits(want_d)), "the constructed triples must defeat rounding to Float64 first"
    # cancellation, zeros of both signs, subnormal results
    sa = np.array([1.0, -1.0, 0.0, -0.0, 1e-30, 3.0, 1e-20], F32)
    sb = np.array([1.0, 1.0, 5.0, 5.0, 1e-12, 1e-39 / 3, -1e-20], F32)
    sc = np.array([-1.0, 1.0, -0.0, -0.0, 1e-44, 1e-45, 1e-40], F32)
    for x, y, z in ((a, b, c), (a2, b2, t), (da, db, dc), (sa, sb, sc)):
        got, want = ref.fma32(x, y, z), _libm_fmaf(x, y, z)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, (bad[:5], x[bad[:5]], y[bad[:5]], z[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_compiled_chain_is_the_fma32_chain():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 17, 64)).astype(F32)
    W = rng.standard_normal((64, 40)).astype(F32)
    assert np.array_equal(_bits(ref.contract(x, W)), _bits(ref.contract_numpy(x, W)))
    # and not the unfused chain (the product rounded first), which differs somewhere on data like this
    unfused = np.zeros((3, 17, 40), F32)
    for c in range(64):
        unfused = (unfused + (x[..., c:c + 1] * W[c]).astype(F32)).astype(F32)
    assert not np.array_equal(_bits(unfused), _bits(ref.contract_numpy(x, W)))


def test_relu_max_and_batchnorm_conventions():
    v = np.array([-0.0, 0.0, -1.0, 2.0, np.nan], F32)
    assert np.array_equal(_bits(ref.relu(v))[:4], _bits(np.array([0.0, 0.0, 0.0, 2.0], F32))) and np.isnan(ref.relu(v)[4])
    m = ref.jmax(np.array([[-0.0, -0.0, 1.0], [0.0, -0.0, np.nan], [-0.0, -0.0, 3.0]], F32), axis=0)
    assert np.array_equal(_bits(m)[:2], _bits(np.array([0.0, -0.0], F32))) and np.isnan(m[2])


def _torch_logits(X, P, tmp_path):
    """tests/pointnet_torch_eval.py in a child process (torch stays out of this one, which loads the HIP library): the
    logits in float64 and in float32."""
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    np.savez(src, X=X, **P)
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "pointnet_torch_eval.py"), src, dst],
                   check=True, timeout=600)
    out = np.load(dst)
    return out["logits64"], out["logits32"]


@pytest.mark.parametrize("num_classes", [10, 40])
def test_the_restatement_is_a_pointnet(num_classes, tmp_path):
    """Logits of the restatement against torch in float64.  The bound is measured, not chosen: both the restatement and a
    float32 torch evaluation are Float32 sums in some order, so the restatement's error may be at most 8 x torch-float32's."""
    rng = np.random.default_rng(100 + num_classes)
    X = rng.standard_normal((3, 64, 2)).astype(F32)
    P = ref.random_params(num_classes, seed=num_classes)
    mine = ref.forward(X, P)["logits"]
    t64, t32 = _torch_logits(X, P, tmp_path)
    assert mine.shape == t64.shape == (num_classes, 2)
    alive = int(np.count_nonzero(t64 > 0))
    scale = float(np.max(np.abs(t64)))
    err_ref = float(np.max(np.abs(mine.astype(np.float64) - t64))) / scale
    err_t32 = float(np.max(np.abs(t32.astype(np.float64) - t64))) / scale
    print(f"num_classes={num_classes}: {alive} of {t64.size} logits survive the relu; relative error of the restatement "
          f"{err_ref:.3e}, of torch float32 {err_t32:.3e}, ratio {err_ref / err_t32:.2f}")
    assert alive * 8 >= t64.size, f"only {alive} of {t64.size} logits survive the relu: the draw proves nothing"
    assert err_t32 > 0 and err_ref <= 8 * err_t32, (err_ref, err_t32)


def _count_from_shapes(num_classes):
    def stn(K):
        return (K * 64 + 64) + 4 * 64 + (64 * 128 + 128) + 4 * 128 + (128 * 1024 + 1024) + 4 * 1024 + (1024 * 512 + 512) + \
            (512 * 256 + 256) + 4 * 256 + (256 * K * K + K * K)
    feat = (64 * 128 + 128) + 4 * 128 + (128 * 1024 + 1024) + 4 * 1024 + (1024 * 512 + 512) + 4 * 512 + (512 * 256 + 256) + 4 * 256
    return stn(3) + (3 * 64 + 64) + 4 * 64 + stn(64) + feat + (256 * num_classes + num_classes)


@pytest.mark.parametrize("num_classes", [10, 40])
def test_param_count_and_shapes(fx, num_classes):
    from flux3d_jl_amd import _lib
    count = ctypes.c_int64(0)
    _lib.call("fx3d_pointnet_param_count", num_classes, ctypes.byref(count))
    assert count.value == _count_from_shapes(num_classes)
    m = fx.PointNet(num_classes)
    want = ref.param_shapes(num_classes)
    assert list(m.params) == list(want)
    assert {k: v.shape for k, v in m.params.items()} == want
    assert all(v.dtype == np.float32 for v in m.params.values())
    flat = m.flat_params()
    assert flat.size == count.value and flat.dtype == np.float32
    # conv W (Cin, Cout) column-major: element [c, o] of the first layer at c + 3 o
    assert flat[1 + 3 * 5] == m.params["stn.conv1.weight"][0, 1, 5]
    # a fresh model has Flux's BatchNorm initialisation and another seed gives other weights
    assert np.all(m.params["feat.bn1.gamma"] == 1) and np.all(m.params["feat.bn1.mu"] == 0) and np.all(m.params["feat.bn1.sigma2"] == 1)
    assert not np.array_equal(fx.PointNet(num_classes, seed=1).params["cls.weight"], m.params["cls.weight"])


def test_workspace_cap_and_argument_errors(fx):
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    _lib.call("fx3d_pointnet_workspace_bytes", 1024, 32, 40, ctypes.byref(nb))
    assert 4 * 64 * 1024 * 32 <= nb.value <= 2 * 4 * 64 * 1024 * 32, nb.value  # the (N,64,B) activations fit, a 1024-channel tensor does not
    for N, B, nc in ((0, 1, 10), (1, 0, 10), (1, 1, 0), (-5, 2, 10)):
        assert lib.fx3d_pointnet_workspace_bytes(N, B, nc, ctypes.byref(nb)) != 0
    assert lib.fx3d_pointnet_workspace_bytes(64, 2, 10, None) != 0
    cnt = ctypes.c_int64(0)
    assert lib.fx3d_pointnet_param_count(0, ctypes.byref(cnt)) != 0 and lib.fx3d_pointnet_param_count(10, None) != 0
    # NULL pointers and bad sizes are refused before anything touches a device
    assert lib.fx3d_pointnet_forward(None, 10, None, 64, 2, None, None, None, None, None, None, 0, None) != 0
    assert "NULL" in _lib.last_error()
    dummy = ctypes.c_void_p(4096)
    assert lib.fx3d_pointnet_forward(dummy, 10, dummy, 0, 2, dummy, None, None, None, None, dummy, 1 << 30, None) != 0
    assert lib.fx3d_pointnet_forward(dummy, 10, dummy, 64, 2, dummy, None, None, None, None, dummy, 16, None) != 0
    assert "workspace" in _lib.last_error()


def test_python_errors_before_any_launch(fx):
    with pytest.raises(ValueError, match="conv_block1"):
        fx.PointNet(10, K=32)
    with pytest.raises(ValueError):
        fx.PointNet(0)
    m = fx.PointNet(10)
    with pytest.raises(ValueError, match="3 channels"):
        m(np.zeros((2, 64, 2), np.float32))
    with pytest.raises(ValueError):
        m(np.zeros((3, 64, 2, 1), np.float32))
    with pytest.raises(ValueError):
        m(np.zeros((3, 0, 2), np.float32))
    P = ref.random_params(10, 0)
    bad = dict(P)
    bad["cls.weight"] = np.zeros((256, 10), np.float32)  # Flux keeps Dense weights as (out, in)
    with pytest.raises(ValueError, match="cls.weight"):
        m.load(bad)
    missing = dict(P)
    del missing["feat.bn3.mu"]
    with pytest.raises(ValueError, match="feat.bn3.mu"):
        m.load(missing)
    assert m.load(P) is m and np.array_equal(m.params["fstn.dense3.weight"], P["fstn.dense3.weight"])
