"""EdgeConv(layers, K) as a layer in its own right, the part that needs no GPU: the host restatement tests/edgeconv_ref.py is an
EdgeConv (cross-checked against an independent evaluation by torch.nn.functional), the parameter count and layout of
fx3d_edgeconv_param_count (a slice of a DGCNN's buffer is an EdgeConv's buffer), and every refusal of the C entry points and of
fx.EdgeConv, all of which come before any device work."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dgcnn_ref
import edgeconv_ref as ref

F32 = np.float32
INVALID, UNSUPPORTED = -1, -5   # FX3D_ERR_INVALID_ARG, FX3D_ERR_UNSUPPORTED (include/flux3d_hip.h)
# the layer lists of tests/test_gpu_edgeconv.py
LAYER_LISTS = [[3, 16], [1, 1], [5, 33, 70], [4, 8, 8, 8, 40], [6, 2, 255], [128, 256, 256], [64, 64, 128, 256],
               [65, 8, 8, 8], [65, 8, 8, 8, 8], [3, 32, 64, 64], [64, 128, 256]]


def _arr(layers):
    return (ctypes.c_int32 * len(layers))(*layers), len(layers)


def _lib():
    from flux3d_jl_amd import _lib
    return _lib


def _package_shapes(layers):
    from flux3d_jl_amd.models import edgeconv_param_shapes
    return dict(edgeconv_param_shapes(layers))


def test_the_restatement_is_an_edgeconv(tmp_path):
    """The restatement against torch in float64 at [5, 33, 70], N = 65, B = 2, K = 6, both torch runs with the restatement's
    neighbours.  The bound is the siblings' (test_dgcnn_host.py, test_pointnet_host.py): the restatement and a float32 torch
    evaluation are both Float32 sums in some order, so the restatement's error may be at most 8 x torch-float32's."""
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    X = np.random.default_rng(300).standard_normal((5, N, B)).astype(F32)
    P = ref.random_params(layers, seed=1)
    assert {k: v.shape for k, v in P.items()} == _package_shapes(layers)  # the restatement's arrays are the package's
    idx, mine = ref.forward(X, P, layers, K)
    ref.check_draw(mine)
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    np.savez(src, X=X, idx=idx, layers=np.array(layers), **P)
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "edgeconv_torch_eval.py"), src, dst],
                   check=True, timeout=600)
    t = np.load(dst)
    t64, t32 = t["out64"], t["out32"]
    assert mine.shape == t64.shape == (70, N, B)
    scale = float(np.max(np.abs(t64)))
    err_ref = float(np.max(np.abs(mine.astype(np.float64) - t64))) / scale
    err_t32 = float(np.max(np.abs(t32.astype(np.float64) - t64))) / scale
    print(f"non-zero share {np.count_nonzero(mine) / mine.size:.2f}; relative error of the restatement {err_ref:.3e}, of torch "
          f"float32 {err_t32:.3e}, ratio {err_ref / err_t32:.2f}")
    assert err_t32 > 0 and err_ref <= 8 * err_t32, (err_ref, err_t32)


def test_the_restatement_is_dgcnn_refs_edgeconv():
    """Its own loop (the neighbour lists may be given) is dgcnn_ref.edgeconv, which is generic in the widths, bit for bit."""
    layers, K = [5, 33, 70], 6
    X = np.random.default_rng(301).standard_normal((5, 40, 2)).astype(F32)
    P = ref.random_params(layers, seed=2)
    assert {k: v.shape for k, v in P.items()} == _package_shapes(layers)
    idx, mine = ref.forward(X, P, layers, K)
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))
    idx2, theirs = dgcnn_ref.edgeconv(x, {"ec." + k: v for k, v in P.items()}, ("ec", 2), K)
    assert np.array_equal(idx, idx2)
    assert np.array_equal(mine.view(np.uint32), np.ascontiguousarray(np.transpose(theirs, (2, 1, 0))).view(np.uint32))
    _, again = ref.forward(X, P, layers, K, idx=idx)
    assert np.array_equal(mine.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("layers", LAYER_LISTS, ids=str)
def test_param_count_and_shapes(fx, layers):
    from flux3d_jl_amd.models import edgeconv_param_shapes
    count = ctypes.c_int64(0)
    _lib().call("fx3d_edgeconv_param_count", *_arr(layers), ctypes.byref(count))
    cins = [2 * layers[0]] + layers[1:-1]
    assert count.value == sum(ci * co + 5 * co for ci, co in zip(cins, layers[1:]))
    want = ref.param_shapes(layers)
    assert count.value == sum(int(np.prod(s)) for s in want.values())
    m = fx.EdgeConv(layers, 3)
    assert list(m.params) == list(want) == list(edgeconv_param_shapes(layers))
    assert {k: v.shape for k, v in m.params.items()} == want
    assert all(v.dtype == np.float32 for v in m.params.values())
    flat = m.flat_params()
    assert flat.size == count.value == m.param_count and flat.dtype == np.float32
    assert (m.layers, m.K) == (layers, 3)
    # conv W (Cin, Cout) column-major: element [c, o] of the first layer at c + Cin o
    c, o = cins[0] - 1, layers[1] - 1
    assert flat[c + cins[0] * o] == m.params["conv1.weight"][0, c, o]
    assert np.all(m.params["bn1.gamma"] == 1) and np.all(m.params["bn1.mu"] == 0) and np.all(m.params["bn1.sigma2"] == 1)
    if cins[0] * layers[1] > 1:
        assert not np.array_equal(fx.EdgeConv(layers, 3, seed=1).params["conv1.weight"], m.params["conv1.weight"])


def test_a_slice_of_a_dgcnn_buffer_is_an_edgeconv_buffer(fx):
    """The ec1 / ec2 slices of fx3d_dgcnn_param_count's buffer have the lengths fx3d_edgeconv_param_count returns, and hold
    what an EdgeConv loaded with those arrays flattens to."""
    P = dgcnn_ref.random_params(10, seed=5)
    flat = fx.DGCNN(10, 10, 64).load(P).flat_params()
    at = 0
    for name, layers in (("ec1", [3, 32, 64, 64]), ("ec2", [64, 128, 256])):
        count = ctypes.c_int64(0)
        _lib().call("fx3d_edgeconv_param_count", *_arr(layers), ctypes.byref(count))
        own = {k[len(name) + 1:]: v for k, v in P.items() if k.startswith(name + ".")}
        assert count.value == sum(v.size for v in own.values())
        e = fx.EdgeConv(layers, 10).load(own)
        assert np.array_equal(e.flat_params().view(np.uint32), flat[at:at + count.value].view(np.uint32)), name
        at += count.value
    total = ctypes.c_int64(0)
    _lib().call("fx3d_dgcnn_param_count", 10, ctypes.byref(total))
    assert at < total.value == flat.size


def test_the_c_entry_points_refuse_before_any_device_work(fx):
    """NULL pointers, depth, widths, F, K, N and the workspace: the status code itself is compared, and the message names the
    offending value.  No call here has arguments that would pass the check: the dummy pointers are never dereferenced."""
    lib_mod = _lib()
    lib = lib_mod.load()
    dummy = ctypes.c_void_p(4096)
    good, ngood = _arr([5, 33, 70])
    cnt, nb = ctypes.c_int64(0), ctypes.c_size_t(0)

    def fwd(layers=(5, 33, 70), nl=None, K=6, N=65, B=2, params=dummy, x=dummy, out=dummy, ws=dummy, ws_bytes=1 << 40, arr=True):
        la, n = _arr(list(layers))
        return lib.fx3d_edgeconv_forward(params, la if arr else None, n if nl is None else nl, K, x, N, B, None, out, None, ws,
                                         ws_bytes, None)

    def says(*words):
        msg = lib_mod.last_error()
        return all(w in msg for w in words)

    # NULL pointers
    assert lib.fx3d_edgeconv_param_count(good, ngood, None) == INVALID and says("NULL")
    assert lib.fx3d_edgeconv_param_count(None, 3, ctypes.byref(cnt)) == INVALID and says("NULL")
    assert lib.fx3d_edgeconv_workspace_bytes(good, ngood, 6, 65, 2, None) == INVALID and says("NULL")
    assert lib.fx3d_edgeconv_workspace_bytes(None, 3, 6, 65, 2, ctypes.byref(nb)) == INVALID and says("NULL")
    for k in ("params", "x", "out", "ws"):
        assert fwd(**{k: None}) == INVALID and says("NULL"), k
    assert fwd(arr=False) == INVALID and says("NULL")
    # depth: nlayers < 2 or > 5
    for layers in ([5], [5, 8, 8, 8, 8, 8]):
        la, n = _arr(layers)
        assert lib.fx3d_edgeconv_param_count(la, n, ctypes.byref(cnt)) == UNSUPPORTED and says(str(n))
        assert lib.fx3d_edgeconv_workspace_bytes(la, n, 6, 65, 2, ctypes.byref(nb)) == UNSUPPORTED
        assert fwd(layers=layers) == UNSUPPORTED and says(str(n))
    assert fwd(nl=0) == UNSUPPORTED and fwd(nl=-1) == UNSUPPORTED
    # widths of 0 and 257, F = 129 and 0
    for layers, value in (([5, 0, 70], "0"), ([5, 33, 257], "257"), ([129, 8], "129"), ([0, 8], "0"), ([5, -4], "-4")):
        la, n = _arr(layers)
        assert lib.fx3d_edgeconv_param_count(la, n, ctypes.byref(cnt)) == UNSUPPORTED and says(value), layers
        assert lib.fx3d_edgeconv_workspace_bytes(la, n, 6, 65, 2, ctypes.byref(nb)) == UNSUPPORTED and says(value), layers
        assert fwd(layers=layers) == UNSUPPORTED and says(value), layers
    # K = 0, K + 1 > N, N = 36865, B
    for kw, words in ((dict(K=0), ("K", "0")), (dict(K=-2), ("K", "-2")), (dict(K=65), ("K + 1", "66")), (dict(N=36865), ("36865",)),
                      (dict(N=0), ("N=0",)), (dict(B=0), ("B=0",)), (dict(B=65536, N=8), ("65536",)),
                      (dict(N=36864, B=65535, K=1), ("2^31",))):
        assert fwd(**kw) == INVALID and says(*words), kw
        a = dict(K=6, N=65, B=2)
        a.update(kw)
        assert lib.fx3d_edgeconv_workspace_bytes(good, ngood, a["K"], a["N"], a["B"], ctypes.byref(nb)) == INVALID and says(*words), kw
    # the workspace: short, misaligned
    assert lib.fx3d_edgeconv_workspace_bytes(good, ngood, 6, 65, 2, ctypes.byref(nb)) == 0 and nb.value >= 6 * 65 * 2 * 4
    assert fwd(ws_bytes=nb.value - 1) == INVALID and says("workspace", str(nb.value))
    assert fwd(ws=ctypes.c_void_p(4096 + 16)) == INVALID and says("aligned")
    assert nb.value % 256 == 0


def test_python_errors_before_any_launch(fx):
    with pytest.raises(ValueError, match="entries"):
        fx.EdgeConv([5], 3)
    with pytest.raises(ValueError, match="entries"):
        fx.EdgeConv([5, 8, 8, 8, 8, 8], 3)
    with pytest.raises(ValueError, match="257"):
        fx.EdgeConv([5, 33, 257], 3)
    with pytest.raises(ValueError, match="layers\\[1\\]"):
        fx.EdgeConv([5, 0, 8], 3)
    with pytest.raises(ValueError, match="129"):
        fx.EdgeConv([129, 8], 3)
    with pytest.raises(ValueError, match="K"):
        fx.EdgeConv([5, 8], 0)
    with pytest.raises(TypeError):
        fx.EdgeConv([5, 8.5], 3)
    with pytest.raises(TypeError):
        fx.EdgeConv(5, 3)
    with pytest.raises(TypeError):
        fx.EdgeConv([5, "a"], 3)
    layers, K = [5, 33, 70], 6
    m = fx.EdgeConv(layers, K)
    X = np.zeros((5, 65, 2), np.float32)
    with pytest.raises(ValueError, match="5 channels"):
        m(np.zeros((3, 65, 2), np.float32))
    with pytest.raises(ValueError):
        m(np.zeros((5, 65, 2, 1), np.float32))
    with pytest.raises(ValueError, match="K"):
        m(np.zeros((5, 6, 2), np.float32))  # K + 1 > N
    with pytest.raises(ValueError, match="PointCloud"):
        m(fx.PointCloud(np.zeros((3, 65, 2), np.float32)))
    with pytest.raises(fx.Flux3DHipError, match="36865"):
        m(np.zeros((5, 36865), np.float32))
    ok = np.zeros((K, 65, 2), np.int64)
    with pytest.raises(ValueError, match="idx must be"):
        m(X, idx=ok[:, :, :1])
    with pytest.raises(ValueError, match="idx must be"):
        m(X, idx=ok[:5])
    with pytest.raises(TypeError, match="integers"):
        m(X, idx=ok.astype(np.float32))
    for bad in (65, -1, 1 << 40):
        lists = ok.copy()
        lists[2, 7, 1] = bad
        with pytest.raises(ValueError, match="0-based"):
            m(X, idx=lists)
    P = ref.random_params(layers, 0)
    bad = dict(P)
    bad["conv1.weight"] = np.zeros((1, 5, 33), np.float32)  # the first layer takes 2 F channels
    with pytest.raises(ValueError, match="conv1.weight"):
        m.load(bad)
    missing = dict(P)
    del missing["bn2.mu"]
    with pytest.raises(ValueError, match="bn2.mu"):
        m.load(missing)
    extra = dict(P)
    extra["conv3.bias"] = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="conv3.bias"):
        m.load(extra)
    assert m.load(P) is m and np.array_equal(m.params["conv2.weight"], P["conv2.weight"])


def test_the_three_symbols_are_exported(fx):
    from flux3d_jl_amd import models
    lib_mod = _lib()
    lib = lib_mod.load()
    for name in ("fx3d_edgeconv_param_count", "fx3d_edgeconv_workspace_bytes", "fx3d_edgeconv_forward"):
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES, name
    assert fx.EdgeConv is models.EdgeConv
