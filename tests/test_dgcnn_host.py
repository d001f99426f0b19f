"""DGCNN inference, the part that needs no GPU: the host restatement tests/dgcnn_ref.py is what it claims to be (its network
is a DGCNN, cross-checked against an independent evaluation by torch.nn.functional; its "maximum over k" is the reference's
cat / reshape / MaxPool / reshape / permute chain, array operation by array operation), and the library's host-side contract
(parameter count and shapes, load errors, the N == npoints rule)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dgcnn_ref as ref

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _torch_logits(X, idx1, idx2, P, tmp_path):
    """tests/dgcnn_torch_eval.py in a child process (torch stays out of this one, which loads the HIP library): the logits in
    float64 and in float32, with the restatement's neighbours."""
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    np.savez(src, X=X, idx1=idx1, idx2=idx2, **P)
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dgcnn_torch_eval.py"), src, dst],
                   check=True, timeout=600)
    out = np.load(dst)
    return out["logits64"], out["logits32"]


@pytest.mark.parametrize("num_classes", [10, 40])
def test_the_restatement_is_a_dgcnn(num_classes, tmp_path):
    """Logits of the restatement against torch in float64, on the reference's test shape (test/models.jl:24-41).  The bound is
    the one of test_pointnet_host.py: both the restatement and a float32 torch evaluation are Float32 sums in some order, so
    the restatement's error may be at most 8 x torch-float32's.  Both torch runs take the restatement's neighbours."""
    rng = np.random.default_rng(200 + num_classes)
    X = rng.standard_normal((3, 64, 2)).astype(F32)
    P = ref.random_params(num_classes, seed=num_classes)
    r = ref.forward(X, P, 10)
    ref.check_draw(r)
    mine = r["logits"]
    t64, t32 = _torch_logits(X, r["idx1"], r["idx2"], P, tmp_path)
    assert mine.shape == t64.shape == (num_classes, 2)
    scale = float(np.max(np.abs(t64)))
    err_ref = float(np.max(np.abs(mine.astype(np.float64) - t64))) / scale
    err_t32 = float(np.max(np.abs(t32.astype(np.float64) - t64))) / scale
    spread = float(np.max(mine.max(axis=0) - mine.min(axis=0)))
    print(f"num_classes={num_classes}: logits of a cloud at most {spread:.2f} apart; non-zero share of x1 "
          f"{np.count_nonzero(r['x1']) / r['x1'].size:.2f}, of x2 {np.count_nonzero(r['x2']) / r['x2'].size:.2f}; relative error of the "
          f"restatement {err_ref:.3e}, of torch float32 {err_t32:.3e}, ratio {err_ref / err_t32:.2f}")
    assert err_t32 > 0 and err_ref <= 8 * err_t32, (err_ref, err_t32)


def _maxpool_dim1(a, window):
    """MaxPool((window,)) on a (W, C, B) array: windows of `window` along dim 1, stride = window, no padding."""
    W = a.shape[0]
    nw = W // window
    return np.stack([ref.jmax(a[w * window:(w + 1) * window], axis=0) for w in range(nw)], axis=0)


def _edgeconv_literal(X, idx, K, mlp):
    """(m::EdgeConv)(X), src/models/dgcnn.jl:32-71, array operation by array operation on column-major arrays.  X (F, N, B),
    idx (K, N, B) 0-based, mlp: (K N, 2F, B) -> (K N, an, B), a 1x1 convolution chain (each row on its own)."""
    Fd, N, B = X.shape
    col = dict(order="F")
    # KNNGraph: cat over the points of X[:, idxs] (F, K) along dims = 3, over the clouds along dims = 4
    graph = np.stack([np.stack([X[:, idx[:, n, b], b] for n in range(N)], axis=2) for b in range(B)], axis=3)  # (F, K, N, B)
    Xr = np.reshape(X, (Fd, 1, N, B), **col)
    Xr = np.concatenate([Xr for _ in range(K)], axis=1)                    # (F, K, N, B)
    with np.errstate(all="ignore"):
        Xc = np.concatenate([Xr, (graph - Xr).astype(F32)], axis=0)        # (2F, K, N, B)
    Xp = np.transpose(Xc, (1, 2, 0, 3))                                    # PermutedDimsArray(X, (2, 3, 1, 4)): (K, N, 2F, B)
    Xm = np.reshape(Xp, (N * K, 2 * Fd, B), **col)
    Y = mlp(Xm)                                                            # (K N, an, B)
    an = Y.shape[1]
    Y = np.reshape(Y, (K, an * N, B), **col)
    Y = _maxpool_dim1(Y, K)                                                # (1, an N, B)
    Y = np.reshape(Y, (N, an, B), **col)
    return np.transpose(Y, (1, 0, 2))                                      # (an, N, B)


@pytest.mark.parametrize("Fd,N,B,K,an", [(3, 17, 2, 4, 5), (8, 12, 3, 11, 7), (5, 9, 1, 1, 3)])
def test_the_reference_reshapes_are_the_maximum_over_k(Fd, N, B, K, an):
    rng = np.random.default_rng(Fd * 100 + N)
    X = rng.standard_normal((Fd, N, B)).astype(F32)
    idx = ref.self_knn(np.ascontiguousarray(np.transpose(X, (2, 1, 0))), K)
    W = rng.standard_normal((2 * Fd, an)).astype(F32)
    bias = rng.standard_normal(an).astype(F32)

    def rows(e):  # (..., 2F) -> (..., an): one conv + relu, each row on its own
        return ref.relu((ref.contract(e, W) + bias).astype(F32))

    literal = _edgeconv_literal(X, idx, K, lambda Xm: np.transpose(rows(np.transpose(Xm, (2, 0, 1))), (1, 2, 0)))
    assert literal.shape == (an, N, B)
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))
    mine = np.stack([ref.jmax(rows(ref.edge_rows(x[b], idx[:, :, b])), axis=0) for b in range(B)])  # (B, N, an)
    assert np.array_equal(_bits(literal), _bits(np.transpose(mine, (2, 1, 0))))
    # and the rows are the ones fx3d_edge_features / the oracle build for the convolution (layout 1)
    from oracle import oracle
    feats = oracle.edge_features(X, idx, layout=1)  # (K N, 2F, B)
    for b in range(B):
        assert np.array_equal(_bits(feats[:, :, b]), _bits(np.reshape(ref.edge_rows(x[b], idx[:, :, b]), (K * N, 2 * Fd), order="F")))


def _count_from_shapes(num_classes):
    conv = lambda i, o: i * o + o + 4 * o  # noqa: E731  weight, bias, BatchNorm
    return (conv(6, 32) + conv(32, 64) + conv(64, 64) + conv(128, 128) + conv(128, 256) + conv(256, 1024) + conv(1024, 512) +
            conv(512, 256) + 256 * num_classes + num_classes)


@pytest.mark.parametrize("num_classes", [10, 40])
def test_param_count_and_shapes(fx, num_classes):
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.models import dgcnn_param_shapes
    count = ctypes.c_int64(0)
    _lib.call("fx3d_dgcnn_param_count", num_classes, ctypes.byref(count))
    assert count.value == _count_from_shapes(num_classes)
    m = fx.DGCNN(num_classes, 10, 64)
    want = ref.param_shapes(num_classes)
    assert list(m.params) == list(want) == list(dgcnn_param_shapes(num_classes))
    assert {k: v.shape for k, v in m.params.items()} == want
    assert all(v.dtype == np.float32 for v in m.params.values())
    flat = m.flat_params()
    assert flat.size == count.value == m.param_count and flat.dtype == np.float32
    # conv W (Cin, Cout) column-major: element [c, o] of the first layer at c + 6 o
    assert flat[4 + 6 * 7] == m.params["ec1.conv1.weight"][0, 4, 7]
    assert np.all(m.params["ec2.bn1.gamma"] == 1) and np.all(m.params["ec2.bn1.mu"] == 0) and np.all(m.params["ec2.bn1.sigma2"] == 1)
    assert not np.array_equal(fx.DGCNN(num_classes, 10, 64, seed=1).params["fc6.weight"], m.params["fc6.weight"])
    assert (m.num_classes, m.K, m.npoints) == (num_classes, 10, 64)
    d = fx.DGCNN()
    assert (d.num_classes, d.K, d.npoints) == (10, 10, 1024)
    cnt = ctypes.c_int64(0)
    lib = _lib.load()
    assert lib.fx3d_dgcnn_param_count(0, ctypes.byref(cnt)) != 0 and lib.fx3d_dgcnn_param_count(10, None) != 0


def test_python_errors_before_any_launch(fx):
    with pytest.raises(ValueError):
        fx.DGCNN(0)
    with pytest.raises(ValueError, match="K"):
        fx.DGCNN(10, 0, 64)
    with pytest.raises(ValueError, match="K"):
        fx.DGCNN(10, 64, 64)
    m = fx.DGCNN(10, 10, 64)
    with pytest.raises(ValueError, match="npoints"):
        m(np.zeros((3, 65, 2), np.float32))  # MaxPool((npoints,)) is the maximum over a cloud only for N == npoints
    with pytest.raises(ValueError, match="npoints"):
        m(np.zeros((3, 128, 2), np.float32))
    with pytest.raises(ValueError, match="3 channels"):
        m(np.zeros((2, 64, 2), np.float32))
    with pytest.raises(ValueError):
        m(np.zeros((3, 64, 2, 1), np.float32))
    P = ref.random_params(10, 0)
    bad = dict(P)
    bad["fc6.weight"] = np.zeros((256, 10), np.float32)  # Flux keeps Dense weights as (out, in)
    with pytest.raises(ValueError, match="fc6.weight"):
        m.load(bad)
    bad = dict(P)
    bad["ec1.conv1.weight"] = np.zeros((1, 3, 32), np.float32)  # the first layer of an EdgeConv takes 2 F channels
    with pytest.raises(ValueError, match="ec1.conv1.weight"):
        m.load(bad)
    missing = dict(P)
    del missing["ec2.bn2.mu"]
    with pytest.raises(ValueError, match="ec2.bn2.mu"):
        m.load(missing)
    assert m.load(P) is m and np.array_equal(m.params["conv3.conv.weight"], P["conv3.conv.weight"])


def test_null_pointers_and_bad_sizes_are_refused_before_any_device_work(fx):
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    assert lib.fx3d_dgcnn_forward(None, 10, 10, None, 64, 2, None, None, None, None, None, None, None, None, 0, None) != 0
    assert "NULL" in _lib.last_error()
    dummy = ctypes.c_void_p(4096)
    for N, B, K, nc in ((0, 2, 10, 10), (64, 0, 10, 10), (64, 2, 0, 10), (64, 2, 64, 10), (64, 2, 10, 0), (40000, 1, 10, 10)):
        rc = lib.fx3d_dgcnn_forward(dummy, nc, K, dummy, N, B, dummy, None, None, None, None, None, None, dummy, 1 << 40, None)
        assert rc != 0, (N, B, K, nc)
