"""DGCNN inference on the device (fx3d_dgcnn_forward through fx.DGCNN) against the host restatement tests/dgcnn_ref.py: both
neighbour lists, both EdgeConv outputs, the pooled feature and the logits bit for bit (uint32 views, no element left out), the
probabilities within 1e-5 relative of the Float64 softmax of the device's own logits -- for the reference's test shape,
partial tiles and small clouds, K up to N - 1 and beyond the matrix-core search's 32, ModelNet size, NaN input, all-negative
channels, a captured graph and host arrays; every way of giving or leaving out the optional outputs; the C entry points'
status codes and the workspace bound.

Every draw of parameters is first held to dgcnn_ref.check_draw on the restatement's own arrays (the relu leaves at least half
of x1 and x2 alive, every probability lies in [1e-4, 1 - 1e-4]), so that what is compared has something in it."""
import ctypes

import numpy as np
import pytest

import dgcnn_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
BITWISE = ("idx1", "x1", "idx2", "x2", "pooled", "logits")


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype == np.int32 else a.astype(F32, copy=False)).view(np.uint32)


def _host(out):
    return {k: (v.to_host() if hasattr(v, "to_host") else np.asarray(v)) for k, v in out.items()}


def _model(fx, num_classes, K, N, seed):
    P = ref.random_params(num_classes, seed)
    return fx.DGCNN(num_classes, K, N).load(P), P


def _cloud(seed, N, B):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((3, N, B)).astype(F32))


def _check_probs(got, num_classes, B):
    assert got["probs"].shape == (num_classes, B)
    want = ref.softmax64(got["logits"])
    rel = float(np.max(np.abs(got["probs"].astype(np.float64) - want) / want))
    spread = float(np.max(got["logits"].max(axis=0) - got["logits"].min(axis=0)))
    print(f"probabilities: largest relative deviation from the Float64 softmax {rel:.3e}; smallest probability {want.min():.3e}, "
          f"logits of a cloud at most {spread:.2f} apart, {np.unique(got['probs']).size} distinct values of {want.size}")
    assert want.min() >= 1e-4 and want.max() <= 1 - 1e-4, (want.min(), want.max())
    assert rel <= 1e-5, rel


def _check_against_ref(got, X, P, K, clouds=None, what="", draw=True):
    """got: host arrays of forward(intermediates=True) for the batch X; clouds: which of them to restate (default all)."""
    B = X.shape[2]
    clouds = list(range(B)) if clouds is None else clouds
    want = ref.forward(np.ascontiguousarray(X[:, :, clouds]), P, K)
    if draw:
        ref.check_draw(want)
    for k in BITWISE:
        g = got[k][..., clouds]
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, (what, k, g.shape, want[k].shape, g.dtype)
        bad = np.flatnonzero(_bits(g).ravel() != _bits(want[k]).ravel())
        print(f"{what} {k}: {bad.size} of {g.size} elements differ from the restatement")
        assert bad.size == 0, (what, k, bad[:5], g.ravel()[bad[:5]], want[k].ravel()[bad[:5]])
    return want


@pytest.mark.parametrize("num_classes", [10, 40])
def test_reference_test_shape(gpu_fx, num_classes):
    """test/models.jl:24-41: DGCNN(num_classes, 10, 64) on a (3, 64, 2) batch gives (num_classes, 2)."""
    m, P = _model(gpu_fx, num_classes, 10, 64, seed=num_classes)
    X = _cloud(1, 64, 2)
    got = _host(m.forward(gpu_fx.gpu(X), intermediates=True))
    _check_against_ref(got, X, P, 10, what=f"(3,64,2) nc={num_classes}")
    _check_probs(got, num_classes, 2)
    assert m(gpu_fx.gpu(X)).shape == (num_classes, 2)


def small_cloud_ks(N):
    """K = 1, the reference's 10 (or all there are), and every other point of the cloud where the restatement of K N rows per
    cloud is affordable on the host (N <= 100)."""
    ks = {1, min(10, N - 1)}
    if N <= 100:
        ks.add(N - 1)
    return sorted(ks)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [2, 3, 63, 65, 100, 1000])
def test_partial_tiles_and_small_clouds(gpu_fx, N, B):
    for K in small_cloud_ks(N):
        m, P = _model(gpu_fx, 3, K, N, seed=3)
        X = _cloud(N * 10 + B, N, B)
        got = _host(m.forward(gpu_fx.gpu(X), intermediates=True))
        _check_against_ref(got, X, P, K, what=f"N={N} B={B} K={K}")
        _check_probs(got, 3, B)


@pytest.mark.parametrize("K", [20, 40])
def test_k_20_and_beyond_the_matrix_core_search(gpu_fx, K):
    """K + 1 = 41 is more than the 32 the matrix-core search selects: the wide routes of fx3d_knn_ws."""
    m, P = _model(gpu_fx, 10, K, 256, seed=K)
    X = _cloud(K, 256, 2)
    got = _host(m.forward(gpu_fx.gpu(X), intermediates=True))
    _check_against_ref(got, X, P, K, what=f"N=256 K={K}")
    _check_probs(got, 10, 2)


def test_modelnet_size(gpu_fx):
    fx = gpu_fx
    m, P = _model(fx, 40, 20, 1024, seed=40)
    X = _cloud(2, 1024, 32)
    xd = fx.gpu(X)
    got = _host(m.forward(xd, intermediates=True))
    _check_against_ref(got, X, P, 20, clouds=[0, 31], what="(3,1024,32)")
    _check_probs(got, 40, 32)
    again = _host(m.forward(xd, intermediates=True))
    for k in BITWISE + ("probs",):
        assert np.array_equal(_bits(again[k]), _bits(got[k])), f"{k}: two runs differ"
    for b in range(32):
        alone = _host(m.forward(fx.gpu(np.asfortranarray(X[:, :, b:b + 1])), intermediates=True))
        for k in BITWISE + ("probs",):
            assert np.array_equal(_bits(alone[k][..., 0]), _bits(got[k][..., b])), f"cloud {b} alone: {k} differs from its batch"


def test_nan_stays_in_its_cloud(gpu_fx):
    fx = gpu_fx
    m, P = _model(fx, 10, 10, 100, seed=10)
    X = _cloud(5, 100, 3)
    clean = _host(m.forward(fx.gpu(X), intermediates=True))
    Xn = X.copy(order="F")
    Xn[1, 37, 1] = np.nan
    got = _host(m.forward(fx.gpu(Xn), intermediates=True))
    assert np.all(np.isnan(got["x1"][:, 37, 1])) and np.all(np.isnan(got["x2"][:, 37, 1]))  # the point itself, at the least
    for k in ("pooled", "logits", "probs"):
        assert np.all(np.isnan(got[k][..., 1])), f"{k} of the NaN cloud"
    for k in ("idx1", "idx2"):
        assert got[k].min() >= 0 and got[k].max() < 100  # a NaN distance sorts last: every index is a point of the cloud
    for k in BITWISE + ("probs",):
        for b in (0, 2):
            assert np.array_equal(_bits(got[k][..., b]), _bits(clean[k][..., b])), f"{k} of cloud {b} changed"


def test_all_negative_channels_give_plus_zero(gpu_fx):
    """Channel 5 of the last layer of EdgeConv1 and channel 9 of EdgeConv2's have a BatchNorm output of -1 on every edge row
    (zero weights, bias = mu, beta = -1): relu gives +0.0 and the maximum over k keeps it, in x1 and x2 themselves.  Channels 7
    and 11 of conv_3 likewise: pooled holds +0.0 there."""
    fx = gpu_fx
    P = ref.random_params(10, seed=11)
    X = _cloud(6, 65, 2)
    base = ref.forward(X, P, 10)  # the draw as it is: these channels are alive, so the zeros below come from the change alone
    assert np.count_nonzero(base["x1"][5]) and np.count_nonzero(base["x2"][9])
    assert np.count_nonzero(base["pooled"][7]) and np.count_nonzero(base["pooled"][11])
    for layer, bn, chans in (("ec1.conv3", "ec1.bn3", (5,)), ("ec2.conv2", "ec2.bn2", (9,)), ("conv3.conv", "conv3.bn", (7, 11))):
        for ch in chans:
            P[layer + ".weight"][0, :, ch] = 0
            P[layer + ".bias"][ch] = P[bn + ".mu"][ch]
            P[bn + ".beta"][ch] = -1
    m = fx.DGCNN(10, 10, 65).load(P)
    got = _host(m.forward(fx.gpu(X), intermediates=True))
    want = _check_against_ref(got, X, P, 10, what="zero channels")
    assert np.all(_bits(want["ec1"][..., 5]) == 0) and np.all(_bits(want["ec2"][..., 9]) == 0)  # +0.0, sign bit clear
    assert np.all(_bits(got["x1"][5]) == 0) and np.all(_bits(got["x2"][9]) == 0)
    assert np.all(_bits(got["pooled"][7]) == 0) and np.all(_bits(got["pooled"][11]) == 0)


def test_graph_replay_and_numpy_in_numpy_out(gpu_fx):
    fx = gpu_fx
    m, P = _model(fx, 10, 10, 200, seed=12)
    X = _cloud(8, 200, 2)
    out = m.forward(X, intermediates=True)  # numpy in, numpy out
    assert all(isinstance(v, np.ndarray) for v in out.values())
    assert out["idx1"].dtype == np.int32 and out["idx2"].dtype == np.int32
    eager = _host(m.forward(fx.gpu(X), intermediates=True))
    for k in BITWISE + ("probs",):
        assert np.array_equal(_bits(out[k]), _bits(eager[k])), k
    m1 = fx.DGCNN(10, 10, 200).load(P)
    one = m1(X[:, :, 0])  # (3, N): one cloud
    assert isinstance(one, np.ndarray) and one.shape == (10, 1) and np.array_equal(_bits(one[:, 0]), _bits(eager["probs"][:, 0]))
    pc = m(fx.PointCloud(fx.gpu(X)))
    assert np.array_equal(_bits(pc.to_host()), _bits(eager["probs"]))
    s = fx.Stream.create()
    with fx.stream(s):
        xd = fx.gpu(X)
        m.forward(xd, intermediates=True)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec = m.forward(xd, intermediates=True)
        g.launch()
        g.launch()
        s.synchronize()
        replay = _host(rec)
    for k in BITWISE + ("probs",):
        assert np.array_equal(_bits(replay[k]), _bits(eager[k])), f"{k}: graph replay differs from the eager run"


def test_status_codes(gpu_fx):
    """Every bad argument is FX3D_ERR_INVALID_ARG (-1 would be any error: the code itself is compared) before any launch."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    lib = _lib.load()
    INVALID = lib.fx3d_dgcnn_param_count(0, ctypes.byref(ctypes.c_int64(0)))
    assert INVALID != 0
    N, B, K, nc = 64, 2, 10, 10
    m, _ = _model(fx, nc, K, N, seed=1)
    x = fx.gpu(_cloud(1, N, B))
    probs = DeviceArray.empty((nc, B), np.float32)
    nb = ctypes.c_size_t(0)
    assert lib.fx3d_dgcnn_workspace_bytes(N, B, K, nc, ctypes.byref(nb)) == 0 and nb.value > 0
    ws = DeviceArray.empty((nb.value + 512,), np.uint8)
    assert ws.ptr % 256 == 0
    pd = m._params_dev()

    def call(params=pd.ptr, nc_=nc, K_=K, x_=x.ptr, N_=N, B_=B, probs_=probs.ptr, ws_=ws.ptr, bytes_=nb.value):
        return lib.fx3d_dgcnn_forward(params, nc_, K_, x_, N_, B_, probs_, None, None, None, None, None, None, ws_, bytes_, None)

    assert call() == 0
    fx.synchronize()
    assert call(params=None) == INVALID and call(x_=None) == INVALID and call(probs_=None) == INVALID and call(ws_=None) == INVALID
    assert call(K_=0) == INVALID and call(K_=-3) == INVALID
    assert call(K_=N) == INVALID and "K + 1" in _lib.last_error()          # K + 1 > N
    assert call(N_=0) == INVALID and call(B_=0) == INVALID and call(nc_=0) == INVALID
    assert call(N_=36865) == INVALID and "neighbour search" in _lib.last_error()
    assert call(bytes_=nb.value - 1) == INVALID and "workspace" in _lib.last_error()
    assert call(ws_=ws.ptr + 16) == INVALID and "aligned" in _lib.last_error()
    for args in ((0, B, K, nc), (N, 0, K, nc), (N, B, 0, nc), (N, B, N, nc), (N, B, K, 0), (36865, 1, K, nc)):
        assert lib.fx3d_dgcnn_workspace_bytes(*args, ctypes.byref(nb)) == INVALID, args
    assert lib.fx3d_dgcnn_workspace_bytes(N, B, K, nc, None) == INVALID


@pytest.mark.parametrize("N,B,K", [(65, 2, 3), (2, 1, 1)])
def test_every_subset_of_optional_outputs(gpu_fx, N, B, K):
    """fx3d_dgcnn_forward with no optional output, with each of logits, idx1, x1, idx2, x2, pooled given alone, and with all of
    them: whatever is not given lives in the workspace (or, the neighbour lists, in the EdgeConv stage's own), and nothing of the
    result may depend on which it is.  probs is the same uint32 array in all eight calls, and each output given alone is the one
    of the all-given call bit for bit.  A partial second tile (65 points) and the smallest legal cloud (2 points, K = 1).  Every
    output array starts as all-ones bits (a NaN, index -1), so that an array the call left alone cannot pass."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    nc = 5
    m, _ = _model(fx, nc, K, N, seed=7)
    x = fx.gpu(_cloud(N + K, N, B))
    shapes = {"logits": ((nc, B), F32), "idx1": ((K, N, B), np.int32), "x1": ((64, N, B), F32), "idx2": ((K, N, B), np.int32),
              "x2": ((256, N, B), F32), "pooled": ((1024, B), F32)}
    ws = DeviceArray.empty((_lib.query_bytes("fx3d_dgcnn_workspace_bytes", N, B, K, nc),), np.uint8)
    assert ws.ptr % 256 == 0

    def run(given):
        blank = lambda shape, dtype: DeviceArray.from_host(np.full(shape, -1, np.int32).view(dtype))  # noqa: E731
        out = {k: blank(*shapes[k]) for k in given}
        probs = blank((nc, B), F32)
        _lib.call("fx3d_dgcnn_forward", m._params_dev().ptr, nc, K, x.ptr, N, B, probs.ptr,
                  *[out[k].ptr if k in out else None for k in shapes], ws.ptr, ws.nbytes, None)
        fx.synchronize()
        return _bits(probs.to_host()), {k: _bits(v.to_host()) for k, v in out.items()}

    probs_none, _ = run(())
    assert not np.any(probs_none == 0xFFFFFFFF)
    alone = {}
    for k in shapes:
        probs, out = run((k,))
        assert np.array_equal(probs, probs_none), f"probs with {k} given differ from probs with nothing given"
        alone[k] = out[k]
    probs, every = run(tuple(shapes))
    assert np.array_equal(probs, probs_none), "probs with every output given differ from probs with nothing given"
    for k in shapes:
        assert alone[k].shape == every[k].shape and np.array_equal(alone[k], every[k]), f"{k} given alone differs from the all-given call"
        assert not np.any(every[k] == 0xFFFFFFFF), f"{k}: elements the call did not write"


def test_workspace_is_smaller_than_the_edge_tensor(gpu_fx):
    """What the path must hold at 32 x 1024, K = 20: x1 (8 MB), x2 (34 MB), two index arrays (5 MB), tile maxima (2 MB) and
    the search's scratch -- about 50 MB.  The (K N, 128, B) input of EdgeConv2's convolutions alone is 335 MB: a path that
    materialises it cannot stay under the bound."""
    from flux3d_jl_amd import _lib
    nb = ctypes.c_size_t(0)
    _lib.call("fx3d_dgcnn_workspace_bytes", 1024, 32, 20, 40, ctypes.byref(nb))
    print(f"fx3d_dgcnn_workspace_bytes(1024, 32, 20, 40) = {nb.value} bytes")
    assert 4 * (64 + 256) * 1024 * 32 <= nb.value < 4 * 20 * 1024 * 128 * 32, nb.value
