"""PointNet inference on the device (fx3d_pointnet_forward through fx.PointNet) against the host restatement
tests/pointnet_ref.py: logits, both transforms and the pooled feature bit for bit (uint32 views), the probabilities within
1e-5 relative of the Float64 softmax of the device's own logits, for the reference's test shape, partial tiles, single
points and clouds, ModelNet size, NaN input, all-negative channels, a captured graph and host arrays."""
import numpy as np
import pytest

import pointnet_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
BITWISE = ("logits", "stn", "fstn", "pooled")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _host(out):
    return {k: (v.to_host() if hasattr(v, "to_host") else np.asarray(v)) for k, v in out.items()}


def _model(fx, num_classes, seed):
    P = ref.random_params(num_classes, seed)
    return fx.PointNet(num_classes).load(P), P


def _cloud(seed, N, B):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((3, N, B)).astype(F32))


def _check_probs(got, num_classes, B):
    assert got["probs"].shape == (num_classes, B)
    want = ref.softmax64(got["logits"])
    rel = float(np.max(np.abs(got["probs"].astype(np.float64) - want) / want))
    spread = float(np.max(got["logits"].max(axis=0) - got["logits"].min(axis=0)))
    print(f"probabilities: largest relative deviation from the Float64 softmax {rel:.3e}; smallest probability {want.min():.3e}, "
          f"logits of a cloud at most {spread:.2f} apart, {np.unique(got['probs']).size} distinct values of {want.size}")
    # the weights of random_params keep a cloud's logits a few units apart: every probability is a normal number well inside
    # (0, 1), so the exponentials, their sum in class order and the division all take part in what is compared
    if num_classes > 1:
        assert want.min() >= 1e-4 and want.max() <= 1 - 1e-4, (want.min(), want.max())
        alive = int(np.count_nonzero(got["logits"] > 0))  # (the classes the relu zeroed share one probability per cloud)
        assert alive * 8 >= want.size and np.unique(got["probs"]).size >= alive, (alive, np.unique(got["probs"]).size)
    assert rel <= 1e-5, rel


def _check_against_ref(got, X, P, clouds=None, what=""):
    """got: host arrays of forward(intermediates=True) for the batch X; clouds: which of them to restate (default all)."""
    B = X.shape[2]
    clouds = list(range(B)) if clouds is None else clouds
    want = ref.forward(np.ascontiguousarray(X[:, :, clouds]), P)
    for k in BITWISE:
        g = got[k][..., clouds]
        assert g.shape == want[k].shape, (what, k, g.shape, want[k].shape)
        bad = np.flatnonzero(_bits(g).ravel() != _bits(want[k]).ravel())
        print(f"{what} {k}: {bad.size} of {g.size} elements differ from the restatement")
        assert bad.size == 0, (what, k, bad[:5], g.ravel()[bad[:5]], want[k].ravel()[bad[:5]])
    return want


@pytest.mark.parametrize("num_classes", [10, 40])
def test_reference_test_shape(gpu_fx, num_classes):
    """test/models.jl:5-22: PointNet(num_classes) on a (3, 64, 2) batch gives (num_classes, 2)."""
    m, P = _model(gpu_fx, num_classes, seed=num_classes)
    X = _cloud(1, 64, 2)
    got = _host(m.forward(gpu_fx.gpu(X), intermediates=True))
    want = _check_against_ref(got, X, P, what=f"(3,64,2) nc={num_classes}")
    assert np.count_nonzero(want["logits"] > 0) * 8 >= want["logits"].size  # the relu before the softmax leaves something
    _check_probs(got, num_classes, 2)
    assert m(gpu_fx.gpu(X)).shape == (num_classes, 2)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 2, 63, 65, 100, 1000])
def test_partial_tiles_and_one_class(gpu_fx, N, B):
    m, P = _model(gpu_fx, 1, seed=3)
    X = _cloud(N * 10 + B, N, B)
    got = _host(m.forward(gpu_fx.gpu(X), intermediates=True))
    _check_against_ref(got, X, P, what=f"N={N} B={B}")
    _check_probs(got, 1, B)
    assert np.all(got["probs"] == 1.0)


def test_modelnet_size(gpu_fx):
    fx = gpu_fx
    m, P = _model(fx, 40, seed=40)
    X = _cloud(2, 1024, 32)
    xd = fx.gpu(X)
    got = _host(m.forward(xd, intermediates=True))
    _check_against_ref(got, X, P, clouds=[0, 31], what="(3,1024,32)")
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
    m, P = _model(fx, 10, seed=10)
    X = _cloud(5, 100, 3)
    clean = _host(m.forward(fx.gpu(X), intermediates=True))
    Xn = X.copy(order="F")
    Xn[1, 37, 1] = np.nan
    got = _host(m.forward(fx.gpu(Xn), intermediates=True))
    for k in BITWISE + ("probs",):
        assert np.all(np.isnan(got[k][..., 1])), f"{k} of the NaN cloud"
        for b in (0, 2):
            assert np.array_equal(_bits(got[k][..., b]), _bits(clean[k][..., b])), f"{k} of cloud {b} changed"


def test_all_negative_channels_give_plus_zero(gpu_fx):
    """Channel 5 of feat.conv1 has pre-activation -1 at every point: +0.0 after the relu.  Channels 7 and 9 of feat.conv2 are
    +0.0 and -0.0 at every point after BatchNorm: the maximum over the points keeps the sign of the zero.  (A contraction
    starts from +0.0, so a pre-activation of -0.0 cannot arise; an all-negative one can.)  The relu's +0.0 is asserted on
    the restatement's intermediate (a host array; the device does not return that layer) and reaches the device only through
    the bit identity of everything downstream; the signed zeros of the maximum are asserted on the device's `pooled`."""
    fx = gpu_fx
    P = ref.random_params(10, seed=11)
    P["feat.conv1.weight"][0, :, 5] = 0
    P["feat.conv1.bias"][5] = -1
    for ch, gamma in ((7, 1.0), (9, -1.0)):
        P["feat.conv2.weight"][0, :, ch] = 0
        P["feat.conv2.bias"][ch] = -2
        P["feat.bn2.mu"][ch], P["feat.bn2.gamma"][ch], P["feat.bn2.beta"][ch] = -2, gamma, 0.0 if gamma > 0 else -0.0
    m = fx.PointNet(10).load(P)
    X = _cloud(6, 65, 2)
    got = _host(m.forward(fx.gpu(X), intermediates=True))
    want = _check_against_ref(got, X, P, what="zero channels")
    assert np.all(_bits(want["feat_relu1"][:, :, 5]) == 0)  # +0.0, sign bit clear
    assert np.all(_bits(got["pooled"][7]) == 0) and np.all(_bits(got["pooled"][9]) == 0x80000000)


def test_graph_replay_and_numpy_in_numpy_out(gpu_fx):
    fx = gpu_fx
    m, P = _model(fx, 10, seed=12)
    X = _cloud(8, 200, 2)
    out = m.forward(X, intermediates=True)  # numpy in, numpy out
    assert all(isinstance(v, np.ndarray) for v in out.values())
    eager = _host(m.forward(fx.gpu(X), intermediates=True))
    for k in BITWISE + ("probs",):
        assert np.array_equal(_bits(out[k]), _bits(eager[k])), k
    one = m(X[:, :, 0])  # (3, N): one cloud
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
