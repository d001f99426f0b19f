"""The PointNet training-mode forward on the device (fx3d_pointnet_forward_train through fx.PointNet.forward_train) against the
host restatement tests/pointnet_train_ref.py: logits, both transforms, the pooled feature, every batch statistic and every
updated running statistic bit for bit (uint32 views), the probabilities within 1e-5 relative of the Float64 softmax of the
device's own logits.  Shapes: one point per cloud, a partial single tile, a tile boundary, a partial last tile of several, an
odd number of clouds.  Then what needs no restatement: the test-mode forward at the returned statistics gives the same bits;
the running statistics in the parameters enter nothing but `running`; dropout masks; momentum and update=True; a captured
graph; a NaN that reaches every cloud."""
import numpy as np
import pytest

import pointnet_ref as ref
import pointnet_train_ref as tref

pytestmark = pytest.mark.gpu

F32 = np.float32
BITWISE = ("logits", "stn", "fstn", "pooled")
STATS = ("batch_stats", "running")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _host(out):
    def one(v):
        if isinstance(v, dict):
            return {k: one(w) for k, w in v.items()}
        return v.to_host() if hasattr(v, "to_host") else np.asarray(v)
    return one(out)


def _cloud(seed, N, B):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((3, N, B)).astype(F32))


_PARAMS, _WANT = {}, {}


def _params(num_classes, seed):
    """random_params: random running statistics too, so a kernel that wrongly reads them shows up.  Shared, never modified."""
    if (num_classes, seed) not in _PARAMS:
        _PARAMS[(num_classes, seed)] = ref.random_params(num_classes, seed)
    return _PARAMS[(num_classes, seed)]


def _want(key, X, P, dropout=None, momentum=0.1):
    """The restatement's run, computed once per key and shared among the tests (never modified)."""
    if key not in _WANT:
        _WANT[key] = tref.forward_train(X, P, dropout=dropout, momentum=momentum)
    return _WANT[key]


def _check_probs(got, num_classes, B):
    """As tests/test_gpu_pointnet.py::_check_probs."""
    assert got["probs"].shape == (num_classes, B)
    want = ref.softmax64(got["logits"])
    rel = float(np.max(np.abs(got["probs"].astype(np.float64) - want) / want))
    spread = float(np.max(got["logits"].max(axis=0) - got["logits"].min(axis=0)))
    print(f"probabilities: largest relative deviation from the Float64 softmax {rel:.3e}; smallest probability {want.min():.3e}, "
          f"logits of a cloud at most {spread:.2f} apart, {np.unique(got['probs']).size} distinct values of {want.size}")
    assert want.min() >= 1e-4 and want.max() <= 1 - 1e-4, (want.min(), want.max())
    alive = int(np.count_nonzero(got["logits"] > 0))
    assert alive * 8 >= want.size and np.unique(got["probs"]).size >= alive, (alive, np.unique(got["probs"]).size)
    assert rel <= 1e-5, rel


def _check_against_ref(got, want, what="", keys=BITWISE, stats=STATS):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.flatnonzero(_bits(got[k]).ravel() != _bits(want[k]).ravel())
        print(f"{what} {k}: {bad.size} of {got[k].size} elements differ from the restatement")
        assert bad.size == 0, (what, k, bad[:5], got[k].ravel()[bad[:5]], want[k].ravel()[bad[:5]])
    for s in stats:
        assert list(got[s]) == list(want[s]) == [f"{bn}.{f}" for bn in tref.BN_ORDER for f in ("mu", "sigma2")]
        for name, w in want[s].items():
            g = got[s][name]
            assert g.shape == w.shape, (what, s, name)
            bad = np.flatnonzero(_bits(g) != _bits(w))
            assert bad.size == 0, (what, s, name, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])
        print(f"{what} {s}: all {sum(v.size for v in want[s].values())} values equal the restatement's")


def _same_bits(a, b, what, keys=BITWISE + ("probs",), stats=STATS):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"
    for s in stats:
        for name in a[s]:
            assert np.array_equal(_bits(a[s][name]), _bits(b[s][name])), f"{what}: {s}[{name}] differs"


@pytest.mark.parametrize("N,B,num_classes", [(1, 2, 10), (2, 2, 10), (63, 3, 10), (65, 2, 10), (100, 3, 10), (130, 2, 10),
                                             (1000, 3, 40)])
def test_parity_with_the_restatement(gpu_fx, N, B, num_classes):
    fx = gpu_fx
    P = _params(num_classes, seed=num_classes)
    m = fx.PointNet(num_classes).load(P)
    X = _cloud(N * 10 + B, N, B)
    got = _host(m.forward_train(fx.gpu(X), intermediates=True))
    want = _want(("parity", N, B, num_classes), X, P)
    _check_against_ref(got, want, what=f"N={N} B={B} nc={num_classes}")
    _check_probs(got, num_classes, B)
    probs = m.forward_train(fx.gpu(X))
    assert np.array_equal(_bits(probs.to_host()), _bits(got["probs"]))


def test_test_mode_forward_at_the_batch_statistics_gives_the_same_bits(gpu_fx):
    fx = gpu_fx
    P = _params(10, seed=21)
    X = _cloud(22, 100, 3)
    xd = fx.gpu(X)
    got = _host(fx.PointNet(10).load(P).forward_train(xd, dropout=None, intermediates=True))
    Q = dict(P)
    Q.update(got["batch_stats"])
    assert any(not np.array_equal(Q[k], P[k]) for k in got["batch_stats"])
    test_mode = _host(fx.PointNet(10).load(Q).forward(xd, intermediates=True))
    for k in BITWISE + ("probs",):
        assert np.array_equal(_bits(test_mode[k]), _bits(got[k])), f"{k}: the test-mode forward at the batch statistics differs"


def test_running_statistics_of_the_parameters_enter_running_only(gpu_fx):
    fx = gpu_fx
    P = _params(10, seed=23)
    Q = dict(P)
    rng = np.random.default_rng(24)
    for k in P:
        if k.endswith(".mu"):
            Q[k] = rng.standard_normal(P[k].shape).astype(F32)
        elif k.endswith(".sigma2"):
            Q[k] = rng.uniform(0.1, 5.0, P[k].shape).astype(F32)
    xd = fx.gpu(_cloud(25, 65, 2))
    a = _host(fx.PointNet(10).load(P).forward_train(xd, dropout=3, intermediates=True))
    b = _host(fx.PointNet(10).load(Q).forward_train(xd, dropout=3, intermediates=True))
    _same_bits(a, b, "other running statistics", stats=("batch_stats",))
    assert all(not np.array_equal(a["running"][k], b["running"][k]) for k in a["running"])


def test_dropout_masks(gpu_fx):
    """A seeded mask against the restatement; all ones is the identity; a zero column makes cloud b's dropped activations
    zero, so its BatchNorm input is 0 in every channel, as the restatement says; and with every column zero the batch mean
    and variance are 0, BatchNorm gives beta, and every cloud's logits are relu(cls(beta))."""
    fx = gpu_fx
    P = _params(10, seed=26)
    m = fx.PointNet(10).load(P)
    N, B = 65, 3
    X = _cloud(27, N, B)
    xd = fx.gpu(X)
    mask = fx.PointNet.dropout_mask(B, seed=5)
    got = _host(m.forward_train(xd, dropout=mask, intermediates=True))
    want = _want(("dropout", "seeded"), X, P, dropout=mask)
    _check_against_ref(got, want, what="seeded mask")
    assert not np.array_equal(want["feat_drop"], _want(("dropout", "none"), X, P)["feat_drop"])
    by_seed = _host(m.forward_train(xd, dropout=5, intermediates=True))
    on_dev = _host(m.forward_train(xd, dropout=fx.gpu(mask), intermediates=True))
    _same_bits(by_seed, got, "dropout=5 against dropout_mask(B, 5)")
    _same_bits(on_dev, got, "a device mask")
    plain = _host(m.forward_train(xd, dropout=None, intermediates=True))
    ones = _host(m.forward_train(xd, dropout=np.ones((256, B), F32), intermediates=True))
    _same_bits(ones, plain, "all ones against None")
    _check_against_ref(plain, _want(("dropout", "none"), X, P), what="no mask")
    col = np.asfortranarray(mask.copy())
    col[:, 1] = 0
    got = _host(m.forward_train(xd, dropout=col, intermediates=True))
    want = _want(("dropout", "column"), X, P, dropout=col)
    assert not want["feat_drop"][1].any() and want["feat_drop"][0].any()
    _check_against_ref(got, want, what="zero column")
    got = _host(m.forward_train(xd, dropout=np.zeros((256, B), F32), intermediates=True))
    _check_against_ref(got, _want(("dropout", "zeros"), X, P, dropout=np.zeros((256, B), F32)), what="all zero")
    assert not got["batch_stats"]["feat.bn4.mu"].any() and not got["batch_stats"]["feat.bn4.sigma2"].any()
    beta_only = ref.relu(ref.dense(np.asarray(P["feat.bn4.beta"], F32)[None, :], P, "cls"))[0]
    for b in range(B):
        assert np.array_equal(_bits(got["logits"][:, b]), _bits(beta_only)), b


@pytest.mark.parametrize("N,B", [(1, 2), (65, 2)])
@pytest.mark.parametrize("momentum", [0.1, 0.5])
def test_momentum_and_update(gpu_fx, N, B, momentum):
    fx = gpu_fx
    P = _params(10, seed=28)
    m = fx.PointNet(10).load(P)
    X = _cloud(29 + N, N, B)
    xd = fx.gpu(X)
    got = _host(m.forward_train(xd, momentum=momentum, update=True, intermediates=True))
    want = _want(("momentum", N, B, momentum), X, P, momentum=momentum)
    _check_against_ref(got, want, what=f"momentum={momentum} N={N}")
    # the model now holds the running statistics, on the host and on the device
    for name, v in got["running"].items():
        assert np.array_equal(_bits(m.params[name]), _bits(v)), name
    assert all(np.array_equal(m.params[k], P[k]) for k in P if not k.endswith((".mu", ".sigma2")))
    after = _host(m.forward(xd, intermediates=True))
    Q = dict(P)
    Q.update(got["running"])
    loaded = _host(fx.PointNet(10).load(Q).forward(xd, intermediates=True))
    for k in BITWISE + ("probs",):
        assert np.array_equal(_bits(after[k]), _bits(loaded[k])), f"{k}: forward after update=True differs from a model loaded with running"
    before = _host(fx.PointNet(10).load(P).forward(xd, intermediates=True))
    assert not np.array_equal(_bits(before["logits"]), _bits(after["logits"]))


def test_graph_replay_and_numpy_in_numpy_out(gpu_fx):
    fx = gpu_fx
    P = _params(10, seed=30)
    m = fx.PointNet(10).load(P)
    X = _cloud(31, 200, 2)
    mask = fx.PointNet.dropout_mask(2, seed=9)
    out = m.forward_train(X, dropout=mask, intermediates=True)  # numpy in, numpy out
    assert all(isinstance(v, np.ndarray) for k, v in out.items() if k not in STATS)
    assert all(isinstance(v, np.ndarray) for s in STATS for v in out[s].values())
    eager = _host(m.forward_train(fx.gpu(X), dropout=fx.gpu(mask), intermediates=True))
    _same_bits(out, eager, "numpy against device arrays")
    assert isinstance(m.forward_train(X), np.ndarray)
    s = fx.Stream.create()
    with fx.stream(s):
        xd, md = fx.gpu(X), fx.gpu(mask)
        m.forward_train(xd, dropout=md, intermediates=True)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec = m.forward_train(xd, dropout=md, intermediates=True)
        g.launch()
        s.synchronize()
        first = _host(rec)
        g.launch()
        s.synchronize()
        second = _host(rec)
    _same_bits(first, eager, "the first replay against the eager call")
    _same_bits(second, eager, "the second replay against the eager call")


def test_a_nan_reaches_every_cloud(gpu_fx):
    """Batch statistics couple the clouds, unlike test mode: one NaN coordinate makes every output of every cloud NaN, and
    every statistic from the first BatchNorm on, as the restatement says."""
    fx = gpu_fx
    P = _params(10, seed=32)
    m = fx.PointNet(10).load(P)
    X = _cloud(33, 100, 3)
    X[1, 37, 1] = np.nan
    got = _host(m.forward_train(fx.gpu(X), intermediates=True))
    want = _want(("nan",), X, P)
    for k in BITWISE + ("probs",):
        assert np.all(np.isnan(want[k])), k
        assert np.all(np.isnan(got[k])), f"{k}: the NaN did not reach every cloud"
    for s in STATS:
        for name in got[s]:
            assert np.array_equal(np.isnan(got[s][name]), np.isnan(want[s][name])), (s, name)
    assert np.all(np.isnan(got["batch_stats"]["feat.bn4.mu"])) and np.all(np.isnan(got["running"]["stn.bn1.sigma2"]))
