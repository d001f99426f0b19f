"""The DGCNN training-mode forward on the device (fx3d_dgcnn_forward_train through fx.DGCNN.forward_train) against the host
restatement tests/dgcnn_train_ref.py: logits, both neighbour lists, both EdgeConv outputs, the pooled feature, every batch
statistic and every updated running statistic bit for bit (uint32 views, no element left out), the probabilities within 1e-5
relative of the Float64 softmax of the device's own logits.  Shapes: m = 4, a partial tile with an odd number of clouds, a tile
boundary, a partial last tile of three, the reference's test shape with 10 and 40 classes, and 48 (tile, cloud) sums, more than
the fold's 32 groups.  Then what needs no restatement: the test-mode forward at the returned statistics gives the same bits;
the running statistics in the parameters enter nothing but `running`; dropout masks; momentum and update=True; two runs, a
captured graph, host arrays; a NaN that reaches every cloud.

Every draw is first held to dgcnn_ref.check_draw on the restatement's training-mode result."""
import numpy as np
import pytest

import dgcnn_ref as ref
import dgcnn_train_ref as tref

pytestmark = pytest.mark.gpu

F32 = np.float32
BITWISE = ("logits", "x1", "x2", "pooled")
LISTS = ("idx1", "idx2")
STATS = ("batch_stats", "running")
STAT_NAMES = [f"{bn}.{f}" for bn in tref.BN_ORDER for f in ("mu", "sigma2")]
SEED = 1


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


def _params(num_classes, seed=SEED):
    """random_params: random running statistics too, so a kernel that wrongly reads them shows up.  Shared, never modified."""
    if (num_classes, seed) not in _PARAMS:
        _PARAMS[(num_classes, seed)] = ref.random_params(num_classes, seed)
    return _PARAMS[(num_classes, seed)]


def _want(key, X, P, K, dropout=None, momentum=0.1, clean=True):
    """The restatement's run, held to check_draw, computed once per key and shared among the tests (never modified)."""
    if key not in _WANT:
        _WANT[key] = tref.forward_train(X, P, K, dropout=dropout, momentum=momentum)
        if clean:
            ref.check_draw(_WANT[key])
    return _WANT[key]


def _check_probs(got, num_classes, B):
    """As tests/test_gpu_dgcnn.py: within 1e-5 relative of the Float64 softmax of the device's own logits."""
    assert got["probs"].shape == (num_classes, B)
    want = ref.softmax64(got["logits"])
    rel = float(np.max(np.abs(got["probs"].astype(np.float64) - want) / want))
    print(f"probabilities: largest relative deviation from the Float64 softmax {rel:.3e}; smallest probability {want.min():.3e}")
    assert want.min() >= 1e-4 and want.max() <= 1 - 1e-4, (want.min(), want.max())
    assert rel <= 1e-5, rel


def _check_against_ref(got, want, what=""):
    for k in LISTS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.int32, (what, k)
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs from the restatement's lists"
    for k in BITWISE:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.flatnonzero(_bits(got[k]).ravel() != _bits(want[k]).ravel())
        print(f"{what} {k}: {bad.size} of {got[k].size} elements differ from the restatement")
        assert bad.size == 0, (what, k, bad[:5], got[k].ravel()[bad[:5]], want[k].ravel()[bad[:5]])
    for s in STATS:
        assert list(got[s]) == list(want[s]) == STAT_NAMES
        for name, w in want[s].items():
            g = got[s][name]
            assert g.shape == w.shape, (what, s, name)
            bad = np.flatnonzero(_bits(g) != _bits(w))
            assert bad.size == 0, (what, s, name, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])
        print(f"{what} {s}: all {sum(v.size for v in want[s].values())} values equal the restatement's")


def _same_bits(a, b, what, keys=BITWISE + ("probs",), stats=STATS):
    for k in LISTS:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"
    for s in stats:
        for name in a[s]:
            assert np.array_equal(_bits(a[s][name]), _bits(b[s][name])), f"{what}: {s}[{name}] differs"


@pytest.mark.parametrize("N,B,K,num_classes", [(2, 2, 1, 10), (63, 3, 3, 10), (65, 2, 3, 10), (130, 2, 5, 10), (64, 2, 10, 10),
                                               (64, 2, 10, 40), (1000, 3, 2, 10)])
def test_parity_with_the_restatement(gpu_fx, N, B, K, num_classes):
    fx = gpu_fx
    P = _params(num_classes)
    m = fx.DGCNN(num_classes, K, N).load(P)
    X = _cloud(SEED + 1000, N, B)
    got = _host(m.forward_train(fx.gpu(X), intermediates=True))
    want = _want(("parity", N, B, K, num_classes), X, P, K)
    _check_against_ref(got, want, what=f"N={N} B={B} K={K} nc={num_classes}")
    _check_probs(got, num_classes, B)
    probs = m.forward_train(fx.gpu(X))
    assert np.array_equal(_bits(probs.to_host()), _bits(got["probs"]))


def test_test_mode_forward_at_the_batch_statistics_gives_the_same_bits(gpu_fx):
    """forward on a model loaded with the returned batch_stats is the training-mode network without dropout, bit for bit --
    idx2 included, which is searched on the training-mode x1 -- and that differs from forward on the original parameters."""
    fx = gpu_fx
    N, B, K = 100, 3, 4
    P = _params(10)
    X = _cloud(SEED + 1000, N, B)
    _want(("stages", N, B, K), X, P, K)
    xd = fx.gpu(X)
    got = _host(fx.DGCNN(10, K, N).load(P).forward_train(xd, dropout=None, intermediates=True))
    Q = dict(P)
    Q.update(got["batch_stats"])
    assert all(not np.array_equal(Q[k], P[k]) for k in got["batch_stats"])
    test_mode = _host(fx.DGCNN(10, K, N).load(Q).forward(xd, intermediates=True))
    for k in LISTS:
        assert np.array_equal(test_mode[k], got[k]), k
    for k in BITWISE + ("probs",):
        assert np.array_equal(_bits(test_mode[k]), _bits(got[k])), f"{k}: the test-mode forward at the batch statistics differs"
    plain = _host(fx.DGCNN(10, K, N).load(P).forward(xd, intermediates=True))
    assert np.array_equal(plain["idx1"], got["idx1"])  # the first search is on the coordinates
    for k in BITWISE + ("idx2",):
        assert not np.array_equal(plain[k], got[k]), f"{k}: training mode gives what test mode gives"


def test_running_statistics_of_the_parameters_enter_running_only(gpu_fx):
    fx = gpu_fx
    N, B, K = 65, 2, 3
    P = _params(10)
    Q = dict(P)
    rng = np.random.default_rng(24)
    for k in P:
        if k.endswith(".mu"):
            Q[k] = rng.standard_normal(P[k].shape).astype(F32)
        elif k.endswith(".sigma2"):
            Q[k] = rng.uniform(0.1, 5.0, P[k].shape).astype(F32)
    xd = fx.gpu(_cloud(SEED + 1000, N, B))
    a = _host(fx.DGCNN(10, K, N).load(P).forward_train(xd, dropout=3, intermediates=True))
    b = _host(fx.DGCNN(10, K, N).load(Q).forward_train(xd, dropout=3, intermediates=True))
    _same_bits(a, b, "other running statistics", stats=("batch_stats",))
    assert all(not np.array_equal(a["running"][k], b["running"][k]) for k in a["running"])


def test_dropout_masks(gpu_fx):
    """Seeded masks against the restatement; all ones is the identity; a host mask is a device mask; a zero column of the first
    mask makes that cloud's fc_5 input zero, so its fc5.bn input is fc_5's bias in every channel, as the restatement says."""
    fx = gpu_fx
    N, B, K = 65, 3, 3
    P = _params(10)
    m = fx.DGCNN(10, K, N).load(P)
    X = _cloud(SEED + 1000, N, B)
    xd = fx.gpu(X)
    masks = fx.DGCNN.dropout_masks(B, seed=7)
    got = _host(m.forward_train(xd, dropout=masks, intermediates=True))
    want = _want(("dropout", "seeded"), X, P, K, dropout=masks)
    _check_against_ref(got, want, what="seeded masks")
    none = _want(("dropout", "none"), X, P, K)
    assert not np.array_equal(want["d4"], none["d4"]) and not np.array_equal(want["logits"], none["logits"])
    by_seed = _host(m.forward_train(xd, dropout=7, intermediates=True))
    on_dev = _host(m.forward_train(xd, dropout=tuple(fx.gpu(k) for k in masks), intermediates=True))
    _same_bits(by_seed, got, "dropout=7 against dropout_masks(B, 7)")
    _same_bits(on_dev, got, "device masks")
    plain = _host(m.forward_train(xd, dropout=None, intermediates=True))
    ones = _host(m.forward_train(xd, dropout=(np.ones((512, B), F32), np.ones((256, B), F32)), intermediates=True))
    _same_bits(ones, plain, "all ones against None")
    _check_against_ref(plain, none, what="no mask")
    col = np.asfortranarray(masks[0].copy())
    col[:, 1] = 0
    got = _host(m.forward_train(xd, dropout=(col, masks[1]), intermediates=True))
    want = _want(("dropout", "column"), X, P, K, dropout=(col, masks[1]), clean=False)
    assert not want["d4"][1].any() and want["d4"][0].any()
    assert np.array_equal(_bits(want["bn_inputs"]["fc5.bn"][1]), _bits(P["fc5.dense.bias"]))  # dense(0) + bias
    _check_against_ref(got, want, what="zero column")


@pytest.mark.parametrize("momentum", [0.1, 0.5])
def test_momentum_and_update(gpu_fx, momentum):
    fx = gpu_fx
    N, B, K = 65, 2, 3
    P = _params(10)
    m = fx.DGCNN(10, K, N).load(P)
    X = _cloud(SEED + 1000, N, B)
    xd = fx.gpu(X)
    got = _host(m.forward_train(xd, momentum=momentum, update=True, intermediates=True))
    want = _want(("momentum", momentum), X, P, K, momentum=momentum)
    _check_against_ref(got, want, what=f"momentum={momentum}")
    for name, v in got["running"].items():  # the model now holds the running statistics, on the host and on the device
        assert np.array_equal(_bits(m.params[name]), _bits(v)), name
    assert all(np.array_equal(m.params[k], P[k]) for k in P if not k.endswith((".mu", ".sigma2")))
    after = _host(m.forward(xd, intermediates=True))
    Q = dict(P)
    Q.update(got["running"])
    loaded = _host(fx.DGCNN(10, K, N).load(Q).forward(xd, intermediates=True))
    for k in BITWISE + ("probs",):
        assert np.array_equal(_bits(after[k]), _bits(loaded[k])), f"{k}: forward after update=True differs from a model loaded with running"
    before = _host(fx.DGCNN(10, K, N).load(P).forward(xd, intermediates=True))
    assert not np.array_equal(_bits(before["logits"]), _bits(after["logits"]))


def test_two_runs_graph_replay_and_numpy_in_numpy_out(gpu_fx):
    fx = gpu_fx
    N, B, K = 130, 2, 5
    P = _params(10)
    m = fx.DGCNN(10, K, N).load(P)
    X = _cloud(SEED + 1000, N, B)
    masks = fx.DGCNN.dropout_masks(B, seed=9)
    out = m.forward_train(X, dropout=masks, intermediates=True)  # numpy in, numpy out
    assert all(isinstance(v, np.ndarray) for k, v in out.items() if k not in STATS)
    assert all(isinstance(v, np.ndarray) for s in STATS for v in out[s].values())
    dev_masks = tuple(fx.gpu(k) for k in masks)
    eager = _host(m.forward_train(fx.gpu(X), dropout=dev_masks, intermediates=True))
    _same_bits(out, eager, "numpy against device arrays")
    _same_bits(_host(m.forward_train(fx.gpu(X), dropout=dev_masks, intermediates=True)), eager, "two calls")
    assert isinstance(m.forward_train(X), np.ndarray)
    s = fx.Stream.create()
    with fx.stream(s):
        xd, md = fx.gpu(X), tuple(fx.gpu(k) for k in masks)
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
    every statistic from ec1.bn1 on, as the restatement says."""
    fx = gpu_fx
    N, B, K = 100, 3, 4
    P = _params(10)
    X = _cloud(SEED + 1000, N, B)
    X[1, 37, 1] = np.nan
    got = _host(fx.DGCNN(10, K, N).load(P).forward_train(fx.gpu(X), intermediates=True))
    want = _want(("nan",), X, P, K, clean=False)
    for k in BITWISE + ("probs",):
        assert np.all(np.isnan(want[k])), k
        assert np.all(np.isnan(got[k])), f"{k}: the NaN did not reach every cloud"
    for k in LISTS:
        assert got[k].min() >= 0 and got[k].max() < N  # a NaN distance sorts last: every index is a point of the cloud
    for s in STATS:
        for name in got[s]:
            assert np.all(np.isnan(want[s][name])), (s, name)
            assert np.all(np.isnan(got[s][name])), (s, name)
