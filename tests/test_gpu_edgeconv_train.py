"""The EdgeConv training-mode forward on the device (fx3d_edgeconv_forward_train through fx.EdgeConv.forward_train) against the
host restatement tests/dgcnn_train_ref.py: the output, the neighbour lists, every batch statistic and every updated running
statistic bit for bit (uint32 views, no element left out), over the forward's envelope: one block, widths that are no multiple
of 4 or 32, four blocks, K = 1, the split_halves layers and the wide ones, the shared_rows LDS plan, the envelope's corner, one
cloud.  Then DGCNN's two stages as this layer; given neighbours; two runs; the test-mode forward at the returned statistics;
momentum and update=True.

Every draw is first held to edgeconv_ref.check_draw on the restatement's training-mode output."""
import numpy as np
import pytest

import dgcnn_ref as dref
import dgcnn_train_ref as tref
import edgeconv_ref as eref

pytestmark = pytest.mark.gpu

F32 = np.float32
STATS = ("batch_stats", "running")
# (layers, N, B, K): each with two clouds where that adds nothing to the cost
CASES = [([3, 16], 7, 2, 6),             # one block, one partial tile, K = N - 1
         ([1, 1], 5, 2, 2),              # one channel: cin = 2 runs on v_fma_f32 alone
         ([5, 33, 70], 65, 2, 3),        # widths that are no multiple of 4 or 32, a tile boundary, a partial slab of a wide layer
         ([4, 8, 8, 8, 40], 66, 2, 1),   # four blocks, K = 1: no maximum over k
         ([6, 2, 255], 40, 2, 4),        # a two-channel hidden layer, 255 = 8 slabs with the last partial (two slabs per wave)
         ([64, 64, 128, 256], 70, 2, 3),  # every stride: 64 (split halves), 128, 256
         ([65, 8, 8, 8, 8], 66, 2, 3),   # shared_rows: three images of stride 258 do not fit
         ([128, 256, 256], 130, 1, 20)]  # the envelope's corner, one cloud (m = K N)
SEED = 1


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _host(out):
    def one(v):
        if isinstance(v, dict):
            return {k: one(w) for k, w in v.items()}
        return v.to_host() if hasattr(v, "to_host") else np.asarray(v)
    return one(out)


def _cloud(seed, F, N, B):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((F, N, B)).astype(F32))


_WANT = {}


def _case(layers, N, B, K, momentum=0.1):
    """(X, P, the restatement's run), computed once per case and shared among the tests (never modified)."""
    key = (tuple(layers), N, B, K, momentum)
    if key not in _WANT:
        P = eref.random_params(layers, SEED)
        X = _cloud(SEED + 1000, layers[0], N, B)
        want = tref.edgeconv_forward_train(X, P, layers, K, momentum=momentum)
        eref.check_draw(want["out"])
        _WANT[key] = (X, P, want)
    return _WANT[key]


def _check_against_ref(got, want, layers, what):
    assert np.array_equal(got["idx"], want["idx"]), f"{what}: the neighbour lists differ"
    assert got["out"].shape == want["out"].shape
    bad = np.flatnonzero(_bits(got["out"]).ravel() != _bits(want["out"]).ravel())
    print(f"{what} out: {bad.size} of {got['out'].size} elements differ from the restatement")
    assert bad.size == 0, (what, bad[:5], got["out"].ravel()[bad[:5]], want["out"].ravel()[bad[:5]])
    names = [f"bn{i}.{f}" for i in range(1, len(layers)) for f in ("mu", "sigma2")]
    for s in STATS:
        assert list(got[s]) == list(want[s]) == names
        for name, w in want[s].items():
            g = got[s][name]
            assert g.shape == w.shape, (what, s, name)
            bad = np.flatnonzero(_bits(g) != _bits(w))
            assert bad.size == 0, (what, s, name, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])
        print(f"{what} {s}: all {sum(v.size for v in want[s].values())} values equal the restatement's")


def _same_bits(a, b, what, stats=STATS):
    assert np.array_equal(a["idx"], b["idx"]), f"{what}: idx differs"
    assert np.array_equal(_bits(a["out"]), _bits(b["out"])), f"{what}: out differs"
    for s in stats:
        for name in a[s]:
            assert np.array_equal(_bits(a[s][name]), _bits(b[s][name])), f"{what}: {s}[{name}] differs"


@pytest.mark.parametrize("layers,N,B,K", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_parity_with_the_restatement(gpu_fx, layers, N, B, K):
    fx = gpu_fx
    X, P, want = _case(layers, N, B, K)
    m = fx.EdgeConv(layers, K).load(P)
    xd = fx.gpu(X)
    got = _host(m.forward_train(xd, intermediates=True))
    _check_against_ref(got, want, layers, what=f"{layers} N={N} B={B} K={K}")
    # the statistics are not the running ones, and the output is not the test-mode layer's
    assert all(not np.array_equal(got["batch_stats"][k], P[k]) for k in got["batch_stats"])
    assert not np.array_equal(_bits(got["out"]), _bits(m.forward(xd).to_host()))
    out, idx = m.forward_train(xd, return_idx=True)
    assert np.array_equal(_bits(out.to_host()), _bits(got["out"])) and np.array_equal(idx.to_host(), got["idx"])
    assert np.array_equal(_bits(m.forward_train(xd).to_host()), _bits(got["out"]))


def test_dgcnn_stages_are_this_layer(gpu_fx):
    """EdgeConv([3, 32, 64, 64], K) on X and EdgeConv([64, 128, 256], K) on x1, with the ec1 / ec2 parameters, give
    DGCNN.forward_train's idx1, x1, idx2, x2 and the matching slices of both statistics buffers, bit for bit."""
    fx = gpu_fx
    N, B, K = 100, 3, 4
    P = dref.random_params(10, SEED)
    X = _cloud(SEED + 1000, 3, N, B)
    dref.check_draw(tref.forward_train(X, P, K))
    xd = fx.gpu(X)
    whole = _host(fx.DGCNN(10, K, N).load(P).forward_train(xd, intermediates=True))
    x_in = xd
    for stage, layers in (("ec1", [3, 32, 64, 64]), ("ec2", [64, 128, 256])):
        Q = {k[len(stage) + 1:]: v for k, v in P.items() if k.startswith(stage + ".")}
        got = _host(fx.EdgeConv(layers, K).load(Q).forward_train(x_in, intermediates=True))
        n = stage[-1]
        assert np.array_equal(got["idx"], whole["idx" + n]), stage
        assert np.array_equal(_bits(got["out"]), _bits(whole["x" + n])), stage
        for s in STATS:
            for name, v in got[s].items():
                assert np.array_equal(_bits(v), _bits(whole[s][f"{stage}.{name}"])), (stage, s, name)
        x_in = fx.gpu(np.asfortranarray(whole["x1"]))


def test_given_neighbours_two_runs_and_numpy(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = CASES[2]
    X, P, want = _case(layers, N, B, K)
    m = fx.EdgeConv(layers, K).load(P)
    xd = fx.gpu(X)
    searched = _host(m.forward_train(xd, intermediates=True))
    again = _host(m.forward_train(xd, intermediates=True))
    _same_bits(again, searched, "two calls")
    given = _host(m.forward_train(xd, idx=fx.gpu(searched["idx"]), intermediates=True))
    _same_bits(given, searched, "given lists against searched ones")
    on_host = m.forward_train(X, idx=searched["idx"].astype(np.int64), intermediates=True)  # numpy in, numpy out
    assert isinstance(on_host["out"], np.ndarray) and all(isinstance(v, np.ndarray) for s in STATS for v in on_host[s].values())
    _same_bits(on_host, searched, "numpy against device arrays")
    assert isinstance(m.forward_train(X), np.ndarray)
    # other lists are another layer: every point's neighbours rotated by one point
    other = np.asfortranarray(((searched["idx"] + 1) % N).astype(np.int32))
    got = _host(m.forward_train(xd, idx=fx.gpu(other), intermediates=True))
    _check_against_ref(got, tref.edgeconv_forward_train(X, P, layers, K, idx=other), layers, what="rotated lists")
    assert not np.array_equal(_bits(got["out"]), _bits(searched["out"]))


@pytest.mark.parametrize("case", [2, 6])
def test_test_mode_forward_at_the_batch_statistics_gives_the_same_bits(gpu_fx, case):
    fx = gpu_fx
    layers, N, B, K = CASES[case]
    X, P, _ = _case(layers, N, B, K)
    xd = fx.gpu(X)
    got = _host(fx.EdgeConv(layers, K).load(P).forward_train(xd, intermediates=True))
    Q = dict(P)
    Q.update(got["batch_stats"])
    out, idx = fx.EdgeConv(layers, K).load(Q).forward(xd, return_idx=True)
    assert np.array_equal(idx.to_host(), got["idx"])
    assert np.array_equal(_bits(out.to_host()), _bits(got["out"])), "the test-mode forward at the batch statistics differs"


def test_running_statistics_of_the_parameters_enter_running_only(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = CASES[2]
    X, P, _ = _case(layers, N, B, K)
    Q = dict(P)
    rng = np.random.default_rng(24)
    for k in P:
        if k.endswith(".mu"):
            Q[k] = rng.standard_normal(P[k].shape).astype(F32)
        elif k.endswith(".sigma2"):
            Q[k] = rng.uniform(0.1, 5.0, P[k].shape).astype(F32)
    xd = fx.gpu(X)
    a = _host(fx.EdgeConv(layers, K).load(P).forward_train(xd, intermediates=True))
    b = _host(fx.EdgeConv(layers, K).load(Q).forward_train(xd, intermediates=True))
    _same_bits(a, b, "other running statistics", stats=("batch_stats",))
    assert all(not np.array_equal(a["running"][k], b["running"][k]) for k in a["running"])


@pytest.mark.parametrize("momentum", [0.1, 0.5])
def test_momentum_and_update(gpu_fx, momentum):
    fx = gpu_fx
    layers, N, B, K = CASES[2]
    X, P, want = _case(layers, N, B, K, momentum=momentum)
    m = fx.EdgeConv(layers, K).load(P)
    xd = fx.gpu(X)
    got = _host(m.forward_train(xd, momentum=momentum, update=True, intermediates=True))
    _check_against_ref(got, want, layers, what=f"momentum={momentum}")
    for name, v in got["running"].items():  # the model now holds the running statistics, on the host and on the device
        assert np.array_equal(_bits(m.params[name]), _bits(v)), name
    assert all(np.array_equal(m.params[k], P[k]) for k in P if not k.endswith((".mu", ".sigma2")))
    after = m.forward(xd).to_host()
    Q = dict(P)
    Q.update(got["running"])
    assert np.array_equal(_bits(after), _bits(fx.EdgeConv(layers, K).load(Q).forward(xd).to_host()))
    assert not np.array_equal(_bits(after), _bits(fx.EdgeConv(layers, K).load(P).forward(xd).to_host()))
