"""stnKD(K) on the device (fx3d_stnkd_forward / fx3d_stnkd_forward_train through fx.stnKD) against the host restatement
tests/stnkd_ref.py: every comparison bit for bit (uint32 views) -- the transform, the pooled feature, every batch statistic and
every updated running statistic.

Shapes, the smallest that cross each boundary: K below 4 (v_fma_f32 only), the MFMA with 1 / 2 / 3 remainder channels, exact
multiples of 4 and of 32, K K beyond the head's 1024 threads; a partial tile, a whole one, one tile plus one point, three tiles;
one cloud and an odd number of clouds.  Then the ties to PointNet's own kernels, whose stn / fstn rounds are this layer at K = 3
and K = 64; a contraction that a zero pad would turn into NaN; draws beyond unit scale; pointers aligned to 4 bytes only, a dirty
workspace of exactly the queried size, a replayed graph, two eager runs; and the refusals with real device buffers."""
import numpy as np
import pytest

import misaligned as mis
import pointnet_ref as ref
import pointnet_train_ref as tref
import stnkd_ref as sref

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID, UNSUPPORTED = -1, -5
KS = (1, 2, 3, 4, 5, 7, 31, 32, 33, 64, 67, 128)
NS = (1, 63, 64, 65, 130)
FORWARD = [(K, 65, 3) for K in KS] + [(K, N, B) for K in (5, 64) for N in NS if N != 65 for B in (1, 3)] + [(5, 65, 1), (64, 65, 1)]
STATS = ("batch_stats", "running")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _host(out):
    def one(v):
        if isinstance(v, dict):
            return {k: one(w) for k, w in v.items()}
        return v.to_host() if hasattr(v, "to_host") else np.asarray(v)
    return one(out)


def _cloud(seed, K, N, B):
    return np.asfortranarray(np.random.default_rng([seed, K, N, B]).standard_normal((K, N, B)).astype(F32))


_PARAMS, _WANT = {}, {}


def _params(K, seed=None):
    """random_params: random running statistics too.  Shared, never modified."""
    key = (K, K if seed is None else seed)
    if key not in _PARAMS:
        _PARAMS[key] = sref.random_params(K, key[1])
    return _PARAMS[key]


def _want(key, fn):
    """A restatement's run, computed once per key and shared among the tests (never modified)."""
    if key not in _WANT:
        _WANT[key] = fn()
    return _WANT[key]


def _same(got, want, what, keys=("out", "pooled"), stats=()):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.flatnonzero(_bits(got[k]).ravel() != _bits(want[k]).ravel())
        print(f"{what} {k}: {bad.size} of {got[k].size} elements differ")
        assert bad.size == 0, (what, k, bad.size, bad[:5], np.asarray(got[k]).ravel()[bad[:5]], np.asarray(want[k]).ravel()[bad[:5]])
    for s in stats:
        assert list(got[s]) == list(want[s]) == [f"{bn}.{f}" for bn in sref.BN_ORDER for f in ("mu", "sigma2")], (what, s)
        for name, w in want[s].items():
            g = got[s][name]
            assert g.shape == w.shape, (what, s, name)
            bad = np.flatnonzero(_bits(g) != _bits(w))
            assert bad.size == 0, (what, s, name, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,B", FORWARD)
def test_forward_parity_with_the_restatement(gpu_fx, K, N, B):
    fx = gpu_fx
    P = _params(K)
    m = fx.stnKD(K).load(P)
    X = _cloud(1, K, N, B)
    got = _host(m.forward(fx.gpu(X), intermediates=True))
    want = _want(("fwd", K, N, B), lambda: sref.forward(X, P, K))
    assert np.all(np.isfinite(want["out"])) and np.unique(want["out"]).size > K * K * B // 2  # the draw has something to compare
    _same(got, want, f"K={K} N={N} B={B}")
    plain = m.forward(fx.gpu(X))
    assert np.array_equal(_bits(plain.to_host()), _bits(got["out"]))
    if (N, B) == (65, 3) and K in (5, 128):  # numpy in, numpy out; (K, N) is one cloud
        host = m(X)
        assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(got["out"]))
        one = m.forward(np.ascontiguousarray(X[:, :, 0]))
        assert one.shape == (K, K, 1) and np.array_equal(_bits(one[:, :, 0]), _bits(got["out"][:, :, 0]))


def test_every_k_meets_n_65_and_every_n_meets_k_5_and_64():
    assert {K for K, N, _ in FORWARD if N == 65} == set(KS)
    for K in (5, 64):
        assert {N for k, N, _ in FORWARD if k == K} == set(NS)
        assert {B for k, _, B in FORWARD if k == K} == {1, 3}


# ---- ties to PointNet: the existing kernels are the yardstick -----------------------------------------------------------------------
def _pointnet_case():
    P = ref.random_params(10, seed=10)
    X = np.asfortranarray(np.random.default_rng(41).standard_normal((3, 65, 3)).astype(F32))
    return P, X


def test_ties_to_pointnet_in_test_mode(gpu_fx):
    fx = gpu_fx
    P, X = _pointnet_case()
    net = fx.PointNet(10).load(P)
    whole = _host(net.forward(fx.gpu(X), intermediates=True))
    stn = fx.stnKD.from_pointnet(net, "stn").forward(fx.gpu(X)).to_host()
    assert np.array_equal(_bits(stn), _bits(whole["stn"])), "stnKD(3) on the stn slice differs from PointNet's stn"
    h = np.asfortranarray(np.transpose(_want(("pointnet",), lambda: ref.forward(X, P))["h"], (2, 1, 0)))  # (64, N, B)
    fstn = fx.stnKD.from_pointnet(net, "fstn").forward(fx.gpu(h)).to_host()
    assert np.array_equal(_bits(fstn), _bits(whole["fstn"])), "stnKD(64) on the fstn slice differs from PointNet's fstn"


def test_ties_to_pointnet_in_training_mode(gpu_fx):
    fx = gpu_fx
    P, X = _pointnet_case()
    net = fx.PointNet(10).load(P)
    whole = _host(net.forward_train(fx.gpu(X), intermediates=True))
    h = np.asfortranarray(np.transpose(_want(("pointnet train",), lambda: tref.forward_train(X, P))["h"], (2, 1, 0)))
    for which, x in (("stn", X), ("fstn", h)):
        got = _host(fx.stnKD.from_pointnet(net, which).forward_train(fx.gpu(x), intermediates=True))
        assert np.array_equal(_bits(got["out"]), _bits(whole[which])), which
        for s in STATS:
            for bn in sref.BN_ORDER:
                for f in ("mu", "sigma2"):
                    assert np.array_equal(_bits(got[s][f"{bn}.{f}"]), _bits(whole[s][f"{which}.{bn}.{f}"])), (which, s, bn, f)


# ---- training mode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.1, 1.0])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("K", [3, 5, 64, 128])
def test_training_mode_parity_with_the_restatement(gpu_fx, K, B, momentum):
    fx = gpu_fx
    N = 65
    P = _params(K)
    m = fx.stnKD(K).load(P)
    X = _cloud(2, K, N, B)
    got = _host(m.forward_train(fx.gpu(X), momentum=momentum, intermediates=True))
    want = _want(("train", K, N, B, momentum), lambda: sref.forward_train(X, P, K, momentum=momentum))
    assert np.all(np.isfinite(want["out"]))
    _same(got, want, f"K={K} B={B} momentum={momentum}", stats=STATS)
    plain = m.forward_train(fx.gpu(X), momentum=momentum)
    assert np.array_equal(_bits(plain.to_host()), _bits(got["out"]))
    assert all(np.array_equal(m.params[k], P[k]) for k in P)  # update=False leaves the layer as it was


@pytest.mark.parametrize("K", [5, 64])
def test_update_then_forward_at_the_batch_statistics(gpu_fx, K):
    """update=True adopts `running`: the next forward is the test-mode layer at those statistics.  And forward on the returned
    batch statistics gives forward_train's output bits."""
    fx = gpu_fx
    N, B = 65, 3
    P = _params(K)
    X = _cloud(3, K, N, B)
    xd = fx.gpu(X)
    m = fx.stnKD(K).load(P)
    got = _host(m.forward_train(xd, momentum=0.1, update=True, intermediates=True))
    want = _want(("train", K, N, B, "update"), lambda: sref.forward_train(X, P, K, momentum=0.1))
    _same(got, want, f"update K={K}", stats=STATS)
    for name, v in got["running"].items():  # the model now holds the running statistics, on the host and on the device
        assert np.array_equal(_bits(m.params[name]), _bits(v)), name
    assert all(np.array_equal(m.params[k], P[k]) for k in P if not k.endswith((".mu", ".sigma2")))
    after = _host(m.forward(xd, intermediates=True))
    loaded = _host(fx.stnKD(K).load({**P, **got["running"]}).forward(xd, intermediates=True))
    _same(after, loaded, "forward after update=True against a layer loaded with running")
    at_stats = _host(fx.stnKD(K).load({**P, **got["batch_stats"]}).forward(xd, intermediates=True))
    _same(at_stats, got, "forward on the returned batch statistics against forward_train")
    assert not np.array_equal(_bits(after["out"]), _bits(got["out"]))


# ---- no zero padding --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True])
def test_no_contraction_is_padded_with_zero_channels(gpu_fx, train):
    """K = 5 with W[0, o + 1] = +Inf.  Channel 0 of every point is negative, so channel o + 1 is relu(-Inf) = +0 everywhere and
    the layer stays finite.  A first layer padded to 8 channels would read W[5 .. 7, o] = W[0 .. 2, o + 1] = (+Inf, ., .) against
    its zero pads: 0 * Inf = NaN in channel o, and from there in every output."""
    fx = gpu_fx
    K, N, B, o = 5, 65, 3, 17
    P = dict(_params(K, seed=50))
    W = P["conv1.weight"].copy()
    W[0, 0, o + 1] = np.inf
    P["conv1.weight"] = W
    X = _cloud(4, K, N, B)
    X[0] = -np.abs(X[0]) - F32(0.1)
    assert np.all(np.isfinite(X)) and np.all(X != 0)
    m = fx.stnKD(K).load(P)
    if train:
        got = _host(m.forward_train(fx.gpu(X), intermediates=True))
        want = _want(("pad", True), lambda: sref.forward_train(X, P, K))
    else:
        got = _host(m.forward(fx.gpu(X), intermediates=True))
        want = _want(("pad", False), lambda: sref.forward(X, P, K))
    a1 = want["a1"]  # (B, N, 64): the first layer as the restatement has it
    assert np.all(np.isfinite(a1[:, :, o])) and np.unique(a1[:, :, o]).size > N, "channel o is an ordinary channel"
    assert np.unique(a1[:, :, o + 1]).size == 1 and np.all(np.isfinite(a1[:, :, o + 1])), "channel o + 1 is relu(-Inf) everywhere"
    assert np.all(np.isfinite(want["out"])) and np.all(np.isfinite(want["pooled"]))
    _same(got, want, f"Inf beside the pad, train={train}", stats=STATS if train else ())


# ---- beyond unit scale ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("scale", [1e4, 1e-4])
def test_beyond_unit_scale(gpu_fx, scale, train):
    """The inputs and the weights of the layer that reads them times `scale` (as tests/model_draws.py scales its models)."""
    fx = gpu_fx
    K, N, B = 7, 65, 3
    P = dict(_params(K, seed=60))
    P["conv1.weight"] = (P["conv1.weight"].astype(np.float64) * scale).astype(F32)
    X = np.asfortranarray((_cloud(5, K, N, B).astype(np.float64) * scale).astype(F32))
    m = fx.stnKD(K).load(P)
    if train:
        got = _host(m.forward_train(fx.gpu(X), intermediates=True))
        want = _want(("scale", scale, True), lambda: sref.forward_train(X, P, K))
    else:
        got = _host(m.forward(fx.gpu(X), intermediates=True))
        want = _want(("scale", scale, False), lambda: sref.forward(X, P, K))
    assert np.all(np.isfinite(want["out"])) and np.unique(want["out"]).size > K * K
    _same(got, want, f"scale={scale} train={train}", stats=STATS if train else ())


# ---- plumbing, at K = 5, N = 65, B = 3, on the C ABI ---------------------------------------------------------------------------------
PK, PN, PB = 5, 65, 3


def _sync(fx):
    try:
        fx.synchronize()
    except fx.Flux3DHipError as e:  # a fault: nothing more is started on the device
        pytest.exit(str(e), returncode=3)


def _abi_case(fx):
    P = _params(PK)
    m = fx.stnKD(PK).load(P)
    X = _cloud(6, PK, PN, PB)
    return m, m.flat_params(), X


def _abi_run(fx, train, params, x, ws, ws_bytes):
    """One call on device pointers; fresh outputs filled with 0xA5 bytes: dict of host arrays."""
    f32 = np.float32
    out = {"out": fx.DeviceArray.empty((PK, PK, PB), f32), "pooled": fx.DeviceArray.empty((1024, PB), f32)}
    if train:
        out["batch_stats"], out["running"] = fx.DeviceArray.empty((2944,), f32), fx.DeviceArray.empty((2944,), f32)
    for v in out.values():
        v.copy_(np.full(v.shape, np.frombuffer(b"\xa5" * 4, f32)[0], f32, order="F"))
    stream = fx.current_stream().handle
    if train:
        fx._lib.call("fx3d_stnkd_forward_train", params, PK, x, PN, PB, 0.1, out["out"].ptr, out["pooled"].ptr,
                     out["batch_stats"].ptr, out["running"].ptr, ws, ws_bytes, stream)
    else:
        fx._lib.call("fx3d_stnkd_forward", params, PK, x, PN, PB, out["out"].ptr, out["pooled"].ptr, ws, ws_bytes, stream)
    _sync(fx)
    return {k: v.to_host() for k, v in out.items()}


def _abi_want(train):
    P, X = _params(PK), _cloud(6, PK, PN, PB)
    if not train:
        w = _want(("abi", False), lambda: sref.forward(X, P, PK))
        return {"out": w["out"], "pooled": w["pooled"]}
    w = _want(("abi", True), lambda: sref.forward_train(X, P, PK, momentum=0.1))
    return {"out": w["out"], "pooled": w["pooled"], "batch_stats": sref.flat_stats(w["batch_stats"]),
            "running": sref.flat_stats(w["running"])}


def _abi_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(_bits(got[k]).ravel(), _bits(want[k]).ravel()), (what, k)


@pytest.mark.parametrize("train", [False, True])
def test_pointers_aligned_to_4_bytes_only(gpu_fx, train):
    fx = gpu_fx
    _, flat, X = _abi_case(fx)
    nb = fx._lib.query_bytes("fx3d_stnkd_train_workspace_bytes" if train else "fx3d_stnkd_workspace_bytes", PN, PB, PK)
    ws = fx.DeviceArray.zeros((nb,), np.uint8)
    for off in (4, 8, 12):
        p, x = mis.place(fx, flat, off), mis.place(fx, X, off)
        assert p.ptr % 16 == off and x.ptr % 16 == off
        _abi_same(_abi_run(fx, train, p.ptr, x.ptr, ws.ptr, nb), _abi_want(train), f"offset {off}")


@pytest.mark.parametrize("train", [False, True])
def test_a_dirty_workspace_of_exactly_the_queried_size(gpu_fx, train):
    fx = gpu_fx
    _, flat, X = _abi_case(fx)
    nb = fx._lib.query_bytes("fx3d_stnkd_train_workspace_bytes" if train else "fx3d_stnkd_workspace_bytes", PN, PB, PK)
    guard = 256
    buf = fx.DeviceArray.empty((nb + guard,), np.uint8)
    buf.copy_(np.full(nb + guard, 0xFF, np.uint8))
    assert buf.ptr % 256 == 0
    p, x = fx.DeviceArray.from_host(flat), fx.DeviceArray.from_host(X)
    _abi_same(_abi_run(fx, train, p.ptr, x.ptr, buf.ptr, nb), _abi_want(train), "dirty workspace")
    assert np.all(buf.to_host()[nb:] == 0xFF), "written beyond the queried size"


@pytest.mark.parametrize("train", [False, True])
def test_a_replayed_graph_and_two_eager_runs(gpu_fx, train):
    fx = gpu_fx
    m, _, X = _abi_case(fx)
    want = _abi_want(train)

    def run(xd):
        r = m.forward_train(xd, intermediates=True) if train else m.forward(xd, intermediates=True)
        return r

    def flat(r):
        r = _host(r)
        out = {"out": r["out"], "pooled": r["pooled"]}
        if train:
            out["batch_stats"], out["running"] = sref.flat_stats(r["batch_stats"]), sref.flat_stats(r["running"])
        return out

    first, second = flat(run(fx.gpu(X))), flat(run(fx.gpu(X)))
    _abi_same(first, want, "eager")
    _abi_same(second, first, "the second eager run")
    s = fx.Stream.create()
    with fx.stream(s):
        xd = fx.gpu(X)
        run(xd)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec = run(xd)
        for what in ("the first replay", "the second replay"):
            g.launch()
            s.synchronize()
            _abi_same(flat(rec), first, what)


# ---- refusals on the device path ------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu_fx):
    """Real device buffers, each large enough for the call as asked: the refusal comes first, and the outputs keep their fill."""
    fx = gpu_fx
    lib = fx._lib.load()
    K, N, B = 129, 65, 3
    params = fx.DeviceArray.zeros((1 << 23,), F32)       # more than stnKD(129) would read
    x = fx.DeviceArray.zeros((K, N, B), F32)
    ws = fx.DeviceArray.zeros((1 << 22,), np.uint8)
    fill = np.frombuffer(b"\xa5" * 4, F32)[0]
    out, pooled = fx.DeviceArray.empty((K, K, B), F32), fx.DeviceArray.empty((1024, B), F32)
    stats, running = fx.DeviceArray.empty((2944,), F32), fx.DeviceArray.empty((2944,), F32)
    outputs = (out, pooled, stats, running)
    for v in outputs:
        v.copy_(np.full(v.shape, fill, F32, order="F"))
    stream = fx.current_stream().handle

    def fwd(K_=5, B_=B, nb=ws.nbytes):
        return lib.fx3d_stnkd_forward(params.ptr, K_, x.ptr, N, B_, out.ptr, pooled.ptr, ws.ptr, nb, stream)

    def train(K_=5, B_=B, nb=ws.nbytes):
        return lib.fx3d_stnkd_forward_train(params.ptr, K_, x.ptr, N, B_, 0.1, out.ptr, pooled.ptr, stats.ptr, running.ptr, ws.ptr, nb,
                                            stream)

    assert fwd(K_=129) == UNSUPPORTED and "129" in fx._lib.last_error()
    assert train(K_=129) == UNSUPPORTED and "129" in fx._lib.last_error()
    assert train(B_=1) == INVALID and "B >= 2" in fx._lib.last_error()
    need = fx._lib.query_bytes("fx3d_stnkd_workspace_bytes", N, B, 5)
    assert fwd(nb=need - 1) == INVALID and str(need) in fx._lib.last_error()
    need = fx._lib.query_bytes("fx3d_stnkd_train_workspace_bytes", N, B, 5)
    assert train(nb=need - 1) == INVALID and str(need) in fx._lib.last_error()
    _sync(fx)
    for v in outputs:
        assert np.all(_bits(v.to_host()) == 0xA5A5A5A5), "a refused call wrote an output"
    with pytest.raises(ValueError):
        fx.stnKD(129)
    with pytest.raises(ValueError, match="at least two clouds"):
        fx.stnKD(5).forward_train(fx.gpu(np.zeros((5, 8, 1), F32)))
