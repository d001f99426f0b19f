"""The training-mode model kernels on the device -- PointNet forward_train and grad_train, DGCNN and EdgeConv forward_train --
against their host restatements, bit for bit, on the training-mode families of tests/model_draws.py: batch statistics that are
subnormal, exactly +0 from a variance that is rounding residue (negative before the clamp, or positive and kept), +Inf from a
variance beyond Float32 with a finite mean, and +Inf and NaN together -- where the four training-mode test files draw unit-scale
clouds and one well-behaved parameter set.

Shapes: model_draws' (N = 65 or 64, B = 2, K <= 6).  Every array is compared as uint32 with tests/test_gpu_model_draws.py's
helpers, no element left out: where the restatement has a NaN the device must have one (payload not compared), +-Inf and both
zeros bit for bit.  The neighbour lists are compared with the oracle's search (through the restatement).  Every draw is first held
to its family's condition on the restatement's own statistics (model_draws.check_train).  Two runs give the same bits, NaN payloads
included.  Then, with no restatement: the test-mode forward at the returned batch statistics gives the training-mode bits for
sigma2 = +0, subnormal and +Inf."""
import numpy as np
import pytest

import model_draws as md
import pointnet_grad_train_ref as gtref
from test_gpu_model_draws import _bits, _check_probs, _host, _id, _same, _same_grads, _same_run

pytestmark = pytest.mark.gpu

F32 = np.float32
STATS = ("batch_stats", "running")
MID = ("gstn", "gfstn", "gh", "gxt")
AT_THE_STATISTICS = ("one_point", "variance_overflow", "subnormal_input")   # sigma2 = +0 (and a positive residue), +Inf, +0 and subnormal


def _host_all(out):
    return {k: ({n: _host(v) for n, v in w.items()} if isinstance(w, dict) else _host(w)) for k, w in out.items()}


def _same_stats(got, want, what):
    for s in STATS:
        assert list(got[s]) == list(want[s]), (what, s, list(got[s]), list(want[s]))
        for name, w in want[s].items():   # in forward order: the first BatchNorm that differs is named first
            _same(got[s][name], w, f"{what}: {s}[{name}]")


def _same_runs(a, b, keys, what):
    for k in keys:
        _same_run(a[k], b[k], f"{what} {k}")
    for s in STATS:
        for name in a[s]:
            _same_run(a[s][name], b[s][name], f"{what} {s}[{name}]")


_restated = {}


def _want(net, family, N, B, K=None, lists=None, dropout=None):
    """(the draw, the restatement's training-mode run held to its family's condition), once per case, shared and unchanged."""
    key = (_id(net), family, lists is not None, dropout is not None)
    if key not in _restated:
        d = md.draw_train(family, net, N, B)
        want = md.restate_forward_train(net, d, K, idx=lists, dropout=dropout)
        if dropout is None:   # (a family's condition speaks of the network without a mask)
            md.check_train(family, net, d, want, tag="" if lists is None else "given lists: ")
        _restated[key] = (d, want)
    return _restated[key]


# ---- PointNet ------------------------------------------------------------------------------------------------------------------

PN_FWD = ("logits", "stn", "fstn", "pooled")
PN_NET = ("pointnet", md.POINTNET[2])
_pointnet = {}


def _pointnet_case(fx, family):
    """The model, the draw on the device and the device's own training-mode forward, once per family."""
    if family not in _pointnet:
        N, B, nc = md.POINTNET
        d, want = _want(PN_NET, family, N, B)
        m = fx.PointNet(nc).load(d["P"])
        xd = fx.gpu(d["X"])
        fwd = m.forward_train(xd, intermediates=True)
        _pointnet[family] = dict(d=d, want=want, m=m, xd=xd, fwd=fwd, hfwd=_host_all(fwd))
    return _pointnet[family]


def _same_adjoint(got, want, what):
    grads, gx, mid = got
    assert list(mid) == list(MID)
    for k in MID:   # upstream first: where a mismatch begins
        _same(mid[k], want[2][k], f"{what}: {k}")
    _same(gx, want[1], f"{what}: gx")
    _same_grads({n: _host(v) for n, v in grads.items()}, want[0], what)


def _same_adjoint_run(a, b, what):
    for n in a[0]:
        _same_run(a[0][n], b[0][n], f"{what} {n}")
    _same_run(a[1], b[1], f"{what} gx")
    for k in MID:
        _same_run(a[2][k], b[2][k], f"{what} {k}")


def _check_adjoint_restatement(family, want):
    """Finite outside overflow; under variance_overflow nothing reaches X (sd = +Inf in the layers that read it)."""
    grads, gx, _ = want
    if family == "overflow":
        assert np.isnan(gtref.family(grads, "dW")).any() and np.isnan(gx).any()
        return
    assert all(np.all(np.isfinite(v)) for v in grads.values()) and np.all(np.isfinite(gx)), family
    assert np.count_nonzero(gtref.family(grads, "dW")) > 0
    assert (family == "variance_overflow") == (not gx.any()), family


@pytest.mark.parametrize("family", md.train_families("pointnet"))
def test_pointnet(gpu_fx, family):
    """forward_train, then grad_train with fwd = None and with the device's own forward handed in."""
    fx = gpu_fx
    N, B, nc = md.POINTNET
    c = _pointnet_case(fx, family)
    d, want, m, xd = c["d"], c["want"], c["m"], c["xd"]
    for k in PN_FWD:
        _same(c["hfwd"][k], want[k], f"{family} PointNet forward_train: {k}")
    _same_stats(c["hfwd"], want, f"{family} PointNet forward_train")
    _check_probs(family, c["hfwd"], f"{family} PointNet forward_train")
    again = m.forward_train(xd, intermediates=True)
    _same_runs(again, c["fwd"], PN_FWD + ("probs",), f"{family} PointNet forward_train")
    glogits = md.upstream(family, PN_NET, N, B)
    wantg = gtref.grad_train(d["X"], d["P"], glogits)
    _check_adjoint_restatement(family, wantg)
    gd = fx.gpu(glogits)
    none = m.grad_train(xd, gd, intermediates=True)
    _same_adjoint(none, wantg, f"{family} PointNet grad_train, fwd = None")
    given = m.grad_train(xd, gd, fwd=c["fwd"], intermediates=True)
    _same_adjoint(given, wantg, f"{family} PointNet grad_train, fwd given")
    _same_adjoint_run(given, none, f"{family} PointNet grad_train")


def test_pointnet_subnormal_input_under_a_dropout_mask(gpu_fx):
    """The same draw under a mask that holds both values: feat.bn4's statistics are over the masked activations."""
    fx = gpu_fx
    N, B, nc = md.POINTNET
    family = "subnormal_input"
    mask = fx.PointNet.dropout_mask(B, seed=3)
    assert np.any(mask == 0) and np.any(mask != 0)
    d, want = _want(PN_NET, family, N, B, dropout=mask)
    plain = _want(PN_NET, family, N, B)[1]
    assert np.any(_bits(want["batch_stats"]["feat.bn4.mu"]) != _bits(plain["batch_stats"]["feat.bn4.mu"]))
    m, xd, dd = _pointnet_case(fx, family)["m"], _pointnet_case(fx, family)["xd"], fx.gpu(mask)
    fwd = m.forward_train(xd, dropout=dd, intermediates=True)
    got = _host_all(fwd)
    for k in PN_FWD:
        _same(got[k], want[k], f"{family} PointNet forward_train under a mask: {k}")
    _same_stats(got, want, f"{family} PointNet forward_train under a mask")
    glogits = md.upstream(family, PN_NET, N, B)
    wantg = gtref.grad_train(d["X"], d["P"], glogits, mask)
    _check_adjoint_restatement(family, wantg)
    _same_adjoint(m.grad_train(xd, fx.gpu(glogits), dropout=dd, fwd=fwd, intermediates=True), wantg,
                  f"{family} PointNet grad_train under a mask")


def test_pointnet_graph_replay_one_point(gpu_fx):
    """flat_grad_train of the one_point draw through a captured graph, replayed twice, against the restatement."""
    fx = gpu_fx
    N, B, nc = md.POINTNET
    c = _pointnet_case(fx, "one_point")
    m, d = c["m"], c["d"]
    glogits = md.upstream("one_point", PN_NET, N, B)
    wantg = gtref.grad_train(d["X"], d["P"], glogits)
    s = fx.Stream.create()
    with fx.stream(s):
        xs, gs = fx.gpu(d["X"]), fx.gpu(glogits)
        fwd = m.forward_train(xs, intermediates=True)
        m.flat_grad_train(xs, gs, fwd=fwd)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec, rgx = m.flat_grad_train(xs, gs, fwd=fwd)
        g.launch()
        g.launch()
        s.synchronize()
        _same(rec, gtref.flat(wantg[0]), "one_point: graph replay of flat_grad_train against the restatement")
        _same(rgx, wantg[1], "one_point: graph replay: gx")


# ---- DGCNN ---------------------------------------------------------------------------------------------------------------------

DG_LISTS = ("idx1", "idx2")
DG_FWD = ("x1", "x2", "pooled", "logits")
DG_NET = ("dgcnn", md.DGCNN[3])
_dgcnn = {}


def _dgcnn_case(fx, family):
    if family not in _dgcnn:
        N, B, K, nc = md.DGCNN
        d, want = _want(DG_NET, family, N, B, K)
        m = fx.DGCNN(nc, K, N).load(d["P"])
        xd = fx.gpu(d["X"])
        fwd = m.forward_train(xd, intermediates=True)
        _dgcnn[family] = dict(d=d, want=want, m=m, xd=xd, fwd=fwd, hfwd=_host_all(fwd))
    return _dgcnn[family]


@pytest.mark.parametrize("family", md.train_families("dgcnn"))
def test_dgcnn(gpu_fx, family):
    c = _dgcnn_case(gpu_fx, family)
    want = c["want"]
    for k in DG_LISTS:
        _same(c["hfwd"][k], want[k], f"{family} DGCNN forward_train: {k} against the oracle's search")
    for k in DG_FWD:
        _same(c["hfwd"][k], want[k], f"{family} DGCNN forward_train: {k}")
    _same_stats(c["hfwd"], want, f"{family} DGCNN forward_train")
    _check_probs(family, c["hfwd"], f"{family} DGCNN forward_train")
    again = c["m"].forward_train(c["xd"], intermediates=True)
    _same_runs(again, c["fwd"], DG_LISTS + DG_FWD + ("probs",), f"{family} DGCNN forward_train")


# ---- EdgeConv ------------------------------------------------------------------------------------------------------------------

EC_CASES = [(layers, N, B, K, f) for layers, N, B, K in md.EDGECONV for f in md.train_families("edgeconv")]
_edgeconv = {}


def _edgeconv_case(fx, layers, N, B, K, family):
    """The layer, the draw on the device and the device's own training-mode forward with its own search, once per case."""
    key = (tuple(layers), family)
    if key not in _edgeconv:
        net = ("edgeconv", layers)
        d, want = _want(net, family, N, B, K)
        m = fx.EdgeConv(layers, K).load(d["P"])
        xd = fx.gpu(d["X"])
        fwd = m.forward_train(xd, return_idx=True, intermediates=True)
        _edgeconv[key] = dict(net=net, d=d, want=want, m=m, xd=xd, fwd=fwd, hfwd=_host_all(fwd))
    return _edgeconv[key]


@pytest.mark.parametrize("layers,N,B,K,family", EC_CASES, ids=_id)
def test_edgeconv(gpu_fx, layers, N, B, K, family):
    """forward_train once with the device's own search (the lists against the oracle's: under one_point and constant_cloud the
    all-tie list, which check_train asserts of the restatement's), once with given lists."""
    fx = gpu_fx
    c = _edgeconv_case(fx, layers, N, B, K, family)
    m, xd = c["m"], c["xd"]
    lists = md.given_lists(N, B, K)
    ld = fx.gpu(lists)
    given = m.forward_train(xd, idx=ld, return_idx=True, intermediates=True)
    for how, fwd, got, want in (("search", c["fwd"], c["hfwd"], c["want"]),
                                ("given lists", given, _host_all(given), _want(c["net"], family, N, B, K, lists=lists)[1])):
        what = f"{family} {layers} {how}"
        _same(got["idx"], want["idx"], f"{what}: idx against the oracle's search" if how == "search" else f"{what}: idx handed back")
        _same(got["out"], want["out"], f"{what}: out")
        _same_stats(got, want, what)
        again = m.forward_train(xd, idx=None if how == "search" else ld, return_idx=True, intermediates=True)
        _same_runs(again, fwd, ("idx", "out"), what)


# ---- the test-mode forward at the batch statistics -----------------------------------------------------------------------------

def _at_the_statistics(d, hfwd):
    Q = dict(d["P"])
    Q.update(hfwd["batch_stats"])
    assert any(not np.array_equal(_bits(Q[k]), _bits(d["P"][k])) for k in hfwd["batch_stats"])
    return Q


@pytest.mark.parametrize("family", AT_THE_STATISTICS)
def test_pointnet_test_mode_forward_at_the_batch_statistics(gpu_fx, family):
    """A fresh model loaded with the returned batch statistics: its test-mode forward gives the training-mode bits.  This ties
    sd for sigma2 = +0, subnormal and +Inf between the two kernel families with no restatement between them."""
    fx = gpu_fx
    c = _pointnet_case(fx, family)
    test_mode = fx.PointNet(md.POINTNET[2]).load(_at_the_statistics(c["d"], c["hfwd"])).forward(c["xd"], intermediates=True)
    for k in PN_FWD + ("probs",):
        _same_run(test_mode[k], c["fwd"][k], f"{family} PointNet: the test-mode forward at the batch statistics: {k}")


@pytest.mark.parametrize("family", AT_THE_STATISTICS)
def test_dgcnn_test_mode_forward_at_the_batch_statistics(gpu_fx, family):
    fx = gpu_fx
    N, B, K, nc = md.DGCNN
    c = _dgcnn_case(fx, family)
    test_mode = fx.DGCNN(nc, K, N).load(_at_the_statistics(c["d"], c["hfwd"])).forward(c["xd"], intermediates=True)
    for k in DG_LISTS + DG_FWD + ("probs",):
        _same_run(test_mode[k], c["fwd"][k], f"{family} DGCNN: the test-mode forward at the batch statistics: {k}")


@pytest.mark.parametrize("layers,N,B,K", md.EDGECONV, ids=_id)
@pytest.mark.parametrize("family", AT_THE_STATISTICS)
def test_edgeconv_test_mode_forward_at_the_batch_statistics(gpu_fx, family, layers, N, B, K):
    fx = gpu_fx
    c = _edgeconv_case(fx, layers, N, B, K, family)
    out, idx = fx.EdgeConv(layers, K).load(_at_the_statistics(c["d"], c["hfwd"])).forward(c["xd"], return_idx=True)
    _same_run(idx, c["fwd"]["idx"], f"{family} {layers}: the test-mode forward at the batch statistics: idx")
    _same_run(out, c["fwd"]["out"], f"{family} {layers}: the test-mode forward at the batch statistics: out")
