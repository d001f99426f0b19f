"""The exact-Float32 model kernels on the device against their host restatements, bit for bit, on the draw families of
tests/model_draws.py: subnormal inputs and intermediates, values over many decades, magnitudes whose squares leave Float32,
overflow to Inf and NaN, negative gamma, sigma2 at 0, -eps and -1, and a constant cloud (every maximum and every neighbour list
one tie) -- where the six model test files draw unit-scale inputs and one well-behaved parameter set.

Entry points and shapes (the smallest at which every path of the kernels is taken): EdgeConv forward / input_grad / grad for
the three layer tables of model_draws.EDGECONV, each with the device's own search and with given lists; DGCNN forward and grad
at N = 65, B = 2, K = 3, 10 classes, with fwd given and with fwd = None; PointNet forward at N = 65, B = 2, 10 classes.

Every array the existing tests compare bitwise is compared as uint32, no element left out.  Where the restatement has a NaN the
device must have one too and the payloads are not compared (test_infinite_weights_in_the_backward_tails' convention); +-Inf and
both zeros are compared bit for bit.  The neighbour lists are compared with the oracle's search (through the restatement) in
every family.  The adjoints are fed the device's own forward.  Every draw is first held to its family's condition on the
restatement's own result.  Two runs give the same bits in every family."""
import numpy as np
import pytest

import dgcnn_grad_ref as gref
import dgcnn_ref
import model_draws as md
import pointnet_ref

pytestmark = pytest.mark.gpu

F32 = np.float32


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype == np.int32 else a.astype(F32, copy=False)).view(np.uint32)


def _host(v):
    return v.to_host() if hasattr(v, "to_host") else np.asarray(v)


def _same(got, want, what):
    """Bit for bit; where `want` is NaN, `got` must be NaN (any payload)."""
    got, want = _host(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if want.dtype == np.int32:
        nan = np.zeros(want.shape, bool)
    else:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, "the NaN masks differ", int(np.isnan(got).sum()), int(nan.sum()))
    bad = np.flatnonzero(((_bits(got) != _bits(want)) & ~nan).ravel())
    print(f"{what}: {bad.size} of {got.size} elements differ" + (f" ({int(nan.sum())} NaN in both)" if nan.any() else ""))
    assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


def _same_grads(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))
    for name in want:
        _same(got[name], want[name], f"{what}: {name}")


def _same_run(a, b, what):
    """Two runs of the device: the same bits, NaN payloads included."""
    a, b = _host(a), _host(b)
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"{what}: two runs differ"


def _id(v):
    return str(v).replace(" ", "").replace("'", "")


# ---- EdgeConv ------------------------------------------------------------------------------------------------------------------

EC_CASES = [(layers, N, B, K, f) for layers, N, B, K in md.EDGECONV for f in md.families("edgeconv")]


@pytest.mark.parametrize("layers,N,B,K,family", EC_CASES, ids=_id)
def test_edgeconv(gpu_fx, layers, N, B, K, family):
    """forward, input_grad and grad: once with the device's own search (inside each call: idx = None, out = None; the lists
    against the oracle's), once with given lists (and the device's own out handed to the adjoints)."""
    fx = gpu_fx
    net = ("edgeconv", layers)
    d = md.draw(family, net, N, B)
    m = fx.EdgeConv(layers, K).load(d["P"])
    xd, gd = fx.gpu(d["X"]), fx.gpu(d["g"])
    for how, lists in (("search", None), ("given lists", md.given_lists(N, B, K))):
        what = f"{family} {layers} {how}"
        want = md.restate_forward(net, d, K, idx=lists)
        if not (family == "constant_cloud" and lists is not None):   # (its condition is on the search's lists)
            md.check_forward(family, net, d, want, tag=how + ": ")
        out, idx = m.forward(xd, idx=None if lists is None else fx.gpu(lists), return_idx=True)
        _same(idx, want["idx"], f"{what}: idx against the oracle's search" if lists is None else f"{what}: idx handed back")
        _same(out, want["out"], f"{what}: out")
        hfwd = {"idx": idx.to_host(), "out": out.to_host()}
        G, gx, _ = md.restate_grads(net, d, K, hfwd)
        md.check_grads(family, net, d, G, gx, tag=how + ": ")
        given = {} if lists is None else dict(idx=idx, out=out)
        got_gx = m.input_grad(xd, gd, **given)
        _same(got_gx, gx, f"{what}: input_grad")
        grads, ggx = m.grad(xd, gd, **given)
        _same_grads(grads, G, f"{what}: grad")
        _same(ggx, gx, f"{what}: grad's gx")
        out2, idx2 = m.forward(xd, idx=None if lists is None else fx.gpu(lists), return_idx=True)
        _same_run(out2, out, what + " out")
        _same_run(idx2, idx, what + " idx")
        _same_run(m.input_grad(xd, gd, **given), got_gx, what + " input_grad")
        again, agx = m.grad(xd, gd, **given)
        for n in grads:
            _same_run(again[n], grads[n], f"{what} grad {n}")
        _same_run(agx, ggx, what + " grad's gx")


# ---- DGCNN ---------------------------------------------------------------------------------------------------------------------

FWD = ("idx1", "x1", "idx2", "x2", "pooled", "logits")
_dgcnn = {}


def _check_probs(family, got, what):
    """expf is no part of the bit-for-bit claim.  Per cloud: finite logits give finite probabilities in [0, 1] whose largest sits
    at the largest logit; a NaN logit gives NaN probabilities.  The 1e-5 relative check of the existing tests runs on the draws
    that meet its own condition (every probability in [1e-4, 1 - 1e-4]): negative_gamma."""
    logits, probs = got["logits"], got["probs"]
    assert probs.shape == logits.shape
    for b in range(logits.shape[1]):
        z, p = logits[:, b], probs[:, b]
        if np.all(np.isfinite(z)):
            assert np.all(np.isfinite(p)) and p.min() >= 0 and p.max() <= 1, (what, b, p)
            assert p[int(np.argmax(z))] == p.max(), (what, b, z, p)
        elif np.isnan(z).any():
            assert np.all(np.isnan(p)), (what, b, p)
    if family == "negative_gamma":
        want = pointnet_ref.softmax64(logits)
        rel = float(np.max(np.abs(probs.astype(np.float64) - want) / want))
        print(f"{what}: probabilities, largest relative deviation from the Float64 softmax {rel:.3e}; smallest probability {want.min():.3e}")
        assert want.min() >= 1e-4 and want.max() <= 1 - 1e-4, (want.min(), want.max())
        assert rel <= 1e-5, rel


def _dgcnn_case(fx, family):
    """The model, the draw on host and device, the device's own forward and the restatement of its gradient, once per family."""
    if family not in _dgcnn:
        N, B, K, nc = md.DGCNN
        net = ("dgcnn", nc)
        d = md.draw(family, net, N, B)
        m = fx.DGCNN(nc, K, N).load(d["P"])
        xd, gd = fx.gpu(d["X"]), fx.gpu(d["g"])
        fwd = m.forward(xd, intermediates=True)
        hfwd = {k: v.to_host() for k, v in fwd.items()}
        G, gx, extra = md.restate_grads(net, d, K, hfwd)
        _dgcnn[family] = dict(net=net, d=d, m=m, xd=xd, gd=gd, fwd=fwd, hfwd=hfwd, want=(G, gx, extra["gx2"], extra["gx1"]))
    return _dgcnn[family]


def _same_all(got, want, what):
    grads, gx, mid = got
    _same_grads({n: _host(v) for n, v in grads.items()}, want[0], what)
    for name, g, w in (("gx", gx, want[1]), ("gx2", mid["gx2"], want[2]), ("gx1", mid["gx1"], want[3])):
        _same(g, w, f"{what}: {name}")


@pytest.mark.parametrize("family", md.families("dgcnn"))
def test_dgcnn(gpu_fx, family):
    fx = gpu_fx
    N, B, K, nc = md.DGCNN
    c = _dgcnn_case(fx, family)
    d, m, net = c["d"], c["m"], c["net"]
    want = dgcnn_ref.forward(d["X"], d["P"], K)
    md.check_forward(family, net, d, want)
    for k in FWD:
        _same(c["hfwd"][k], want[k], f"{family} DGCNN forward: {k}" + (" against the oracle's search" if k.startswith("idx") else ""))
    _check_probs(family, c["hfwd"], f"{family} DGCNN")
    md.check_grads(family, net, d, c["want"][0], c["want"][1])
    got = m.grad(c["xd"], c["gd"], fwd=c["fwd"], intermediates=True)
    _same_all(got, c["want"], f"{family} DGCNN.grad, fwd given")
    none = m.grad(c["xd"], c["gd"], intermediates=True)
    _same_all(none, c["want"], f"{family} DGCNN.grad, fwd = None")
    again = m.forward(c["xd"], intermediates=True)
    for k in FWD + ("probs",):
        _same_run(again[k], c["fwd"][k], f"{family} forward {k}")
    for n in got[0]:
        _same_run(none[0][n], got[0][n], f"{family} grad {n}")
    for a, b, n in ((none[1], got[1], "gx"), (none[2]["gx2"], got[2]["gx2"], "gx2"), (none[2]["gx1"], got[2]["gx1"], "gx1")):
        _same_run(a, b, f"{family} grad {n}")


def test_dgcnn_constant_cloud_ties(gpu_fx):
    """Every activation is tied over k and over the points: point 0 takes all of gx2 (rows 1 .. N-1 are +0 bits, row 0 is not), the
    first k takes every last-layer gradient of both EdgeConv stages (dbeta of the stage's last layer is the sum of its gout over
    the points on the live channels, not K times it), and the ec2 / ec1 slices are EdgeConv.grad's on the same stage."""
    fx = gpu_fx
    N, B, K, nc = md.DGCNN
    c = _dgcnn_case(fx, "constant_cloud")
    m, fwd, hfwd, P = c["m"], c["fwd"], c["hfwd"], c["d"]["P"]
    grads, gx, mid = m.grad(c["xd"], c["gd"], fwd=fwd, intermediates=True)
    grads = {n: _host(v) for n, v in grads.items()}
    gx2, gx1 = _host(mid["gx2"]), _host(mid["gx1"])
    assert not _bits(gx2[:, 1:, :]).any(), "gx2 beyond point 0"
    assert all(np.count_nonzero(gx2[:, 0, b]) > 0 for b in range(B))
    for stage, L, g, out in (("ec2", 2, gx2, hfwd["x2"]), ("ec1", 3, gx1, hfwd["x1"])):
        live = out[:, 0, :] > 0
        want = np.where(live, g.astype(np.float64).sum(axis=1), 0.0).sum(axis=1)
        assert np.count_nonzero(want) > 0
        assert np.allclose(grads[f"{stage}.bn{L}.beta"].astype(np.float64), want, rtol=1e-4, atol=1e-6 * np.abs(want).max()), stage
    for name, layers, x, g, idx, out, gin in (("ec2", gref.L2, fwd["x1"], gx2, fwd["idx2"], fwd["x2"], gx1),
                                              ("ec1", gref.L1, c["xd"], gx1, fwd["idx1"], fwd["x1"], _host(gx))):
        ec = fx.EdgeConv(layers, K).load(gref.stage_params(P, name))
        eg, egx = ec.grad(x, fx.gpu(g), idx, out)
        _same_grads({f"{name}.{n}": _host(v) for n, v in eg.items()}, {n: v for n, v in grads.items() if n.startswith(name + ".")},
                    f"constant cloud: the {name} slice against EdgeConv.grad")
        _same(egx, gin, f"constant cloud: {name}: the input gradient against EdgeConv.grad's")


def test_dgcnn_graph_replay_subnormal_mid(gpu_fx):
    """flat_grad of the subnormal_mid draw through a captured graph, the search and the forward inside the capture."""
    fx = gpu_fx
    c = _dgcnn_case(fx, "subnormal_mid")
    m, d = c["m"], c["d"]
    s = fx.Stream.create()
    with fx.stream(s):
        xs, gs = fx.gpu(d["X"]), fx.gpu(d["g"])
        m.flat_grad(xs, gs)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec, rgx = m.flat_grad(xs, gs)
        g.launch()
        g.launch()
        s.synchronize()
        _same(rec, gref.flat(c["want"][0]), "subnormal_mid: graph replay of flat_grad against the restatement")
        _same(rgx, c["want"][1], "subnormal_mid: graph replay: gx")


# ---- PointNet ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", md.families("pointnet"))
def test_pointnet(gpu_fx, family):
    fx = gpu_fx
    N, B, nc = md.POINTNET
    net = ("pointnet", nc)
    d = md.draw(family, net, N, B)
    want = pointnet_ref.forward(d["X"], d["P"])
    md.check_forward(family, net, d, want)
    m = fx.PointNet(nc).load(d["P"])
    xd = fx.gpu(d["X"])
    got = m.forward(xd, intermediates=True)
    hgot = {k: v.to_host() for k, v in got.items()}
    for k in ("logits", "stn", "fstn", "pooled"):
        md.describe(f"{family} pointnet {k}", want[k])
        _same(hgot[k], want[k], f"{family} PointNet forward: {k}")
    _check_probs(family, hgot, f"{family} PointNet")
    again = m.forward(xd, intermediates=True)
    for k in hgot:
        _same_run(again[k], got[k], f"{family} PointNet {k}")


# ---- the search itself on small clouds -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1e-11, 1e-13, 1e-20, 1e-29, 1e-36])
@pytest.mark.parametrize("D", [3, 5, 64])
def test_search_where_squared_distances_underflow(gpu_fx, oracle, D, scale):
    """fx3d_knn on a standard normal cloud times `scale` against the oracle, D = 3 and D = 64 (the two fp16-filtered kernels) and
    D = 5 (the general one).  At 1e-11 and 1e-13 (either side of the filter's smallest extent) the squared distances are normal
    numbers, at 1e-20 subnormal ones with a few bits each, at 1e-29 and 1e-36 all +0: one tie, ordered by index.  (The decades_small
    draw found the filter ranking a cloud of extent 1e-29 by its scaled image.)"""
    fx = gpu_fx
    N, B, K = 130, 2, 6
    x = np.asfortranarray((np.random.default_rng([D, 9]).standard_normal((D, N, B)) * scale).astype(F32))
    want, wd = oracle.knn(x, K, drop_first=True)
    distinct = len({tuple(want[:, n, b]) for n in range(N) for b in range(B)})
    print(f"D = {D}, scale {scale:g}: {distinct} distinct lists of {N * B}; largest distance {wd.max():.3e}")
    assert (distinct == 1) == (scale < 1e-25), distinct
    idx, dist = fx.knn(fx.gpu(x), K, drop_first=True)
    _same(idx, want, f"fx3d_knn D = {D}, scale {scale:g}: idx against the oracle")
    _same(dist, wd, f"fx3d_knn D = {D}, scale {scale:g}: distances against the oracle")
