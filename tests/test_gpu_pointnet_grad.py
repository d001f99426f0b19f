"""The PointNet adjoint on the device (fx3d_pointnet_grad through fx.PointNet.grad / flat_grad / crossentropy_grad) against the
host restatement tests/pointnet_grad_ref.py, bit for bit (uint32 views, no element left out): the shape table -- one partial
tile with chains of one cloud and one class, a second tile of one point, a third tile and three clouds in every chain over b
--, tied maxima, dead channels, glogits = 0, run-to-run bits, batch independence, draws beyond unit scale, the ways to call it,
a captured graph, the cross-entropy wrapper and the C entry point's status codes.

The restatement is fed the same X.  The parameters are pointnet_ref.random_params(nc, seed=10), X and glogits standard normal;
a case's model and restatement are computed once and shared, unchanged."""
import ctypes

import numpy as np
import pytest

import model_draws
import pointnet_grad_ref as gref
import pointnet_ref as ref
from test_gpu_model_draws import _same as _same_nan

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID = -1   # FX3D_ERR_INVALID_ARG (include/flux3d_hip.h)
MID = ("gstn", "gfstn", "gh", "gxt")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a).astype(F32, copy=False)).view(np.uint32)


def _host(v):
    return v.to_host() if hasattr(v, "to_host") else np.asarray(v)


def _same(got, want, what):
    got = _host(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    print(f"{what}: {bad.size} of {got.size} elements differ")
    assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


def _same_grads(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))
    for name in want:
        _same(got[name], want[name], f"{what}: {name}")


def _all(got):
    """(grads, gx, mid) of grad(..., intermediates=True) on the host."""
    grads, gx, mid = got
    return {n: _host(v) for n, v in grads.items()}, _host(gx), {k: _host(v) for k, v in mid.items()}


def _same_all(got, want, what):
    grads, gx, mid = _all(got)
    assert list(mid) == list(MID)
    for k in MID:   # upstream first: where a mismatch begins
        _same(mid[k], want[2][k], f"{what}: {k}")
    _same(gx, want[1], f"{what}: gx")
    _same_grads(grads, want[0], what)


_cases = {}


def _case(fx, N, B, nc, P=None, X=None, tag=None, glogits=None, finite=True):
    """The model, X and glogits on host and device and the restatement of the gradient, computed once per shape.  finite=False
    lifts the assertion that the restatement is finite: for the draws that are non-finite on purpose, and no others."""
    key = (N, B, nc, tag)
    if key not in _cases:
        P = ref.random_params(nc, seed=10) if P is None else P
        m = fx.PointNet(nc).load(P)
        if X is None:
            X = np.asfortranarray(np.random.default_rng(500 + N).standard_normal((3, N, B)).astype(F32))
        if glogits is None:
            glogits = np.asfortranarray(np.random.default_rng(600 + N).standard_normal((nc, B)).astype(F32))
        keep = {}
        want = gref.grad(X, P, glogits, keep)
        assert not finite or (all(np.all(np.isfinite(v)) for v in want[0].values()) and np.all(np.isfinite(want[1])))
        _cases[key] = dict(m=m, P=P, X=X, glogits=glogits, xd=fx.gpu(X), gd=fx.gpu(glogits), want=want, **keep)
    return _cases[key]


# (N, B, num_classes)
CASES = [(33, 1, 1),      # one partial tile, chains of one cloud and one class
         (64, 2, 10),
         (65, 2, 40),     # the second tile holds one point
         (130, 3, 10)]    # a third tile of two points, three clouds in every chain over b


@pytest.mark.parametrize("N,B,nc", CASES, ids=lambda v: str(v))
def test_the_shape_table_against_the_restatement(gpu_fx, N, B, nc):
    c = _case(gpu_fx, N, B, nc)
    assert np.count_nonzero(c["want"][1]) > 0
    if N == 65:  # winners on both sides of the tile boundary in at least one round
        both = [k for k, n in c["nstar"].items() if np.any(n == 64) and np.any((n >= 0) & (n < 64))]
        print("rounds with winners on both sides of the tile boundary:", both)
        assert both
    _same_all(c["m"].grad(c["xd"], c["gd"], intermediates=True), c["want"], f"{(N, B, nc)} against the restatement")


def test_ties_go_to_the_first_point(gpu_fx):
    """Point 3 of X copied onto point 7 in every cloud: the transforms are per cloud, so the two rows stay identical through all
    three rounds; point 7 wins nothing, point 3 does, and gx[:, 7, :] is all +0."""
    N, B, nc = 65, 2, 40
    X = np.asfortranarray(np.random.default_rng(500 + N).standard_normal((3, N, B)).astype(F32))
    X[:, 7, :] = X[:, 3, :]
    c = _case(gpu_fx, N, B, nc, X=X, tag="ties")
    takes = {k: int(np.count_nonzero(n == 3)) for k, n in c["nstar"].items()}
    print("channels point 3 wins per round:", takes)
    assert all(not np.any(n == 7) for n in c["nstar"].values()) and all(v > 0 for v in takes.values())
    got = c["m"].grad(c["xd"], c["gd"], intermediates=True)
    _same_all(got, c["want"], "ties against the restatement")
    gx = _host(got[1])
    assert not _bits(gx[:, 7, :]).any() and np.count_nonzero(gx[:, 3, :]) > 0


def test_dead_channels(gpu_fx):
    """stn.conv3.bias = -1e3 on two channels: their relu is zero at every point, the winner is point 0, dW and db are +0, dbeta and
    dgamma the restatement's.  The same on feat.conv1: its dW column is +0, feat.conv2's rows for that channel are not."""
    N, B, nc = 65, 2, 10
    P = ref.random_params(nc, seed=10)
    P["stn.conv3.bias"][[9, 1000]] = -1e3
    P["feat.conv1.bias"][[5, 100]] = -1e3
    c = _case(gpu_fx, N, B, nc, P, tag="dead")
    fwd = c["forward"]
    assert not fwd["stn_stage"]["relu3"][:, :, [9, 1000]].any() and not fwd["feat_relu1"][:, :, [5, 100]].any()
    assert np.all(c["nstar"]["stn"][:, [9, 1000]] == 0)
    got = c["m"].grad(c["xd"], c["gd"], intermediates=True)
    _same_all(got, c["want"], "dead channels against the restatement")
    grads = _all(got)[0]
    for ch in (9, 1000):
        assert not _bits(grads["stn.conv3.weight"][0, :, ch]).any() and not _bits(grads["stn.conv3.bias"][ch]).any()
        assert grads["stn.bn3.beta"][ch] != 0 and grads["stn.bn3.gamma"][ch] != 0
    for ch in (5, 100):
        assert not _bits(grads["feat.conv1.weight"][0, :, ch]).any() and not _bits(grads["feat.conv1.bias"][ch]).any()
        assert np.count_nonzero(grads["feat.conv2.weight"][0, ch, :]) > 0


def test_zero_glogits_and_two_runs(gpu_fx):
    """glogits = 0: every result compares == 0.  Two runs give the same bits."""
    fx = gpu_fx
    c = _case(fx, 65, 2, 40)
    m = c["m"]
    first = _all(m.grad(c["xd"], c["gd"], intermediates=True))
    _same_all(m.grad(c["xd"], c["gd"], intermediates=True), first, "two runs")
    zg, zx, zmid = _all(m.grad(c["xd"], fx.gpu(np.zeros_like(c["glogits"])), intermediates=True))
    assert all(np.all(v == 0) for v in zg.values()) and np.all(zx == 0) and all(np.all(v == 0) for v in zmid.values())


def test_batch_independence(gpu_fx):
    """Each cloud alone gives that cloud's slice of gx, gh, gxt, gstn and gfstn bit for bit.  gparams is not expected to add up:
    its sums over the clouds are one chain, not the sum of the clouds' separate results (include/flux3d_hip.h)."""
    fx = gpu_fx
    c = _case(fx, 130, 3, 10)
    _, gx, mid = c["want"]
    for b in range(3):
        xb, gb = np.asfortranarray(c["X"][:, :, b:b + 1]), np.asfortranarray(c["glogits"][:, b:b + 1])
        _, gx1, mid1 = c["m"].grad(fx.gpu(xb), fx.gpu(gb), intermediates=True)
        _same(gx1, np.asfortranarray(gx[:, :, b:b + 1]), f"cloud {b} alone: gx")
        for k in MID:
            _same(mid1[k], np.asfortranarray(mid[k][:, :, b:b + 1]), f"cloud {b} alone: {k}")


UNIT_GLOGITS = ("negative_gamma", "sigma2_zero", "decades", "large")   # the first four: unit-scale glogits, no NaN anywhere


def _same_all_nan(got, want, what):
    """_same_all where the restatement may hold NaN: there the device must hold one (payload not compared), everything else --
    +-Inf and both zeros included -- bit for bit (tests/test_gpu_model_draws.py's _same)."""
    grads, gx, mid = _all(got)
    assert list(mid) == list(MID) and list(grads) == list(want[0])
    for k in MID:
        _same_nan(mid[k], want[2][k], f"{what}: {k}")
    _same_nan(gx, want[1], f"{what}: gx")
    for name in want[0]:
        _same_nan(grads[name], want[0][name], f"{what}: {name}")


@pytest.mark.parametrize("family", model_draws.families("pointnet"))
def test_draws_beyond_unit_scale(gpu_fx, family):
    """tests/model_draws.py's families at its PointNet shape.  negative_gamma, sigma2_zero, decades and large run with a seeded
    unit-scale glogits and are finite in the restatement before the device is compared, every bit.  negative_gamma makes whole
    channels of stn / fstn tie at the first point (a negative gamma turns the relu's zeros into the channel's maximum).  The others
    take model_draws.upstream's glogits (small on the even clouds under decades_small / decades_edge) and are finite too, except
    the two that are non-finite on purpose: overflow (the restatement's dW holds NaN -- measured 19 % -- and, one cloud's pooled
    being NaN and the other's logits dead, its gx is all zero) and sigma2_edges (gx, gstn, gfstn, gh and gxt are NaN throughout and
    every parameter family holds NaN).  Where the restatement has a NaN the device must have one."""
    N, B, nc = model_draws.POINTNET
    net = ("pointnet", nc)
    d = model_draws.draw(family, net, N, B)
    if family in UNIT_GLOGITS:
        c = _case(gpu_fx, N, B, nc, d["P"], d["X"], tag=family)
        if family == "negative_gamma":
            n0 = {k: int(np.count_nonzero(c["nstar"][k] == 0)) for k in ("stn", "fstn")}
            print("channels won by point 0:", n0)
            assert all(v > 1024 * B // 8 for v in n0.values())
        _same_all(c["m"].grad(c["xd"], c["gd"], intermediates=True), c["want"], f"{family} against the restatement")
        return
    c = _case(gpu_fx, N, B, nc, d["P"], d["X"], tag=family, glogits=model_draws.upstream(family, net, N, B),
              finite=family not in ("overflow", "sigma2_edges"))
    grads, gx, mid = c["want"]
    nan = {f: float(np.mean(np.isnan(gref.family(grads, f)))) for f in gref.FAMILIES}
    print(f"{family}: NaN shares of the restatement {nan}, of gx {float(np.mean(np.isnan(gx))):.2f}")
    if family == "overflow":
        assert nan["dW"] >= 0.1 and not gx.any(), (nan, int(np.count_nonzero(gx)))
    elif family == "sigma2_edges":
        assert all(v > 0 for v in nan.values()) and np.all(np.isnan(gx)) and all(np.all(np.isnan(v)) for v in mid.values()), nan
    else:
        assert np.count_nonzero(gx) > 0 and np.count_nonzero(gref.family(grads, "dW")) > 0
    _same_all_nan(c["m"].grad(c["xd"], c["gd"], intermediates=True), c["want"], f"{family} against the restatement")


def test_the_ways_to_call_it_agree(gpu_fx):
    fx = gpu_fx
    c = _case(fx, 130, 3, 10)
    m, xd, gd = c["m"], c["xd"], c["gd"]
    grads, gx, mid = c["want"]
    flat, fgx = m.flat_grad(xd, gd)
    _same(flat, gref.flat(grads), "flat_grad against grad, flattened")
    _same(fgx, gx, "flat_grad's gx")
    assert _host(flat).shape == (m.param_count,)
    f2, g2, mid2 = m.flat_grad(xd, gd, intermediates=True)
    _same(f2, gref.flat(grads), "flat_grad with intermediates")
    for k in MID:
        _same(mid2[k], mid[k], f"flat_grad's {k}")
    alone, none = m.grad(xd, gd, input_grad=False)
    assert none is None and m.flat_grad(xd, gd, input_grad=False)[1] is None
    _same_grads({n: _host(v) for n, v in alone.items()}, grads, "input_grad = False")


def test_numpy_in_numpy_out(gpu_fx):
    c = _case(gpu_fx, 33, 1, 1)
    m = c["m"]
    got = m.grad(c["X"], c["glogits"], intermediates=True)
    assert all(isinstance(v, np.ndarray) and v.dtype == F32 for v in got[0].values()) and isinstance(got[1], np.ndarray)
    assert {n: v.shape for n, v in got[0].items()} == ref.param_shapes(1) and got[1].shape == (3, 33, 1)
    _same_all(got, c["want"], "numpy in, numpy out")
    flat, gx = m.flat_grad(c["X"][:, :, 0], c["glogits"][:, 0])   # one cloud as (3, N), its glogits as (nc,)
    assert isinstance(flat, np.ndarray) and flat.shape == (m.param_count,)
    _same(flat, gref.flat(c["want"][0]), "flat_grad, numpy, one cloud")
    _same(gx, c["want"][1], "flat_grad, numpy: gx")
    with pytest.raises(TypeError, match="where X lives"):
        m.grad(c["xd"], c["glogits"])
    with pytest.raises(TypeError, match="where X lives"):
        m.grad(c["X"], c["gd"])


def test_graph_replay(gpu_fx):
    fx = gpu_fx
    c = _case(fx, 65, 2, 40)
    m = c["m"]
    s = fx.Stream.create()
    with fx.stream(s):
        xs, gs = fx.gpu(c["X"]), fx.gpu(c["glogits"])
        m.flat_grad(xs, gs)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec, rgx = m.flat_grad(xs, gs)  # the forward's rounds are inside the capture
        g.launch()
        g.launch()
        s.synchronize()
        _same(rec, gref.flat(c["want"][0]), "graph replay against the eager bits")
        _same(rgx, c["want"][1], "graph replay: gx")


def test_crossentropy_grad(gpu_fx):
    fx = gpu_fx
    N, B, nc = 65, 2, 40
    c = _case(fx, N, B, nc)
    m, labels = c["m"], np.array([3, 17])
    loss, grads, gx = m.crossentropy_grad(c["xd"], labels)
    probs = m.forward(c["xd"]).to_host()
    want_loss = float(-np.mean(np.log(probs[labels, np.arange(B)].astype(np.float64))))
    assert isinstance(loss, float) and loss == want_loss and np.isfinite(loss) and loss > 0
    onehot = np.zeros((nc, B), F32)
    onehot[labels, np.arange(B)] = 1
    glogits = np.asfortranarray(((probs - onehot).astype(F32) / F32(B)).astype(F32))
    wg, wx = m.grad(c["xd"], fx.gpu(glogits))
    _same_grads({n: _host(v) for n, v in grads.items()}, {n: _host(v) for n, v in wg.items()}, "crossentropy_grad against grad")
    _same(gx, _host(wx), "crossentropy_grad: gx")
    assert np.count_nonzero(_host(gx)) > 0
    hl, hg, hx = m.crossentropy_grad(c["X"], [3, 17])
    assert hl == loss and isinstance(hx, np.ndarray)
    _same(hx, _host(wx), "crossentropy_grad, numpy: gx")
    with pytest.raises(ValueError, match="labels must be in"):
        m.crossentropy_grad(c["xd"], [3, nc])


def test_status_codes(gpu_fx):
    """The refusals of tests/test_pointnet_grad_host.py with real device arrays around calls that run."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    lib = _lib.load()
    N, B, nc = 65, 2, 40
    c = _case(fx, N, B, nc)
    m, x, g = c["m"], c["xd"], c["gd"]
    gp = DeviceArray.empty((m.param_count,), np.float32)
    gx = DeviceArray.empty((3, N, B), np.float32)
    nb = ctypes.c_size_t(0)
    assert lib.fx3d_pointnet_grad_workspace_bytes(N, B, nc, ctypes.byref(nb)) == 0 and nb.value > 0
    ws = DeviceArray.empty((nb.value + 512,), np.uint8)
    assert ws.ptr % 256 == 0
    pd = m._params_dev()

    def call(params=pd.ptr, nc_=nc, x_=x.ptr, N_=N, B_=B, g_=g.ptr, gp_=gp.ptr, gx_=gx.ptr, ws_=ws.ptr, bytes_=nb.value):
        return lib.fx3d_pointnet_grad(params, nc_, x_, N_, B_, g_, gp_, gx_, None, None, None, None, ws_, bytes_, None)

    assert call() == 0
    fx.synchronize()
    _same(gp, gref.flat(c["want"][0]), "the C entry point")
    _same(gx, c["want"][1], "the C entry point: gx")
    assert call(gx_=None) == 0   # every optional output NULL
    fx.synchronize()
    _same(gp, gref.flat(c["want"][0]), "optional outputs NULL through the C entry point")
    assert call(params=None) == INVALID and call(x_=None) == INVALID and call(g_=None) == INVALID
    assert call(gp_=None) == INVALID and call(ws_=None) == INVALID
    assert call(nc_=0) == INVALID and "num_classes" in _lib.last_error()
    assert call(N_=0) == INVALID and call(B_=0) == INVALID
    assert call(bytes_=nb.value - 1) == INVALID and "workspace" in _lib.last_error()
    assert call(ws_=ws.ptr + 16) == INVALID and "aligned" in _lib.last_error()
    for args in ((0, B, nc), (N, 0, nc), (N, B, 0)):
        assert lib.fx3d_pointnet_grad_workspace_bytes(*args, ctypes.byref(nb)) == INVALID, args
    assert lib.fx3d_pointnet_grad_workspace_bytes(N, B, nc, None) == INVALID
    fx.synchronize()
    _same(gp, gref.flat(c["want"][0]), "gparams after the refusals")
    with pytest.raises(TypeError, match="Float32"):
        m.grad(x, DeviceArray.empty((nc, B), np.float64))
    with pytest.raises(ValueError, match="glogits must be"):
        m.grad(x, DeviceArray.empty((nc, 1), np.float32))
