"""The PointNet training-mode adjoint on the device (fx3d_pointnet_grad_train through fx.PointNet.grad_train / flat_grad_train /
crossentropy_grad_train) against the host restatement tests/pointnet_grad_train_ref.py, bit for bit (uint32 views, no element left
out): gparams by name, gx, gstn, gfstn, gh and gxt, upstream first.  The shape table -- one partial tile, a full tile, a second tile
of one point, three clouds in every chain over b, more tile sums than FX3D_POINTNET_STAT_GROUPS --, a dropout mask with both values,
tied maxima, a channel dead over the whole batch (sigma2 = 0), run-to-run bits, the ways to call it, a captured graph, the
cross-entropy wrapper and the C entry point's status codes.

The parameters are pointnet_ref.random_params(nc, seed=10), X and glogits standard normal; a case's model and restatement are
computed once and shared, unchanged."""
import ctypes

import numpy as np
import pytest

import pointnet_grad_train_ref as gtref
import pointnet_ref as ref

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


def _case(fx, N, B, nc, P=None, X=None, dropout=None, tag=None):
    """The model, X, glogits and the dropout mask on host and device and the restatement of the gradient, once per case."""
    key = (N, B, nc, tag)
    if key not in _cases:
        P = ref.random_params(nc, seed=10) if P is None else P
        m = fx.PointNet(nc).load(P)
        if X is None:
            X = np.asfortranarray(np.random.default_rng(500 + N).standard_normal((3, N, B)).astype(F32))
        glogits = np.asfortranarray(np.random.default_rng(600 + N).standard_normal((nc, B)).astype(F32))
        keep = {}
        want = gtref.grad_train(X, P, glogits, dropout, keep)
        assert all(np.all(np.isfinite(v)) for v in want[0].values()) and np.all(np.isfinite(want[1]))
        _cases[key] = dict(m=m, P=P, X=X, glogits=glogits, xd=fx.gpu(X), gd=fx.gpu(glogits), dropout=dropout,
                           dd=None if dropout is None else fx.gpu(dropout), want=want, **keep)
    return _cases[key]


# (N, B, num_classes)
CASES = [(33, 2, 1),      # one partial tile
         (64, 2, 10),
         (65, 2, 40),     # the second tile holds one point
         (130, 3, 10),    # three clouds in every chain over b
         (65, 34, 10)]    # 68 tile sums: the interleaved fold of FX3D_POINTNET_STAT_GROUPS = 32 chains wraps


@pytest.mark.parametrize("N,B,nc", CASES, ids=lambda v: str(v))
def test_the_shape_table_against_the_restatement(gpu_fx, N, B, nc):
    c = _case(gpu_fx, N, B, nc)
    assert np.count_nonzero(c["want"][1]) > 0
    if (N, B) == (65, 2):  # winners on both sides of the tile boundary in at least one round
        both = [k for k, n in c["nstar"].items() if np.any(n == 64) and np.any((n >= 0) & (n < 64))]
        print("rounds with winners on both sides of the tile boundary:", both)
        assert both
    _same_all(c["m"].grad_train(c["xd"], c["gd"], intermediates=True), c["want"], f"{(N, B, nc)} against the restatement")


def _mask(fx, B, seed=3):
    mask = fx.PointNet.dropout_mask(B, seed)
    assert np.any(mask == 0) and np.any(mask != 0)
    return mask


def test_a_dropout_mask(gpu_fx):
    N, B, nc = 65, 2, 40
    c = _case(gpu_fx, N, B, nc, dropout=_mask(gpu_fx, B), tag="dropout")
    plain = _case(gpu_fx, N, B, nc)
    assert np.any(_bits(c["want"][1]) != _bits(plain["want"][1]))   # the mask reaches gx
    _same_all(c["m"].grad_train(c["xd"], c["gd"], dropout=c["dd"], intermediates=True), c["want"], "a dropout mask")
    ones = gpu_fx.gpu(np.asfortranarray(np.ones((256, B), F32)))
    _same_all(c["m"].grad_train(c["xd"], c["gd"], dropout=ones, intermediates=True), plain["want"], "an all-one mask")


def test_ties_go_to_the_first_point(gpu_fx):
    """Point 3 of X copied onto point 7 in every cloud: the two rows stay identical through all three rounds; point 7 wins
    nothing, point 3 does.  (gx[:, 7] is not zero here: dbeta / m and xh dgamma / m reach every point.)"""
    N, B, nc = 65, 2, 40
    X = np.asfortranarray(np.random.default_rng(500 + N).standard_normal((3, N, B)).astype(F32))
    X[:, 7, :] = X[:, 3, :]
    c = _case(gpu_fx, N, B, nc, X=X, tag="ties")
    takes = {k: int(np.count_nonzero(n == 3)) for k, n in c["nstar"].items()}
    print("channels point 3 wins per round:", takes)
    assert all(not np.any(n == 7) for n in c["nstar"].values()) and all(v > 0 for v in takes.values())
    _same_all(c["m"].grad_train(c["xd"], c["gd"], intermediates=True), c["want"], "ties against the restatement")


def test_a_channel_dead_over_the_batch(gpu_fx):
    """stn.conv2.bias = feat.conv1.bias = -1e3 on two channels: their relu is zero at every point of the batch, so sigma2 = 0,
    xh = 0, sd = sqrt(eps); dW and db of the channel are +0, dgamma is 0 and dbeta the restatement's."""
    N, B, nc = 65, 2, 10
    P = ref.random_params(nc, seed=10)
    P["stn.conv2.bias"][[9, 100]] = -1e3
    P["feat.conv1.bias"][[5, 100]] = -1e3
    c = _case(gpu_fx, N, B, nc, P, tag="dead")
    stats = c["forward"]["batch_stats"]
    assert not stats["stn.bn2.sigma2"][[9, 100]].any() and not stats["feat.bn1.sigma2"][[5, 100]].any()
    got = c["m"].grad_train(c["xd"], c["gd"], intermediates=True)
    _same_all(got, c["want"], "dead channels against the restatement")
    grads = _all(got)[0]
    for name, bn, chans in (("stn.conv2", "stn.bn2", (9, 100)), ("feat.conv1", "feat.bn1", (5, 100))):
        for ch in chans:
            assert not _bits(grads[name + ".weight"][0, :, ch]).any() and not _bits(grads[name + ".bias"][ch]).any()
            assert grads[bn + ".gamma"][ch] == 0 and grads[bn + ".beta"][ch] != 0


def test_two_runs(gpu_fx):
    c = _case(gpu_fx, 65, 2, 40)
    first = _all(c["m"].grad_train(c["xd"], c["gd"], intermediates=True))
    _same_all(c["m"].grad_train(c["xd"], c["gd"], intermediates=True), first, "two runs")


def test_the_ways_to_call_it_agree(gpu_fx):
    fx = gpu_fx
    N, B, nc = 65, 2, 40
    c = _case(fx, N, B, nc, dropout=_mask(fx, B), tag="dropout")
    m, xd, gd, dd = c["m"], c["xd"], c["gd"], c["dd"]
    grads, gx, mid = c["want"]
    fwd = m.forward_train(xd, dropout=dd, intermediates=True)
    _same_all(m.grad_train(xd, gd, dropout=dd, fwd=fwd, intermediates=True), c["want"], "fwd given")
    flat, fgx = m.flat_grad_train(xd, gd, dropout=dd)
    _same(flat, gtref.flat(grads), "flat_grad_train against grad_train, flattened")
    _same(fgx, gx, "flat_grad_train's gx")
    assert _host(flat).shape == (m.param_count,)
    alone, none = m.grad_train(xd, gd, dropout=dd, input_grad=False)
    assert none is None
    _same_grads({n: _host(v) for n, v in alone.items()}, grads, "input_grad = False")
    got = m.grad_train(c["X"], c["glogits"], dropout=c["dropout"], intermediates=True)   # numpy in, numpy out
    assert all(isinstance(v, np.ndarray) and v.dtype == F32 for v in got[0].values()) and isinstance(got[1], np.ndarray)
    _same_all(got, c["want"], "numpy in, numpy out")
    hfwd = m.forward_train(c["X"], dropout=c["dropout"], intermediates=True)
    _same_all(m.grad_train(c["X"], c["glogits"], dropout=c["dropout"], fwd=hfwd, intermediates=True), c["want"], "numpy, fwd given")
    _same(m.flat_grad_train(xd, gd, dropout=3)[0], gtref.flat(grads), "dropout as the seed of dropout_mask")
    with pytest.raises(TypeError, match="where X lives"):
        m.grad_train(xd, c["glogits"])
    with pytest.raises(TypeError, match="where X lives"):
        m.grad_train(c["X"], c["glogits"], fwd=fwd)
    with pytest.raises(ValueError, match="two clouds"):
        m.grad_train(c["X"][:, :, :1], c["glogits"][:, :1])


def test_graph_replay(gpu_fx):
    fx = gpu_fx
    c = _case(fx, 65, 2, 40)
    m = c["m"]
    s = fx.Stream.create()
    with fx.stream(s):
        xs, gs = fx.gpu(c["X"]), fx.gpu(c["glogits"])
        fwd = m.forward_train(xs, intermediates=True)
        m.flat_grad_train(xs, gs, fwd=fwd)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec, rgx = m.flat_grad_train(xs, gs, fwd=fwd)
        g.launch()
        g.launch()
        s.synchronize()
        _same(rec, gtref.flat(c["want"][0]), "graph replay against the eager bits")
        _same(rgx, c["want"][1], "graph replay: gx")


def test_crossentropy_grad_train(gpu_fx):
    fx = gpu_fx
    N, B, nc = 65, 2, 40
    c = _case(fx, N, B, nc, dropout=_mask(fx, B), tag="dropout")
    m, labels = c["m"], np.array([3, 17])
    loss, grads, gx = m.crossentropy_grad_train(c["xd"], labels, dropout=c["dd"])
    probs = m.forward_train(c["xd"], dropout=c["dd"]).to_host()
    want_loss = float(-np.mean(np.log(probs[labels, np.arange(B)].astype(np.float64))))
    assert isinstance(loss, float) and loss == want_loss and np.isfinite(loss) and loss > 0
    onehot = np.zeros((nc, B), F32)
    onehot[labels, np.arange(B)] = 1
    glogits = np.asfortranarray(((probs - onehot).astype(F32) / F32(B)).astype(F32))
    wg, wx, _ = gtref.grad_train(c["X"], c["P"], glogits, c["dropout"])
    _same_grads({n: _host(v) for n, v in grads.items()}, wg, "crossentropy_grad_train against the restatement")
    _same(gx, wx, "crossentropy_grad_train: gx")
    assert np.count_nonzero(wx) > 0
    hl, hg, hx = m.crossentropy_grad_train(c["X"], [3, 17], dropout=c["dropout"])
    assert hl == loss and isinstance(hx, np.ndarray)
    _same(hx, wx, "crossentropy_grad_train, numpy: gx")
    with pytest.raises(ValueError, match="labels must be in"):
        m.crossentropy_grad_train(c["xd"], [3, nc])


def test_status_codes(gpu_fx):
    """The refusals of tests/test_pointnet_grad_train_host.py with real device arrays around calls that run."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    lib = _lib.load()
    N, B, nc = 65, 2, 40
    c = _case(fx, N, B, nc)
    m, x, g = c["m"], c["xd"], c["gd"]
    stats = fx.gpu(np.concatenate([c["forward"]["batch_stats"][k] for k in c["forward"]["batch_stats"]]).astype(F32))
    gp = DeviceArray.empty((m.param_count,), np.float32)
    gx = DeviceArray.empty((3, N, B), np.float32)
    nb = ctypes.c_size_t(0)
    assert lib.fx3d_pointnet_grad_train_workspace_bytes(N, B, nc, ctypes.byref(nb)) == 0 and nb.value > 0
    ws = DeviceArray.empty((nb.value + 512,), np.uint8)
    assert ws.ptr % 256 == 0
    pd = m._params_dev()

    def call(params=pd.ptr, nc_=nc, x_=x.ptr, N_=N, B_=B, st_=stats.ptr, g_=g.ptr, gp_=gp.ptr, gx_=gx.ptr, ws_=ws.ptr, bytes_=nb.value):
        return lib.fx3d_pointnet_grad_train(params, nc_, x_, N_, B_, None, st_, g_, gp_, gx_, None, None, None, None, ws_, bytes_, None)

    assert call() == 0
    fx.synchronize()
    _same(gp, gtref.flat(c["want"][0]), "the C entry point")
    _same(gx, c["want"][1], "the C entry point: gx")
    assert call(gx_=None) == 0   # every optional output NULL
    fx.synchronize()
    _same(gp, gtref.flat(c["want"][0]), "optional outputs NULL through the C entry point")
    assert call(params=None) == INVALID and call(x_=None) == INVALID and call(g_=None) == INVALID and call(st_=None) == INVALID
    assert call(gp_=None) == INVALID and call(ws_=None) == INVALID
    assert call(nc_=0) == INVALID and "num_classes" in _lib.last_error()
    assert call(N_=0) == INVALID and call(B_=0) == INVALID
    assert call(B_=1) == INVALID and "B >= 2" in _lib.last_error()
    assert call(bytes_=nb.value - 1) == INVALID and "workspace" in _lib.last_error()
    assert call(ws_=ws.ptr + 16) == INVALID and "aligned" in _lib.last_error()
    for args in ((0, B, nc), (N, 0, nc), (N, 1, nc), (N, B, 0)):
        assert lib.fx3d_pointnet_grad_train_workspace_bytes(*args, ctypes.byref(nb)) == INVALID, args
    assert lib.fx3d_pointnet_grad_train_workspace_bytes(N, B, nc, None) == INVALID
    fx.synchronize()
    _same(gp, gtref.flat(c["want"][0]), "gparams after the refusals")
    with pytest.raises(TypeError, match="Float32"):
        m.grad_train(x, DeviceArray.empty((nc, B), np.float64))
    with pytest.raises(ValueError, match="glogits must be"):
        m.grad_train(x, DeviceArray.empty((nc, 1), np.float32))
