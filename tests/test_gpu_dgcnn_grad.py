"""The DGCNN adjoint on the device (fx3d_dgcnn_grad through fx.DGCNN.grad / flat_grad / crossentropy_grad) against the host
restatement tests/dgcnn_grad_ref.py, bit for bit (uint32 views, no element left out): the shape table -- one partial tile, a
second tile of one point, two parameter-adjoint chunks, one to three clouds in the chains over b, K = 1, one class --, tied
maxima, dead channels, glogits = 0, run-to-run bits, the equivalences between the ways to call it, the EdgeConv slices against
EdgeConv.grad, numpy in and out, a captured graph, the cross-entropy wrapper and the C entry point's status codes.

The restatement is fed the device's own forward (idx1, x1, idx2, x2, pooled).  The parameters are dgcnn_ref.random_params(nc,
seed=3), X and glogits standard normal; a case's model, forward and restatement are computed once and shared, unchanged."""
import ctypes

import numpy as np
import pytest

import dgcnn_grad_ref as gref
import dgcnn_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID = -1   # FX3D_ERR_INVALID_ARG (include/flux3d_hip.h)
FIVE = ("idx1", "x1", "idx2", "x2", "pooled")


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
    _same_grads(grads, want[0], what)
    for name, g, w in (("gx", gx, want[1]), ("gx2", mid["gx2"], want[2]), ("gx1", mid["gx1"], want[3])):
        _same(g, w, f"{what}: {name}")


_cases = {}


def _case(fx, N, B, K, nc, P=None, tag=None):
    """The model, X and glogits on host and device, the device's own forward (device and host) and the restatement of its
    gradient, computed once per shape."""
    key = (N, B, K, nc, tag)
    if key not in _cases:
        P = dgcnn_ref.random_params(nc, seed=3) if P is None else P
        m = fx.DGCNN(nc, K, N).load(P)
        X = np.asfortranarray(np.random.default_rng(500 + N).standard_normal((3, N, B)).astype(F32))
        glogits = np.asfortranarray(np.random.default_rng(600 + N).standard_normal((nc, B)).astype(F32))
        xd, gd = fx.gpu(X), fx.gpu(glogits)
        fwd = m.forward(xd, intermediates=True)
        hfwd = {k: v.to_host() for k, v in fwd.items()}
        dgcnn_ref.check_draw(hfwd)
        want = gref.grad(X, P, K, glogits, hfwd)
        assert all(np.all(np.isfinite(v)) for v in want[0].values()) and np.count_nonzero(want[1]) > 0
        _cases[key] = dict(m=m, P=P, X=X, glogits=glogits, xd=xd, gd=gd, fwd=fwd, hfwd=hfwd, want=want)
    return _cases[key]


# (N = npoints, B, K, num_classes)
CASES = [(33, 1, 1, 1),      # one partial tile, chains of one cloud, K = 1, one class
         (64, 2, 10, 10),
         (65, 2, 3, 40),     # conv_3's second tile holds one point
         (130, 3, 4, 10)]    # two parameter-adjoint chunks, three clouds in every chain over b


@pytest.mark.parametrize("N,B,K,nc", CASES, ids=lambda v: str(v))
def test_the_shape_table_against_the_restatement(gpu_fx, N, B, K, nc):
    c = _case(gpu_fx, N, B, K, nc)
    if N == 65:  # winners on both sides of the tile boundary
        nstar = gref.winners(gref.conv3(c["P"], c["hfwd"]["x2"]), c["hfwd"]["pooled"])
        assert np.any(nstar == 64) and np.any((nstar >= 0) & (nstar < 64)), np.bincount(nstar[nstar >= 0], minlength=65)
    _same_all(c["m"].grad(c["xd"], c["gd"], fwd=c["fwd"], intermediates=True), c["want"], f"{(N, B, K, nc)} against the restatement")


def test_ties_go_to_the_first_point(gpu_fx):
    """Point 3's row of x2 copied onto point 7 in both clouds, pooled recomputed with the restatement's conv_3: point 3 takes
    every tied channel, and point 7's gx2 row is all +0 (every channel it reaches is tied with point 3, the earlier index)."""
    fx = gpu_fx
    N, B, K, nc = 65, 2, 3, 40
    c = _case(fx, N, B, K, nc)
    x2 = c["hfwd"]["x2"].copy(order="F")
    x2[:, 7, :] = x2[:, 3, :]
    a3 = gref.conv3(c["P"], x2)
    hfwd = dict(c["hfwd"], x2=x2, pooled=gref.pool(a3))
    nstar = gref.winners(a3, hfwd["pooled"])
    takes = [int(np.count_nonzero(nstar[b] == 3)) for b in range(B)]   # (in this draw point 3 wins channels in the second cloud only)
    assert not np.any(nstar == 7) and sum(takes) > 0, takes
    want = gref.grad(c["X"], c["P"], K, c["glogits"], hfwd)
    fwd = dict(c["fwd"], x2=fx.gpu(x2), pooled=fx.gpu(hfwd["pooled"]))
    got = c["m"].grad(c["xd"], c["gd"], fwd=fwd, intermediates=True)
    _same_all(got, want, "ties against the restatement")
    gx2 = _host(got[2]["gx2"])
    assert not _bits(gx2[:, 7, :]).any() and all(np.count_nonzero(gx2[:, 3, b]) > 0 for b in range(B) if takes[b])


def test_dead_channels_zero_glogits_and_two_runs(gpu_fx):
    """conv3.bn.beta = -1e3 on channels 9 and 1000: pooled is zero there, nothing wins, and all four families are zero; the rest is
    the restatement's.  glogits = 0: every bit of every result is zero.  Two runs give the same bits."""
    fx = gpu_fx
    N, B, K, nc = 65, 2, 3, 10
    P = dgcnn_ref.random_params(nc, seed=3)
    P["conv3.bn.beta"][[9, 1000]] = -1e3
    c = _case(fx, N, B, K, nc, P, "dead")
    assert not c["hfwd"]["pooled"][[9, 1000]].any()
    got = c["m"].grad(c["xd"], c["gd"], fwd=c["fwd"], intermediates=True)
    _same_all(got, c["want"], "dead channels against the restatement")
    grads, gx, mid = _all(got)
    for ch in (9, 1000):
        assert not _bits(grads["conv3.conv.weight"][0, :, ch]).any()
        assert all(not _bits(grads[n][ch]).any() for n in ("conv3.conv.bias", "conv3.bn.gamma", "conv3.bn.beta"))
    _same_all(c["m"].grad(c["xd"], c["gd"], fwd=c["fwd"], intermediates=True), (grads, gx, mid["gx2"], mid["gx1"]), "two runs")
    zg, zx, zmid = _all(c["m"].grad(c["xd"], fx.gpu(np.zeros_like(c["glogits"])), fwd=c["fwd"], intermediates=True))
    assert all(not _bits(v).any() for v in zg.values()) and not _bits(zx).any()
    assert not _bits(zmid["gx2"]).any() and not _bits(zmid["gx1"]).any()


def test_the_ways_to_call_it_agree(gpu_fx):
    """fwd given and fwd = None; flat_grad and grad; input_grad = False; and the ec2 / ec1 slices against EdgeConv.grad on the
    ``ec2.`` / ``ec1.`` parameters with gout = gx2 / gx1, bit for bit."""
    fx = gpu_fx
    N, B, K, nc = 130, 3, 4, 10
    c = _case(fx, N, B, K, nc)
    m, xd, gd, fwd = c["m"], c["xd"], c["gd"], c["fwd"]
    grads, gx, gx2, gx1 = c["want"]
    _same_all(m.grad(xd, gd, intermediates=True), c["want"], "fwd = None")
    flat, fgx = m.flat_grad(xd, gd, fwd=fwd)
    _same(flat, gref.flat(grads), "flat_grad against grad, flattened")
    _same(fgx, gx, "flat_grad's gx")
    assert _host(flat).shape == (m.param_count,)
    alone, none = m.grad(xd, gd, fwd=fwd, input_grad=False)
    assert none is None and m.flat_grad(xd, gd, input_grad=False)[1] is None
    _same_grads({n: _host(v) for n, v in alone.items()}, grads, "input_grad = False")
    for name, layers, x, g, idx, out, gin in (("ec2", gref.L2, fwd["x1"], gx2, fwd["idx2"], fwd["x2"], gx1),
                                              ("ec1", gref.L1, xd, gx1, fwd["idx1"], fwd["x1"], gx)):
        ec = fx.EdgeConv(layers, K).load(gref.stage_params(c["P"], name))
        eg, egx = ec.grad(x, fx.gpu(g), idx, out)
        _same_grads({f"{name}.{n}": _host(v) for n, v in eg.items()}, {n: v for n, v in grads.items() if n.startswith(name + ".")},
                    f"the {name} slice against EdgeConv.grad")
        _same(egx, gin, f"{name}: the input gradient against EdgeConv.grad's")


def test_numpy_in_numpy_out(gpu_fx):
    c = _case(gpu_fx, 33, 1, 1, 1)
    m = c["m"]
    got = m.grad(c["X"], c["glogits"], fwd=c["hfwd"], intermediates=True)
    assert all(isinstance(v, np.ndarray) and v.dtype == F32 for v in got[0].values()) and isinstance(got[1], np.ndarray)
    assert {n: v.shape for n, v in got[0].items()} == dgcnn_ref.param_shapes(1) and got[1].shape == (3, 33, 1)
    _same_all(got, c["want"], "numpy in, numpy out")
    flat, gx = m.flat_grad(c["X"][:, :, 0], c["glogits"][:, 0])   # one cloud as (3, N), its glogits as (nc,)
    assert isinstance(flat, np.ndarray) and flat.shape == (m.param_count,)
    _same(flat, gref.flat(c["want"][0]), "flat_grad, numpy, fwd = None")
    _same(gx, c["want"][1], "flat_grad, numpy: gx")
    with pytest.raises(TypeError, match="where X lives"):
        m.grad(c["xd"], c["glogits"])
    with pytest.raises(TypeError, match="where X lives"):
        m.grad(c["X"], c["glogits"], fwd=c["fwd"])


def test_graph_replay(gpu_fx):
    fx = gpu_fx
    c = _case(fx, 65, 2, 3, 40)
    m = c["m"]
    s = fx.Stream.create()
    with fx.stream(s):
        xs, gs = fx.gpu(c["X"]), fx.gpu(c["glogits"])
        m.flat_grad(xs, gs)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec, rgx = m.flat_grad(xs, gs)  # the search and the forward are inside the capture
        g.launch()
        g.launch()
        s.synchronize()
        _same(rec, gref.flat(c["want"][0]), "graph replay against the eager bits")
        _same(rgx, c["want"][1], "graph replay: gx")


def test_crossentropy_grad(gpu_fx):
    fx = gpu_fx
    N, B, K, nc = 65, 2, 3, 40
    c = _case(fx, N, B, K, nc)
    m, labels = c["m"], np.array([3, 17])
    loss, grads, gx = m.crossentropy_grad(c["xd"], labels)
    probs = c["hfwd"]["probs"]
    want_loss = float(-np.mean(np.log(probs[labels, np.arange(B)].astype(np.float64))))
    assert isinstance(loss, float) and loss == want_loss and np.isfinite(loss) and loss > 0
    onehot = np.zeros((nc, B), F32)
    onehot[labels, np.arange(B)] = 1
    glogits = np.asfortranarray(((probs - onehot).astype(F32) / F32(B)).astype(F32))
    wg, wx = m.grad(c["xd"], fx.gpu(glogits), fwd=c["fwd"])
    _same_grads({n: _host(v) for n, v in grads.items()}, {n: _host(v) for n, v in wg.items()}, "crossentropy_grad against grad")
    _same(gx, _host(wx), "crossentropy_grad: gx")
    assert np.count_nonzero(_host(gx)) > 0
    hl, hg, hx = m.crossentropy_grad(c["X"], [3, 17])
    assert hl == loss and isinstance(hx, np.ndarray)
    _same(hx, _host(wx), "crossentropy_grad, numpy: gx")
    with pytest.raises(ValueError, match="labels must be in"):
        m.crossentropy_grad(c["xd"], [3, nc])


def test_status_codes(gpu_fx):
    """The refusals of tests/test_dgcnn_grad_host.py with real device arrays around calls that run."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    lib = _lib.load()
    N, B, K, nc = 65, 2, 3, 40
    c = _case(fx, N, B, K, nc)
    m, x, g, fwd = c["m"], c["xd"], c["gd"], c["fwd"]
    gp = DeviceArray.empty((m.param_count,), np.float32)
    gx = DeviceArray.empty((3, N, B), np.float32)
    nb = ctypes.c_size_t(0)
    assert lib.fx3d_dgcnn_grad_workspace_bytes(N, B, K, nc, ctypes.byref(nb)) == 0 and nb.value > 0
    ws = DeviceArray.empty((nb.value + 512,), np.uint8)
    assert ws.ptr % 256 == 0
    pd = m._params_dev()
    five = {k: fwd[k].ptr for k in FIVE}

    def call(params=pd.ptr, nc_=nc, K_=K, x_=x.ptr, N_=N, B_=B, g_=g.ptr, gp_=gp.ptr, gx_=gx.ptr, ws_=ws.ptr, bytes_=nb.value, **mid):
        mid = dict(five, **mid)
        return lib.fx3d_dgcnn_grad(params, nc_, K_, x_, N_, B_, *(mid[k] for k in FIVE), g_, gp_, gx_, None, None, ws_, bytes_, None)

    assert call() == 0
    fx.synchronize()
    _same(gp, gref.flat(c["want"][0]), "the C entry point")
    _same(gx, c["want"][1], "the C entry point: gx")
    assert call(gx_=None, **{k: None for k in FIVE}) == 0   # none of the five, no gx
    fx.synchronize()
    _same(gp, gref.flat(c["want"][0]), "intermediates and gx NULL through the C entry point")
    assert call(params=None) == INVALID and call(x_=None) == INVALID and call(g_=None) == INVALID
    assert call(gp_=None) == INVALID and call(ws_=None) == INVALID
    for k in FIVE:
        assert call(**{k: None}) == INVALID and "all five or none" in _lib.last_error(), k
    assert call(nc_=0) == INVALID and "num_classes" in _lib.last_error()
    assert call(K_=0) == INVALID and call(K_=-3) == INVALID
    assert call(K_=N) == INVALID and "K + 1" in _lib.last_error()
    assert call(N_=0) == INVALID and call(B_=0) == INVALID
    assert call(N_=36865) == INVALID and "neighbour search" in _lib.last_error()
    assert call(bytes_=nb.value - 1) == INVALID and "workspace" in _lib.last_error()
    assert call(ws_=ws.ptr + 16) == INVALID and "aligned" in _lib.last_error()
    for args in ((0, B, K, nc), (N, 0, K, nc), (N, B, 0, nc), (N, B, N, nc), (36865, 1, K, nc), (N, B, K, 0)):
        assert lib.fx3d_dgcnn_grad_workspace_bytes(*args, ctypes.byref(nb)) == INVALID, args
    assert lib.fx3d_dgcnn_grad_workspace_bytes(N, B, K, nc, None) == INVALID
    fx.synchronize()
    _same(gp, gref.flat(c["want"][0]), "gparams after the refusals")
    with pytest.raises(TypeError, match="Float32"):
        m.grad(x, DeviceArray.empty((nc, B), np.float64))
    with pytest.raises(ValueError, match="glogits must be"):
        m.grad(x, DeviceArray.empty((nc, 1), np.float32))
    with pytest.raises(ValueError, match="x2'. must be"):
        m.grad(x, g, fwd=dict(fwd, x2=DeviceArray.empty((255, N, B), np.float32)))
    with pytest.raises(TypeError, match="int32"):
        m.grad(x, g, fwd=dict(fwd, idx1=DeviceArray.empty((K, N, B), np.float32)))
