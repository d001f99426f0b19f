"""The DGCNN training-mode adjoint on the device (fx3d_dgcnn_grad_train through fx.DGCNN.grad_train / flat_grad_train /
crossentropy_grad_train) against the host restatement tests/dgcnn_grad_train_ref.py, bit for bit (uint32 views, no element left
out): the shape table -- one partial tile with K = 1 and one class (the scalar fc_6 chain), a second tile of one point with an odd
number of clouds, three tiles (the dW walk over a full, a full and a two-point tile) --, the dropout multipliers, tied maxima, a
channel that wins nowhere, a cloud without a winner, gamma = 0 and glogits = 0, the ways to call it, a captured graph, the
cross-entropy wrapper and the C entry point's status codes.

The restatement is evaluated at the device's own forward_train outputs (idx1, x1, idx2, x2, pooled, batch_stats).  The parameters are
dgcnn_ref.random_params(nc, seed=3), X and glogits standard normal; a case's model, forward and restatement are computed once and
shared, unchanged.  Every draw is first held to dgcnn_grad_train_ref.check_draw (every family finite, at least half of dW
non-zero)."""
import ctypes

import numpy as np
import pytest

import dgcnn_grad_ref as tmode
import dgcnn_grad_train_ref as gref
import dgcnn_ref
import edgeconv_grad_train_ref as ect

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID = -1   # FX3D_ERR_INVALID_ARG (include/flux3d_hip.h)
FIVE = ("idx1", "x1", "idx2", "x2", "pooled")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a).astype(F32, copy=False)).view(np.uint32)


def _host(v):
    if isinstance(v, dict):
        return {k: _host(w) for k, w in v.items()}
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


def _same_all(got, want, what):
    """(grads, gx, mid) of grad_train(..., intermediates=True) against the restatement's (grads, gx, gx2, gx1)."""
    grads, gx, mid = got
    _same_grads(grads, want[0], what)
    for name, g, w in (("gx", gx, want[1]), ("gx2", mid["gx2"], want[2]), ("gx1", mid["gx1"], want[3])):
        _same(g, w, f"{what}: {name}")


def _gpu_pair(fx, dropout):
    return None if dropout is None else tuple(fx.gpu(m) for m in dropout)


def _want(c, hfwd=None, dropout=None, glogits=None, P=None, keep=None):
    want = gref.grad_train(c["X"], c["P"] if P is None else P, c["K"], c["glogits"] if glogits is None else glogits,
                           c["hfwd"] if hfwd is None else hfwd, dropout, keep)
    return want


_cases = {}


def _case(fx, N, B, K, nc, P=None, tag=None, dropout=None):
    """The model, X and glogits on host and device, the device's own training-mode forward (device and host) and the restatement
    of its gradient, computed once per shape."""
    key = (N, B, K, nc, tag)
    if key not in _cases:
        P = dgcnn_ref.random_params(nc, seed=3) if P is None else P
        m = fx.DGCNN(nc, K, N).load(P)
        X = np.asfortranarray(np.random.default_rng(700 + N).standard_normal((3, N, B)).astype(F32))
        glogits = np.asfortranarray(np.random.default_rng(800 + N).standard_normal((nc, B)).astype(F32))
        xd, gd = fx.gpu(X), fx.gpu(glogits)
        dd = _gpu_pair(fx, dropout)
        fwd = m.forward_train(xd, dropout=dd, intermediates=True)
        hfwd = _host(fwd)
        c = dict(m=m, P=P, X=X, K=K, glogits=glogits, xd=xd, gd=gd, fwd=fwd, hfwd=hfwd, dropout=dropout, dd=dd)
        c["want"] = _want(c, dropout=dropout)
        gref.check_draw(c["want"][0])
        assert np.count_nonzero(c["want"][1]) > 0
        _cases[key] = c
    return _cases[key]


# (N = npoints, B, K, num_classes)
CASES = [(33, 2, 1, 1),      # one partial tile, K = 1, one class: the scalar fc_6 chain
         (64, 2, 3, 10),
         (65, 3, 3, 10),     # a second tile of one point, odd B
         (130, 2, 3, 40)]    # three tiles: the dW walk over a full, a full and a two-point tile
SPECIAL = (65, 3, 3, 10)


@pytest.mark.parametrize("N,B,K,nc", CASES, ids=lambda v: str(v))
def test_the_shape_table_against_the_restatement(gpu_fx, N, B, K, nc):
    c = _case(gpu_fx, N, B, K, nc)
    if N == 65:  # winners on both sides of the tile boundary
        keep = {}
        _want(c, keep=keep)
        nstar = keep["nstar"]
        assert np.any(nstar == 64) and np.any((nstar >= 0) & (nstar < 64)), np.bincount(nstar[nstar >= 0], minlength=65)
    got = c["m"].grad_train(c["xd"], c["gd"], fwd=c["fwd"], intermediates=True)
    _same_all(got, c["want"], f"{(N, B, K, nc)} against the restatement")
    assert all(not _bits(_host(v)).any() for n, v in got[0].items() if n.endswith((".mu", ".sigma2")))
    # the test-mode adjoint at the same statistics is another function: conv_3's input gradient is dense here
    assert np.count_nonzero(_host(got[2]["gx2"])) > _host(got[2]["gx2"]).size // 2


def test_the_dropout_multipliers(gpu_fx):
    """None and multipliers of all ones give the same bits; an int seed equals the explicit pair; a mask whose column of cloud 1
    is all zero (fc_5's whole output of that cloud dropped) equals the restatement."""
    fx = gpu_fx
    N, B, K, nc = SPECIAL
    c = _case(fx, N, B, K, nc)
    m, xd, gd = c["m"], c["xd"], c["gd"]
    ones = (np.ones((512, B), F32, order="F"), np.ones((256, B), F32, order="F"))
    _same_all(m.grad_train(xd, gd, dropout=_gpu_pair(fx, ones), fwd=c["fwd"], intermediates=True), c["want"], "all-ones multipliers")
    pair = fx.DGCNN.dropout_masks(B, 11)
    s = _case(fx, N, B, K, nc, tag="seed11", dropout=pair)
    assert not np.array_equal(_bits(s["want"][0]["fc4.dense.weight"]), _bits(c["want"][0]["fc4.dense.weight"]))
    _same_all(m.grad_train(xd, gd, dropout=s["dd"], fwd=s["fwd"], intermediates=True), s["want"], "the explicit pair")
    _same_all(m.grad_train(xd, gd, dropout=11, intermediates=True), s["want"], "the int seed, its own forward")
    zero = (pair[0].copy(order="F"), pair[1].copy(order="F"))
    zero[1][:, 1] = 0
    z = _case(fx, N, B, K, nc, tag="zerocol", dropout=zero)
    _same_all(m.grad_train(xd, gd, dropout=z["dd"], fwd=z["fwd"], intermediates=True), z["want"], "an all-zero column")


def _at_stats(c):
    return ect.at_stats(c["P"], {k: v for k, v in c["hfwd"]["batch_stats"].items() if not k.startswith("ec")})


def test_ties_go_to_the_first_point(gpu_fx):
    """Point 3's row of x2 copied onto point 7 in every cloud, pooled recomputed with the restatement's conv_3 at the batch
    statistics: point 3 takes every tied channel, point 7 wins nothing."""
    fx = gpu_fx
    c = _case(fx, *SPECIAL)
    x2 = c["hfwd"]["x2"].copy(order="F")
    x2[:, 7, :] = x2[:, 3, :]
    a3 = tmode.conv3(_at_stats(c), x2)
    hfwd = dict(c["hfwd"], x2=x2, pooled=tmode.pool(a3))
    keep = {}
    want = _want(c, hfwd, keep=keep)
    nstar = keep["nstar"]
    assert not np.any(nstar == 7) and np.count_nonzero(nstar == 3) > 0
    fwd = dict(c["fwd"], x2=fx.gpu(x2), pooled=fx.gpu(hfwd["pooled"]))
    _same_all(c["m"].grad_train(c["xd"], c["gd"], fwd=fwd, intermediates=True), want, "ties against the restatement")


def test_a_channel_that_wins_nowhere_and_a_cloud_without_a_winner(gpu_fx):
    """conv3.bn.beta = -1e3 on channels 9 and 1000: pooled is zero there in every cloud, nothing wins, dbeta and dgamma are +0 and
    the dW3 columns are the restatement's.  pooled of channels 5 and 700 set to zero in cloud 1 alone: that cloud has no winner
    there, the chain over the clouds skips it, and it still receives gv3 from the other clouds' sums."""
    fx = gpu_fx
    N, B, K, nc = SPECIAL
    P = dgcnn_ref.random_params(nc, seed=3)
    P["conv3.bn.beta"][[9, 1000]] = -1e3
    c = _case(fx, N, B, K, nc, P, "dead")
    assert not c["hfwd"]["pooled"][[9, 1000]].any()
    got = c["m"].grad_train(c["xd"], c["gd"], fwd=c["fwd"], intermediates=True)
    _same_all(got, c["want"], "a channel without a winner")
    grads = _host(got[0])
    for ch in (9, 1000):
        assert not _bits(grads["conv3.bn.beta"][ch]).any() and not _bits(grads["conv3.bn.gamma"][ch]).any()
        assert not grads["conv3.conv.weight"][0, :, ch].any()
    pooled = c["hfwd"]["pooled"].copy(order="F")
    assert np.all(pooled[[5, 700]] > 0)
    pooled[[5, 700], 1] = 0
    hfwd = dict(c["hfwd"], pooled=pooled)
    keep = {}
    want = _want(c, hfwd, keep=keep)
    assert np.all(keep["nstar"][1, [5, 700]] == -1) and np.all(keep["nstar"][[0, 2]][:, [5, 700]] >= 0)
    assert np.all(want[0]["conv3.bn.beta"][[5, 700]] != 0)
    fwd = dict(c["fwd"], pooled=fx.gpu(pooled))
    _same_all(c["m"].grad_train(c["xd"], c["gd"], fwd=fwd, intermediates=True), want, "a cloud without a winner")


def test_gamma_zero_and_zero_glogits(gpu_fx):
    """gamma = 0 on conv3.bn's channels 7 and 900: gv3 of those channels is zero, so their dW3 and db3 are zero; dgamma and dbeta
    are the restatement's.  glogits = 0: every bit of every result is zero."""
    fx = gpu_fx
    N, B, K, nc = SPECIAL
    P = dgcnn_ref.random_params(nc, seed=3)
    P["conv3.bn.gamma"][[7, 900]] = 0
    c = _case(fx, N, B, K, nc, P, "gamma0")
    got = c["m"].grad_train(c["xd"], c["gd"], fwd=c["fwd"], intermediates=True)
    _same_all(got, c["want"], "gamma = 0 against the restatement")
    grads = _host(got[0])
    for ch in (7, 900):
        assert not grads["conv3.conv.weight"][0, :, ch].any() and grads["conv3.conv.bias"][ch] == 0
    zg, zx, zmid = c["m"].grad_train(c["xd"], fx.gpu(np.zeros_like(c["glogits"])), fwd=c["fwd"], intermediates=True)
    assert all(not _bits(_host(v)).any() for v in zg.values()) and not _bits(_host(zx)).any()
    assert not _bits(_host(zmid["gx2"])).any() and not _bits(_host(zmid["gx1"])).any()


def test_the_ways_to_call_it_agree(gpu_fx):
    """fwd given and fwd = None; flat_grad_train and grad_train; input_grad = False; two runs; and the ec2 / ec1 slices against
    EdgeConv.grad_train on the ``ec2.`` / ``ec1.`` parameters and statistics with gout = gx2 / gx1, bit for bit."""
    fx = gpu_fx
    N, B, K, nc = 130, 2, 3, 40
    c = _case(fx, N, B, K, nc)
    m, xd, gd, fwd = c["m"], c["xd"], c["gd"], c["fwd"]
    grads, gx, gx2, gx1 = c["want"]
    _same_all(m.grad_train(xd, gd, intermediates=True), c["want"], "fwd = None")
    _same_all(m.grad_train(xd, gd, fwd=fwd, intermediates=True), c["want"], "fwd given, a second run")
    flat, fgx = m.flat_grad_train(xd, gd, fwd=fwd)
    _same(flat, gref.flat(grads), "flat_grad_train against grad_train, flattened")
    _same(fgx, gx, "flat_grad_train's gx")
    assert _host(flat).shape == (m.param_count,)
    alone, none = m.grad_train(xd, gd, fwd=fwd, input_grad=False)
    assert none is None
    _same_grads(alone, grads, "input_grad = False")
    stats = fwd["batch_stats"]
    for name, layers, x, g, idx, out, gin in (("ec2", gref.L2, fwd["x1"], gx2, fwd["idx2"], fwd["x2"], gx1),
                                              ("ec1", gref.L1, xd, gx1, fwd["idx1"], fwd["x1"], gx)):
        ec = fx.EdgeConv(layers, K).load(gref.stage_params(c["P"], name))
        f = {"out": out, "idx": idx, "batch_stats": gref.stage_stats(stats, name)}
        eg, egx = ec.grad_train(x, fx.gpu(g), fwd=f)
        _same_grads({f"{name}.{n}": v for n, v in eg.items()}, {n: v for n, v in grads.items() if n.startswith(name + ".")},
                    f"the {name} slice against EdgeConv.grad_train")
        _same(egx, gin, f"{name}: the input gradient against EdgeConv.grad_train's")


def test_numpy_in_numpy_out(gpu_fx):
    c = _case(gpu_fx, 33, 2, 1, 1)
    m = c["m"]
    got = m.grad_train(c["X"], c["glogits"], fwd=c["hfwd"], intermediates=True)
    assert all(isinstance(v, np.ndarray) and v.dtype == F32 for v in got[0].values()) and isinstance(got[1], np.ndarray)
    assert {n: v.shape for n, v in got[0].items()} == dgcnn_ref.param_shapes(1) and got[1].shape == (3, 33, 2)
    _same_all(got, c["want"], "numpy in, numpy out")
    flat, gx = m.flat_grad_train(c["X"], c["glogits"])
    assert isinstance(flat, np.ndarray) and flat.shape == (m.param_count,)
    _same(flat, gref.flat(c["want"][0]), "flat_grad_train, numpy, fwd = None")
    _same(gx, c["want"][1], "flat_grad_train, numpy: gx")
    with pytest.raises(TypeError, match="where X lives"):
        m.grad_train(c["xd"], c["glogits"])
    with pytest.raises(TypeError, match="where X lives"):
        m.grad_train(c["X"], c["glogits"], fwd=c["fwd"])
    with pytest.raises(TypeError, match="where X lives"):
        m.grad_train(c["xd"], c["gd"], fwd=c["hfwd"])


def test_graph_replay(gpu_fx):
    fx = gpu_fx
    c = _case(fx, 65, 3, 3, 10)
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
        _same(rec, gref.flat(c["want"][0]), "graph replay against the eager bits")
        _same(rgx, c["want"][1], "graph replay: gx")


def test_crossentropy_grad_train(gpu_fx):
    fx = gpu_fx
    N, B, K, nc = SPECIAL
    pair = fx.DGCNN.dropout_masks(B, 11)
    c = _case(fx, N, B, K, nc, tag="seed11", dropout=pair)
    m, labels = c["m"], np.array([3, 7, 0])
    loss, grads, gx = m.crossentropy_grad_train(c["xd"], labels, dropout=11)
    probs = c["hfwd"]["probs"]
    want_loss = float(-np.mean(np.log(probs[labels, np.arange(B)].astype(np.float64))))
    assert isinstance(loss, float) and loss == want_loss and np.isfinite(loss) and loss > 0
    onehot = np.zeros((nc, B), F32)
    onehot[labels, np.arange(B)] = 1
    glogits = np.asfortranarray(((probs - onehot).astype(F32) / F32(B)).astype(F32))
    wg, wx = m.grad_train(c["xd"], fx.gpu(glogits), dropout=c["dd"], fwd=c["fwd"])
    _same_grads(grads, _host(wg), "crossentropy_grad_train against grad_train")
    _same(gx, _host(wx), "crossentropy_grad_train: gx")
    assert np.count_nonzero(_host(gx)) > 0
    hl, hg, hx = m.crossentropy_grad_train(c["X"], [3, 7, 0], dropout=pair)
    assert hl == loss and isinstance(hx, np.ndarray)
    _same(hx, _host(wx), "crossentropy_grad_train, numpy: gx")
    with pytest.raises(ValueError, match="labels must be in"):
        m.crossentropy_grad_train(c["xd"], [3, nc, 0])


def test_status_codes_and_the_workspace_bound(gpu_fx):
    """Each NULL required pointer, B = 1, a short and a misaligned workspace are refused with the outputs left untouched; the
    workspace query equals what the call accepts."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    lib = _lib.load()
    N, B, K, nc = SPECIAL
    c = _case(fx, N, B, K, nc)
    m, x, g, fwd = c["m"], c["xd"], c["gd"], c["fwd"]
    stats = fx.gpu(np.concatenate([_host(v) for v in fwd["batch_stats"].values()]))
    gp = DeviceArray.empty((m.param_count,), np.float32)
    gx = DeviceArray.empty((3, N, B), np.float32)
    nb = ctypes.c_size_t(0)
    assert lib.fx3d_dgcnn_grad_train_workspace_bytes(N, B, K, nc, ctypes.byref(nb)) == 0 and nb.value > 0 and nb.value % 256 == 0
    ws = DeviceArray.empty((nb.value + 512,), np.uint8)
    assert ws.ptr % 256 == 0
    pd = m._params_dev()
    five = {k: fwd[k].ptr for k in FIVE}

    def call(params=pd.ptr, nc_=nc, K_=K, x_=x.ptr, N_=N, B_=B, d4=None, d5=None, st_=stats.ptr, g_=g.ptr, gp_=gp.ptr, gx_=gx.ptr,
             ws_=ws.ptr, bytes_=nb.value, **mid):
        mid = dict(five, **mid)
        return lib.fx3d_dgcnn_grad_train(params, nc_, K_, x_, N_, B_, d4, d5, *(mid[k] for k in FIVE), st_, g_, gp_, gx_, None, None,
                                         ws_, bytes_, None)

    assert call() == 0   # exactly the queried size is accepted
    fx.synchronize()
    _same(gp, gref.flat(c["want"][0]), "the C entry point")
    _same(gx, c["want"][1], "the C entry point: gx")
    assert call(gx_=None) == 0
    fx.synchronize()
    _same(gp, gref.flat(c["want"][0]), "gx NULL through the C entry point")
    for kw in (dict(params=None), dict(x_=None), dict(st_=None), dict(g_=None), dict(gp_=None), dict(ws_=None)):
        assert call(**kw) == INVALID and "NULL" in _lib.last_error(), kw
    for k in FIVE:
        assert call(**{k: None}) == INVALID and "NULL" in _lib.last_error(), k
    assert call(B_=1) == INVALID and "B >= 2" in _lib.last_error()
    assert call(nc_=0) == INVALID and "num_classes" in _lib.last_error()
    assert call(K_=0) == INVALID and call(K_=N) == INVALID and "K + 1" in _lib.last_error()
    assert call(N_=0) == INVALID and call(N_=36865) == INVALID and "neighbour search" in _lib.last_error()
    assert call(bytes_=nb.value - 1) == INVALID and "workspace" in _lib.last_error()
    assert call(ws_=ws.ptr + 16) == INVALID and "aligned" in _lib.last_error()
    for args in ((0, B, K, nc), (N, 0, K, nc), (N, 1, K, nc), (N, B, 0, nc), (N, B, N, nc), (36865, 2, K, nc), (N, B, K, 0)):
        assert lib.fx3d_dgcnn_grad_train_workspace_bytes(*args, ctypes.byref(nb)) == INVALID, args
    assert lib.fx3d_dgcnn_grad_train_workspace_bytes(N, B, K, nc, None) == INVALID
    fx.synchronize()
    _same(gp, gref.flat(c["want"][0]), "gparams after the refusals")
    _same(gx, c["want"][1], "gx after the refusals")
    with pytest.raises(TypeError, match="Float32"):
        m.grad_train(x, DeviceArray.empty((nc, B), np.float64), fwd=fwd)
    with pytest.raises(ValueError, match="glogits must be"):
        m.grad_train(x, DeviceArray.empty((nc, 1), np.float32), fwd=fwd)
    with pytest.raises(ValueError, match="x2'. must be"):
        m.grad_train(x, g, fwd=dict(fwd, x2=DeviceArray.empty((255, N, B), np.float32)))
    with pytest.raises(TypeError, match="int32"):
        m.grad_train(x, g, fwd=dict(fwd, idx1=DeviceArray.empty((K, N, B), np.float32)))
