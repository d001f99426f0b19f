"""The EdgeConv parameter adjoint on the device (fx3d_edgeconv_grad through fx.EdgeConv.grad / flat_grad) against the host
restatement tests/edgeconv_pgrad_ref.py, bit for bit (uint32 views, no element left out): the shape table -- channel tails in
both directions, K = 1, the three LDS plans (L = 1, L = 2 with its extra image, L >= 3 with the second gather), several passes
over the tile list, several chunks with a short last one --, gx against the input adjoint, run and batch order, gamma = 0 and
dead channels, gout = 0, hand-made neighbour lists, the optional arguments, a captured graph, the C entry point's status
codes and the workspace bound.

idx and out are the device's own forward's.  Every draw is first held to edgeconv_pgrad_ref.check_draw on the restatement's
own gradients (every family finite, at least half of dW non-zero)."""
import ctypes

import numpy as np
import pytest

import edgeconv_pgrad_ref as pref
import edgeconv_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID, UNSUPPORTED = -1, -5   # FX3D_ERR_INVALID_ARG, FX3D_ERR_UNSUPPORTED (include/flux3d_hip.h)
SEED = 1


def _bits(a):
    return np.ascontiguousarray(np.asarray(a).astype(F32, copy=False)).view(np.uint32)


def _host(v):
    return v.to_host() if hasattr(v, "to_host") else np.asarray(v)


def _normal(seed, C, N, B):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((C, N, B)).astype(F32))


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


def _setup(fx, layers, N, B, K, P=None):
    """The model, its parameters, X and gout (standard normal) on host and device, and the device's own forward."""
    P = ref.random_params(layers, SEED) if P is None else P
    m = fx.EdgeConv(layers, K).load(P)
    X, gout = _normal(1000 + SEED, layers[0], N, B), _normal(2000 + SEED, layers[-1], N, B)
    xd, gd = fx.gpu(X), fx.gpu(gout)
    out, idx = m.forward(xd, return_idx=True)
    return m, P, X, gout, xd, gd, idx, out


def _want(P, layers, K, X, gout, idx, out):
    G, gx = pref.grad(X, P, layers, K, gout, _host(idx), _host(out))
    return {n: G[n] for n in ref.param_shapes(layers)}, gx


# (layers, N, B, K)
CASES = [([3, 16], 7, 1, 6),
         ([1, 1], 9, 2, 3),
         ([5, 33, 70], 65, 3, 6),                    # tails in both directions; a third tile of one point
         ([4, 8, 8, 8, 40], 64, 2, 1),               # L = 4, K = 1
         ([6, 2, 255], 33, 2, 4),                    # cin = 2 < 4, a tail of 31 output channels
         ([64, 128, 256], 64, 2, 10),                # DGCNN's second stage
         ([3, 32, 64, 64], 64, 2, 10),               # DGCNN's first stage
         ([64, 64, 128, 256], 70, 1, 5),
         ([40, 8, 8, 8, 72], 34, 2, 3),              # stride 130 at L = 4, a second tile of two points, tails of 8 channels
         ([128, 256, 256, 256, 256], 33, 1, 2),      # the LDS corner, several passes over the tile list
         ([5, 33, 70], 130, 2, 3),                   # two chunks: a full one and a tail of two points
         ([3, 16, 16], 257, 1, 2)]                   # three chunks, L = 2's extra image


@pytest.mark.parametrize("layers,N,B,K", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_the_shape_table_against_the_restatement(gpu_fx, layers, N, B, K):
    fx = gpu_fx
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K)
    want, wx = _want(P, layers, K, X, gout, idx, out)
    pref.check_draw(want, layers)
    got, gx = m.grad(xd, gd, idx, out)
    _same_grads(got, want, "grads against the restatement")
    _same(gx, wx, "gx against the restatement")


def test_gx_is_the_input_adjoints_and_optional(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 130, 2, 3
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K)
    got, gx = m.grad(xd, gd, idx, out)
    pref.check_draw({n: _host(v) for n, v in got.items()}, layers)
    _same(gx, m.input_grad(xd, gd, idx, out).to_host(), "gx against EdgeConv.input_grad")
    alone, none = m.grad(xd, gd, idx, out, input_grad=False)
    assert none is None
    _same_grads(alone, {n: _host(v) for n, v in got.items()}, "input_grad=False")
    flat, fgx = m.flat_grad(xd, gd, idx, out)
    _same(flat, pref.flat({n: _host(v) for n, v in got.items()}, layers), "flat_grad against grad")
    _same(fgx, gx.to_host(), "flat_grad's gx")
    assert m.flat_grad(xd, gd, idx, out, input_grad=False)[1] is None


def test_run_and_batch_order(gpu_fx):
    """Two runs give the same bits.  A batch of three is the chain over (b, chunk) the restatement states; the clouds' separate
    results need not add up to it, since each of them is rounded on its own before the sum."""
    fx = gpu_fx
    layers, N, B, K = [64, 64, 128, 256], 70, 3, 5
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K)
    first, gx = m.grad(xd, gd, idx, out)
    first = {n: _host(v) for n, v in first.items()}
    pref.check_draw(first, layers)
    again, gx2 = m.grad(xd, gd, idx, out)
    _same_grads(again, first, "two runs")
    _same(gx2, gx.to_host(), "two runs: gx")
    want, _ = _want(P, layers, K, X, gout, idx, out)
    _same_grads(first, want, "B = 3 against the restatement's chain over the chunk partials")


def test_gamma_zero_dead_channels_and_zero_gout(gpu_fx):
    """gamma = 0 on hidden channel 7: dW and db of that channel are zero, dgamma and dbeta are the restatement's and finite.
    Last-layer channels 9 and 69 dead (test_gpu_edgeconv_bwd.py's construction, beta = -1): all four families are zero there.
    gout = 0: every bit of every family and of gx is zero."""
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    P = ref.random_params(layers, SEED)
    P["bn1.gamma"][7] = 0
    for ch in (9, 69):
        P["conv2.weight"][0, :, ch] = 0
        P["conv2.bias"][ch] = P["bn2.mu"][ch]
        P["bn2.beta"][ch] = -1
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K, P)
    want, wx = _want(P, layers, K, X, gout, idx, out)
    pref.check_draw(want, layers)
    got, gx = m.grad(xd, gd, idx, out)
    got = {n: _host(v) for n, v in got.items()}
    _same_grads(got, want, "gamma = 0 and dead channels against the restatement")
    _same(gx, wx, "gx")
    assert not got["conv1.weight"][0, :, 7].any() and got["conv1.bias"][7] == 0
    assert np.isfinite(got["bn1.gamma"][7]) and np.isfinite(got["bn1.beta"][7])
    for ch in (9, 69):
        assert not got["conv2.weight"][0, :, ch].any()
        assert all(got[n][ch] == 0 for n in ("conv2.bias", "bn2.gamma", "bn2.beta"))
    zero, zx = m.grad(xd, fx.gpu(np.zeros_like(gout)), idx, out)
    assert all(not _bits(_host(v)).any() for v in zero.values()) and not _bits(zx.to_host()).any()


def test_hand_made_lists(gpu_fx):
    """test_gpu_edgeconv_bwd.py's lists: the point itself twice, repeats, a permutation; and on the device path an index out
    of range, which reads the point itself."""
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P, X, gout, xd, gd, _, _ = _setup(fx, layers, N, B, K)
    made = np.empty((K, N, B), np.int32, order="F")
    n = np.arange(N)
    made[0], made[1], made[2] = n[:, None], n[:, None], ((n + 1) % N)[:, None]
    made[3], made[4], made[5] = 0, N - 1, ((7 * n + 3) % N)[:, None]
    made[5, :, 1] = made[2, :, 1]
    _, out = ref.forward(X, P, layers, K, idx=made)
    want, wx = _want(P, layers, K, X, gout, made, out)
    pref.check_draw(want, layers)
    got, gx = m.grad(xd, gd, idx=fx.gpu(made))
    _same_grads(got, want, "hand-made lists, out computed on the device")
    _same(gx, wx, "hand-made lists: gx")
    beyond = made.copy(order="F")
    beyond[3, 5, 0], beyond[4, 64, 1] = N, -1      # read as the points 5 and 64 themselves
    itself = made.copy(order="F")
    itself[3, 5, 0], itself[4, 64, 1] = 5, 64
    _, out2 = ref.forward(X, P, layers, K, idx=itself)
    want2, wx2 = _want(P, layers, K, X, gout, itself, out2)
    got2, gx2 = m.grad(xd, gd, idx=fx.gpu(beyond))
    _same_grads(got2, want2, "an index out of range on the device path")
    _same(gx2, wx2, "an index out of range: gx")


def test_optional_arguments_and_numpy_in_numpy_out(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K)
    full, gx = m.grad(xd, gd, idx, out)
    full, gx = {n: _host(v) for n, v in full.items()}, gx.to_host()
    pref.check_draw(full, layers)
    for what, kw in (("idx = None, out = None", {}), ("out = None", dict(idx=idx)), ("idx = None", dict(out=out))):
        got, g = m.grad(xd, gd, **kw)
        _same_grads(got, full, what)
        _same(g, gx, what + ": gx")
    got, g = m.grad(X, gout, idx.to_host(), out.to_host())
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in got.values()) and isinstance(g, np.ndarray)
    assert {n: v.shape for n, v in got.items()} == ref.param_shapes(layers)
    _same_grads(got, full, "numpy in, numpy out")
    _same(g, gx, "numpy in, numpy out: gx")
    flat, _ = m.flat_grad(X, gout)
    assert isinstance(flat, np.ndarray) and flat.shape == (m.param_count,)
    _same(flat, pref.flat(full, layers), "flat_grad, numpy")


def test_graph_replay(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 200, 2, 10
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K)
    eager, egx = m.flat_grad(xd, gd, idx, out)
    eager, egx = eager.to_host(), egx.to_host()
    assert np.all(np.isfinite(eager)) and 2 * np.count_nonzero(eager) >= eager.size
    s = fx.Stream.create()
    with fx.stream(s):
        xs, gs = fx.gpu(X), fx.gpu(gout)
        m.flat_grad(xs, gs)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec, rgx = m.flat_grad(xs, gs)  # the search and the forward are inside the capture
        g.launch()
        g.launch()
        s.synchronize()
        _same(rec, eager, "graph replay against the eager run")
        _same(rgx, egx, "graph replay: gx")


def test_workspace_is_smaller_than_the_edge_tensor(gpu_fx):
    """[64, 128, 256] at 32 x 1024, K = 20: the (K N, 2F, B) edge tensor is 335 MB; the call holds the input adjoint's
    workspace and one partial of the parameter count per chunk and cloud (8 x 32 of them).  A query only: nothing runs."""
    from flux3d_jl_amd import _lib
    la = (ctypes.c_int32 * 3)(64, 128, 256)
    nb = _lib.query_bytes("fx3d_edgeconv_grad_workspace_bytes", la, 3, 20, 1024, 32)
    bwd = _lib.query_bytes("fx3d_edgeconv_bwd_workspace_bytes", la, 3, 20, 1024, 32)
    print(f"fx3d_edgeconv_grad_workspace_bytes([64, 128, 256], K = 20, N = 1024, B = 32) = {nb} bytes (the input adjoint: {bwd})")
    assert bwd < nb < 20 * 1024 * 2 * 64 * 32 * 4, nb


def test_status_codes(gpu_fx):
    """The refusals of tests/test_edgeconv_pgrad_host.py with real device arrays around one call that runs."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    lib = _lib.load()
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P, X, gout, x, g, idx, out = _setup(fx, layers, N, B, K)
    gp = DeviceArray.empty((m.param_count,), np.float32)
    gx = DeviceArray.empty((5, N, B), np.float32)
    la = (ctypes.c_int32 * 3)(*layers)
    nb = ctypes.c_size_t(0)
    assert lib.fx3d_edgeconv_grad_workspace_bytes(la, 3, K, N, B, ctypes.byref(nb)) == 0 and nb.value > 0
    ws = DeviceArray.empty((nb.value + 512,), np.uint8)
    assert ws.ptr % 256 == 0
    pd = m._params_dev()

    def call(params=pd.ptr, layers_=layers, nl=None, K_=K, x_=x.ptr, N_=N, B_=B, idx_=idx.ptr, out_=out.ptr, g_=g.ptr, gp_=gp.ptr,
             gx_=gx.ptr, ws_=ws.ptr, bytes_=nb.value):
        arr = (ctypes.c_int32 * len(layers_))(*layers_)
        return lib.fx3d_edgeconv_grad(params, arr, len(layers_) if nl is None else nl, K_, x_, N_, B_, idx_, out_, g_, gp_, gx_,
                                      ws_, bytes_, None)

    assert call() == 0
    fx.synchronize()
    want, wantx = gp.to_host(), gx.to_host()
    assert np.all(np.isfinite(want)) and np.count_nonzero(want) > 0
    assert call(idx_=None, out_=None, gx_=None) == 0   # all three optional
    fx.synchronize()
    _same(gp, want, "idx, out and gx NULL through the C entry point")
    assert call(params=None) == INVALID and call(x_=None) == INVALID and call(g_=None) == INVALID
    assert call(gp_=None) == INVALID and call(ws_=None) == INVALID
    assert lib.fx3d_edgeconv_grad(pd.ptr, None, 3, K, x.ptr, N, B, None, None, g.ptr, gp.ptr, None, ws.ptr, nb.value, None) == INVALID
    assert call(layers_=[5]) == UNSUPPORTED and call(layers_=[5, 8, 8, 8, 8, 8]) == UNSUPPORTED and call(nl=0) == UNSUPPORTED
    assert call(layers_=[5, 0, 70]) == UNSUPPORTED and call(layers_=[5, 33, 257]) == UNSUPPORTED and "257" in _lib.last_error()
    assert call(layers_=[129, 33, 70]) == UNSUPPORTED and "129" in _lib.last_error()
    assert call(K_=0) == INVALID and call(K_=-3) == INVALID
    assert call(K_=N) == INVALID and "K + 1" in _lib.last_error()
    assert call(N_=0) == INVALID and call(B_=0) == INVALID
    assert call(N_=36865) == INVALID and "neighbour search" in _lib.last_error()
    assert call(bytes_=nb.value - 1) == INVALID and "workspace" in _lib.last_error()
    assert call(ws_=ws.ptr + 16) == INVALID and "aligned" in _lib.last_error()
    for args in ((K, 0, B), (K, N, 0), (0, N, B), (N, N, B), (K, 36865, 1)):
        assert lib.fx3d_edgeconv_grad_workspace_bytes(la, 3, *args, ctypes.byref(nb)) == INVALID, args
    assert lib.fx3d_edgeconv_grad_workspace_bytes(la, 3, K, N, B, None) == INVALID
    _same(gp, want, "gparams after the refusals")
    _same(gx, wantx, "gx after the refusals")
    with pytest.raises(TypeError, match="Float32"):
        m.grad(x, DeviceArray.empty((70, N, B), np.float64))
    with pytest.raises(ValueError, match="gout must be"):
        m.grad(x, DeviceArray.empty((70, N, 1), np.float32))
    with pytest.raises(ValueError, match="out must be"):
        m.grad(x, g, out=DeviceArray.empty((69, N, B), np.float32))
    with pytest.raises(TypeError, match="int32"):
        m.grad(x, g, idx=DeviceArray.empty((K, N, B), np.float32))
    with pytest.raises(TypeError, match="where X lives"):
        m.grad(x, gout)
