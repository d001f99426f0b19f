"""The EdgeConv training-mode adjoint on the device (fx3d_edgeconv_grad_train through fx.EdgeConv.grad_train / flat_grad_train)
against the host restatement tests/edgeconv_grad_train_ref.py, bit for bit (uint32 views, no element left out): the shape table --
channel tails in both directions, K = 1, the three LDS plans, several closing passes, several chunks, a fold past its 32 groups --,
gx alone, the optional arguments, run and batch order, gout = 0, gamma = 0, hand-made neighbour lists, a captured graph, the C
entry point's status codes, the workspace bound and DGCNN's two-stage composition.

idx, out and batch_stats are the device's own forward_train's.  Every draw is first held to edgeconv_pgrad_ref.check_draw on the
restatement's own gradients (every family finite, at least half of dW non-zero)."""
import ctypes

import numpy as np
import pytest

import dgcnn_ref
import edgeconv_grad_train_ref as gref
import edgeconv_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID, UNSUPPORTED = -1, -5   # FX3D_ERR_INVALID_ARG, FX3D_ERR_UNSUPPORTED (include/flux3d_hip.h)
SEED = 1


def _bits(a):
    return np.ascontiguousarray(np.asarray(a).astype(F32, copy=False)).view(np.uint32)


def _host(v):
    if isinstance(v, dict):
        return {k: _host(w) for k, w in v.items()}
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


def _setup(fx, layers, N, B, K, P=None, X=None, gout=None, idx=None):
    """The model, its parameters, X and gout (standard normal) on host and device, and the device's own training-mode forward."""
    P = ref.random_params(layers, SEED) if P is None else P
    m = fx.EdgeConv(layers, K).load(P)
    X = _normal(1000 + SEED, layers[0], N, B) if X is None else X
    gout = _normal(2000 + SEED, layers[-1], N, B) if gout is None else gout
    xd, gd = fx.gpu(X), fx.gpu(gout)
    fwd = m.forward_train(xd, idx=idx, intermediates=True)
    return m, P, X, gout, xd, gd, fwd


def _want(P, layers, K, X, gout, fwd):
    f = _host(fwd)
    G, gx = gref.grad(X, P, layers, K, gout, f["batch_stats"], f["idx"], f["out"])
    gref.check_draw(G, layers)
    return G, gx


# (layers, N, B, K)
CASES = [([3, 16], 7, 1, 6),
         ([1, 1], 9, 2, 3),
         ([5, 33, 70], 65, 3, 6),                    # tails in both directions; a third half-tile of one point
         ([4, 8, 8, 8, 40], 64, 2, 1),               # L = 4, K = 1
         ([6, 2, 255], 33, 2, 4),                    # cin = 2 < 4, a tail of 31 output channels
         ([64, 128, 256], 64, 2, 3),                 # DGCNN's second stage
         ([3, 32, 64, 64], 65, 2, 3),                # DGCNN's first stage
         ([64, 64, 128, 256], 70, 1, 3),             # two closing passes
         ([65, 8, 8, 8, 8], 66, 2, 3),               # the forward's shared_rows
         ([128, 256, 256, 256, 256], 33, 1, 2),      # the LDS corner
         ([5, 33, 70], 130, 2, 3),                   # two chunks: a full one and a tail of two points
         ([3, 16, 16], 257, 1, 2),                   # three chunks, L = 2's extra image
         ([3, 16], 1057, 1, 2)]                      # 34 half-tiles: the fold past its 32 groups


@pytest.mark.parametrize("layers,N,B,K", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_the_shape_table_against_the_restatement(gpu_fx, layers, N, B, K):
    fx = gpu_fx
    m, P, X, gout, xd, gd, fwd = _setup(fx, layers, N, B, K)
    want, wx = _want(P, layers, K, X, gout, fwd)
    got, gx = m.grad_train(xd, gd, fwd=fwd)
    _same_grads(got, want, "grads against the restatement")
    _same(gx, wx, "gx against the restatement")
    assert all(not _bits(_host(got[f"bn{i}.{f}"])).any() for i in range(1, len(layers)) for f in ("mu", "sigma2"))


def test_gx_optional_and_the_flat_gradient(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 130, 2, 3
    m, P, X, gout, xd, gd, fwd = _setup(fx, layers, N, B, K)
    want, wx = _want(P, layers, K, X, gout, fwd)
    got, gx = m.grad_train(xd, gd, fwd=fwd)
    _same(gx, wx, "gx")
    alone, none = m.grad_train(xd, gd, fwd=fwd, input_grad=False)
    assert none is None
    _same_grads(alone, want, "input_grad=False")
    flat, fgx = m.flat_grad_train(xd, gd, fwd=fwd)
    _same(flat, gref.flat(want, layers), "flat_grad_train against grad_train")
    _same(fgx, wx, "flat_grad_train's gx")
    assert m.flat_grad_train(xd, gd, fwd=fwd, input_grad=False)[1] is None
    # the test-mode adjoint at the running statistics is another function
    other, _ = m.grad(xd, gd)
    assert not np.array_equal(_bits(_host(other["conv1.weight"])), _bits(want["conv1.weight"]))


def test_optional_arguments_two_runs_and_numpy_in_numpy_out(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P, X, gout, xd, gd, fwd = _setup(fx, layers, N, B, K)
    want, wx = _want(P, layers, K, X, gout, fwd)
    full, gx = m.grad_train(xd, gd, fwd=fwd)
    _same_grads(full, want, "fwd given")
    again, gx2 = m.grad_train(xd, gd, fwd=fwd)
    _same_grads(again, want, "two runs")
    _same(gx2, wx, "two runs: gx")
    for what, kw in (("fwd not given", {}), ("fwd not given, idx given", dict(idx=fwd["idx"])), ("fwd and idx given", dict(fwd=fwd, idx=fwd["idx"]))):
        got, g = m.grad_train(xd, gd, **kw)
        _same_grads(got, want, what)
        _same(g, wx, what + ": gx")
    hf = _host(fwd)
    got, g = m.grad_train(X, gout, fwd=hf)
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in got.values()) and isinstance(g, np.ndarray)
    assert {n: v.shape for n, v in got.items()} == ref.param_shapes(layers)
    _same_grads(got, want, "numpy in, numpy out")
    _same(g, wx, "numpy in, numpy out: gx")
    flat, g = m.flat_grad_train(X, gout)
    assert isinstance(flat, np.ndarray) and flat.shape == (m.param_count,)
    _same(flat, gref.flat(want, layers), "flat_grad_train, numpy, its own forward")
    _same(g, wx, "flat_grad_train, numpy: gx")


def test_a_batch_of_three(gpu_fx):
    """A batch of three is the chain over (b, chunk) and the fold over (half-tile, b) the restatement states; the clouds' separate
    results do not add up to it (every cloud's statistics would be its own)."""
    fx = gpu_fx
    layers, N, B, K = [64, 64, 128, 256], 70, 3, 3
    m, P, X, gout, xd, gd, fwd = _setup(fx, layers, N, B, K)
    want, wx = _want(P, layers, K, X, gout, fwd)
    got, gx = m.grad_train(xd, gd, fwd=fwd)
    _same_grads(got, want, "B = 3 against the restatement")
    _same(gx, wx, "B = 3: gx")


def test_gamma_zero_and_zero_gout(gpu_fx):
    """gamma = 0 on hidden channels 7 and 20 and on the last layer's channel 9: gv of those channels is zero, so dW and db are zero
    there, dgamma and dbeta are the restatement's and finite.  gout = 0: every bit of every family and of gx is zero."""
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    P = ref.random_params(layers, SEED)
    P["bn1.gamma"][[7, 20]] = 0
    P["bn2.gamma"][9] = 0
    m, P, X, gout, xd, gd, fwd = _setup(fx, layers, N, B, K, P)
    want, wx = _want(P, layers, K, X, gout, fwd)
    got, gx = m.grad_train(xd, gd, fwd=fwd)
    got = _host(got)
    _same_grads(got, want, "gamma = 0 against the restatement")
    _same(gx, wx, "gx")
    for ch in (7, 20):
        assert not got["conv1.weight"][0, :, ch].any() and got["conv1.bias"][ch] == 0
        assert np.isfinite(got["bn1.gamma"][ch]) and np.isfinite(got["bn1.beta"][ch])
    assert not got["conv2.weight"][0, :, 9].any() and got["conv2.bias"][9] == 0
    zero, zx = m.grad_train(xd, fx.gpu(np.zeros_like(gout)), fwd=fwd)
    assert all(not _bits(_host(v)).any() for v in zero.values()) and not _bits(zx.to_host()).any()


def test_hand_made_lists(gpu_fx):
    """Every point's searched neighbours rotated by one point (test_gpu_edgeconv_train.py's lists), and lists with the point itself
    twice, repeats and a permutation (test_gpu_edgeconv_pgrad.py's)."""
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P, X, gout, xd, gd, fwd = _setup(fx, layers, N, B, K)
    rotated = np.asfortranarray(((_host(fwd["idx"]) + 1) % N).astype(np.int32))
    made = np.empty((K, N, B), np.int32, order="F")
    n = np.arange(N)
    made[0], made[1], made[2] = n[:, None], n[:, None], ((n + 1) % N)[:, None]
    made[3], made[4], made[5] = 0, N - 1, ((7 * n + 3) % N)[:, None]
    made[5, :, 1] = made[2, :, 1]
    for what, lists in (("rotated lists", rotated), ("hand-made lists", made)):
        f = m.forward_train(xd, idx=fx.gpu(lists), intermediates=True)
        assert np.array_equal(_host(f["idx"]), lists)
        want, wx = _want(P, layers, K, X, gout, f)
        got, gx = m.grad_train(xd, gd, fwd=f)
        _same_grads(got, want, what)
        _same(gx, wx, what + ": gx")
        got, gx = m.grad_train(xd, gd, idx=fx.gpu(lists))
        _same_grads(got, want, what + ", the forward run inside")
        _same(gx, wx, what + ", the forward run inside: gx")


def test_graph_replay(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 200, 2, 4
    m, P, X, gout, xd, gd, fwd = _setup(fx, layers, N, B, K)
    eager, egx = m.flat_grad_train(xd, gd, fwd=fwd)
    eager, egx = eager.to_host(), egx.to_host()
    assert np.all(np.isfinite(eager)) and 2 * np.count_nonzero(eager) >= eager.size
    s = fx.Stream.create()
    with fx.stream(s):
        xs, gs = fx.gpu(X), fx.gpu(gout)
        m.flat_grad_train(xs, gs)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec, rgx = m.flat_grad_train(xs, gs)  # the search, the training-mode forward and the adjoint are inside the capture
        g.launch()
        g.launch()
        s.synchronize()
        _same(rec, eager, "graph replay against the eager run")
        _same(rgx, egx, "graph replay: gx")


def test_status_codes_and_the_workspace_bound(gpu_fx):
    """The refusals of tests/test_edgeconv_grad_train_host.py with real device arrays around one call that runs; out NULL through
    the C entry point gives the bits of out given; a workspace one byte short is refused."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    lib = _lib.load()
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P, X, gout, x, g, fwd = _setup(fx, layers, N, B, K)
    idx, out = fwd["idx"], fwd["out"]
    stats = fx.gpu(np.concatenate([_host(v) for v in fwd["batch_stats"].values()]))
    gp = DeviceArray.empty((m.param_count,), np.float32)
    gx = DeviceArray.empty((5, N, B), np.float32)
    la = (ctypes.c_int32 * 3)(*layers)
    nb = ctypes.c_size_t(0)
    assert lib.fx3d_edgeconv_grad_train_workspace_bytes(la, 3, K, N, B, ctypes.byref(nb)) == 0 and nb.value > 0
    ws = DeviceArray.empty((nb.value + 512,), np.uint8)
    assert ws.ptr % 256 == 0
    pd = m._params_dev()

    def call(params=pd.ptr, layers_=layers, nl=None, K_=K, x_=x.ptr, N_=N, B_=B, idx_=idx.ptr, out_=out.ptr, st_=stats.ptr, g_=g.ptr,
             gp_=gp.ptr, gx_=gx.ptr, ws_=ws.ptr, bytes_=nb.value):
        arr = (ctypes.c_int32 * len(layers_))(*layers_)
        return lib.fx3d_edgeconv_grad_train(params, arr, len(layers_) if nl is None else nl, K_, x_, N_, B_, idx_, out_, st_, g_, gp_,
                                            gx_, ws_, bytes_, None)

    assert call() == 0
    fx.synchronize()
    want, wantx = gp.to_host(), gx.to_host()
    G, wx = _want(P, layers, K, X, gout, fwd)
    _same(want, gref.flat(G, layers), "the C entry point against the restatement")
    _same(wantx, wx, "the C entry point: gx")
    assert call(idx_=None, out_=None, gx_=None) == 0   # all three optional: the search and the closing forward run first
    fx.synchronize()
    _same(gp, want, "idx, out and gx NULL through the C entry point")
    assert call(out_=None) == 0
    fx.synchronize()
    _same(gp, want, "out NULL through the C entry point")
    _same(gx, wantx, "out NULL: gx")
    assert call(params=None) == INVALID and call(x_=None) == INVALID and call(g_=None) == INVALID
    assert call(st_=None) == INVALID and "batch_stats" in _lib.last_error()
    assert call(gp_=None) == INVALID and call(ws_=None) == INVALID
    assert lib.fx3d_edgeconv_grad_train(pd.ptr, None, 3, K, x.ptr, N, B, None, None, stats.ptr, g.ptr, gp.ptr, None, ws.ptr, nb.value,
                                        None) == INVALID
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
        assert lib.fx3d_edgeconv_grad_train_workspace_bytes(la, 3, *args, ctypes.byref(nb)) == INVALID, args
    assert lib.fx3d_edgeconv_grad_train_workspace_bytes(la, 3, K, N, B, None) == INVALID
    fx.synchronize()
    _same(gp, want, "gparams after the refusals")
    _same(gx, wantx, "gx after the refusals")
    with pytest.raises(TypeError, match="Float32"):
        m.grad_train(x, DeviceArray.empty((70, N, B), np.float64), fwd=fwd)
    with pytest.raises(ValueError, match="gout must be"):
        m.grad_train(x, DeviceArray.empty((70, N, 1), np.float32), fwd=fwd)
    with pytest.raises(TypeError, match="where X lives"):
        m.grad_train(x, gout, fwd=fwd)
    with pytest.raises(TypeError, match="where X lives"):
        m.grad_train(x, g, fwd=_host(fwd))


def test_the_two_stage_composition(gpu_fx):
    """DGCNN's two EdgeConv stages on its ec1 / ec2 parameters at N = 64, B = 2, K = 3:
    ec1.grad_train(X, ec2.grad_train(x1, g, fwd=...)[1], fwd=...) against the restatement's composition."""
    fx = gpu_fx
    N, B, K = 64, 2, 3
    L1, L2 = [3, 32, 64, 64], [64, 128, 256]
    P = dgcnn_ref.random_params(10, seed=3)
    P1 = {k[4:]: v for k, v in P.items() if k.startswith("ec1.")}
    P2 = {k[4:]: v for k, v in P.items() if k.startswith("ec2.")}
    X, gout = _normal(311, 3, N, B), _normal(312, 256, N, B)
    ec1, ec2 = fx.EdgeConv(L1, K).load(P1), fx.EdgeConv(L2, K).load(P2)
    xd, gd = fx.gpu(X), fx.gpu(gout)
    f1 = ec1.forward_train(xd, intermediates=True)
    f2 = ec2.forward_train(f1["out"], intermediates=True)
    got2, g1 = ec2.grad_train(f1["out"], gd, fwd=f2)
    got1, gx = ec1.grad_train(xd, g1, fwd=f1)
    want2, w1 = _want(P2, L2, K, _host(f1["out"]), gout, f2)
    want1, wx = _want(P1, L1, K, X, w1, f1)
    _same_grads(got2, want2, "stage 2")
    _same(g1, w1, "stage 2's gx, stage 1's gout")
    _same_grads(got1, want1, "stage 1")
    _same(gx, wx, "gx")
