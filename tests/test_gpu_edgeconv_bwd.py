"""The EdgeConv input adjoint on the device (fx3d_edgeconv_bwd through fx.EdgeConv.input_grad) against the host restatement
tests/edgeconv_bwd_ref.py, bit for bit (uint32 views, no element left out): the shape table -- partial tiles, a second tile of
one point, tails of 1 to 3 channels in both contraction directions, K = 1, tied maxima, the LDS corner --, the optional
arguments, hand-made neighbour lists, dead channels, infinite weights in the backward tails, run and batch independence, a
captured graph, DGCNN's two-stage chain, the workspace bound and the C entry point's status codes.

idx and out are the device's own forward's (tests/test_gpu_edgeconv.py holds them to the forward restatement).  Every draw is
first held to edgeconv_bwd_ref.check_draw on the restatement's own gradient (finite, at least half of it non-zero)."""
import ctypes

import numpy as np
import pytest

import dgcnn_ref
import edgeconv_bwd_ref as bref
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


def _setup(fx, layers, N, B, K, P=None):
    """The model, its parameters, X and gout (standard normal) on host and device, and the device's own forward."""
    P = ref.random_params(layers, SEED) if P is None else P
    m = fx.EdgeConv(layers, K).load(P)
    X, gout = _normal(1000 + SEED, layers[0], N, B), _normal(2000 + SEED, layers[-1], N, B)
    xd, gd = fx.gpu(X), fx.gpu(gout)
    out, idx = m.forward(xd, return_idx=True)
    return m, P, X, gout, xd, gd, idx, out


# (layers, N, B, K)
CASES = [([3, 16], 7, 1, 6),
         ([1, 1], 9, 2, 3),
         ([5, 33, 70], 65, 3, 6),                    # tails of 2, 1, 2 channels forward, 1 and 2 backward; a second tile of one point
         ([4, 8, 8, 8, 40], 64, 2, 1),               # L = 4, K = 1
         ([6, 2, 255], 33, 2, 4),                    # tied maxima (dead hidden rows), a backward tail of 3
         ([128, 256, 256], 130, 1, 20),              # two images of stride 258, three tiles
         ([64, 64, 128, 256], 70, 1, 5),             # 32-point tiles
         ([65, 8, 8, 8], 66, 1, 3),
         ([65, 8, 8, 8, 8], 66, 2, 3),
         ([40, 8, 8, 8, 72], 34, 2, 3),              # stride 130 at L = 4: 32-point tiles, a second tile of two points, tails of 8
         ([128, 256, 256, 256, 256], 33, 1, 2),      # the LDS corner: four images of stride 258 at 32 points
         ([3, 32, 64, 64], 64, 2, 10),               # DGCNN's two stages
         ([64, 128, 256], 64, 2, 10)]


@pytest.mark.parametrize("layers,N,B,K", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_the_shape_table_against_the_restatement(gpu_fx, layers, N, B, K):
    fx = gpu_fx
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K)
    want = bref.input_grad(X, P, layers, K, gout, idx.to_host(), out.to_host())
    bref.check_draw(want)
    print(f"non-zero share of the restatement's gradient {np.count_nonzero(want) / want.size:.2f}")
    _same(m.input_grad(xd, gd, idx, out), want, "gx against the restatement")


def test_optional_arguments_and_numpy_in_numpy_out(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K)
    full = m.input_grad(xd, gd, idx, out).to_host()
    bref.check_draw(full)
    _same(m.input_grad(xd, gd), full, "idx = None, out = None")
    _same(m.input_grad(xd, gd, idx=idx), full, "out = None")
    _same(m.input_grad(xd, gd, out=out), full, "idx = None")
    got = m.input_grad(X, gout, idx.to_host(), out.to_host())
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    _same(got, full, "numpy in, numpy out")
    one = m.input_grad(X[:, :, 0], gout[:, :, 0])
    assert isinstance(one, np.ndarray) and one.shape == (5, N, 1)
    _same(one, full[:, :, :1], "one cloud as (F, N)")


def test_hand_made_lists(gpu_fx):
    """test_given_neighbours' lists: the point itself twice, repeats, a permutation.  Repeated neighbours tie the maximum; a rule
    that pays every tied k would double these."""
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P, X, gout, xd, gd, _, _ = _setup(fx, layers, N, B, K)
    made = np.empty((K, N, B), np.int32, order="F")
    n = np.arange(N)
    made[0], made[1], made[2] = n[:, None], n[:, None], ((n + 1) % N)[:, None]
    made[3], made[4], made[5] = 0, N - 1, ((7 * n + 3) % N)[:, None]
    made[5, :, 1] = made[2, :, 1]
    _, out = ref.forward(X, P, layers, K, idx=made)
    want = bref.input_grad(X, P, layers, K, gout, made, out)
    bref.check_draw(want)
    _same(m.input_grad(xd, gd, idx=fx.gpu(made)), want, "hand-made lists, out computed on the device")
    _same(m.input_grad(X, gout, idx=made, out=out), want, "hand-made lists, numpy in and out")


def test_dead_channels_pass_nothing(gpu_fx):
    """test_gpu_edgeconv.py's construction: channels 9 and 69 of the last layer are -1 before the relu on every edge row, so
    out is +0 there and gout on them must not reach gx: the same bits as with gout zeroed on those channels."""
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    P = ref.random_params(layers, SEED)
    for ch in (9, 69):
        P["conv2.weight"][0, :, ch] = 0
        P["conv2.bias"][ch] = P["bn2.mu"][ch]
        P["bn2.beta"][ch] = -1
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K, P)
    oh = out.to_host()
    assert np.all(_bits(oh[9]) == 0) and np.all(_bits(oh[69]) == 0)
    zeroed = gout.copy(order="F")
    zeroed[[9, 69]] = 0
    want = bref.input_grad(X, P, layers, K, gout, idx.to_host(), oh)
    bref.check_draw(want)
    got = m.input_grad(xd, gd, idx, out)
    _same(got, want, "dead channels against the restatement")
    _same(m.input_grad(xd, fx.gpu(zeroed), idx, out), got.to_host(), "gout zeroed on the dead channels")


def test_infinite_weights_in_the_backward_tails(gpu_fx):
    """[5, 33, 70]: walking back, layer 2 contracts over 70 channels (68 and 69 are the tail beyond 4 floor(70 / 4)) and layer 1
    over 33 (channel 32).  One +Inf weight in each tail: NaN exactly where the restatement's chains make it (0 * Inf among
    them; no term is skipped, no contraction padded), every other element bit for bit.  NaN payloads are not compared."""
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    P = ref.random_params(layers, SEED)
    X, gout = _normal(1000 + SEED, 5, N, B), _normal(2000 + SEED, 70, N, B)
    bref.check_draw(bref.input_grad(X, P, layers, K, gout))   # the draw before the change
    P["conv2.weight"][0, 7, 69] = np.inf
    P["conv1.weight"][0, 3, 32] = np.inf
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K, P)
    want = bref.input_grad(X, P, layers, K, gout, idx.to_host(), out.to_host())
    nan = np.isnan(want)
    print(f"{int(nan.sum())} NaN of {want.size} in the restatement")
    assert nan.any() and not nan.all()
    got = m.input_grad(xd, gd, idx, out).to_host()
    assert np.array_equal(np.isnan(got), nan), "the NaN masks differ"
    bad = (_bits(got) != _bits(want)) & ~nan
    print(f"{int(bad.sum())} of {int((~nan).sum())} elements that are no NaN differ")
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def test_independence_of_run_and_batch(gpu_fx):
    fx = gpu_fx
    layers, N, K = [64, 64, 128, 256], 70, 5
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, 3, K)
    first = m.input_grad(xd, gd, idx, out).to_host()
    bref.check_draw(first)
    _same(m.input_grad(xd, gd, idx, out), first, "two runs")
    for b in range(3):
        alone = m.input_grad(fx.gpu(np.asfortranarray(X[:, :, b:b + 1])), fx.gpu(np.asfortranarray(gout[:, :, b:b + 1])))
        _same(alone, first[:, :, b:b + 1], f"cloud {b} alone against its batch")


def test_graph_replay(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 200, 2, 10
    m, P, X, gout, xd, gd, idx, out = _setup(fx, layers, N, B, K)
    eager = m.input_grad(xd, gd, idx, out).to_host()
    bref.check_draw(eager)
    s = fx.Stream.create()
    with fx.stream(s):
        xs, gs = fx.gpu(X), fx.gpu(gout)
        m.input_grad(xs, gs)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec = m.input_grad(xs, gs)  # the search and the forward are inside the capture
        g.launch()
        g.launch()
        s.synchronize()
        _same(rec, eager, "graph replay against the eager run")


def test_the_dgcnn_chain(gpu_fx):
    """d sum(g x2) / d X through both EdgeConv stages of a DGCNN, composed on the device from the DGCNN's own idx1, x1, idx2, x2,
    against the composed restatement."""
    fx = gpu_fx
    N, B, K = 64, 2, 10
    L1, L2 = [3, 32, 64, 64], [64, 128, 256]
    P = dgcnn_ref.random_params(10, seed=3)
    P1 = {k[4:]: v for k, v in P.items() if k.startswith("ec1.")}
    P2 = {k[4:]: v for k, v in P.items() if k.startswith("ec2.")}
    X, g = _normal(1000 + SEED, 3, N, B), _normal(2000 + SEED, 256, N, B)
    xd = fx.gpu(X)
    d = fx.DGCNN(10, K, N).load(P).forward(xd, intermediates=True)
    ec1, ec2 = fx.EdgeConv(L1, K).load(P1), fx.EdgeConv(L2, K).load(P2)
    g1 = ec2.input_grad(d["x1"], fx.gpu(g), d["idx2"], d["x2"])
    got = ec1.input_grad(xd, g1, d["idx1"], d["x1"])
    x1 = d["x1"].to_host()
    want1 = bref.input_grad(x1, P2, L2, K, g, d["idx2"].to_host(), d["x2"].to_host())
    want = bref.input_grad(X, P1, L1, K, want1, d["idx1"].to_host(), x1)
    bref.check_draw(want1)
    bref.check_draw(want)
    _same(g1, want1, "d x2 / d x1")
    _same(got, want, "d x2 / d X")


def test_workspace_is_smaller_than_the_edge_tensor(gpu_fx):
    """[64, 128, 256] at 32 x 1024, K = 20: the (K N, 2F, B) edge tensor that edge_features_grad needs is 335 MB; the adjoint
    holds the lists, out (33.5 MB), the transposed weights and the search's scratch.  A query only: nothing runs."""
    from flux3d_jl_amd import _lib
    la = (ctypes.c_int32 * 3)(64, 128, 256)
    nb = _lib.query_bytes("fx3d_edgeconv_bwd_workspace_bytes", la, 3, 20, 1024, 32)
    print(f"fx3d_edgeconv_bwd_workspace_bytes([64, 128, 256], K = 20, N = 1024, B = 32) = {nb} bytes")
    assert 4 * (20 + 256) * 1024 * 32 <= nb < 20 * 1024 * 2 * 64 * 32 * 4, nb


def test_status_codes(gpu_fx):
    """The refusals of tests/test_edgeconv_bwd_host.py with real device arrays around one call that runs."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    lib = _lib.load()
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P, X, gout, x, g, idx, out = _setup(fx, layers, N, B, K)
    gx = DeviceArray.empty((5, N, B), np.float32)
    la = (ctypes.c_int32 * 3)(*layers)
    nb = ctypes.c_size_t(0)
    assert lib.fx3d_edgeconv_bwd_workspace_bytes(la, 3, K, N, B, ctypes.byref(nb)) == 0 and nb.value > 0
    ws = DeviceArray.empty((nb.value + 512,), np.uint8)
    assert ws.ptr % 256 == 0
    pd = m._params_dev()

    def call(params=pd.ptr, layers_=layers, nl=None, K_=K, x_=x.ptr, N_=N, B_=B, idx_=idx.ptr, out_=out.ptr, g_=g.ptr, gx_=gx.ptr,
             ws_=ws.ptr, bytes_=nb.value):
        arr = (ctypes.c_int32 * len(layers_))(*layers_)
        return lib.fx3d_edgeconv_bwd(params, arr, len(layers_) if nl is None else nl, K_, x_, N_, B_, idx_, out_, g_, gx_, ws_,
                                     bytes_, None)

    assert call() == 0
    fx.synchronize()
    want = gx.to_host()
    assert call(idx_=None, out_=None) == 0   # both optional
    fx.synchronize()
    _same(gx, want, "idx and out NULL through the C entry point")
    assert call(params=None) == INVALID and call(x_=None) == INVALID and call(g_=None) == INVALID
    assert call(gx_=None) == INVALID and call(ws_=None) == INVALID
    assert lib.fx3d_edgeconv_bwd(pd.ptr, None, 3, K, x.ptr, N, B, None, None, g.ptr, gx.ptr, ws.ptr, nb.value, None) == INVALID
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
        assert lib.fx3d_edgeconv_bwd_workspace_bytes(la, 3, *args, ctypes.byref(nb)) == INVALID, args
    assert lib.fx3d_edgeconv_bwd_workspace_bytes(la, 3, K, N, B, None) == INVALID
    _same(gx, want, "gx after the refusals")
    with pytest.raises(TypeError, match="Float32"):
        m.input_grad(x, DeviceArray.empty((70, N, B), np.float64))
    with pytest.raises(ValueError, match="gout must be"):
        m.input_grad(x, DeviceArray.empty((70, N, 1), np.float32))
    with pytest.raises(ValueError, match="out must be"):
        m.input_grad(x, g, out=DeviceArray.empty((69, N, B), np.float32))
    with pytest.raises(TypeError, match="int32"):
        m.input_grad(x, g, idx=DeviceArray.empty((K, N, B), np.float32))
    with pytest.raises(TypeError, match="where X lives"):
        m.input_grad(x, gout)
