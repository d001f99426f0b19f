"""EdgeConv(layers, K) on the device (fx3d_edgeconv_forward through fx.EdgeConv) against the host restatement
tests/edgeconv_ref.py: the neighbour lists and the output bit for bit (uint32 views, no element left out) -- DGCNN's two
instances against fx3d_dgcnn_forward's own x1 / x2 as well, widths that are no multiple of 4 or 32, one channel, four blocks,
the envelope's corner, given neighbour lists, an infinite weight in a tail channel, NaN input, all-negative channels, batch and
launch independence, a captured graph and host arrays; the workspace bound and the C entry points' status codes.

Every draw is first held to edgeconv_ref.check_draw on the restatement's own output (finite, at least half of it non-zero), so
that what is compared has something in it."""
import ctypes

import numpy as np
import pytest

import dgcnn_ref
import edgeconv_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID, UNSUPPORTED = -1, -5   # FX3D_ERR_INVALID_ARG, FX3D_ERR_UNSUPPORTED (include/flux3d_hip.h)
SEED = 1                        # edgeconv_ref.check_draw holds for every case below with this seed (asserted in each)


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype == np.int32 else a.astype(F32, copy=False)).view(np.uint32)


def _host(v):
    return v.to_host() if hasattr(v, "to_host") else np.asarray(v)


def _cloud(seed, F, N, B):
    return np.asfortranarray(np.random.default_rng(1000 + seed).standard_normal((F, N, B)).astype(F32))


def _same(got, want, what):
    got = _host(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    print(f"{what}: {bad.size} of {got.size} elements differ")
    assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


def _model(fx, layers, K, seed=SEED):
    P = ref.random_params(layers, seed)
    return fx.EdgeConv(layers, K).load(P), P


def test_same_bits_as_dgcnn(gpu_fx):
    """EdgeConv([3, 32, 64, 64], 10) with a DGCNN's ec1 arrays gives idx1 and x1 of DGCNN.forward(intermediates=True),
    EdgeConv([64, 128, 256], 10) on that x1 gives idx2 and x2; both are also the restatement's."""
    fx = gpu_fx
    N, B, K = 64, 2, 10
    P = dgcnn_ref.random_params(10, seed=3)
    X = _cloud(3, 3, N, B)
    d = fx.DGCNN(10, K, N).load(P).forward(fx.gpu(X), intermediates=True)
    x_in = fx.gpu(X)
    for name, layers, i_key, x_key in (("ec1", [3, 32, 64, 64], "idx1", "x1"), ("ec2", [64, 128, 256], "idx2", "x2")):
        own = {k[len(name) + 1:]: v for k, v in P.items() if k.startswith(name + ".")}
        out, idx = fx.EdgeConv(layers, K).load(own).forward(x_in, return_idx=True)
        _same(idx, d[i_key].to_host(), f"{name} idx against DGCNN's {i_key}")
        _same(out, d[x_key].to_host(), f"{name} out against DGCNN's {x_key}")
        want_idx, want = ref.forward(x_in.to_host(), own, layers, K)
        ref.check_draw(want)
        _same(idx, want_idx, f"{name} idx against the restatement")
        _same(out, want, f"{name} out against the restatement")
        x_in = d[x_key]


# (layers, N, B, K): the issue's table, then the two shapes at which three LDS images of stride 258 do not fit and the x_n
# half of the rows is gathered again with every k (L = 3: the fold reads the shared image; L = 4: a hidden layer does)
CASES = [([3, 16], 7, 1, 6),              # one block, all-VALU first layer, partial tile, K = N - 1
         ([1, 1], 9, 2, 3),               # Cin = 2 < 4, one channel
         ([5, 33, 70], 65, 3, 6),         # Cin = 10 and 33 no multiples of 4, partial output slabs, a second tile of one point
         ([4, 8, 8, 8, 40], 64, 2, 1),    # L = 4, K = 1
         ([6, 2, 255], 33, 2, 4),         # Cin = 2, 255-wide fold
         ([128, 256, 256], 130, 1, 20),   # the envelope's corner: stride 258, 256-channel input, three tiles
         ([64, 64, 128, 256], 70, 1, 5),
         ([65, 8, 8, 8], 66, 1, 3),
         ([65, 8, 8, 8, 8], 66, 2, 3)]


@pytest.mark.parametrize("layers,N,B,K", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_generic_widths_against_the_restatement(gpu_fx, layers, N, B, K):
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    m, P = _model(fx, layers, K)
    X = _cloud(SEED, layers[0], N, B)
    want_idx, want = ref.forward(X, P, layers, K)
    ref.check_draw(want)
    xd = fx.gpu(X)
    out, idx = m.forward(xd, return_idx=True)
    _same(idx, want_idx, "idx against the restatement")
    _same(out, want, "out against the restatement")
    plain = DeviceArray.empty((K, N, B), np.int32)
    _lib.call("fx3d_knn", xd.ptr, N, xd.ptr, N, B, layers[0], K, 1, plain.ptr, None, fx.current_stream().handle)
    _same(idx, plain.to_host(), "idx against fx3d_knn(x, x, D = F, k = K, drop_first = 1)")
    assert m(xd).shape == (layers[-1], N, B)


def test_given_neighbours(gpu_fx):
    """idx_in: the restatement's lists, then a hand-made valid list with repeated and self indices; out is the restatement
    evaluated on those lists and idx_out is not touched."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P = _model(fx, layers, K)
    X = _cloud(SEED, 5, N, B)
    xd = fx.gpu(X)
    searched, want = ref.forward(X, P, layers, K)
    ref.check_draw(want)
    _same(m.forward(xd, idx=searched), want, "the restatement's lists, host")
    out, used = m.forward(xd, idx=fx.gpu(searched), return_idx=True)
    _same(out, want, "the restatement's lists, device")
    _same(used, searched, "the lists handed back")
    made = np.empty((K, N, B), np.int32, order="F")
    n = np.arange(N)
    made[0], made[1], made[2] = n[:, None], n[:, None], ((n + 1) % N)[:, None]     # the point itself twice, its successor
    made[3], made[4], made[5] = 0, N - 1, ((7 * n + 3) % N)[:, None]                # the first and the last point, a permutation
    made[5, :, 1] = made[2, :, 1]                                                   # a repeated neighbour in cloud 1
    _, want_made = ref.forward(X, P, layers, K, idx=made)
    ref.check_draw(want_made)
    assert not np.array_equal(_bits(want_made), _bits(want))
    _same(m.forward(X, idx=made), want_made, "hand-made lists, numpy in and out")
    # idx_out with idx_in given: through the C entry point
    la = (ctypes.c_int32 * 3)(*layers)
    nb = _lib.query_bytes("fx3d_edgeconv_workspace_bytes", la, 3, K, N, B)
    ws = DeviceArray.empty((nb + 256,), np.uint8)
    sentinel = np.full((K, N, B), -77, np.int32, order="F")
    idx_out, made_dev, out = fx.gpu(sentinel), fx.gpu(made), DeviceArray.empty((70, N, B), np.float32)
    _lib.call("fx3d_edgeconv_forward", m._params_dev().ptr, la, 3, K, xd.ptr, N, B, made_dev.ptr, out.ptr, idx_out.ptr, ws.ptr,
              nb, fx.current_stream().handle)
    _same(out, want_made, "hand-made lists, C entry point")
    _same(idx_out, sentinel, "idx_out with idx_in given")


def test_infinite_weight_in_a_tail_channel(gpu_fx):
    """[5, 33, 70]: input channels 8 and 9 of layer 1 and channel 32 of layer 2 are the tail beyond 4 floor(Cin / 4), which the
    kernel walks with v_fma_f32.  One +Inf weight in each: the output is the restatement's, Inf or NaN exactly where the chain
    makes them and nowhere else -- a zero-padded contraction would make NaN (0 * Inf) in every channel of the slab instead.
    Bit for bit, the NaNs included: the restatement's own NaN pattern (0xffc00000, what 0 * Inf gives) is the device's."""
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P = _model(fx, layers, K)
    X = _cloud(SEED, 5, N, B)
    ref.check_draw(ref.forward(X, P, layers, K)[1])   # the draw before the change
    P["conv1.weight"][0, 9, 3] = np.inf
    P["conv2.weight"][0, 32, 5] = np.inf
    m.load(P)
    want_idx, want = ref.forward(X, P, layers, K)
    nonfinite = ~np.isfinite(want)
    assert np.isnan(want).any() and np.isinf(want).any() and not nonfinite.all()
    out, idx = m.forward(fx.gpu(X), return_idx=True)
    got = _host(out)
    _same(idx, want_idx, "idx")
    print(f"{int(np.isnan(want).sum())} NaN and {int(np.isinf(want).sum())} Inf of {want.size} in the restatement")
    _same(got, want, "out")


def test_nan_stays_in_its_cloud(gpu_fx):
    fx = gpu_fx
    layers, N, K = [5, 33, 70], 65, 6
    m, P = _model(fx, layers, K)
    X = _cloud(SEED, 5, N, 3)
    ref.check_draw(ref.forward(X, P, layers, K)[1])
    Xn = X.copy(order="F")
    Xn[1, 37, 1] = np.nan
    out, idx = m.forward(fx.gpu(Xn), return_idx=True)
    out, idx = out.to_host(), idx.to_host()
    assert np.all(np.isnan(out[:, 37, 1]))  # the point itself, at the least
    assert idx.min() >= 0 and idx.max() < N  # a NaN distance sorts last: every index is a point of the cloud
    for b in (0, 2):
        alone, alone_idx = m.forward(fx.gpu(np.asfortranarray(X[:, :, b:b + 1])), return_idx=True)
        _same(out[:, :, b:b + 1], alone.to_host(), f"cloud {b} beside the NaN cloud")
        _same(idx[:, :, b:b + 1], alone_idx.to_host(), f"idx of cloud {b} beside the NaN cloud")


def test_all_negative_channels_give_plus_zero(gpu_fx):
    """test_gpu_dgcnn.py's construction on [5, 33, 70]: channels 9 and 69 of the last layer have a BatchNorm output of -1 on
    every edge row (zero weights, bias = mu, beta = -1): relu gives +0.0 and the maximum over k keeps it."""
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, P = _model(fx, layers, K)
    X = _cloud(SEED, 5, N, B)
    base = ref.forward(X, P, layers, K)[1]  # the draw as it is: these channels are alive, so the zeros come from the change alone
    ref.check_draw(base)
    assert np.count_nonzero(base[9]) and np.count_nonzero(base[69])
    for ch in (9, 69):
        P["conv2.weight"][0, :, ch] = 0
        P["conv2.bias"][ch] = P["bn2.mu"][ch]
        P["bn2.beta"][ch] = -1
    m.load(P)
    want = ref.forward(X, P, layers, K)[1]
    got = m(fx.gpu(X)).to_host()
    _same(got, want, "zero channels")
    assert np.all(_bits(want[9]) == 0) and np.all(_bits(want[69]) == 0)  # +0.0, sign bit clear
    assert np.all(_bits(got[9]) == 0) and np.all(_bits(got[69]) == 0)


def test_independence_of_batch_and_launch(gpu_fx):
    fx = gpu_fx
    layers, N, K = [64, 64, 128, 256], 70, 5
    m, _ = _model(fx, layers, K)
    X = _cloud(SEED, 64, N, 3)
    xd = fx.gpu(X)
    out, idx = m.forward(xd, return_idx=True)
    out, idx = out.to_host(), idx.to_host()
    again, again_idx = m.forward(xd, return_idx=True)
    _same(again, out, "two runs, out")
    _same(again_idx, idx, "two runs, idx")
    for b in range(3):
        alone, alone_idx = m.forward(fx.gpu(np.asfortranarray(X[:, :, b:b + 1])), return_idx=True)
        _same(alone, out[:, :, b:b + 1], f"cloud {b} alone against its batch, out")
        _same(alone_idx, idx[:, :, b:b + 1], f"cloud {b} alone against its batch, idx")


def test_graph_replay_and_numpy_in_numpy_out(gpu_fx):
    fx = gpu_fx
    layers, N, B, K = [5, 33, 70], 200, 2, 10
    m, P = _model(fx, layers, K)
    X = _cloud(SEED, 5, N, B)
    out, idx = m.forward(X, return_idx=True)  # numpy in, numpy out
    assert isinstance(out, np.ndarray) and isinstance(idx, np.ndarray) and idx.dtype == np.int32 and out.dtype == np.float32
    eager, eager_idx = m.forward(fx.gpu(X), return_idx=True)
    _same(eager, out, "device in against numpy in, out")
    _same(eager_idx, idx, "device in against numpy in, idx")
    one = m(X[:, :, 0])  # (F, N): one cloud
    assert isinstance(one, np.ndarray) and one.shape == (70, N, 1)
    _same(one, out[:, :, :1], "one cloud as (F, N)")
    e3, _ = _model(fx, [3, 16], 4)
    Y = _cloud(SEED, 3, 30, 2)
    _same(e3(fx.PointCloud(fx.gpu(Y))), e3(Y), "a PointCloud at F = 3")
    s = fx.Stream.create()
    with fx.stream(s):
        xd = fx.gpu(X)
        m.forward(xd, return_idx=True)  # eager once on this stream: workspace and kernel attributes
        s.synchronize()
        g = fx.Graph()
        with g.capture(s):
            rec, rec_idx = m.forward(xd, return_idx=True)  # the search is inside the capture
        g.launch()
        g.launch()
        s.synchronize()
        _same(rec, out, "graph replay against the eager run, out")
        _same(rec_idx, idx, "graph replay against the eager run, idx")


def test_workspace_is_smaller_than_the_edge_tensor(gpu_fx):
    """[64, 128, 256] at 32 x 1024, K = 20: the (K N, 2F, B) input of the convolutions is 335 MB; the path holds the neighbour
    lists (2.6 MB) and the search's scratch.  A query only: nothing runs."""
    from flux3d_jl_amd import _lib
    la = (ctypes.c_int32 * 3)(64, 128, 256)
    nb = _lib.query_bytes("fx3d_edgeconv_workspace_bytes", la, 3, 20, 1024, 32)
    print(f"fx3d_edgeconv_workspace_bytes([64, 128, 256], K = 20, N = 1024, B = 32) = {nb} bytes")
    assert 4 * 20 * 1024 * 32 <= nb < 20 * 1024 * 2 * 64 * 32 * 4, nb


def test_status_codes(gpu_fx):
    """The refusals of tests/test_edgeconv_host.py with real device arrays around one call that runs: the code itself is
    compared, and every refusal comes before any launch."""
    fx = gpu_fx
    from flux3d_jl_amd import _lib
    from flux3d_jl_amd.device import DeviceArray
    lib = _lib.load()
    layers, N, B, K = [5, 33, 70], 65, 2, 6
    m, _ = _model(fx, layers, K)
    x = fx.gpu(_cloud(SEED, 5, N, B))
    out = DeviceArray.empty((70, N, B), np.float32)
    la = (ctypes.c_int32 * 3)(*layers)
    nb = ctypes.c_size_t(0)
    assert lib.fx3d_edgeconv_workspace_bytes(la, 3, K, N, B, ctypes.byref(nb)) == 0 and nb.value > 0
    ws = DeviceArray.empty((nb.value + 512,), np.uint8)
    assert ws.ptr % 256 == 0
    pd = m._params_dev()

    def call(params=pd.ptr, layers_=layers, nl=None, K_=K, x_=x.ptr, N_=N, B_=B, out_=out.ptr, ws_=ws.ptr, bytes_=nb.value):
        arr = (ctypes.c_int32 * len(layers_))(*layers_)
        return lib.fx3d_edgeconv_forward(params, arr, len(layers_) if nl is None else nl, K_, x_, N_, B_, None, out_, None, ws_,
                                         bytes_, None)

    assert call() == 0
    fx.synchronize()
    assert call(params=None) == INVALID and call(x_=None) == INVALID and call(out_=None) == INVALID and call(ws_=None) == INVALID
    assert lib.fx3d_edgeconv_forward(pd.ptr, None, 3, K, x.ptr, N, B, None, out.ptr, None, ws.ptr, nb.value, None) == INVALID
    assert call(layers_=[5]) == UNSUPPORTED and call(layers_=[5, 8, 8, 8, 8, 8]) == UNSUPPORTED and call(nl=0) == UNSUPPORTED
    assert call(layers_=[5, 0, 70]) == UNSUPPORTED and call(layers_=[5, 33, 257]) == UNSUPPORTED and "257" in _lib.last_error()
    assert call(layers_=[129, 33, 70]) == UNSUPPORTED and "129" in _lib.last_error()
    assert call(K_=0) == INVALID and call(K_=-3) == INVALID
    assert call(K_=N) == INVALID and "K + 1" in _lib.last_error()          # K + 1 > N
    assert call(N_=0) == INVALID and call(B_=0) == INVALID
    assert call(N_=36865) == INVALID and "neighbour search" in _lib.last_error()
    assert call(bytes_=nb.value - 1) == INVALID and "workspace" in _lib.last_error()
    assert call(ws_=ws.ptr + 16) == INVALID and "aligned" in _lib.last_error()
    for args in ((K, 0, B), (K, N, 0), (0, N, B), (N, N, B), (K, 36865, 1)):
        assert lib.fx3d_edgeconv_workspace_bytes(la, 3, *args, ctypes.byref(nb)) == INVALID, args
    assert lib.fx3d_edgeconv_workspace_bytes(la, 3, K, N, B, None) == INVALID
    with pytest.raises(TypeError, match="int32"):
        m(x, idx=DeviceArray.empty((K, N, B), np.float32))
    with pytest.raises(ValueError, match="idx must be"):
        m(x, idx=DeviceArray.empty((K, N, 1), np.int32))
    with pytest.raises(TypeError, match="Float32"):
        m(DeviceArray.empty((5, N, B), np.float64))
