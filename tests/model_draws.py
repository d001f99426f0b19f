"""Named families of (X, parameters, upstream gradient) beyond unit scale for the exact-Float32 model kernels -- PointNet forward,
EdgeConv forward / input_grad / grad, DGCNN forward / grad -- and the condition each family must meet on the host restatement's
OWN result before a device result is compared with it.  A plain helper (numpy and the ``*_ref`` modules only): tests/
test_model_draws_host.py holds every family to its condition on the host, tests/test_gpu_model_draws.py compares the device.

A network is ``("edgeconv", layers)``, ``("dgcnn", num_classes)`` or ``("pointnet", num_classes)``.  :func:`draw` returns a dict
with ``X`` (F, N, B), ``P`` (name -> array, Flux's shapes), ``g`` (gout (cL, N, B) / glogits (nc, B) / None for PointNet) and the
family's own notes (edited channels).  Everything is seeded: a (family, network, N, B) names one draw.

The families (where a scale differs between networks the line says why; the measured shares are printed by the host test):

subnormal_mid    X = standard normal x 1e-20, the weights of the layers that read X x 1e-19; bias, mu, beta of every layer
                 exactly +0 (nothing of order 0.1 absorbs the small values).  The first layer's output is of order 1e-39.
                 PointNet keeps the last dense bias of its two transform nets (stn.dense3, fstn.dense3): the reference adds no
                 identity, so with a zero bias the transform is itself of order 1e-39 and x T underflows to zero everywhere.
subnormal_input  X x 1e-39 (every coordinate subnormal), the same zeroed offsets, weights unscaled.
decades          every element of X and of the upstream gradient is a standard normal x 10 ** integers(-6, 7); random_params.
decades_small    X elements x 10 ** integers(-44, -29) with the zeroed offsets: normal and subnormal terms in one chain.  The
                 upstream gradient is drawn the same way on the even points (clouds, for glogits) and is unit scale on the odd
                 ones, so that both the input adjoint's chains and the parameter sums see small and ordinary rows.
decades_edge     as decades_small with exponents in [-41, -36]: the largest terms of a chain are barely normal, so that the
                 subnormal ones are within Float32's 7 digits of them and a flushed term changes the result's bits.  (In
                 decades_small the largest term, of order 1e-30, hides every subnormal one.)
large            X x 1e20 with random_params.  (At 1e18 a squared distance is of order 1e37, inside Float32; at 1e20 more than
                 half of the search's squared distances are +Inf -- asserted -- and every chain stays finite.)  PointNet has no
                 search and multiplies by its own transforms twice (activations grow like the 4th power): X x 1e9, pooled up to 1e37.
overflow         X x 1e30, the weights of the layers that read X x 1e8: +Inf, NaN and finite values in one output (+Inf present,
                 the other two at least 1 % each).  [64, 128, 256] (chains of 128 products) takes 6e7, [3, 32, 64, 64] 7e7 and
                 DGCNN 4e7 instead of 1e8: at 1e8 under 1 % of their outputs stays finite or no +Inf is left.  PointNet: an
                 overflow in its first layers makes both transforms NaN and with them everything; X x 3.5e9 with unscaled weights
                 overflows in feat.conv2 instead: one cloud's pooled is NaN, the other's +Inf and finite, the logits are NaN.
negative_gamma   random_params with the sign of gamma flipped on a seeded half of the channels of every BatchNorm.
sigma2_edges     random_params with, in EVERY BatchNorm of C channels, sigma2 = 0 on channels (0, C - 3), sigma2 = -eps (Float32:
                 sigma2 + eps == 0, sd = 0) on (1, C - 2) and sigma2 = -1 (sd = NaN) on (2, C - 1).  A NaN hidden channel reaches
                 every later element, so this draw is NaN almost everywhere: it pins how NaN and Inf spread.
sigma2_edges_last  EdgeConv only: the same edit on the LAST BatchNorm alone, so that `out` is non-finite in exactly the edited
                 channels and the last layer's families are finite in every other channel.
sigma2_zero      sigma2 = 0 alone (sd = sqrt(eps), a factor 316) on the same two channels of every BatchNorm: all finite, so unlike
                 the two draws above it reaches every chain of the adjoints; the host test also holds it to float64 autograd.
constant_cloud   every point of a cloud is the same finite point (one per cloud); random_params.  EdgeConv and DGCNN only.

The training-mode entry points -- PointNet forward_train / grad_train, EdgeConv and DGCNN forward_train -- have a section of their
own below (train_families, draw_train, upstream, check_train): the same draws plus one_point and variance_overflow, held to
conditions on the batch statistics; tests/test_gpu_model_draws_train.py compares the device.
"""
import numpy as np

import dgcnn_grad_ref
import dgcnn_ref
import dgcnn_train_ref
import edgeconv_bwd_ref
import edgeconv_pgrad_ref
import edgeconv_ref
import pointnet_ref
import pointnet_train_ref
from pointnet_ref import BN_EPS, F32

TINY = float(np.finfo(np.float32).tiny)   # the smallest normal Float32

# (layers, N, B, K): the smallest shapes at which every path of the EdgeConv kernels is taken
EDGECONV = [([5, 33, 70], 65, 2, 6),       # MFMA and v_fma_f32 tails in both directions, a third tile of one point
            ([3, 32, 64, 64], 65, 2, 3),   # the all-VALU first layer, L = 3
            ([64, 128, 256], 64, 2, 3)]    # stride 258, two slabs per wave
DGCNN = (65, 2, 3, 10)                     # N, B, K, num_classes
POINTNET = (65, 2, 10)                     # N, B, num_classes

FAMILIES = ("subnormal_mid", "subnormal_input", "decades", "decades_small", "decades_edge", "large", "overflow", "negative_gamma",
            "sigma2_edges", "sigma2_zero", "constant_cloud")
NON_FINITE = ("overflow", "sigma2_edges", "sigma2_edges_last")   # the families that are non-finite on purpose
ZEROED = ("subnormal_mid", "subnormal_input", "decades_small", "decades_edge")   # the families with bias = mu = beta = +0
PARAM_SEED = {"edgeconv": 1, "dgcnn": 3, "pointnet": 10}         # the seeds of the existing GPU tests


SEEDS = ("subnormal_mid", "subnormal_input", "decades", "decades_small", "large", "overflow", "negative_gamma", "sigma2_edges",
         "constant_cloud", "sigma2_edges_last", "sigma2_zero", "decades_edge")   # a family's place here seeds its draws
LARGE = {"edgeconv": 1e20, "dgcnn": 1e20, "pointnet": 1e9}


def overflow_scales(net):
    """(the factor on X, the factor on the weights that read X), chosen on the host so that the restatement's output holds +Inf
    and at least 1 % each of NaN and of finite values (the shares: tests/test_model_draws_host.py prints them)."""
    kind, arg = net
    if kind == "edgeconv":
        if len(arg) > 3:
            return 1e30, 7e7   # three layers: an Inf seldom survives two more chains as an Inf, a finite value seldom at all
        return 1e30, (6e7 if 2 * arg[0] >= 128 else 1e8)   # a chain of 128 products overflows sooner than one of 6 or 10
    if kind == "dgcnn":
        return 1e30, 4e7                                   # x1 AND x2 hold all three kinds
    return 3.5e9, 1.0   # PointNet: see the module docstring


def families(kind):
    """The families that apply to a network kind."""
    fams = [f for f in FAMILIES if not (kind == "pointnet" and f == "constant_cloud")]
    return fams + (["sigma2_edges_last"] if kind == "edgeconv" else [])


def base_params(net):
    kind, arg = net
    if kind == "edgeconv":
        return edgeconv_ref.random_params(arg, PARAM_SEED[kind])
    return (dgcnn_ref if kind == "dgcnn" else pointnet_ref).random_params(arg, PARAM_SEED[kind])


def first_weights(net):
    """The weights of the layers that read X itself."""
    return {"edgeconv": ["conv1.weight"], "dgcnn": ["ec1.conv1.weight"],
            "pointnet": ["stn.conv1.weight", "conv_block1.conv.weight"]}[net[0]]


def batchnorms(P):
    return [n[:-len(".gamma")] for n in P if n.endswith(".gamma")]


def last_batchnorm(net):
    assert net[0] == "edgeconv"
    return f"bn{len(net[1]) - 1}"


def in_channels(net):
    return net[1][0] if net[0] == "edgeconv" else 3


def upstream_shape(net, N, B):
    kind, arg = net
    return None if kind == "pointnet" else ((arg[-1], N, B) if kind == "edgeconv" else (arg, B))


def _zero_offsets(net, P):
    keep = ("stn.dense3.bias", "fstn.dense3.bias") if net[0] == "pointnet" else ()
    for n in P:
        if n.rsplit(".", 1)[1] in ("bias", "mu", "beta") and n not in keep:
            P[n] = np.zeros_like(P[n])   # +0 bits


def _scale(P, names, s):
    for n in names:
        P[n] = (P[n].astype(np.float64) * s).astype(F32)


def edge_channels(C):
    """kind -> the channels of a BatchNorm of C channels that sigma2_edges edits."""
    assert C >= 6, C
    return {"zero": (0, C - 3), "inf": (1, C - 2), "nan": (2, C - 1)}


def _edit_sigma2(P, bns, kinds):
    value = {"zero": F32(0.0), "inf": -BN_EPS, "nan": F32(-1.0)}
    edited = {}
    for bn in bns:
        ch = edge_channels(P[bn + ".sigma2"].size)
        for k in kinds:
            P[bn + ".sigma2"][list(ch[k])] = value[k]
        edited[bn] = {k: ch[k] for k in kinds}
    assert (-BN_EPS) + BN_EPS == 0 and np.sqrt(F32(0.0) + BN_EPS) > 0   # sd = 0 exactly; sd = sqrt(eps)
    return edited


def draw(family, net, N, B):
    """One seeded draw of the family for the network: dict(X, P, g, ...)."""
    assert family in families(net[0]), (family, net[0])
    return _draw(family, net, N, B)


def _draw(family, net, N, B):
    kind = net[0]
    rng = np.random.default_rng([SEEDS.index(family), N, B, in_channels(net)])
    F = in_channels(net)
    P = base_params(net)
    X = rng.standard_normal((F, N, B))
    gshape = upstream_shape(net, N, B)
    g = None if gshape is None else rng.standard_normal(gshape)
    d = {}
    if family in ZEROED:
        _zero_offsets(net, P)
    if family == "subnormal_mid":
        X = X * 1e-20
        _scale(P, first_weights(net), 1e-19)
    elif family == "subnormal_input":
        X = X * 1e-39
    elif family == "decades":
        X = X * 10.0 ** rng.integers(-6, 7, X.shape)
        if g is not None:
            g = g * 10.0 ** rng.integers(-6, 7, g.shape)
    elif family in ("decades_small", "decades_edge"):
        lo, hi = (-44, -29) if family == "decades_small" else (-41, -35)
        X = X * 10.0 ** rng.integers(lo, hi, X.shape)
        if g is not None:
            small = g * 10.0 ** rng.integers(lo, hi, g.shape)
            if kind == "edgeconv":
                g[:, 0::2, :] = small[:, 0::2, :]   # the even points
            else:
                g[:, 0::2] = small[:, 0::2]         # the even clouds
    elif family == "large":
        X = X * LARGE[kind]
    elif family == "overflow":
        xs, ws = overflow_scales(net)
        X = X * xs
        _scale(P, first_weights(net), ws)
    elif family == "negative_gamma":
        flipped = {}
        for bn in batchnorms(P):
            C = P[bn + ".gamma"].size
            ch = np.sort(rng.permutation(C)[:C // 2])
            P[bn + ".gamma"][ch] *= F32(-1)
            flipped[bn] = ch
        d["flipped"] = flipped
    elif family == "sigma2_edges":
        d["edited"] = _edit_sigma2(P, batchnorms(P), ("zero", "inf", "nan"))
    elif family == "sigma2_edges_last":
        d["edited"] = _edit_sigma2(P, [last_batchnorm(net)], ("zero", "inf", "nan"))
    elif family == "sigma2_zero":
        d["edited"] = _edit_sigma2(P, batchnorms(P), ("zero",))
    elif family == "constant_cloud":
        X = np.broadcast_to(rng.standard_normal((F, 1, B)), (F, N, B))
    with np.errstate(all="ignore"):
        d.update(X=np.asfortranarray(np.asarray(X).astype(F32)), P=P, g=None if g is None else np.asfortranarray(g.astype(F32)))
    if family == "large" and kind != "pointnet":   # the search's squared distances leave Float32
        x = d["X"]
        with np.errstate(all="ignore"):
            d2 = np.sum(((x[:, :, None, :] - x[:, None, :, :]).astype(F32) ** 2).astype(F32), axis=0, dtype=F32)
        assert 2 * np.count_nonzero(np.isinf(d2)) >= d2.size, "large: fewer than half of the squared distances are +Inf"
    return d


def given_lists(N, B, K, seed=77):
    """Seeded neighbour lists (K, N, B) that no search made: any point of the cloud, repeats and the point itself included."""
    return np.asfortranarray(np.random.default_rng([seed, N, B, K]).integers(0, N, (K, N, B)).astype(np.int32))


# ---- shares and conditions ---------------------------------------------------------------------------------------------------

def shares(a):
    """(subnormal, non-zero, finite, NaN) shares of an array."""
    a = np.asarray(a, F32)
    with np.errstate(all="ignore"):
        mag = np.abs(a)
        return (float(np.mean((mag > 0) & (mag < TINY))), float(np.mean(a != 0)), float(np.mean(np.isfinite(a))),
                float(np.mean(np.isnan(a))))


def describe(what, a):
    s = shares(a)
    line = f"{what}: subnormal {s[0]:.2f}, non-zero {s[1]:.2f}, finite {s[2]:.2f}, NaN {s[3]:.2f} of {np.asarray(a).size}"
    print(line)
    return s


def outputs(net):
    """The arrays the forward conditions speak of: out of an EdgeConv, x1 and x2 of a DGCNN, pooled of a PointNet."""
    return {"edgeconv": ("out",), "dgcnn": ("x1", "x2"), "pointnet": ("pooled",)}[net[0]]


def check_forward(family, net, d, fwd, tag=""):
    """The family's condition on the restatement's own forward (a dict: out / x1, x2, ... / pooled, logits)."""
    kind = net[0]
    if family in ("decades_small", "decades_edge"):   # subnormal and normal terms, a quarter of X each at the least
        sub = shares(d["X"])[0]
        assert 0.25 <= sub <= 0.75, sub
    for k in outputs(net):
        a = np.asarray(fwd[k])
        sub, nz, fin, nan = describe(f"{tag}{family} {kind} {k}", a)
        if family in ("subnormal_mid", "subnormal_input"):
            assert fin == 1 and sub >= 0.25, (family, k, sub)
        elif family == "decades":
            assert fin == 1 and nz >= 0.5, (family, k, nz)
        elif family in ("decades_small", "decades_edge"):   # (the maxima over k and the points pick the largest terms: the output is normal)
            assert fin == 1 and nz >= 0.5, (family, k, nz)
        elif family in ("large", "sigma2_zero", "constant_cloud"):
            assert fin == 1 and nz > 0, (family, k)
        elif family == "overflow":
            inf = float(np.mean(np.isinf(a)))
            print(f"{tag}{family} {kind} {k}: Inf {inf:.3f}")
            assert inf > 0 and nan >= 0.01 and fin >= 0.01, (family, k, inf, nan, fin)
        elif family == "sigma2_edges":
            assert fin < 1, (family, k)
    if family == "negative_gamma":
        if kind == "edgeconv":
            edgeconv_ref.check_draw(fwd["out"])
        elif kind == "dgcnn":
            dgcnn_ref.check_draw(fwd)
        else:   # tests/test_gpu_pointnet.py's condition: finite, the relu before the softmax leaves something
            assert np.all(np.isfinite(fwd["logits"])) and np.count_nonzero(fwd["logits"] > 0) * 8 >= fwd["logits"].size
    if family in ("sigma2_edges", "sigma2_edges_last", "sigma2_zero"):
        for bn, ch in d["edited"].items():
            assert all(len(c) >= 1 for c in ch.values()) and len(ch) == (1 if family == "sigma2_zero" else 3), (bn, ch)
    if family == "sigma2_edges_last":
        out = np.asarray(fwd["out"])
        ch = d["edited"][last_batchnorm(net)]
        rest = np.setdiff1d(np.arange(out.shape[0]), ch["inf"] + ch["nan"])
        assert np.all(np.isnan(out[list(ch["nan"])])), "a sigma2 = -1 channel is not all NaN"
        for c in ch["inf"]:   # +Inf where some k is positive, +0 where none is; 0 / 0 = NaN where z + b == mu
            assert np.isinf(out[c]).any() and not np.any(np.isfinite(out[c]) & (out[c] != 0)), c
        assert np.all(np.isfinite(out[rest])) and 2 * np.count_nonzero(out[rest]) >= out[rest].size
    if family == "constant_cloud" and kind != "pointnet":
        for k in [n for n in ("idx", "idx1", "idx2") if n in fwd]:
            idx = np.asarray(fwd[k])
            K = idx.shape[0]
            # the oracle's order is (distance, index) and every distance is 0: ranks 0 .. K are the points 0 .. K, rank 0 is
            # dropped for every point alike -- one list for the whole cloud
            assert np.array_equal(idx, np.broadcast_to(np.arange(1, K + 1, dtype=np.int32)[:, None, None], idx.shape)), k


def weight_families(net, G):
    """family -> one flat array over all layers."""
    if net[0] == "edgeconv":
        return {f: edgeconv_pgrad_ref.family(G, net[1], f) for f in edgeconv_pgrad_ref.FAMILIES}
    return {f: dgcnn_grad_ref.family(G, f) for f in dgcnn_grad_ref.FAMILIES}


def check_grads(family, net, d, G, gx, tag=""):
    """The family's condition on the restatement's own gradients: G (name -> array) and gx."""
    kind = net[0]
    fam = weight_families(net, G)
    stats = {f: describe(f"{tag}{family} {kind} {f}", a) for f, a in fam.items()}
    sx = describe(f"{tag}{family} {kind} gx", gx)
    if family in ZEROED:
        for n, a in G.items():
            if n.endswith(".weight") or n.endswith(".gamma"):
                describe(f"{tag}{family} {kind} d {n}", a)
    if family not in NON_FINITE:
        assert all(s[2] == 1 for s in stats.values()) and sx[2] == 1, (family, stats, sx)
    if family == "subnormal_mid":   # a quarter of some layer's weight gradient is subnormal
        best = max(shares(a)[0] for n, a in G.items() if n.endswith(".weight"))
        assert best >= 0.25, (family, best)
    elif family in ("decades", "large", "constant_cloud", "sigma2_zero"):
        assert stats["dW"][1] > 0 and sx[1] > 0
    elif family == "negative_gamma":
        if kind == "edgeconv":
            edgeconv_pgrad_ref.check_draw(G, net[1])
            edgeconv_bwd_ref.check_draw(gx)
        else:   # dgcnn_ref.check_draw has held the forward; the gradients are finite (above) and not empty
            assert all(s[1] > 0 for s in stats.values()) and sx[1] > 0
    elif family == "sigma2_edges_last":
        L = len(net[1]) - 1
        ch = d["edited"][f"bn{L}"]
        rest = np.setdiff1d(np.arange(net[1][-1]), ch["inf"] + ch["nan"])
        for n in (f"conv{L}.bias", f"bn{L}.gamma", f"bn{L}.beta"):
            assert np.all(np.isfinite(G[n][rest])), n
        assert np.all(np.isfinite(G[f"conv{L}.weight"][0][:, rest]))
        assert not np.all(np.isfinite(G[f"conv{L}.weight"][0][:, list(ch["nan"])]))


# ---- training mode: batch-statistic BatchNorm --------------------------------------------------------------------------------
# PointNet forward_train / grad_train, EdgeConv and DGCNN forward_train.  Every BatchNorm takes its mean and variance from Float64
# sums over the batch, rounded to Float32 once; the families below put subnormal, +0, +Inf and NaN values into those statistics.
# The draws are draw()'s wherever the family exists there; what is new:
#
# constant_cloud     for PointNet too: one point per cloud and two clouds, so a convolution BatchNorm sees two values.
# one_point          every point of every cloud is one seeded point: every BatchNorm's input is constant, S2 / m - mu64 mu64 is
#                    pure rounding residue -- negative (clamped to +0) or positive (a tiny sigma2 whose bits depend on the order
#                    of the chain).
# variance_overflow  X x 1e25 for PointNet (x 1e20, `large`'s scale, for EdgeConv and DGCNN): the first BatchNorm's Float64 variance
#                    is beyond Float32, sigma2 = +Inf with a finite mu, (v - mu) / Inf = 0 and every later BatchNorm sees beta.
# overflow           PointNet takes overflow_scales_train's factors in training mode (see there).
# The sigma2_* families stay out: in training mode the running statistics of the parameters enter `running` only.
TRAIN_FAMILIES = ("subnormal_mid", "subnormal_input", "decades", "decades_small", "decades_edge", "large", "overflow",
                  "negative_gamma", "constant_cloud", "one_point", "variance_overflow")   # a family's place here seeds a new draw
TRAIN_ONLY = ("one_point", "variance_overflow")    # the families draw() does not have
VARIANCE_OVERFLOW = {"edgeconv": 1e20, "dgcnn": 1e20, "pointnet": 1e25}


def overflow_scales_train(net):
    """overflow_scales for the training-mode networks.  EdgeConv and DGCNN keep the test-mode factors: the first BatchNorm's
    statistics then hold finite, +Inf and NaN values together (DGCNN ec1.bn1: mu 6 % +Inf, sigma2 94 % +Inf and 6 % NaN).
    PointNet at the test-mode 3.5e9 is finite everywhere once every layer is renormalised, so it takes factors of its own,
    chosen on the host (tests/test_model_draws_host.py prints the shares): see POINTNET_OVERFLOW_TRAIN."""
    return POINTNET_OVERFLOW_TRAIN if net[0] == "pointnet" else overflow_scales(net)


# X x 1e30, stn.conv1 and conv_block1.conv x 1e8.  The first BatchNorm, stn.bn1, then holds all three kinds: mu is finite in 50 %
# of its 64 channels and +Inf in 50 % (a channel with one +Inf value after the relu), sigma2 is +Inf in the first half (S2 / m
# beyond Float32 with a finite mean) and NaN in the second (Inf - Inf); every later statistic and every output is NaN.  Measured
# at X x 1e30 with the weights x 1e6, 1e7, 3e7: mu all finite, sigma2 all +Inf, no NaN, outputs finite (variance_overflow's
# picture); x 3e8: 3 % / 97 %; x 1e9: mu all +Inf, sigma2 all NaN.  No pair gives a FINITE sigma2 next to a +Inf one in one
# BatchNorm: that needs values below 1.8e19 and above 3.4e38 in one layer, a spread the weights do not have.
POINTNET_OVERFLOW_TRAIN = (1e30, 1e8)


def train_families(kind):
    """The families that apply to a network kind in training mode."""
    assert kind in PARAM_SEED, kind
    return list(TRAIN_FAMILIES)


def draw_train(family, net, N, B):
    """One seeded draw of a training-mode family: draw()'s own arrays wherever draw() has the family."""
    kind = net[0]
    assert family in train_families(kind), (family, kind)
    if family not in TRAIN_ONLY and not (family == "overflow" and kind == "pointnet"):
        return _draw(family, net, N, B)          # constant_cloud for PointNet: the same code, which draw() only refuses
    F = in_channels(net)
    rng = np.random.default_rng([1000 + TRAIN_FAMILIES.index(family), N, B, F])
    P = base_params(net)
    X = rng.standard_normal((F, N, B))
    gshape = upstream_shape(net, N, B)
    g = None if gshape is None else rng.standard_normal(gshape)
    if family == "one_point":
        X = np.broadcast_to(X[:, :1, :1], (F, N, B))
    elif family == "variance_overflow":
        X = X * VARIANCE_OVERFLOW[kind]
    else:
        xs, ws = overflow_scales_train(net)
        X = X * xs
        _scale(P, first_weights(net), ws)
    with np.errstate(all="ignore"):
        return dict(X=np.asfortranarray(np.asarray(X).astype(F32)), P=P, g=None if g is None else np.asfortranarray(g.astype(F32)))


def upstream(family, net, N, B):
    """glogits (nc, B) for PointNet's adjoints, from a generator of its own (draw() gives PointNet none, and a shape from
    upstream_shape would shift the generator under the existing draws).  DGCNN's rule: unit scale, except under decades (every
    element x 10 ** integers(-6, 7)) and under decades_small / decades_edge (small on the even clouds, unit scale on the odd)."""
    kind, nc = net
    assert kind == "pointnet", kind
    names = FAMILIES + TRAIN_ONLY
    rng = np.random.default_rng([2000 + names.index(family), N, B, nc])
    g = rng.standard_normal((nc, B))
    if family == "decades":
        g = g * 10.0 ** rng.integers(-6, 7, g.shape)
    elif family in ("decades_small", "decades_edge"):
        lo, hi = (-44, -29) if family == "decades_small" else (-41, -35)
        small = g * 10.0 ** rng.integers(lo, hi, g.shape)
        g[:, 0::2] = small[:, 0::2]
    with np.errstate(all="ignore"):
        return np.asfortranarray(g.astype(F32))


def train_batchnorms(net):
    """(every BatchNorm in forward order, those that follow a convolution)."""
    kind, arg = net
    if kind == "edgeconv":
        bns = [f"bn{i}" for i in range(1, len(arg))]
        return bns, bns
    if kind == "dgcnn":
        bns = list(dgcnn_train_ref.BN_ORDER)
        return bns, [b for b in bns if not b.startswith("fc")]
    bns = list(pointnet_train_ref.BN_ORDER)
    return bns, [b for b in bns if b not in pointnet_train_ref.DENSE_BN]


def train_outputs(net):
    """The arrays the training-mode conditions speak of."""
    return {"edgeconv": ("out",), "dgcnn": ("x1", "x2", "pooled", "logits"), "pointnet": ("stn", "fstn", "pooled", "logits")}[net[0]]


def stat_shares(a):
    """(subnormal, +0 or -0, +Inf, NaN) shares of a Float32 statistics array."""
    a = np.asarray(a, F32)
    with np.errstate(all="ignore"):
        mag = np.abs(a)
        return (float(np.mean((mag > 0) & (mag < TINY))), float(np.mean(a == 0)), float(np.mean(a == np.inf)), float(np.mean(np.isnan(a))))


def _plus_zero(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32) == 0


def check_train(family, net, d, fwd, tag=""):
    """The family's condition on the restatement's own training-mode forward (a dict with batch_stats, bn_inputs, raw_var and the
    outputs).  Prints, per BatchNorm, the subnormal / zero / +Inf / NaN shares of mu and sigma2 (and under one_point the negative
    / zero / positive shares of the variance before the clamp).  The floors are the measured values rounded down; the host test
    prints the values themselves."""
    kind = net[0]
    bns, convs = train_batchnorms(net)
    st = fwd["batch_stats"]
    assert [k for k in st] == [f"{bn}.{f}" for bn in bns for f in ("mu", "sigma2")]
    sh = {}
    for bn in bns:
        for f in ("mu", "sigma2"):
            s = sh[f"{bn}.{f}"] = stat_shares(st[f"{bn}.{f}"])
            print(f"{tag}{family} {kind} {bn}.{f}: subnormal {s[0]:.2f}, zero {s[1]:.2f}, +Inf {s[2]:.2f}, NaN {s[3]:.2f} of {st[f'{bn}.{f}'].size}")
    outs = {k: describe(f"{tag}{family} {kind} {k}", fwd[k]) for k in train_outputs(net)}
    every = np.concatenate([np.asarray(v, F32).ravel() for v in st.values()])
    finite_out = all(s[2] == 1 for s in outs.values())
    first, later = bns[0], bns[1:]
    if family == "subnormal_input":
        x0 = fwd["bn_inputs"][first]
        assert sh[first + ".mu"][0] >= 0.5, (first, sh[first + ".mu"])
        assert np.all(_plus_zero(st[first + ".sigma2"])) and np.count_nonzero(x0) > 0, first
        best = max(sh[bn + ".sigma2"][0] for bn in later)
        print(f"{tag}{family} {kind}: the largest subnormal share of a later sigma2 {best:.2f}")
        if kind == "dgcnn":   # measured: fc5.bn.sigma2 0.92
            assert best >= 0.25, best
        else:
            # measured: 0.00 for the three EdgeConv tables and for PointNet, where EVERY sigma2 is +0.  A BatchNorm with
            # sigma2 = +0 multiplies by gamma / sqrt(eps), about 300, and a Float32 variance leaves zero only from values of
            # 1e-23: an EdgeConv of two or three blocks is too shallow, and PointNet multiplies by x, of order 1e-39, again
            # after each transform net.  They are held to that picture instead (PointNet's subnormal statistics are its means:
            # measured 0.124 of all its batch statistics, with stn.bn1, conv_block1.bn and feat.bn2 subnormal in every channel).
            assert all(np.all(_plus_zero(st[bn + ".sigma2"])) for bn in later)
            if kind == "pointnet":
                assert stat_shares(every)[0] >= 0.05 and sh["feat.bn2.mu"][0] >= 0.5, stat_shares(every)
        assert np.all(np.isfinite(every)) and finite_out
    elif family in ("subnormal_mid", "decades_edge"):
        sub = stat_shares(every)[0]
        print(f"{tag}{family} {kind}: subnormal share of all {every.size} batch statistics {sub:.3f}")
        # measured: subnormal_mid 0.057 (DGCNN), 0.11 .. 0.19 (EdgeConv), 0.12 (PointNet); decades_edge 0.124 (DGCNN), 0.12
        # (PointNet), but for EdgeConv 0.063 / 0.073 at [5, 33, 70] (search / given lists), 0.006 / 0.053 at [3, 32, 64, 64] and
        # 0.009 / 0.042 at [64, 128, 256]: one BatchNorm after the small values, and the search picks neighbours whose
        # differences cancel.  An EdgeConv under decades_edge is held to one subnormal statistic at the least.
        assert sub >= 0.05 or (kind == "edgeconv" and family == "decades_edge" and sub > 0), sub
        assert np.all(np.isfinite(every)) and finite_out
    elif family == "variance_overflow" or (family == "large" and kind != "pointnet"):
        assert sh[first + ".sigma2"][2] >= 0.9 and np.all(np.isfinite(st[first + ".mu"])), (first, sh[first + ".sigma2"])
        assert finite_out, outs
        best = max(sh[bn + ".sigma2"][1] for bn in convs if bn != first)
        print(f"{tag}{family} {kind}: the largest share of sigma2 = 0 in a later convolution BatchNorm {best:.2f}")
        assert best > 0.5, best
    elif family == "one_point":
        assert finite_out and np.all(np.isfinite(every)), outs
        moved, neg_any, pos32 = 0, False, False
        for bn in convs:
            raw = fwd["raw_var"][bn]
            neg, zero, pos = float(np.mean(raw < 0)), float(np.mean(raw == 0)), float(np.mean(raw > 0))
            print(f"{tag}{family} {kind} {bn}: variance before the clamp negative {neg:.2f}, zero {zero:.2f}, positive {pos:.2f}; "
                  f"largest magnitude {np.abs(raw).max():.3e}")
            moved += (neg + pos) >= 0.05
            neg_any |= neg > 0
            pos32 |= bool(np.any(st[bn + ".sigma2"] > 0))
            assert np.all(st[bn + ".sigma2"][raw < 0] == 0) and np.all(_plus_zero(st[bn + ".sigma2"][raw < 0]))
        assert moved >= min(3, len(convs)), moved   # (two of the EdgeConv tables have two BatchNorms in all)
        # measured: [64, 128, 256] at N = 64 (full tiles: every chain is 48 equal terms, every fold a power of two of them) has
        # 0.09 / 0.08 negative and NO positive residue in its two BatchNorms, so it is held to a negative one, as PointNet is;
        # the other EdgeConv tables and DGCNN have 0.09 .. 0.33 positive in every EdgeConv BatchNorm.
        full_tiles = kind == "edgeconv" and d["X"].shape[1] % 64 == 0
        assert neg_any if kind == "pointnet" or full_tiles else pos32, (neg_any, pos32)
    elif family == "overflow":
        assert np.any(every == np.inf) and np.any(np.isnan(every)), stat_shares(every)
        both = np.concatenate([st[first + ".mu"], st[first + ".sigma2"]])   # the first BatchNorm holds all three kinds
        assert np.any(np.isfinite(both)) and np.any(both == np.inf) and np.any(np.isnan(both)), (first, stat_shares(both))
        assert all(s[3] == 1 for s in outs.values()), outs
    else:   # decades, decades_small, negative_gamma, constant_cloud, and large for PointNet: finite, and not empty
        assert np.all(np.isfinite(every)) and finite_out and all(s[1] > 0 for s in outs.values()), outs
    if family in ("one_point", "constant_cloud") and kind != "pointnet":
        for k in [n for n in ("idx", "idx1", "idx2") if n in fwd and not fwd.get("given")]:
            idx = np.asarray(fwd[k])
            K = idx.shape[0]   # check_forward's note: every distance is 0, the ranks are the points, rank 0 is dropped
            assert np.array_equal(idx, np.broadcast_to(np.arange(1, K + 1, dtype=np.int32)[:, None, None], idx.shape)), k
    return sh


def restate_forward_train(net, d, K=None, idx=None, dropout=None):
    """The training-mode restatement's forward as a dict of the arrays the device returns, with bn_inputs and raw_var."""
    kind, arg = net
    if kind == "edgeconv":
        r = dgcnn_train_ref.edgeconv_forward_train(d["X"], d["P"], arg, K, idx=idx)
        r["given"] = idx is not None
        return r
    if kind == "dgcnn":
        return dgcnn_train_ref.forward_train(d["X"], d["P"], K, dropout=dropout)
    return pointnet_train_ref.forward_train(d["X"], d["P"], dropout=dropout)


# ---- the restatements, one call per entry point ------------------------------------------------------------------------------

def restate_forward(net, d, K=None, idx=None):
    """The restatement's forward as a dict of the arrays the device returns."""
    kind, arg = net
    if kind == "edgeconv":
        i, out = edgeconv_ref.forward(d["X"], d["P"], arg, K, idx=idx)
        return {"idx": i, "out": out}
    if kind == "dgcnn":
        return dgcnn_ref.forward(d["X"], d["P"], K)
    return pointnet_ref.forward(d["X"], d["P"])


def restate_grads(net, d, K, fwd):
    """(G, gx, extra) from the forward arrays `fwd` (the device's own, or the restatement's)."""
    kind, arg = net
    if kind == "edgeconv":
        G, gx = edgeconv_pgrad_ref.grad(d["X"], d["P"], arg, K, d["g"], fwd["idx"], fwd["out"])
        return {n: G[n] for n in edgeconv_ref.param_shapes(arg)}, gx, {}
    G, gx, gx2, gx1 = dgcnn_grad_ref.grad(d["X"], d["P"], K, d["g"], fwd)
    return G, gx, {"gx2": gx2, "gx1": gx1}
