"""The draw families of tests/model_draws.py, the part that needs no GPU: every family meets its condition on the host
restatements for every layer table and network that tests/test_gpu_model_draws.py runs (the shares -- subnormal, non-zero,
finite, NaN -- are printed); under negative gamma and under sigma2 = 0 the three adjoint restatements are still the gradient
(torch float64 autograd, the siblings' bound: at most 8 x torch-float32's error); and pointnet_ref.fma32 agrees bit for bit with
the compiled fmaf chain on subnormal and many-decade operands, where the module's own self-check draws exponents in [-3, 3].
The training-mode families (model_draws.train_families) meet check_train on the training-mode restatements: the shares of
subnormal, zero, +Inf and NaN batch statistics per BatchNorm are printed, and the variance before the clamp under one_point."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dgcnn_grad_ref as gref
import dgcnn_ref
import edgeconv_bwd_ref as bref
import edgeconv_pgrad_ref as pref
import edgeconv_ref as ref
import model_draws as md
import pointnet_grad_train_ref
import pointnet_ref
from pointnet_ref import F32

HERE = os.path.dirname(os.path.abspath(__file__))
NETS = [(("edgeconv", layers), N, B, K) for layers, N, B, K in md.EDGECONV]
NETS += [(("dgcnn", md.DGCNN[3]),) + md.DGCNN[:3], (("pointnet", md.POINTNET[2]), md.POINTNET[0], md.POINTNET[1], None)]
PAIRS = [(net, N, B, K, f) for net, N, B, K in NETS for f in md.families(net[0])]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _id(v):
    return str(v).replace(" ", "").replace("'", "")


@pytest.mark.parametrize("net,N,B,K,family", PAIRS, ids=_id)
def test_the_family_meets_its_condition(net, N, B, K, family):
    """The restatement's own forward and gradients, with its own search and (EdgeConv) with given lists."""
    d = md.draw(family, net, N, B)
    again = md.draw(family, net, N, B)
    assert np.array_equal(_bits(d["X"]), _bits(again["X"])) and all(np.array_equal(_bits(d["P"][n]), _bits(again["P"][n])) for n in d["P"])
    if family in md.ZEROED:
        assert all(not _bits(v).any() for n, v in d["P"].items() if n.rsplit(".", 1)[1] in ("mu", "beta"))
    fwd = md.restate_forward(net, d, K)
    md.check_forward(family, net, d, fwd)
    if net[0] == "pointnet":
        return
    G, gx, extra = md.restate_grads(net, d, K, fwd)
    md.check_grads(family, net, d, G, gx)
    if net[0] == "edgeconv":
        assert np.array_equal(_bits(gx), _bits(bref.input_grad(d["X"], d["P"], net[1], K, d["g"], fwd["idx"], fwd["out"]))) or family in md.NON_FINITE
        if family != "constant_cloud":   # (its condition is on the search's lists)
            given = md.restate_forward(net, d, K, idx=md.given_lists(N, B, K))
            md.check_forward(family, net, d, given, tag="given lists: ")
            md.check_grads(family, net, d, *md.restate_grads(net, d, K, given)[:2], tag="given lists: ")


TRAIN_PAIRS = [(net, N, B, K, f) for net, N, B, K in NETS for f in md.train_families(net[0])]


@pytest.mark.parametrize("net,N,B,K,family", TRAIN_PAIRS, ids=_id)
def test_the_train_family_meets_its_condition(net, N, B, K, family):
    """The training-mode restatement's own batch statistics and outputs (check_train prints the shares per BatchNorm), with its
    own search and (EdgeConv) with given lists; for PointNet the training-mode adjoint's restatement as well, finite outside
    overflow.  A family that draw() has is draw()'s arrays, bit for bit."""
    kind = net[0]
    d = md.draw_train(family, net, N, B)
    if family in md.families(kind) and not (family == "overflow" and kind == "pointnet"):
        same = md.draw(family, net, N, B)
        assert np.array_equal(_bits(d["X"]), _bits(same["X"])) and all(np.array_equal(_bits(d["P"][n]), _bits(same["P"][n])) for n in d["P"])
        assert (d["g"] is None and same["g"] is None) or np.array_equal(_bits(d["g"]), _bits(same["g"]))
    again = md.draw_train(family, net, N, B)
    assert np.array_equal(_bits(d["X"]), _bits(again["X"])) and all(np.array_equal(_bits(d["P"][n]), _bits(again["P"][n])) for n in d["P"])
    if family == "one_point":
        assert all(np.array_equal(_bits(d["X"][:, n, b]), _bits(d["X"][:, 0, 0])) for n in range(N) for b in range(B))
    if family == "constant_cloud":
        assert all(np.array_equal(_bits(d["X"][:, n, :]), _bits(d["X"][:, 0, :])) for n in range(N))
        assert not np.array_equal(_bits(d["X"][:, 0, 0]), _bits(d["X"][:, 0, 1]))   # two values per BatchNorm channel
    fwd = md.restate_forward_train(net, d, K)
    md.check_train(family, net, d, fwd)
    if kind == "edgeconv":
        given = md.restate_forward_train(net, d, K, idx=md.given_lists(N, B, K))
        md.check_train(family, net, d, given, tag="given lists: ")
    if kind != "pointnet":
        return
    glogits = md.upstream(family, net, N, B)
    assert glogits.shape == (net[1], B) and np.array_equal(_bits(glogits), _bits(md.upstream(family, net, N, B)))
    G, gx, mid = pointnet_grad_train_ref.grad_train(d["X"], d["P"], glogits)
    fam = {f: pointnet_grad_train_ref.family(G, f) for f in pointnet_grad_train_ref.FAMILIES}
    stats = {f: md.describe(f"{family} pointnet grad_train {f}", a) for f, a in fam.items()}
    sx = md.describe(f"{family} pointnet grad_train gx", gx)
    for k, v in mid.items():
        md.describe(f"{family} pointnet grad_train {k}", v)
    if family == "overflow":
        assert sx[3] > 0 and all(s[3] > 0 for s in stats.values()), (sx, stats)
        return
    assert sx[2] == 1 and all(s[2] == 1 for s in stats.values()) and all(np.all(np.isfinite(v)) for v in mid.values()), (sx, stats)
    if family == "variance_overflow":   # sd = +Inf in stn.bn1 and conv_block1.bn: nothing reaches X, the later layers still learn
        assert not gx.any() and stats["dW"][1] > 0.25, (sx, stats)
    else:
        assert stats["dW"][1] > 0, stats


@pytest.mark.parametrize("family", md.families("pointnet") + list(md.TRAIN_ONLY))
def test_the_pointnet_upstream_gradient(family):
    """upstream(): seeded, Float32, finite and non-zero; over many decades under decades, small (subnormal values among them) on
    the even clouds alone under decades_small and decades_edge, unit scale elsewhere."""
    N, B, nc = md.POINTNET
    g = md.upstream(family, ("pointnet", nc), N, B)
    assert g.shape == (nc, B) and g.dtype == F32 and np.all(np.isfinite(g)) and np.isfortran(g)
    assert np.array_equal(_bits(g), _bits(md.upstream(family, ("pointnet", nc), N, B)))
    mag = np.abs(g.astype(np.float64))
    if family == "decades":
        assert mag.max() / mag[mag > 0].min() > 1e6
    elif family in ("decades_small", "decades_edge"):
        assert mag[:, 0::2].max() < 1e-28 and mag[:, 1::2].max() > 0.1 and np.count_nonzero(g[:, 0::2]) > 0
    else:
        assert 0.1 < mag.max() < 10 and np.count_nonzero(g) == g.size
    other = [f for f in md.families("pointnet") if f != family][0]
    assert not np.array_equal(_bits(g), _bits(md.upstream(other, ("pointnet", nc), N, B)))


def test_constant_cloud_gives_everything_to_the_first_k_and_point_0():
    """The restatement on a constant cloud: every edge row of a point is the same, so the first k takes every last-layer gradient of
    both stages; every point's x2 row is the same, so point 0 wins every live channel of conv_3 and gx2 is +0 bits elsewhere."""
    N, B, K, nc = md.DGCNN
    net = ("dgcnn", nc)
    d = md.draw("constant_cloud", net, N, B)
    fwd = dgcnn_ref.forward(d["X"], d["P"], K)
    md.check_forward("constant_cloud", net, d, fwd)
    for k in ("x1", "x2"):
        assert all(np.array_equal(_bits(fwd[k][:, n]), _bits(fwd[k][:, 0])) for n in range(N)), k
    G, gx, gx2, gx1 = gref.grad(d["X"], d["P"], K, d["g"], fwd)
    nstar = gref.winners(gref.conv3(d["P"], fwd["x2"]), fwd["pooled"])
    assert set(np.unique(nstar).tolist()) <= {-1, 0} and np.count_nonzero(nstar == 0) > 512
    assert not _bits(gx2[:, 1:, :]).any() and all(np.count_nonzero(gx2[:, 0, b]) > 0 for b in range(B))
    # the first k: dbeta of a stage's last layer is the sum over the points of gout on the live channels, not K times it
    for stage, L, g, out in (("ec2", 2, gx2, fwd["x2"]), ("ec1", 3, gx1, fwd["x1"])):
        live = out[:, 0, :] > 0   # (C, B)
        want = np.where(live, g.astype(np.float64).sum(axis=1), 0.0).sum(axis=1)
        got = G[f"{stage}.bn{L}.beta"].astype(np.float64)
        assert np.allclose(got, want, rtol=1e-4, atol=1e-6 * np.abs(want).max()), stage
        assert np.count_nonzero(want) > 0


def _ratio(what, mine, t64, t32, failed):
    mine, t64, t32 = (np.asarray(v, np.float64).ravel() for v in (mine, t64, t32))
    assert mine.shape == t64.shape and np.all(np.isfinite(mine)) and np.all(np.isfinite(t64))
    scale = float(np.max(np.abs(t64)))
    err_ref, err_t32 = float(np.max(np.abs(mine - t64))) / scale, float(np.max(np.abs(t32 - t64))) / scale
    print(f"{what}: {mine.size} elements, non-zero share {np.count_nonzero(mine) / mine.size:.2f}; relative error of the restatement "
          f"{err_ref:.3e}, of torch float32 {err_t32:.3e}, ratio {err_ref / err_t32:.2f}")
    if not (err_t32 > 0 and err_ref <= 8 * err_t32):
        failed.append((what, err_ref, err_t32))


def _torch(tmp_path, script, case):
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    np.savez(src, **case)
    subprocess.run([sys.executable, os.path.join(HERE, script), src, dst], check=True, timeout=600)
    return np.load(dst)


def _channels(d, bn):
    """The channels of a BatchNorm the comparison is restricted to: the sigma2 = 0 ones, or all of them."""
    return list(d["edited"][bn]["zero"]) if "edited" in d else slice(None)


@pytest.mark.parametrize("family", ["negative_gamma", "sigma2_zero"])
def test_the_edgeconv_restatements_are_the_gradient(tmp_path, family):
    """edgeconv_bwd_ref and edgeconv_pgrad_ref at [5, 33, 70], N = 65, B = 2, K = 6 against torch float64 autograd through the
    existing scripts, the siblings' bound unchanged; under sigma2 = 0 the four families are restricted to those channels."""
    layers, N, B, K = md.EDGECONV[0]
    net = ("edgeconv", layers)
    d = md.draw(family, net, N, B)
    X, P, gout = d["X"], d["P"], d["g"]
    idx, out = ref.forward(X, P, layers, K)
    md.check_forward(family, net, d, {"idx": idx, "out": out})
    G, gx = pref.grad(X, P, layers, K, gout, idx, out)
    mine = bref.input_grad(X, P, layers, K, gout, idx, out)
    assert np.array_equal(_bits(gx), _bits(mine))
    md.check_grads(family, net, d, {n: G[n] for n in ref.param_shapes(layers)}, gx)
    case = {"X": X, "gout": gout, "nstages": np.array(1), "s0.layers": np.array(layers), "s0.idx": idx}
    case.update({f"s0.{k}": v for k, v in P.items()})
    failed = []
    t = _torch(tmp_path, "edgeconv_bwd_torch_eval.py", case)
    _ratio(f"{family} edgeconv_bwd_ref gx", mine, t["g64"], t["g32"], failed)
    t = _torch(tmp_path, "edgeconv_pgrad_torch_eval.py", case)
    for fam, pattern in pref.FAMILIES.items():
        def gather(get):
            return np.concatenate([np.asarray(get(pattern.format(i)))[..., _channels(d, f"bn{i}")].ravel() for i in range(1, len(layers))])
        _ratio(f"{family} edgeconv_pgrad_ref {fam}", gather(lambda n: G[n]), gather(lambda n: t["g64.s0." + n]),
               gather(lambda n: t["g32.s0." + n]), failed)
    assert not failed, failed


@pytest.mark.parametrize("family", ["negative_gamma", "sigma2_zero"])
def test_the_dgcnn_restatement_is_the_gradient(tmp_path, family):
    """dgcnn_grad_ref at N = 65, B = 2, K = 3, 10 classes against torch float64 autograd of the whole network."""
    N, B, K, nc = md.DGCNN
    net = ("dgcnn", nc)
    d = md.draw(family, net, N, B)
    fwd = dgcnn_ref.forward(d["X"], d["P"], K)
    md.check_forward(family, net, d, fwd)
    G, gx, _, _ = gref.grad(d["X"], d["P"], K, d["g"], fwd)
    md.check_grads(family, net, d, G, gx)
    t = _torch(tmp_path, "dgcnn_grad_torch_eval.py", dict(X=d["X"], glogits=d["g"], idx1=fwd["idx1"], idx2=fwd["idx2"], **d["P"]))
    failed = []
    for fam, suffix in gref.FAMILIES.items():
        names = [n for n in G if n.endswith(suffix) and not ("edited" in d and n.startswith("fc6."))]   # fc_6 has no BatchNorm

        def gather(get):
            return np.concatenate([np.asarray(get(n))[_sel(d, n)].ravel() for n in names])
        _ratio(f"{family} dgcnn_grad_ref {fam}", gather(lambda n: G[n]), gather(lambda n: t["g64." + n]), gather(lambda n: t["g32." + n]),
               failed)
    _ratio(f"{family} dgcnn_grad_ref X", gx, t["g64.X"], t["g32.X"], failed)
    assert not failed, failed


def _bn_of(name):
    """The BatchNorm that follows the layer a DGCNN parameter belongs to."""
    layer = name.rsplit(".", 1)[0]                      # ec1.conv2 / ec1.bn2 / conv3.conv / conv3.bn / fc4.dense / fc4.bn
    if layer.startswith("ec"):
        return layer.replace(".conv", ".bn")
    return layer.rsplit(".", 1)[0] + ".bn"


def _sel(d, name):
    """The index of the compared elements of a DGCNN gradient: under sigma2 = 0, the output channels so edited."""
    if "edited" not in d:
        return (Ellipsis,)
    ch = list(d["edited"][_bn_of(name)]["zero"])
    if name.endswith(".dense.weight"):   # Flux's (out, in)
        return (ch,)
    return (Ellipsis, ch)


@pytest.mark.parametrize("family", ["subnormal_mid", "decades", "decades_small", "decades_edge"])
def test_fma32_is_the_compiled_chain_on_these_operands(family):
    """pointnet_ref.contract (libm's fmaf, compiled) and contract_numpy (fma32: the Float64 product, one round-to-odd addition,
    one rounding) on the family's own operands: the edge rows against conv1's weights, then the first layer's output against
    conv2's -- subnormal products, subnormal sums and sums that cross the normal boundary."""
    layers, N, B, K = md.EDGECONV[0]
    d = md.draw(family, ("edgeconv", layers), N, B)
    x = np.ascontiguousarray(np.transpose(d["X"], (2, 1, 0)))
    idx = md.given_lists(N, B, K)
    a0 = dgcnn_ref.edge_rows(x[0], idx[:, :, 0])
    W1, W2 = d["P"]["conv1.weight"][0], d["P"]["conv2.weight"][0]
    z1 = pointnet_ref.contract(a0, W1)
    assert np.array_equal(_bits(z1), _bits(pointnet_ref.contract_numpy(a0, W1)))
    a1 = dgcnn_ref.relu(dgcnn_ref.batchnorm(dgcnn_ref.conv(a0, d["P"], "conv1"), d["P"], "bn1"))
    z2 = pointnet_ref.contract(a1, W2)
    assert np.array_equal(_bits(z2), _bits(pointnet_ref.contract_numpy(a1, W2)))
    s1, s2 = md.describe(f"{family} z1", z1), md.describe(f"{family} z2", z2)
    assert s1[2] == 1 and s2[2] == 1 and s1[1] > 0.5
    if family == "subnormal_mid":
        assert s1[0] >= 0.25 and s2[0] >= 0.25
