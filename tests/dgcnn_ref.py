"""Host restatement of DGCNN inference (include/flux3d_hip.h "DGCNN inference"; src/models/dgcnn.jl:3-7,32-71,99-147,
src/models/utils.jl:1-7) in numpy: the definition the device kernels are held to, bit for bit, up to the logits.

The arithmetic is tests/pointnet_ref.py's (the fma32 chain, Float32 BatchNorm, Julia's max); the neighbours are the CPU
oracle's (oracle/oracle.py: knn, the (distance, index) order of the reference's sorted KD-tree query).  An EdgeConv is written
as what it computes -- per point the maximum over its K edge rows -- and tests/test_dgcnn_host.py checks, on random data and
bit for bit, that the reference's cat / reshape / MaxPool / reshape / permute chain is that."""
import os
import sys

import numpy as np

from pointnet_ref import F32, batchnorm, contract, conv, dense, jmax, relu, softmax32, softmax64  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.oracle import knn  # noqa: E402

EC1 = ("ec1", 3)   # (name, number of conv_bn_blocks): EdgeConv([3, 32, 64, 64], K)
EC2 = ("ec2", 2)   # EdgeConv([64, 128, 256], K)


def self_knn(x, K):
    """x (B, N, F) -> idx (K, N, B) int32, 0-based: knn(KDTree(X), X[:, i], K + 1, true)[1][2:K+1] for every point
    (CreateSingleKNNGraph, src/models/dgcnn.jl:3-7)."""
    return knn(np.asfortranarray(np.transpose(x, (2, 1, 0))), K, drop_first=True, want_dist=False)


def edge_rows(xb, idxb):
    """xb (N, F), idxb (K, N) -> (K, N, 2F): row (k, n) = [x_n, x_idx(k,n) - x_n], the difference one Float32 subtraction."""
    with np.errstate(all="ignore"):
        centre = np.broadcast_to(xb[None, :, :], (idxb.shape[0],) + xb.shape)
        return np.concatenate([centre, (xb[idxb] - centre).astype(F32)], axis=2).astype(F32)


def edgeconv(x, P, spec, K, keep=None):
    """(m::EdgeConv)(X): x (B, N, F) -> (idx (K, N, B), y (B, N, C)).  keep: a dict that receives the last layer before the
    maximum, (B, K, N, C), under spec's name."""
    name, nlayers = spec
    idx = self_knn(x, K)
    out, last = [], []
    for b in range(x.shape[0]):
        a = edge_rows(x[b], idx[:, :, b])
        for i in range(1, nlayers + 1):
            a = relu(batchnorm(conv(a, P, f"{name}.conv{i}"), P, f"{name}.bn{i}"))  # conv_bn_block: Conv, BatchNorm, relu
        last.append(a)
        out.append(jmax(a, axis=0))
    if keep is not None:
        keep[name] = np.stack(last)
    return idx, np.stack(out)


def forward(X, P, K):
    """X (3, N, B) or (3, N), P: name -> array in Flux's shapes.  A dict: ``idx1``, ``idx2`` (K, N, B), ``x1`` (64, N, B),
    ``x2`` (256, N, B), ``pooled`` (1024, B), ``logits`` (num_classes, B) and ``probs`` laid out as the library returns them;
    ``ec1`` / ``ec2`` (B, K, N, C): the EdgeConvs' last layers before the maximum over k; ``conv3`` (B, N, 1024)."""
    X = np.asarray(X, F32)
    if X.ndim == 2:
        X = X[:, :, None]
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, 3)
    r = {}
    r["idx1"], x1 = edgeconv(x, P, EC1, K, r)
    r["idx2"], x2 = edgeconv(x1, P, EC2, K, r)
    r["conv3"] = relu(batchnorm(conv(x2, P, "conv3.conv"), P, "conv3.bn"))
    pooled = jmax(r["conv3"], axis=1)  # (B, 1024): MaxPool((npoints,)) with N == npoints
    d4 = relu(batchnorm(dense(pooled, P, "fc4.dense"), P, "fc4.bn"))  # fc_bn_block: Dense, BatchNorm, relu
    d5 = relu(batchnorm(dense(d4, P, "fc5.dense"), P, "fc5.bn"))
    logits = dense(d5, P, "fc6")  # no activation before the softmax
    r["x1"] = np.asfortranarray(np.transpose(x1, (2, 1, 0)))
    r["x2"] = np.asfortranarray(np.transpose(x2, (2, 1, 0)))
    r["pooled"] = np.asfortranarray(pooled.T)
    r["logits"] = np.asfortranarray(logits.T)
    r["probs"] = softmax32(r["logits"])
    return r


def param_shapes(num_classes):
    """name -> shape in Flux's shapes, in forward order, derived here from the layer table (not from the package)."""
    layers = [("ec1.conv1", (6, 32)), ("ec1.bn1", 32), ("ec1.conv2", (32, 64)), ("ec1.bn2", 64), ("ec1.conv3", (64, 64)),
              ("ec1.bn3", 64), ("ec2.conv1", (128, 128)), ("ec2.bn1", 128), ("ec2.conv2", (128, 256)), ("ec2.bn2", 256),
              ("conv3.conv", (256, 1024)), ("conv3.bn", 1024), ("fc4.dense", [1024, 512]), ("fc4.bn", 512),
              ("fc5.dense", [512, 256]), ("fc5.bn", 256), ("fc6", [256, num_classes])]
    shapes = {}
    for name, ch in layers:
        if isinstance(ch, tuple):    # conv Cin => Cout
            shapes[name + ".weight"], shapes[name + ".bias"] = (1, ch[0], ch[1]), (ch[1],)
        elif isinstance(ch, list):   # dense in => out
            shapes[name + ".weight"], shapes[name + ".bias"] = (ch[1], ch[0]), (ch[1],)
        else:
            for f in ("gamma", "beta", "mu", "sigma2"):
                shapes[f"{name}.{f}"] = (ch,)
    return shapes


# He-scaled layers keep the activations of order one from layer to layer; the maxima over K neighbours and over N points pick
# the upper tail, so without a factor the three dense layers would spread a cloud's logits up to ten units apart and push
# probabilities towards 1e-4 at 40 classes.  The factor is on the last layer alone: everything up to `pooled` keeps its He
# scale.  BatchNorm's beta is centred at BETA_MEAN instead of zero: with K = 1 there is no maximum to lift an EdgeConv's
# output, and a relu of a centred value leaves just about half of x1 and x2 alive -- the first condition of check_draw, missed
# or met by chance.
WEIGHT_SCALE = {"fc6.weight": 0.15}
BETA_MEAN = 0.2


def random_params(num_classes, seed):
    """Random weights AND random running statistics (mu = 0, sigma2 = 1 would hide BatchNorm): He-scaled weights (times
    WEIGHT_SCALE), small biases, gamma in [0.5, 1.5], mu of order 0.1, beta of order 0.1 about BETA_MEAN, sigma2 in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    P = {}
    for name, shape in param_shapes(num_classes).items():
        field = name.rsplit(".", 1)[1]
        if field == "weight":
            fan_in = shape[1]
            P[name] = (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in) * WEIGHT_SCALE.get(name, 1.0)).astype(F32)
        elif field == "gamma":
            P[name] = rng.uniform(0.5, 1.5, shape).astype(F32)
        elif field == "sigma2":
            P[name] = rng.uniform(0.5, 2.0, shape).astype(F32)
        else:
            P[name] = ((BETA_MEAN if field == "beta" else 0.0) + 0.1 * rng.standard_normal(shape)).astype(F32)
    return P


def check_draw(r):
    """The two conditions a draw of random_params must meet for a comparison to mean something, asserted on the
    restatement's own arrays: the relu has not killed the EdgeConvs (at least half of x1 and of x2 is non-zero), and every
    probability is a normal number in [1e-4, 1 - 1e-4] (more than one class)."""
    for k in ("x1", "x2"):
        nz = np.count_nonzero(r[k])
        assert 2 * nz >= r[k].size, f"{k}: only {nz} of {r[k].size} elements are non-zero"
    if r["logits"].shape[0] > 1 and not np.isnan(r["logits"]).any():
        p = softmax64(r["logits"])
        assert p.min() >= 1e-4 and p.max() <= 1 - 1e-4, (p.min(), p.max())
