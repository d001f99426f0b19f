"""Host restatement of the DGCNN training-mode adjoint (include/flux3d_hip.h "DGCNN training-mode adjoint") in numpy: the definition
fx3d_dgcnn_grad_train is held to, bit for bit, every sum in the header's order.

The two EdgeConv stages are tests/edgeconv_grad_train_ref.py's grad, composed as tests/dgcnn_grad_ref.py composes the test-mode
stages: stage 2 on (x1, idx2, x2) with gout = gx2, stage 1 on (X, idx1, x1) with gout = gx1, each at its slice of the statistics.
The tail -- fc_6, fc_5, fc_4, the maximum, conv_3 -- takes its BatchNorm back (bn_back: the Float64 sums, mb, mg, gv), its dense
sums and conv_3's dense adjoint (last_conv with a 256-channel input and no relu mask below the BatchNorm) from
tests/pointnet_grad_train_ref.py.  What is DGCNN's own: every block is dense, BatchNorm, relu, then the dropout multiplier, so on
the way back the multiplier comes first and the relu's mask second; and n* is test mode's winner (tests/dgcnn_grad_ref.py: no
winner where pooled is not positive)."""
import numpy as np

import dgcnn_ref
import edgeconv_grad_train_ref as ect
import pointnet_grad_train_ref as pgt
from dgcnn_grad_ref import FAMILIES, L1, L2, family, flat, stage_params  # noqa: F401
from pointnet_ref import F32, batchnorm, contract, conv, dense, relu

ZERO = F32(0.0)
BN_NAMES = ("ec1.bn1", "ec1.bn2", "ec1.bn3", "ec2.bn1", "ec2.bn2", "conv3.bn", "fc4.bn", "fc5.bn")


def _block_back(G, Q, bn, up, W_next, mask, r, v, B, keep):
    """One head block back: up (B, nout_next) the gradient at the next dense layer's output, W_next (nout_next, n) its weights;
    the chain over that layer's outputs, the multiplier, the relu's own mask, the BatchNorm back.  Returns gv (B, n)."""
    g = contract(up, W_next)
    if mask is not None:
        g = (g * mask).astype(F32)
    gy = np.where(r > 0, g, ZERO).astype(F32)
    return pgt.bn_back(G, Q, bn, gy, v, B, keep=keep)


def tail(P, stats, x2, pooled, glogits, dropout=None, keep=None):
    """(G, gx2, nstar): the gradients of conv3, fc4, fc5 and fc6 (Flux's shapes), gx2 (256, N, B) and n* (B, 1024).  stats: the
    batch statistics name -> (C,) (conv3.bn, fc4.bn and fc5.bn are read); dropout: None or the pair (512, B), (256, B).  keep: a
    dict that receives per BatchNorm its gy, xh, m and Float64 sums (``bn``), the gradient at pooled ``gp`` (B, 1024), and the head's
    relu outputs and dense inputs ``r4``, ``in5``, ``r5``, ``in6``."""
    x2 = np.asarray(x2, F32)
    _, N, B = x2.shape
    Q = ect.at_stats(P, {k: v for k, v in stats.items() if not k.startswith("ec")})
    p = np.ascontiguousarray(np.asarray(pooled, F32).reshape((1024, B), order="F").T)  # (B, 1024)
    d6 = np.ascontiguousarray(np.asarray(glogits, F32).reshape((-1, B), order="F").T)  # (B, nc)
    m4, m5 = (None, None) if dropout is None else (np.ascontiguousarray(np.asarray(m, F32).T) for m in dropout)
    x = np.ascontiguousarray(np.transpose(x2, (2, 1, 0)))  # (B, N, 256)
    G = {}
    with np.errstate(all="ignore"):
        # the forward's head again
        v4 = dense(p, P, "fc4.dense")
        r4 = relu(batchnorm(v4, Q, "fc4.bn"))
        in5 = r4 if m4 is None else (r4 * m4).astype(F32)
        v5 = dense(in5, P, "fc5.dense")
        r5 = relu(batchnorm(v5, Q, "fc5.bn"))
        in6 = r5 if m5 is None else (r5 * m5).astype(F32)
        W6, W5, W4 = (np.asarray(P[n], F32) for n in ("fc6.weight", "fc5.dense.weight", "fc4.dense.weight"))  # (out, in)
        gv5 = _block_back(G, Q, "fc5.bn", d6, W6, m5, r5, v5, B, keep)
        gv4 = _block_back(G, Q, "fc4.bn", gv5, W5, m4, r4, v4, B, keep)
        gp = contract(gv4, W4)
        if keep is not None:
            keep.update(gp=gp, r4=r4, r5=r5, in5=in5, in6=in6)
        pgt._dense_sums(G, (("fc4.dense", gv4, p), ("fc5.dense", gv5, in5), ("fc6", d6, in6)))
        # the maximum and conv_3, dense.  last_conv's winner is the first point that equals pooled; with the relu's zeros taken out
        # of a3 that is test mode's rule: no winner where pooled is not positive
        pre = conv(x, P, "conv3.conv")
        a3 = relu(batchnorm(pre, Q, "conv3.bn"))
        a3 = np.where(a3 > 0, a3, F32(np.nan)).astype(F32)
        g_x2, nstar = pgt.last_conv(G, Q, "conv3.conv", "conv3.bn", x, pre, a3, p, gp, False, keep)
    return G, np.asfortranarray(np.transpose(g_x2, (2, 1, 0))), nstar


def stage_stats(stats, name):
    """The ``ec1.`` / ``ec2.`` statistics with the prefix dropped: the EdgeConv layer's own."""
    return stage_params(stats, name)


def grad_train(X, P, K, glogits, fwd, dropout=None, keep=None):
    """(grads, gx, gx2, gx1) for X (3, N, B), B >= 2.  fwd: a mapping with the training-mode forward's idx1, x1, idx2, x2, pooled
    (the library's layouts) and batch_stats (name -> (C,)); dropout: None or the pair of multipliers.  grads maps every name of
    dgcnn_ref.param_shapes to its gradient in Flux's shape (mu and sigma2: zeros)."""
    X = np.asarray(X, F32)
    assert X.ndim == 3 and X.shape[2] >= 2
    idx1, x1, idx2, x2, pooled = (np.asarray(fwd[k]) for k in ("idx1", "x1", "idx2", "x2", "pooled"))
    stats = {k: np.asarray(v, F32) for k, v in fwd["batch_stats"].items()}
    nc = np.asarray(P["fc6.weight"]).shape[0]
    G, gx2, nstar = tail(P, stats, x2, pooled, glogits, dropout, keep)
    if keep is not None:
        keep["nstar"] = nstar
    G2, gx1 = ect.grad(x1, stage_params(P, "ec2"), L2, K, gx2, stage_stats(stats, "ec2"), idx2, x2)
    G1, gx = ect.grad(X, stage_params(P, "ec1"), L1, K, gx1, stage_stats(stats, "ec1"), idx1, x1)
    G.update({"ec1." + k: v for k, v in G1.items()})
    G.update({"ec2." + k: v for k, v in G2.items()})
    return {n: G[n] for n in dgcnn_ref.param_shapes(nc)}, gx, gx2, gx1


def check_draw(G):
    """A draw is worth comparing: every family finite and at least half of dW non-zero (edgeconv_pgrad_ref.check_draw's rule)."""
    for fam in FAMILIES:
        v = family(G, fam)
        assert np.all(np.isfinite(v)), fam
    w = family(G, "dW")
    assert 2 * np.count_nonzero(w) >= w.size, (np.count_nonzero(w), w.size)
