"""Host restatement of the EdgeConv input adjoint (include/flux3d_hip.h "EdgeConv input adjoint") in numpy: the definition
fx3d_edgeconv_bwd is held to, bit for bit.  BatchNorm in test mode, the neighbours constants (CreateSingleKNNGraph is @nograd,
src/models/dgcnn.jl:9): gradient reaches X only through the repeated x_n of cat(X, KNNGraph - X).

Written from the forward restatement's pieces -- edge_rows, conv, batchnorm, relu, the fmaf chain ``contract`` of
tests/pointnet_ref.py -- so that a_0 .. a_L are exactly what tests/edgeconv_ref.py computes."""
import numpy as np

import edgeconv_ref
from dgcnn_ref import F32, batchnorm, conv, edge_rows, relu
from pointnet_ref import BN_EPS, contract


def input_grad(X, P, layers, K, gout, idx=None, out=None):
    """X (F, N, B) or (F, N); gout (cL, N, B); idx (K, N, B) 0-based and out (cL, N, B): the forward's, computed here when not
    given.  Returns gx (F, N, B) laid out as the library returns it."""
    X = np.asarray(X, F32)
    if X.ndim == 2:
        X = X[:, :, None]
    F, N, B = X.shape
    L = len(layers) - 1
    if idx is None or out is None:
        found, made = edgeconv_ref.forward(X, P, layers, K, idx=idx)
        idx = found if idx is None else idx
        out = made if out is None else out
    idx = np.asarray(idx).reshape((K, N, B), order="F")
    out = np.asarray(out, F32).reshape((layers[-1], N, B), order="F")
    gout = np.asarray(gout, F32).reshape((layers[-1], N, B), order="F")
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, F)
    gx = np.empty((B, N, F), F32)
    zero = F32(0.0)
    with np.errstate(all="ignore"):
        for b in range(B):
            a = [edge_rows(x[b], idx[:, :, b])]  # a_0 (K, N, 2F)
            for i in range(1, L + 1):
                a.append(relu(batchnorm(conv(a[-1], P, f"conv{i}"), P, f"bn{i}")))
            o, g = out[:, :, b].T, gout[:, :, b].T  # (N, cL)
            # the maximum over k: the first k that equals a positive maximum takes the gradient
            hit = (a[L] == o[None]) & (o[None] > 0)
            first = hit & (np.cumsum(hit, axis=0) == 1)
            d = np.where(first, g[None], zero).astype(F32)
            for i in range(L, 0, -1):
                if i < L:
                    d = np.where(a[i] > 0, d, zero).astype(F32)
                gamma, var = np.asarray(P[f"bn{i}.gamma"], F32), np.asarray(P[f"bn{i}.sigma2"], F32)
                dz = ((d * gamma).astype(F32) / np.sqrt(var + BN_EPS).astype(F32)).astype(F32)
                d = contract(dz, np.asarray(P[f"conv{i}.weight"], F32)[0].T)  # the chain over ALL o ascending: Wt (cout, cin)
            S = np.zeros((N, 2 * F), F32)
            for k in range(K):
                S = (S + d[k]).astype(F32)
            gx[b] = (S[:, :F] - S[:, F:]).astype(F32)
    return np.asfortranarray(np.transpose(gx, (2, 1, 0)))


def check_draw(gx):
    """The condition a draw must meet for a comparison to mean something, asserted on the restatement's own gradient: it is
    finite and at least half of it is non-zero."""
    assert np.all(np.isfinite(gx)), "the restatement's gradient is not finite"
    nz = np.count_nonzero(gx)
    assert 2 * nz >= gx.size, f"only {nz} of {gx.size} elements are non-zero"
