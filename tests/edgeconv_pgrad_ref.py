"""Host restatement of the EdgeConv parameter adjoint (include/flux3d_hip.h "EdgeConv parameter adjoint") in numpy: the
definition fx3d_edgeconv_grad is held to, bit for bit, sums in the header's order.

Built on the forward's and the input adjoint's pieces (tests/edgeconv_ref.py, tests/edgeconv_bwd_ref.py): a_0 .. a_L and d_L ..
d_1 are formed exactly as edgeconv_bwd_ref.input_grad forms them, so gx is that function's result.  H_l and h_l are then summed
chunk by chunk (128 points of one cloud), inside a chunk as one fmaf chain over tiles, k and the tile's points in the header's
permutation, and over the chunks as one chain of additions, b ascending, chunk ascending."""
import numpy as np

import edgeconv_ref
from dgcnn_ref import F32, batchnorm, conv, edge_rows, relu
from pointnet_ref import BN_EPS, contract, fma32

CHUNK = 128   # FX3D_EDGECONV_GRAD_CHUNK
TILE = 32
# pair r = 0 .. 15 is (q, q + 4), q = (r mod 4) + 8 (r div 4)
FIRST = np.array([(r & 3) + 8 * (r >> 2) for r in range(16)])
PERM = np.stack([FIRST, FIRST + 4], axis=1).ravel()


def chunk_rows(N, K, c0):
    """The (k, n) of the edge rows of the chunk that begins at point c0, in the order of the H chain; and the same split into the
    two h chains (first and second points of the pairs)."""
    ks, ns, half = [], [], []
    for t0 in range(c0, min(c0 + CHUNK, N), TILE):
        for k in range(K):
            for i, q in enumerate(PERM):
                if t0 + q < N:
                    ks.append(k)
                    ns.append(t0 + q)
                    half.append(i & 1)
    return np.array(ks), np.array(ns), np.array(half)


def _add_chain(rows):
    """Float32 additions from +0 over the rows of a (P, C) array, in order."""
    acc = np.zeros(rows.shape[1:], F32)
    for v in rows:
        acc = (acc + v).astype(F32)
    return acc


def sums(X, P, layers, K, gout, idx=None, out=None):
    """H (a list of (cin_l, cout_l)), h (a list of (cout_l,)) and gx (F, N, B), each in the header's order."""
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
    H = [None] * L
    h = [None] * L
    with np.errstate(all="ignore"):
        for b in range(B):
            a = [edge_rows(x[b], idx[:, :, b])]  # a_0 (K, N, 2F)
            for i in range(1, L + 1):
                a.append(relu(batchnorm(conv(a[-1], P, f"conv{i}"), P, f"bn{i}")))
            o, g = out[:, :, b].T, gout[:, :, b].T  # (N, cL)
            hit = (a[L] == o[None]) & (o[None] > 0)
            first = hit & (np.cumsum(hit, axis=0) == 1)
            d = np.where(first, g[None], zero).astype(F32)
            ds = [None] * (L + 1)  # d_1 .. d_L (K, N, cout_l)
            for i in range(L, 0, -1):
                if i < L:
                    d = np.where(a[i] > 0, d, zero).astype(F32)
                ds[i] = d
                gamma, var = np.asarray(P[f"bn{i}.gamma"], F32), np.asarray(P[f"bn{i}.sigma2"], F32)
                dz = ((d * gamma).astype(F32) / np.sqrt(var + BN_EPS).astype(F32)).astype(F32)
                d = contract(dz, np.asarray(P[f"conv{i}.weight"], F32)[0].T)
            S = np.zeros((N, 2 * F), F32)
            for k in range(K):
                S = (S + d[k]).astype(F32)
            gx[b] = (S[:, :F] - S[:, F:]).astype(F32)
            for c0 in range(0, N, CHUNK):
                ks, ns, half = chunk_rows(N, K, c0)
                for i in range(1, L + 1):
                    A, D = a[i - 1][ks, ns], ds[i][ks, ns]  # (P, cin), (P, cout)
                    Hc = contract(np.ascontiguousarray(A.T), D)  # the chain over the rows, from +0
                    hc = (_add_chain(D[half == 0]) + _add_chain(D[half == 1])).astype(F32)
                    if H[i - 1] is None:  # the chain over the chunks begins at +0
                        H[i - 1], h[i - 1] = np.zeros_like(Hc), np.zeros_like(hc)
                    H[i - 1] = (H[i - 1] + Hc).astype(F32)
                    h[i - 1] = (h[i - 1] + hc).astype(F32)
    return H, h, np.asfortranarray(np.transpose(gx, (2, 1, 0)))


def grad(X, P, layers, K, gout, idx=None, out=None):
    """(grads, gx): grads maps every name of edgeconv_ref.param_shapes(layers) to its gradient in Flux's shape (mu and sigma2:
    zeros); gx as edgeconv_bwd_ref.input_grad returns it."""
    H, h, gx = sums(X, P, layers, K, gout, idx, out)
    G = {}
    with np.errstate(all="ignore"):
        for i in range(1, len(layers)):
            Hl, hl = H[i - 1], h[i - 1]
            W = np.asarray(P[f"conv{i}.weight"], F32)[0]  # (cin, cout)
            bias, gamma = np.asarray(P[f"conv{i}.bias"], F32), np.asarray(P[f"bn{i}.gamma"], F32)
            mu, var = np.asarray(P[f"bn{i}.mu"], F32), np.asarray(P[f"bn{i}.sigma2"], F32)
            sd = np.sqrt(var + BN_EPS).astype(F32)
            G[f"conv{i}.weight"] = ((Hl * gamma).astype(F32) / sd).astype(F32)[None]
            G[f"conv{i}.bias"] = ((hl * gamma).astype(F32) / sd).astype(F32)
            acc = np.zeros_like(hl)
            for c in range(W.shape[0]):
                acc = fma32(W[c], Hl[c], acc)
            G[f"bn{i}.gamma"] = ((acc + ((bias - mu).astype(F32) * hl).astype(F32)).astype(F32) / sd).astype(F32)
            G[f"bn{i}.beta"] = hl.copy()
            G[f"bn{i}.mu"], G[f"bn{i}.sigma2"] = np.zeros_like(hl), np.zeros_like(hl)
    return G, gx


FAMILIES = {"dW": "conv{}.weight", "db": "conv{}.bias", "dgamma": "bn{}.gamma", "dbeta": "bn{}.beta"}


def family(G, layers, fam):
    """One of the four families of every layer as one flat array."""
    return np.concatenate([np.asarray(G[FAMILIES[fam].format(i)]).ravel() for i in range(1, len(layers))])


def flat(G, layers):
    """The gradients in the parameter buffer's layout (forward order; W column-major (cin, cout))."""
    parts = []
    for i in range(1, len(layers)):
        parts.append(np.asarray(G[f"conv{i}.weight"], F32)[0].ravel(order="F"))
        for n in (f"conv{i}.bias", f"bn{i}.gamma", f"bn{i}.beta", f"bn{i}.mu", f"bn{i}.sigma2"):
            parts.append(np.asarray(G[n], F32).ravel())
    return np.concatenate(parts)


def check_draw(G, layers):
    """The condition a draw must meet for a comparison to mean something, on the restatement's own gradients: every family is
    finite and at least half of dW is non-zero."""
    for fam in FAMILIES:
        assert np.all(np.isfinite(family(G, layers, fam))), f"the restatement's {fam} is not finite"
    dW = family(G, layers, "dW")
    nz = np.count_nonzero(dW)
    assert 2 * nz >= dW.size, f"only {nz} of {dW.size} elements of dW are non-zero"
