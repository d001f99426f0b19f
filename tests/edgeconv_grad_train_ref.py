"""Host restatement of the EdgeConv training-mode adjoint (include/flux3d_hip.h "EdgeConv training-mode adjoint") in numpy: the
definition fx3d_edgeconv_grad_train is held to, bit for bit, sums in the header's order.

The forward quantities are tests/edgeconv_ref.py's at the batch statistics: v_l = conv_l(a_{l-1}), xh_l = (v_l - mu_l) / sd_l,
a_l = relu((gamma_l xh_l) + beta_l), which is relu(batchnorm(v_l)) bit for bit.  Per layer, from L down:

  the Float64 sums of gy and gy xh in the header's order (half_sums: per half-tile of 32 points two chains by bit 2 of the
    point's position, over k and the chain's 16 rows ascending, chain(0) + chain(1), then dgcnn_train_ref.fold_tiles over
    t = half-tile + nhalf b): dbeta, dgamma, mb, mg;
  gv = (((gy - mb) - (xh mg)) gamma) / sd for every row of the clouds;
  dW and db: gv contracted with a_{l-1} and summed in the orders tests/edgeconv_pgrad_ref.py gives H and h (chunk_rows, the two h
    chains, the chain over (b, chunk));
  d_{l-1} = the fmaf chain of gv with W, gy_{l-1} = a_{l-1} > 0 ? d_{l-1} : +0."""
import numpy as np

import edgeconv_ref
from dgcnn_ref import F32, conv, edge_rows, relu
from dgcnn_train_ref import fold_tiles
from edgeconv_pgrad_ref import CHUNK, FAMILIES, _add_chain, check_draw, chunk_rows, family, flat  # noqa: F401
from pointnet_ref import BN_EPS, contract

F64 = np.float64
HALF = 32


def at_stats(P, stats):
    """P with every BatchNorm's mu / sigma2 replaced by the batch statistics (name -> (C,))."""
    Q = dict(P)
    for k, v in stats.items():
        assert k in Q and k.rsplit(".", 1)[1] in ("mu", "sigma2"), k
        Q[k] = np.asarray(v, F32)
    return Q


def half_rows(N, K, t):
    """The (k, n) of the rows of the two chains of half-tile t, in the order they are added: chain h holds the points whose
    position p in the half-tile has bit 2 equal to h, over k ascending and within a k over ascending p; points beyond the
    cloud's last one left out."""
    chains = []
    for h in (0, 1):
        ks, ns = [], []
        for k in range(K):
            for p in range(HALF):
                if ((p >> 2) & 1) == h and HALF * t + p < N:
                    ks.append(k)
                    ns.append(HALF * t + p)
        chains.append((np.array(ks, int), np.array(ns, int)))
    return chains


def half_sums(gy, xh):
    """gy, xh (B, K, N, C) Float32 -> (S1, S2) (C,) Float64: the sums of gy and of gy xh in the header's order.  Rows that take no
    part must hold gy = +0 and xh = +0 (adding +0.0 changes no bit of a chain that began at +0.0)."""
    B, K, N, C = gy.shape
    nh = (N + HALF - 1) // HALF
    with np.errstate(all="ignore"):
        g = np.zeros((B, K, nh * HALF, C), F64)
        x = np.zeros((B, K, nh * HALF, C), F64)
        g[:, :, :N], x[:, :, :N] = gy, xh
        g = g.reshape(B, K, nh, 4, 2, 4, C)  # row p = 8 q + 4 h + i of its half-tile: axes (q, h, i)
        x = x.reshape(B, K, nh, 4, 2, 4, C)
        s1, s2 = np.zeros((B, nh, 2, C), F64), np.zeros((B, nh, 2, C), F64)  # chains h
        for k in range(K):
            for q in range(4):
                for i in range(4):  # ascending p within the chain
                    s1 = s1 + g[:, k, :, q, :, i, :]
                    s2 = s2 + g[:, k, :, q, :, i, :] * x[:, k, :, q, :, i, :]  # exact product
        return fold_tiles(s1[:, :, 0] + s1[:, :, 1]), fold_tiles(s2[:, :, 0] + s2[:, :, 1])


def grad(X, P, layers, K, gout, stats, idx=None, out=None, keep=None):
    """X (F, N, B) or (F, N); P: name -> array in Flux's shapes (its mu / sigma2 are not read); stats: name -> (C,), the batch
    statistics under the ``bnK.mu`` / ``.sigma2`` names; gout (cL, N, B); idx (K, N, B) 0-based and out (cL, N, B): the training
    forward's, computed here (edgeconv_ref.forward at the statistics) when not given.  Returns (grads, gx) as
    edgeconv_pgrad_ref.grad does.  keep: a dict that receives ``gv`` and ``xh``, lists of (B, K, N, C_l) for l = 1 .. L."""
    X = np.asarray(X, F32)
    if X.ndim == 2:
        X = X[:, :, None]
    F, N, B = X.shape
    L = len(layers) - 1
    Q = at_stats(P, stats)
    if idx is None or out is None:
        found, made = edgeconv_ref.forward(X, Q, layers, K, idx=idx)
        idx = found if idx is None else idx
        out = made if out is None else out
    idx = np.asarray(idx).reshape((K, N, B), order="F")
    out = np.asarray(out, F32).reshape((layers[-1], N, B), order="F")
    gout = np.asarray(gout, F32).reshape((layers[-1], N, B), order="F")
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, F)
    zero = F32(0.0)
    m = F64(K * N * B)
    G = {}
    with np.errstate(all="ignore"):
        a = [np.stack([edge_rows(x[b], idx[:, :, b]) for b in range(B)])]  # a_0 (B, K, N, 2F)
        xh = [None]
        for i in range(1, L + 1):
            mu, var = Q[f"bn{i}.mu"], Q[f"bn{i}.sigma2"]
            g, be = np.asarray(P[f"bn{i}.gamma"], F32), np.asarray(P[f"bn{i}.beta"], F32)
            sd = np.sqrt(var + BN_EPS).astype(F32)
            xh.append(((conv(a[-1], P, f"conv{i}") - mu).astype(F32) / sd).astype(F32))
            a.append(relu(((g * xh[-1]).astype(F32) + be).astype(F32)))
        o, gu = np.transpose(out, (2, 1, 0))[:, None], np.transpose(gout, (2, 1, 0))[:, None]  # (B, 1, N, cL)
        hit = (a[L] == o) & (o > 0)
        first = hit & (np.cumsum(hit, axis=1) == 1)
        gy = np.where(first, gu, zero).astype(F32)
        part = first  # the rows whose xh enters the sums
        for i in range(L, 0, -1):
            gamma, var = np.asarray(P[f"bn{i}.gamma"], F32), Q[f"bn{i}.sigma2"]
            sd = np.sqrt(var + BN_EPS).astype(F32)
            s1, s2 = half_sums(gy, xh[i] if part is None else np.where(part, xh[i], zero).astype(F32))
            G[f"bn{i}.beta"], G[f"bn{i}.gamma"] = s1.astype(F32), s2.astype(F32)
            G[f"bn{i}.mu"], G[f"bn{i}.sigma2"] = np.zeros(layers[i], F32), np.zeros(layers[i], F32)
            mb, mg = (s1 / m).astype(F32), (s2 / m).astype(F32)
            t = (gy - mb).astype(F32)
            t = (t - (xh[i] * mg).astype(F32)).astype(F32)
            gv = ((t * gamma).astype(F32) / sd).astype(F32)
            if keep is not None:
                keep.setdefault("gv", [None] * L)[i - 1] = gv
                keep.setdefault("xh", [None] * L)[i - 1] = xh[i]
            H, h = None, None
            for b in range(B):
                for c0 in range(0, N, CHUNK):
                    ks, ns, half = chunk_rows(N, K, c0)
                    A, D = a[i - 1][b][ks, ns], gv[b][ks, ns]  # (P, cin), (P, cout)
                    Hc = contract(np.ascontiguousarray(A.T), D)  # the chain over the rows, from +0
                    hc = (_add_chain(D[half == 0]) + _add_chain(D[half == 1])).astype(F32)
                    if H is None:  # the chain over the chunks begins at +0
                        H, h = np.zeros_like(Hc), np.zeros_like(hc)
                    H, h = (H + Hc).astype(F32), (h + hc).astype(F32)
            G[f"conv{i}.weight"], G[f"conv{i}.bias"] = H[None], h
            d = contract(gv, np.asarray(P[f"conv{i}.weight"], F32)[0].T)  # the chain over ALL o ascending: Wt (cout, cin)
            if i > 1:
                gy = np.where(a[i - 1] > 0, d, zero).astype(F32)
                part = None
        S = np.zeros((B, N, 2 * F), F32)
        for k in range(K):
            S = (S + d[:, k]).astype(F32)
        gx = (S[:, :, :F] - S[:, :, F:]).astype(F32)
    G = {n: G[n] for n in edgeconv_ref.param_shapes(layers)}
    return G, np.asfortranarray(np.transpose(gx, (2, 1, 0)))
