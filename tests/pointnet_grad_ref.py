"""Host restatement of the PointNet adjoint (include/flux3d_hip.h "PointNet adjoint") in numpy: the definition
fx3d_pointnet_grad is held to, bit for bit, every sum in the header's order.

The forward is tests/pointnet_ref.py's; the relus' outputs that it does not keep are computed again with its functions (the same
bits).  Chains are pointnet_ref.fma32 / contract (the compiled fmaf chain), sums are Float32 additions from +0, rows of a tile
ascending, tiles of TILE = 64 points, then clouds ascending and tiles ascending."""
import numpy as np

import pointnet_ref as ref
from pointnet_ref import BN_EPS, F32, batchnorm, contract, conv, dense, fma32, relu

TILE = 64   # FX3D_POINTNET_GRAD_TILE
FAMILIES = {"dW": ".weight", "db": ".bias", "dgamma": ".gamma", "dbeta": ".beta"}
ZERO = F32(0.0)


def _bn(P, name):
    g, mu = (np.asarray(P[f"{name}.{f}"], F32) for f in ("gamma", "mu"))
    return g, mu, np.sqrt(np.asarray(P[name + ".sigma2"], F32) + BN_EPS).astype(F32)


def _scaled(d, g, sd):
    """(d gamma) / sd, each operation rounded to Float32."""
    return ((d * g).astype(F32) / sd).astype(F32)


def _add_chain(rows):
    acc = np.zeros(rows.shape[1:], F32)
    for v in rows:
        acc = (acc + v).astype(F32)
    return acc


def _fma_chain(a, b):
    """The chain over the first axis of fma32(a[k], b[k], acc) from +0."""
    acc = np.zeros(a.shape[1:], F32)
    for u, v in zip(a, b):
        acc = fma32(u, v, acc)
    return acc


def _zeros_bn(G, bn, n):
    G[bn + ".mu"], G[bn + ".sigma2"] = np.zeros(n, F32), np.zeros(n, F32)


def _tiles(N):
    return [slice(t, min(t + TILE, N)) for t in range(0, N, TILE)]


def _over_tiles(parts):
    """One sum of Float32 additions from +0 over the tile values, in the order given (b ascending, tiles ascending)."""
    return _add_chain(np.stack(parts))


def relu_bn_back(gy, r, P, bn, mask=True):
    """(d, xh) of a (relu, BatchNorm) layer: d = r > 0 ? (gy gamma) / sd : +0 (no mask: feat.conv2), xh = (r - mu) / sd."""
    g, mu, sd = _bn(P, bn)
    xh = ((r - mu).astype(F32) / sd).astype(F32)
    d = _scaled(gy, g, sd)
    if mask:
        d = np.where(r > 0, d, ZERO).astype(F32)
    return d, xh


def conv_sums(G, name, bn, a_in, gy, r, P):
    """The four families of a conv (relu, BatchNorm) layer below a round's last, per tile one chain over the points, then the
    sum over (b, tile); returns d (B, N, cout)."""
    B, N, cout = gy.shape
    d, xh = relu_bn_back(gy, r, P, bn)
    H, hb, hg, hbe = [], [], [], []
    for b in range(B):
        for t in _tiles(N):
            H.append(contract(np.ascontiguousarray(a_in[b, t].T), d[b, t]))
            hb.append(_add_chain(d[b, t]))
            hg.append(_fma_chain(gy[b, t], xh[b, t]))
            hbe.append(_add_chain(gy[b, t]))
    G[name + ".weight"] = _over_tiles(H)[None]
    G[name + ".bias"], G[bn + ".gamma"], G[bn + ".beta"] = _over_tiles(hb), _over_tiles(hg), _over_tiles(hbe)
    _zeros_bn(G, bn, cout)
    return d


def winners(a3, pooled):
    """n* (B, 1024): the smallest n with a3[b, n, c] == pooled[b, c], -1 where no point equals it (a NaN maximum)."""
    with np.errstate(invalid="ignore"):
        hit = a3 == pooled[:, None, :]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


def last_conv(G, name, bn, a_in, pre, a3, pooled, gp, P, mask):
    """The round's last convolution and the maximum over the points.  a_in (B, N, 128): its input; pre: what its BatchNorm was
    given; a3: the BatchNorm's output; gp (B, 1024): the gradient at pooled.  Fills G, returns (the gradient at a_in, n*)."""
    B, N, _ = a_in.shape
    W = np.asarray(P[name + ".weight"], F32)[0]  # (128, 1024)
    nstar = winners(a3, pooled)
    won = nstar >= 0
    bi = np.arange(B)[:, None]
    pw = pre[bi, np.maximum(nstar, 0), np.arange(1024)[None, :]]
    gy = np.where(won, gp, ZERO).astype(F32)
    d, xh = relu_bn_back(gy, pw, P, bn, mask)
    d, xh = np.where(won, d, ZERO).astype(F32), np.where(won, xh, ZERO).astype(F32)
    g_in = np.zeros((B, N, 128), F32)
    for b in range(B):
        for c in np.flatnonzero(won[b]):  # ascending
            n = nstar[b, c]
            g_in[b, n] = fma32(d[b, c], W[:, c], g_in[b, n])
    H, sb, sg, sbe = np.zeros((128, 1024), F32), np.zeros(1024, F32), np.zeros(1024, F32), np.zeros(1024, F32)
    for b in range(B):
        w = np.flatnonzero(won[b])
        H[:, w] = fma32(a_in[b, nstar[b, w], :].T, d[b, w][None, :], H[:, w])
        sb[w] = (sb[w] + d[b, w]).astype(F32)
        sbe[w] = (sbe[w] + gy[b, w]).astype(F32)
        sg[w] = fma32(gy[b, w], xh[b, w], sg[w])
    G[name + ".weight"], G[name + ".bias"], G[bn + ".gamma"], G[bn + ".beta"] = H[None], sb, sg, sbe
    _zeros_bn(G, bn, 1024)
    return g_in, nstar


def head(G, P, pooled, names, up, feat):
    """The dense layers above a maximum, forward again and back.  names = (d1, bn1 or None, d2, bn2, d3); up (B, n3): glogits
    (feat) or the gradient at d3's output.  Fills G, returns gp (B, 1024)."""
    d1, bn1, d2, bn2, d3 = names
    with np.errstate(all="ignore"):
        r1 = relu(dense(pooled, P, d1))
        a1 = batchnorm(r1, P, bn1) if feat else r1
        r2 = relu(dense(a1, P, d2))
        a2 = batchnorm(r2, P, bn2)
        if feat:
            dd3 = np.where(relu(dense(a2, P, d3)) > 0, up, ZERO).astype(F32)
        else:
            dd3 = np.asarray(up, F32)
        W1, W2, W3 = (np.asarray(P[n + ".weight"], F32) for n in (d1, d2, d3))  # (out, in)
        g2 = contract(dd3, W3)
        dd2, xh2 = relu_bn_back(g2, r2, P, bn2)
        g1 = contract(dd2, W2)
        if feat:
            dd1, xh1 = relu_bn_back(g1, r1, P, bn1)
        else:
            dd1 = np.where(r1 > 0, g1, ZERO).astype(F32)
        gp = contract(dd1, W1)
        for name, dd, a in ((d1, dd1, pooled), (d2, dd2, a1), (d3, dd3, a2)):
            G[name + ".weight"] = _fma_chain(dd[:, :, None], a[:, None, :])  # (out, in), the chain over b
            G[name + ".bias"] = _add_chain(dd)
        for bn, g, xh in ((bn1, g1, xh1 if feat else None), (bn2, g2, xh2)):
            if bn is not None and xh is not None:
                G[bn + ".gamma"], G[bn + ".beta"] = _fma_chain(g, xh), _add_chain(g)
                _zeros_bn(G, bn, g.shape[1])
    return gp


def stn_back(G, P, name, x_in, stage, gmat, K):
    """One transform net back: x_in (B, N, K) its input, stage = pointnet_ref.stn_stage's dict, gmat (K, K, B) the gradient at its
    matrix.  Fills G, returns (the gradient at x_in, n*)."""
    B = x_in.shape[0]
    up = np.ascontiguousarray(np.transpose(gmat, (2, 0, 1))).reshape(B, K * K)  # d3[K i + j] = T[i, j]
    gp = head(G, P, stage["max"], (f"{name}.dense1", None, f"{name}.dense2", f"{name}.bn4", f"{name}.dense3"), up, False)
    g2, nstar = last_conv(G, f"{name}.conv3", f"{name}.bn3", stage["a2"], stage["relu3"], stage["a3"], stage["max"], gp, P, True)
    with np.errstate(all="ignore"):
        r2 = relu(conv(stage["a1"], P, f"{name}.conv2"))
        r1 = relu(conv(x_in, P, f"{name}.conv1"))
        d2 = conv_sums(G, f"{name}.conv2", f"{name}.bn2", stage["a1"], g2, r2, P)
        g1 = contract(d2, np.ascontiguousarray(np.asarray(P[f"{name}.conv2.weight"], F32)[0].T))
        d1 = conv_sums(G, f"{name}.conv1", f"{name}.bn1", x_in, g1, r1, P)
        return contract(d1, np.ascontiguousarray(np.asarray(P[f"{name}.conv1.weight"], F32)[0].T)), nstar


def _gmat(x_in, g_out):
    """gM[i, j, b] = per tile the chain over n of fma32(x_in[b, n, i], g_out[b, n, j]), then the sum over the cloud's tiles."""
    B, N, K = x_in.shape
    out = np.zeros((K, K, B), F32)
    for b in range(B):
        out[:, :, b] = _over_tiles([contract(np.ascontiguousarray(x_in[b, t].T), g_out[b, t]) for t in _tiles(N)])
    return out


def _through(g, M):
    """The path into a transform's input: out[b, n, i] = the chain over j of fma32(g[b, n, j], M[i, j, b])."""
    return np.stack([contract(g[b], np.ascontiguousarray(M[:, :, b].T)) for b in range(g.shape[0])])


def grad(X, P, glogits, keep=None):
    """(grads, gx, mid) for X (3, N, B) or (3, N) and glogits (num_classes, B): grads maps every name of
    pointnet_ref.param_shapes to its gradient in Flux's shape (mu and sigma2: zeros), gx is (3, N, B), mid the dict of gstn
    (3, 3, B), gfstn (64, 64, B), gh (64, N, B) and gxt (3, N, B).  keep: a dict that receives the three rounds' n* (B, 1024)
    and the forward."""
    X = np.asarray(X, F32)
    if X.ndim == 2:
        X = X[:, :, None]
    B = X.shape[2]
    nc = np.asarray(P["cls.weight"]).shape[0]
    r = ref.forward(X, P)
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, 3)
    up = np.ascontiguousarray(np.asarray(glogits, F32).reshape((nc, B), order="F").T)
    G = {}
    with np.errstate(all="ignore"):
        # feat and cls
        pooled = np.ascontiguousarray(r["pooled"].T)
        gp = head(G, P, pooled, ("feat.dense1", "feat.bn3", "feat.dense2", "feat.bn4", "cls"), up, True)
        pre = conv(r["feat_a1"], P, "feat.conv2")
        g_a1, n_feat = last_conv(G, "feat.conv2", "feat.bn2", r["feat_a1"], pre, r["feat_a2"], pooled, gp, P, False)
        d1 = conv_sums(G, "feat.conv1", "feat.bn1", r["h_t"], g_a1, r["feat_relu1"], P)
        g_ht = contract(d1, np.ascontiguousarray(np.asarray(P["feat.conv1.weight"], F32)[0].T))
        gF = _gmat(r["h"], g_ht)
        ghf = _through(g_ht, r["fstn"])
        # fstn, conv_block1, the input transform
        g_fstn, n_fstn = stn_back(G, P, "fstn", r["h"], r["fstn_stage"], gF, 64)
        gh = (ghf + g_fstn).astype(F32)
        d0 = np.where(r["h"] > 0, gh, ZERO).astype(F32)
        N = x.shape[1]
        H0 = _over_tiles([contract(np.ascontiguousarray(r["x_t"][b, t].T), d0[b, t]) for b in range(B) for t in _tiles(N)])
        h0 = _over_tiles([_add_chain(d0[b, t]) for b in range(B) for t in _tiles(N)])
        g, mu, sd = _bn(P, "conv_block1.bn")
        W0, b0 = np.asarray(P["conv_block1.conv.weight"], F32)[0], np.asarray(P["conv_block1.conv.bias"], F32)
        G["conv_block1.conv.weight"] = _scaled(H0, g, sd)[None]
        G["conv_block1.conv.bias"] = _scaled(h0, g, sd)
        G["conv_block1.bn.gamma"] = ((_fma_chain(W0, H0) + ((b0 - mu).astype(F32) * h0).astype(F32)).astype(F32) / sd).astype(F32)
        G["conv_block1.bn.beta"] = h0.copy()
        _zeros_bn(G, "conv_block1.bn", 64)
        gxt = contract(_scaled(d0, g, sd), np.ascontiguousarray(W0.T))
        gT = _gmat(x, gxt)
        # stn, and the two paths into x
        g_stn, n_stn = stn_back(G, P, "stn", x, r["stn_stage"], gT, 3)
        gx = (_through(gxt, r["stn"]) + g_stn).astype(F32)
    if keep is not None:
        keep.update(nstar={"stn": n_stn, "fstn": n_fstn, "feat": n_feat}, forward=r)
    lay = lambda a: np.asfortranarray(np.transpose(a, (2, 1, 0)))  # (B, N, C) -> (C, N, B)
    mid = {"gstn": np.asfortranarray(gT), "gfstn": np.asfortranarray(gF), "gh": lay(gh), "gxt": lay(gxt)}
    return {n: G[n] for n in ref.param_shapes(nc)}, lay(gx), mid


def family(G, fam):
    """One of the four families over all parameterised layers as one flat array."""
    return np.concatenate([np.asarray(v).ravel() for n, v in G.items() if n.endswith(FAMILIES[fam])])


def flat(G):
    """The gradients in the parameter buffer's layout: every array column-major, in forward order."""
    return np.concatenate([np.asarray(v, F32).ravel(order="F") for v in G.values()])
