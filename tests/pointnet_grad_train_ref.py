"""Host restatement of the PointNet training-mode adjoint (include/flux3d_hip.h "PointNet training-mode adjoint") in numpy: the
definition fx3d_pointnet_grad_train is held to, bit for bit, every sum in the header's order.

The forward is tests/pointnet_train_ref.py's (its ``bn_inputs`` are what every BatchNorm was given); the chains and the Float32
tile sums are tests/pointnet_grad_ref.py's.  What is new: per BatchNorm the Float64 sums dbeta64 = sum gy and dgamma64 = sum gy xh
(a convolution's BatchNorm in the forward's order of S1 / S2, a dense one over b, a round's last one over the clouds that have a
winner), the gradient at the BatchNorm's input  gv = (((gy - mb) - xh mg) gamma) / sd  with mb = Float32(dbeta64 / m) and
mg = Float32(dgamma64 / m), the dropout multiplier on the way back, and the rounds' last convolutions as dense sums: per cloud one
chain over its points, then the clouds in ascending b."""
import numpy as np

import pointnet_grad_ref as gref
import pointnet_ref as ref
import pointnet_train_ref as tref
from pointnet_grad_ref import ZERO, _add_chain, _bn, _fma_chain, _gmat, _over_tiles, _through, _tiles, _zeros_bn, winners
from pointnet_ref import F32, contract, dense, relu

F64 = np.float64
TILE, GROUPS = tref.TILE, tref.GROUPS


def point_fold(d):
    """d (B, N, C) Float64 -> (C,): the forward's order of a convolution BatchNorm's sums (pointnet_train_ref.point_sums): per
    tile of 64 two chains (bit 2 of the row), their sum, then GROUPS interleaved chains over t = tile + ntiles b, added ascending."""
    B, N, C = d.shape
    nt = (N + TILE - 1) // TILE
    with np.errstate(all="ignore"):
        pad = np.zeros((B, nt * TILE, C), F64)
        pad[:, :N] = d
        pad = pad.reshape(B, nt, 8, 2, 4, C)
        s = np.zeros((B, nt, 2, C), F64)
        for q in range(8):
            for i in range(4):
                s = s + pad[:, :, q, :, i, :]
        t = (s[:, :, 0] + s[:, :, 1]).reshape(B * nt, C)
        rows = (B * nt + GROUPS - 1) // GROUPS
        f = np.zeros((rows * GROUPS, C), F64)
        f[:B * nt] = t
        f = f.reshape(rows, GROUPS, C)
        chains = np.zeros((GROUPS, C), F64)
        for k in range(rows):
            chains = chains + f[k]
        out = np.zeros(C, F64)
        for g in range(GROUPS):
            out = out + chains[g]
    return out


def cloud_fold(d, take=None):
    """d (B, C) Float64 -> (C,): one chain over b ascending; take (B, C) bool: over the clouds where it holds."""
    out = np.zeros(d.shape[1], F64)
    with np.errstate(all="ignore"):
        for b in range(d.shape[0]):
            out = np.where(True if take is None else take[b], out + d[b], out)
    return out


def bn_sums(gy, xh, take=None):
    """(dbeta64, dgamma64) of a BatchNorm from gy and xh, (B, N, C) after a convolution, (B, C) otherwise."""
    with np.errstate(all="ignore"):
        g64 = gy.astype(F64)
        prod = g64 * xh.astype(F64)  # exact
    if gy.ndim == 3:
        return point_fold(g64), point_fold(prod)
    return cloud_fold(g64, take), cloud_fold(prod, take)


def bn_back(G, Q, bn, gy, v, m, sums=None, keep=None):
    """A BatchNorm back: fills dgamma, dbeta (and the +0 of mu / sigma2) of `bn` in G and returns gv, the gradient at what it was
    given (v).  Q: the parameters at the batch statistics; m: values per channel; sums: (dbeta64, dgamma64) where they are not
    bn_sums(gy, xh) (a round's last BatchNorm)."""
    g, mu, sd = _bn(Q, bn)
    with np.errstate(all="ignore"):
        xh = ((v - mu).astype(F32) / sd).astype(F32)
        s1, s2 = bn_sums(gy, xh) if sums is None else sums
        G[bn + ".beta"], G[bn + ".gamma"] = s1.astype(F32), s2.astype(F32)
        _zeros_bn(G, bn, g.shape[0])
        mb, mg = (s1 / F64(m)).astype(F32), (s2 / F64(m)).astype(F32)
        t = (gy - mb).astype(F32)
        t = (t - (xh * mg).astype(F32)).astype(F32)
        gv = ((t * g).astype(F32) / sd).astype(F32)
    if keep is not None:
        keep.setdefault("bn", {})[bn] = dict(gy=gy, xh=xh, m=m, dbeta64=s1, dgamma64=s2)
    return gv


def _masked(r, g):
    return np.where(r > 0, g, ZERO).astype(F32)


def conv_back(G, Q, name, bn, a_in, gy, r, keep):
    """A conv (relu, BatchNorm) layer below a round's last: the BatchNorm back, d = r > 0 ? gv : +0, dW and db per tile one chain
    over the points, then the sum over (b, tile).  Returns d (B, N, cout)."""
    B, N, _ = gy.shape
    d = _masked(r, bn_back(G, Q, bn, gy, r, B * N, keep=keep))
    conv_param_sums(G, name, a_in, d)
    return d


def conv_param_sums(G, name, a_in, d):
    B, N, _ = d.shape
    H = [contract(np.ascontiguousarray(a_in[b, t].T), d[b, t]) for b in range(B) for t in _tiles(N)]
    hb = [_add_chain(d[b, t]) for b in range(B) for t in _tiles(N)]
    G[name + ".weight"], G[name + ".bias"] = _over_tiles(H)[None], _over_tiles(hb)


def last_conv(G, Q, name, bn, a_in, pre, a3, pooled, gp, mask, keep):
    """A round's last convolution and the maximum over the points, dense: a_in (B, N, 128) its input, pre what its BatchNorm was
    given, a3 the BatchNorm's output, gp (B, 1024) the gradient at pooled.  Returns (the gradient at a_in, n*)."""
    B, N, _ = a_in.shape
    W = np.asarray(Q[name + ".weight"], F32)[0]  # (128, 1024)
    g, mu, sd = _bn(Q, bn)
    nstar = winners(a3, pooled)
    won = nstar >= 0
    bi, ci = np.arange(B)[:, None], np.arange(1024)[None, :]
    with np.errstate(all="ignore"):
        pw = pre[bi, np.maximum(nstar, 0), ci]
        gyw = np.where(won, gp, ZERO).astype(F32)
        xhw = np.where(won, ((pw - mu).astype(F32) / sd).astype(F32), ZERO).astype(F32)
        sums = bn_sums(gyw, xhw, won)
        gy = np.zeros((B, N, 1024), F32)
        for b in range(B):
            c = np.flatnonzero(won[b])
            gy[b, nstar[b, c], c] = gp[b, c]
        d = bn_back(G, Q, bn, gy, pre, B * N, sums=sums, keep=keep)
        if mask:
            d = _masked(pre, d)
        g_in = contract(d, np.ascontiguousarray(W.T))
        # per cloud one chain over its points, then the clouds in ascending b
        G[name + ".weight"] = _add_chain(np.stack([contract(np.ascontiguousarray(a_in[b].T), d[b]) for b in range(B)]))[None]
        G[name + ".bias"] = _add_chain(np.stack([_add_chain(d[b]) for b in range(B)]))
    return g_in, nstar


def _dense_sums(G, layers):
    for name, dd, a in layers:
        G[name + ".weight"] = _fma_chain(dd[:, :, None], a[:, None, :])  # (out, in), the chain over b
        G[name + ".bias"] = _add_chain(dd)


def _weights(Q, *names):
    return (np.asarray(Q[n + ".weight"], F32) for n in names)


def stn_head(G, Q, name, stage, bnin, up, keep):
    """A transform net's dense layers back: up (B, K K) the gradient at dense3's output.  Returns gp (B, 1024)."""
    B = up.shape[0]
    r1, r2, a2 = stage["d1"], bnin[f"{name}.bn4"], stage["d2"]
    W1, W2, W3 = _weights(Q, f"{name}.dense1", f"{name}.dense2", f"{name}.dense3")
    with np.errstate(all="ignore"):
        dd3 = np.asarray(up, F32)
        dd2 = _masked(r2, bn_back(G, Q, f"{name}.bn4", contract(dd3, W3), r2, B, keep=keep))
        dd1 = _masked(r1, contract(dd2, W2))
        gp = contract(dd1, W1)
    _dense_sums(G, ((f"{name}.dense1", dd1, stage["max"]), (f"{name}.dense2", dd2, r1), (f"{name}.dense3", dd3, a2)))
    return gp


def feat_head(G, Q, r, bnin, pooled, up, mask, keep):
    """feat's dense layers and cls back: up (B, nc) = glogits, mask (B, 256) the dropout multipliers or None."""
    B = up.shape[0]
    r1, a1, v2, a2 = bnin["feat.bn3"], r["feat_d1"], bnin["feat.bn4"], r["feat_d2"]
    W1, W2, W3 = _weights(Q, "feat.dense1", "feat.dense2", "cls")
    with np.errstate(all="ignore"):
        r2 = relu(dense(a1, Q, "feat.dense2"))
        dd3 = np.where(np.ascontiguousarray(r["logits"].T) > 0, up, ZERO).astype(F32)
        g2 = bn_back(G, Q, "feat.bn4", contract(dd3, W3), v2, B, keep=keep)
        if mask is not None:
            g2 = (g2 * mask).astype(F32)
        dd2 = _masked(r2, g2)
        dd1 = _masked(r1, bn_back(G, Q, "feat.bn3", contract(dd2, W2), r1, B, keep=keep))
        gp = contract(dd1, W1)
    _dense_sums(G, (("feat.dense1", dd1, pooled), ("feat.dense2", dd2, a1), ("cls", dd3, a2)))
    return gp


def _wt(Q, name):
    return np.ascontiguousarray(np.asarray(Q[name + ".weight"], F32)[0].T)


def stn_back(G, Q, name, x_in, stage, bnin, gmat, K, keep):
    """One transform net back: x_in (B, N, K) its input, gmat (K, K, B) the gradient at its matrix.  Returns (the gradient at
    x_in, n*)."""
    B = x_in.shape[0]
    up = np.ascontiguousarray(np.transpose(gmat, (2, 0, 1))).reshape(B, K * K)  # d3[K i + j] = T[i, j]
    gp = stn_head(G, Q, name, stage, bnin, up, keep)
    g2, nstar = last_conv(G, Q, f"{name}.conv3", f"{name}.bn3", stage["a2"], bnin[f"{name}.bn3"], stage["a3"], stage["max"], gp, True,
                          keep)
    with np.errstate(all="ignore"):
        d2 = conv_back(G, Q, f"{name}.conv2", f"{name}.bn2", stage["a1"], g2, bnin[f"{name}.bn2"], keep)
        d1 = conv_back(G, Q, f"{name}.conv1", f"{name}.bn1", x_in, contract(d2, _wt(Q, f"{name}.conv2")), bnin[f"{name}.bn1"], keep)
        return contract(d1, _wt(Q, f"{name}.conv1")), nstar


def grad_train(X, P, glogits, dropout=None, keep=None):
    """(grads, gx, mid) as pointnet_grad_ref.grad returns them, for the training-mode network on X (3, N, B), B >= 2, under the
    dropout multipliers (256, B) or None.  keep: a dict that receives the rounds' n*, the forward, and per BatchNorm its gy, xh, m
    and Float64 sums."""
    X = np.asarray(X, F32)
    B = X.shape[2]
    nc = np.asarray(P["cls.weight"]).shape[0]
    r = tref.forward_train(X, P, dropout)
    Q = dict(P)
    Q.update(r["batch_stats"])
    bnin = r["bn_inputs"]
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, 3)
    N = x.shape[1]
    up = np.ascontiguousarray(np.asarray(glogits, F32).reshape((nc, B), order="F").T)
    mask = None if dropout is None else np.ascontiguousarray(np.asarray(dropout, F32).T)
    G = {}
    with np.errstate(all="ignore"):
        # feat and cls
        pooled = np.ascontiguousarray(r["pooled"].T)
        gp = feat_head(G, Q, r, bnin, pooled, up, mask, keep)
        g_a1, n_feat = last_conv(G, Q, "feat.conv2", "feat.bn2", r["feat_a1"], bnin["feat.bn2"], r["feat_a2"], pooled, gp, False, keep)
        d1 = conv_back(G, Q, "feat.conv1", "feat.bn1", r["h_t"], g_a1, bnin["feat.bn1"], keep)
        g_ht = contract(d1, _wt(Q, "feat.conv1"))
        gF = _gmat(r["h"], g_ht)
        ghf = _through(g_ht, r["fstn"])
        # fstn, conv_block1, the input transform
        g_fstn, n_fstn = stn_back(G, Q, "fstn", r["h"], r["fstn_stage"], bnin, gF, 64, keep)
        gh = (ghf + g_fstn).astype(F32)
        d0 = bn_back(G, Q, "conv_block1.bn", _masked(r["h"], gh), bnin["conv_block1.bn"], B * N, keep=keep)
        conv_param_sums(G, "conv_block1.conv", r["x_t"], d0)
        gxt = contract(d0, _wt(Q, "conv_block1.conv"))
        gT = _gmat(x, gxt)
        # stn, and the two paths into x
        g_stn, n_stn = stn_back(G, Q, "stn", x, r["stn_stage"], bnin, gT, 3, keep)
        gx = (_through(gxt, r["stn"]) + g_stn).astype(F32)
    if keep is not None:
        keep.update(nstar={"stn": n_stn, "fstn": n_fstn, "feat": n_feat}, forward=r)
    lay = lambda a: np.asfortranarray(np.transpose(a, (2, 1, 0)))  # (B, N, C) -> (C, N, B)
    mid = {"gstn": np.asfortranarray(gT), "gfstn": np.asfortranarray(gF), "gh": lay(gh), "gxt": lay(gxt)}
    return {n: G[n] for n in ref.param_shapes(nc)}, lay(gx), mid


family, flat, FAMILIES = gref.family, gref.flat, gref.FAMILIES
