"""Host restatement of the DGCNN adjoint (include/flux3d_hip.h "DGCNN adjoint") in numpy: the definition fx3d_dgcnn_grad is held
to, bit for bit, every sum in the header's order.

The two EdgeConv stages are tests/edgeconv_pgrad_ref.py's grad, composed: stage 2 on (x1, idx2, x2) with gout = gx2, stage 1 on
(X, idx1, x1) with gout = gx1.  The tail -- conv_3, the maximum over the points, fc_4, fc_5, fc_6 -- is written here with
tests/pointnet_ref.py's fma32 chains: the head's chains over the layer outputs, the first point that equals the maximum, the
gather of W3's rows for gx2, and the chains over the clouds for the parameter sums."""
import numpy as np

import dgcnn_ref
import edgeconv_pgrad_ref as pref
from pointnet_ref import BN_EPS, F32, batchnorm, contract, conv, dense, fma32, relu

L1, L2 = [3, 32, 64, 64], [64, 128, 256]   # the layers of the two EdgeConv stages
FAMILIES = {"dW": ".weight", "db": ".bias", "dgamma": ".gamma", "dbeta": ".beta"}


def stage_params(P, name):
    """The ``ec1.`` / ``ec2.`` arrays of a DGCNN with the prefix dropped: the parameters of the EdgeConv layer."""
    return {k[len(name) + 1:]: v for k, v in P.items() if k.startswith(name + ".")}


def conv3(P, x2):
    """a3 (B, N, 1024) = relu(BN3(conv_3(x2))) for x2 (256, N, B), the forward's bits."""
    x = np.ascontiguousarray(np.transpose(np.asarray(x2, F32), (2, 1, 0)))
    return relu(batchnorm(conv(x, P, "conv3.conv"), P, "conv3.bn"))


def pool(a3):
    """pooled (1024, B) of a3 (B, N, 1024): Julia's maximum over the points."""
    return np.asfortranarray(dgcnn_ref.jmax(a3, axis=1).T)


def winners(a3, pooled):
    """n* (B, 1024): the smallest n with a3[b, n, c] == pooled[c, b] where pooled is positive, -1 where there is none."""
    p = np.asarray(pooled, F32).T[:, None, :]  # (B, 1, 1024)
    with np.errstate(invalid="ignore"):
        hit = (a3 == p) & (p > 0)
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


def _sd(P, name):
    return np.sqrt(np.asarray(P[name + ".sigma2"], F32) + BN_EPS).astype(F32)


def _scaled(d, P, name):
    """dz = (d gamma) / sd, each operation rounded to Float32."""
    return ((d * np.asarray(P[name + ".gamma"], F32)).astype(F32) / _sd(P, name)).astype(F32)


def _add_chain(rows):
    acc = np.zeros(rows.shape[1:], F32)
    for v in rows:
        acc = (acc + v).astype(F32)
    return acc


def _families(G, wname, bnname, W_in_out, H_in_out, h, P, as_conv):
    """The four families of a layer from H (cin, cout) and h (cout,); W_in_out: the weights as (cin, cout)."""
    bias, gamma, mu = (np.asarray(P[n], F32) for n in (wname + ".bias", bnname + ".gamma", bnname + ".mu"))
    sd = _sd(P, bnname)
    dW = ((H_in_out * gamma).astype(F32) / sd).astype(F32)
    G[wname + ".weight"] = dW[None] if as_conv else np.ascontiguousarray(dW.T)
    G[wname + ".bias"] = ((h * gamma).astype(F32) / sd).astype(F32)
    acc = np.zeros_like(h)
    for i in range(W_in_out.shape[0]):
        acc = fma32(W_in_out[i], H_in_out[i], acc)
    G[bnname + ".gamma"] = ((acc + ((bias - mu).astype(F32) * h).astype(F32)).astype(F32) / sd).astype(F32)
    G[bnname + ".beta"] = h.copy()
    G[bnname + ".mu"], G[bnname + ".sigma2"] = np.zeros_like(h), np.zeros_like(h)


def tail(P, x2, pooled, glogits, keep=None):
    """(G, gx2, nstar): the gradients of conv3, fc4, fc5 and fc6 (Flux's shapes), gx2 (256, N, B) and n* (B, 1024).  keep: a
    dict that receives d3 and dz3, (B, 1024) each."""
    x2 = np.asarray(x2, F32)
    _, N, B = x2.shape
    pooled = np.asarray(pooled, F32).reshape((1024, B), order="F")
    d6 = np.ascontiguousarray(np.asarray(glogits, F32).reshape((-1, B), order="F").T)  # (B, nc)
    zero = F32(0.0)
    with np.errstate(all="ignore"):
        a3 = conv3(P, x2)
        nstar = winners(a3, pooled)
        won = nstar >= 0
        p = np.ascontiguousarray(pooled.T)  # (B, 1024)
        a4 = relu(batchnorm(dense(p, P, "fc4.dense"), P, "fc4.bn"))
        a5 = relu(batchnorm(dense(a4, P, "fc5.dense"), P, "fc5.bn"))
        W6, W5, W4 = (np.asarray(P[n], F32) for n in ("fc6.weight", "fc5.dense.weight", "fc4.dense.weight"))  # (out, in)
        W3 = np.asarray(P["conv3.conv.weight"], F32)[0]  # (256, 1024)
        d5 = np.where(a5 > 0, contract(d6, W6), zero).astype(F32)
        d4 = np.where(a4 > 0, contract(_scaled(d5, P, "fc5.bn"), W5), zero).astype(F32)
        gp = contract(_scaled(d4, P, "fc4.bn"), W4)
        d3 = np.where(won, gp, zero).astype(F32)
        dz3 = _scaled(d3, P, "conv3.bn")
        if keep is not None:
            keep.update(d3=d3, dz3=dz3)
        # conv_3's input gradient: per point the chain over the channels it wins, ascending
        gx2 = np.zeros((B, N, 256), F32)
        for b in range(B):
            for c in np.flatnonzero(won[b]):
                n = nstar[b, c]
                gx2[b, n] = fma32(dz3[b, c], W3[:, c], gx2[b, n])
        # the sums over the clouds, b ascending
        H6, H5, H4 = np.zeros(W6.shape, F32), np.zeros(W5.shape, F32), np.zeros(W4.shape, F32)
        H3, h3 = np.zeros(W3.shape, F32), np.zeros(1024, F32)
        for b in range(B):
            H6 = fma32(d6[b][:, None], a5[b][None, :], H6)
            H5 = fma32(d5[b][:, None], a4[b][None, :], H5)
            H4 = fma32(d4[b][:, None], p[b][None, :], H4)
            w = np.flatnonzero(won[b])
            H3[:, w] = fma32(x2[:, nstar[b, w], b], d3[b, w][None, :], H3[:, w])
            h3[w] = (h3[w] + d3[b, w]).astype(F32)
        G = {}
        _families(G, "conv3.conv", "conv3.bn", W3, H3, h3, P, True)
        _families(G, "fc4.dense", "fc4.bn", np.ascontiguousarray(W4.T), np.ascontiguousarray(H4.T), _add_chain(d4), P, False)
        _families(G, "fc5.dense", "fc5.bn", np.ascontiguousarray(W5.T), np.ascontiguousarray(H5.T), _add_chain(d5), P, False)
        G["fc6.weight"], G["fc6.bias"] = H6, _add_chain(d6)
    return G, np.asfortranarray(np.transpose(gx2, (2, 1, 0))), nstar


def grad(X, P, K, glogits, fwd=None):
    """(grads, gx, gx2, gx1) for X (3, N, B) or (3, N).  fwd: a mapping with the forward's idx1, x1, idx2, x2 and pooled (the
    library's layouts); without it dgcnn_ref.forward computes them.  grads maps every name of dgcnn_ref.param_shapes to its
    gradient in Flux's shape (mu and sigma2: zeros)."""
    X = np.asarray(X, F32)
    if X.ndim == 2:
        X = X[:, :, None]
    if fwd is None:
        fwd = dgcnn_ref.forward(X, P, K)
    idx1, x1, idx2, x2, pooled = (np.asarray(fwd[k]) for k in ("idx1", "x1", "idx2", "x2", "pooled"))
    nc = np.asarray(P["fc6.weight"]).shape[0]
    G, gx2, _ = tail(P, x2, pooled, glogits)
    G2, gx1 = pref.grad(x1, stage_params(P, "ec2"), L2, K, gx2, idx2, x2)
    G1, gx = pref.grad(X, stage_params(P, "ec1"), L1, K, gx1, idx1, x1)
    G.update({"ec1." + k: v for k, v in G1.items()})
    G.update({"ec2." + k: v for k, v in G2.items()})
    return {n: G[n] for n in dgcnn_ref.param_shapes(nc)}, gx, gx2, gx1


def family(G, fam):
    """One of the four families over all 8 parameterised layers as one flat array."""
    return np.concatenate([np.asarray(v).ravel() for n, v in G.items() if n.endswith(FAMILIES[fam])])


def flat(G):
    """The gradients in the parameter buffer's layout: every array column-major, in forward order."""
    return np.concatenate([np.asarray(v, F32).ravel(order="F") for v in G.values()])
