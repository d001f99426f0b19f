"""Host restatement of the DGCNN / EdgeConv training-mode forward (include/flux3d_hip.h "DGCNN / EdgeConv training-mode forward")
in numpy, on top of tests/dgcnn_ref.py and tests/edgeconv_ref.py: the definition the device kernels are held to, bit for bit, up
to the logits, for every batch statistic and for the updated running statistics.

The networks and their Float32 arithmetic are dgcnn_ref's; mean, variance and the running update are pointnet_train_ref's
(mean_var, running_update), and so are the orders of conv3.bn (point_sums) and of the dense BatchNorms (dense_sums).  What is
new is the order of an EdgeConv BatchNorm's Float64 sums over its K N B edge rows --

  per tile of 64 points of a cloud the rows p with p div 32 = q and bit 2 of p equal to h form the chain (q, h): it runs over
    the neighbour rank k ascending and, within a k, over its 16 rows in ascending p; the tile's sum is
    (chain(0,0) + chain(0,1)) + (chain(1,0) + chain(1,1)); the tile sums t = tile + ntiles b are folded as GROUPS chains
    (t = g, g + GROUPS, ... ascending), which are then added in ascending g;

every chain from +0.0.  Rows beyond a cloud's last point and chains without a tile are padded with +0.0 here, which changes no
bit (pointnet_train_ref's note)."""
import numpy as np

import dgcnn_ref as ref
from pointnet_train_ref import GROUPS, TILE, dense_sums, mean_var, point_sums, raw_var, running_update  # noqa: F401

F32, F64 = np.float32, np.float64
BN_ORDER = ["ec1.bn1", "ec1.bn2", "ec1.bn3", "ec2.bn1", "ec2.bn2", "conv3.bn", "fc4.bn", "fc5.bn"]
BN_WIDTH = [32, 64, 64, 128, 256, 1024, 512, 256]  # 2336 channels


def fold_tiles(t):
    """t (B, nt, C) Float64 tile sums -> (C,): GROUPS interleaved chains over t = tile + nt b, added in ascending g."""
    B, nt, C = t.shape
    T = B * nt
    rows = (T + GROUPS - 1) // GROUPS
    f = np.zeros((rows * GROUPS, C), F64)
    f[:T] = t.reshape(T, C)
    f = f.reshape(rows, GROUPS, C)
    chains = np.zeros((GROUPS, C), F64)
    for k in range(rows):
        chains = chains + f[k]
    s = np.zeros(C, F64)
    for g in range(GROUPS):
        s = s + chains[g]
    return s


def edge_sums(v):
    """v (B, K, N, C) Float32 -> (S1, S2) (C,) Float64 in the header's order for an EdgeConv's BatchNorm."""
    B, K, N, C = v.shape
    nt = (N + TILE - 1) // TILE
    with np.errstate(all="ignore"):
        d = np.zeros((B, K, nt * TILE, C), F64)
        d[:, :, :N] = v
        d = d.reshape(B, K, nt, 2, 4, 2, 4, C)  # row p = 32 q + 8 g + 4 h + i of its tile: axes (q, g, h, i)
        s1, s2 = np.zeros((B, nt, 2, 2, C), F64), np.zeros((B, nt, 2, 2, C), F64)  # chains (q, h)
        for k in range(K):
            for g in range(4):
                for i in range(4):  # ascending p within the chain
                    x = d[:, k, :, :, g, :, i, :]  # (B, nt, q, h, C)
                    s1 = s1 + x
                    s2 = s2 + x * x  # exact product
        t1 = (s1[:, :, 0, 0] + s1[:, :, 0, 1]) + (s1[:, :, 1, 0] + s1[:, :, 1, 1])
        t2 = (s2[:, :, 0, 0] + s2[:, :, 0, 1]) + (s2[:, :, 1, 0] + s2[:, :, 1, 1])
        return fold_tiles(t1), fold_tiles(t2)


class _Train:
    """The parameters with every BatchNorm's mu / sigma2 replaced, as the layers run, by the batch statistics."""

    def __init__(self, P, momentum):
        self.P, self.Q, self.momentum = P, dict(P), momentum
        self.batch_stats, self.running, self.bn_inputs, self.raw_var = {}, {}, {}, {}

    def bn(self, v, name):
        """v: (B, K, N, C) in an EdgeConv, (B, N, C) after conv_3, (B, C) after a dense layer."""
        v = np.asarray(v, F32)
        s1, s2 = (edge_sums, point_sums, dense_sums)[4 - v.ndim](v)
        m = int(np.prod(v.shape[:-1]))
        mu, var = mean_var(s1, s2, m)
        self.raw_var[name] = raw_var(s1, s2, m)
        self.bn_inputs[name] = v
        self.batch_stats[name + ".mu"], self.batch_stats[name + ".sigma2"] = mu, var
        self.running[name + ".mu"], self.running[name + ".sigma2"] = running_update(
            np.asarray(self.P[name + ".mu"], F32), np.asarray(self.P[name + ".sigma2"], F32), mu, var, m, self.momentum)
        self.Q[name + ".mu"], self.Q[name + ".sigma2"] = mu, var
        return ref.batchnorm(v, self.Q, name)


def _edgeconv(x, t, prefix, nblocks, K, idx=None):
    """x (B, N, F) -> (idx (K, N, B), y (B, N, cL)): the edge rows of all clouds, the blocks with their BatchNorms at the batch
    statistics over all (b, k, n), the maximum over k."""
    if idx is None:
        idx = ref.self_knn(x, K)
    a = np.stack([ref.edge_rows(x[b], idx[:, :, b]) for b in range(x.shape[0])])  # (B, K, N, 2F)
    for i in range(1, nblocks + 1):
        a = ref.relu(t.bn(ref.conv(a, t.P, f"{prefix}conv{i}"), f"{prefix}bn{i}"))  # conv_bn_block: Conv, BatchNorm, relu
    return idx, ref.jmax(a, axis=1)


def edgeconv_forward_train(X, P, layers, K, idx=None, momentum=0.1):
    """EdgeConv(layers, K) in training mode.  X (F, N, B) or (F, N); P: name -> array in Flux's shapes with edgeconv_ref's names
    (its mu / sigma2 are the running statistics); idx: (K, N, B) 0-based lists to use instead of the search.  A dict: ``idx``
    (K, N, B) int32 and ``out`` (cL, N, B) laid out as the library returns them; ``batch_stats`` and ``running``: name -> (C,)
    under the ``bnK.mu`` / ``.sigma2`` names; ``bn_inputs``: BatchNorm name -> what it was given, (B, K, N, C); ``raw_var``:
    BatchNorm name -> (C,) Float64, the variance before the clamp."""
    X = np.asarray(X, F32)
    if X.ndim == 2:
        X = X[:, :, None]
    assert X.shape[0] == layers[0], (X.shape, layers)
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, F)
    if idx is not None:
        idx = np.asarray(idx).reshape((K,) + x.shape[1::-1], order="F")
    t = _Train(P, momentum)
    idx, y = _edgeconv(x, t, "", len(layers) - 1, K, idx)
    return {"idx": np.asfortranarray(idx.astype(np.int32)), "out": np.asfortranarray(np.transpose(y, (2, 1, 0))),
            "batch_stats": t.batch_stats, "running": t.running, "bn_inputs": t.bn_inputs, "raw_var": t.raw_var}


def forward_train(X, P, K, dropout=None, momentum=0.1):
    """DGCNN in training mode.  X (3, N, B) with B >= 2; P: name -> array in Flux's shapes (its mu / sigma2 are the running
    statistics); dropout: None or the pair of multipliers (512, B), (256, B).  A dict as dgcnn_ref.forward's -- ``idx1``, ``idx2``,
    ``x1``, ``x2``, ``pooled``, ``logits``, ``probs`` laid out as the library returns them -- with ``batch_stats`` and ``running``:
    name -> (C,) under the ``...bn.mu`` / ``.sigma2`` names; ``bn_inputs``: BatchNorm name -> what it was given; ``raw_var``:
    BatchNorm name -> (C,) Float64, the variance before the clamp; ``d4`` (B, 512): fc_4's output after its dropout multiplier,
    fc_5's input."""
    X = np.asarray(X, F32)
    assert X.ndim == 3 and X.shape[2] >= 2
    B = X.shape[2]
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, 3)
    masks = [None, None] if dropout is None else [np.asarray(m, F32) for m in dropout]
    assert all(m is None or m.shape == (C, B) for m, C in zip(masks, (512, 256)))
    t, r = _Train(P, momentum), {}

    def drop(v, mask):
        if mask is None:
            return v
        with np.errstate(all="ignore"):
            return (v * mask.T).astype(F32)

    r["idx1"], x1 = _edgeconv(x, t, "ec1.", 3, K)
    r["idx2"], x2 = _edgeconv(x1, t, "ec2.", 2, K)  # the search runs on the training-mode x1
    r["conv3"] = ref.relu(t.bn(ref.conv(x2, P, "conv3.conv"), "conv3.bn"))
    pooled = ref.jmax(r["conv3"], axis=1)  # (B, 1024)
    r["d4"] = drop(ref.relu(t.bn(ref.dense(pooled, P, "fc4.dense"), "fc4.bn")), masks[0])  # fc_bn_block, then Dropout(0.5)
    d5 = drop(ref.relu(t.bn(ref.dense(r["d4"], P, "fc5.dense"), "fc5.bn")), masks[1])
    logits = ref.dense(d5, P, "fc6")
    r["x1"] = np.asfortranarray(np.transpose(x1, (2, 1, 0)))
    r["x2"] = np.asfortranarray(np.transpose(x2, (2, 1, 0)))
    r["pooled"] = np.asfortranarray(pooled.T)
    r["logits"] = np.asfortranarray(logits.T)
    r["probs"] = ref.softmax32(r["logits"])
    r["batch_stats"], r["running"], r["bn_inputs"], r["raw_var"] = t.batch_stats, t.running, t.bn_inputs, t.raw_var
    assert [k[:-3] for k in t.batch_stats if k.endswith(".mu")] == BN_ORDER  # the BatchNorms ran in the layout's order
    return r


def flat_stats(named, order=BN_ORDER):
    """name -> (C,) as the library's flat statistics buffer: per BatchNorm in forward order mu (C), then sigma2 (C)."""
    return np.concatenate([np.asarray(named[f"{bn}.{f}"], F32) for bn in order for f in ("mu", "sigma2")])

