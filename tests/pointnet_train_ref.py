"""Host restatement of the PointNet training-mode forward (include/flux3d_hip.h "PointNet training-mode forward") in numpy, on
top of tests/pointnet_ref.py: the definition the device kernels are held to, bit for bit, up to the logits, for every batch
statistic and for the updated running statistics.

The network and its Float32 arithmetic are pointnet_ref's.  What is new is BatchNorm's statistics: Float64 sums S1 = sum v and
S2 = sum v v of the Float32 values a BatchNorm is given, in the header's order --

  after a convolution: per tile of 64 points of a cloud the rows whose bit 2 is h form chain h (ascending), the tile's sum is
    chain(0) + chain(1); the tile sums t = tile + ntiles b are folded as GROUPS chains (t = g, g + GROUPS, ... ascending),
    which are then added in ascending g;
  after a dense layer: one chain over the clouds in ascending b;

every chain from +0.0.  Rows beyond a cloud's last point and chains without a tile are padded with +0.0 here, which changes no
bit: a chain that starts at +0.0 never holds -0.0, and x + 0.0 == x for every other x.  Then mu64 = S1 / m, var64 = max(0, S2 / m
- mu64 mu64) (a NaN stays), both rounded to Float32 once, and the running update in Float32 with one rounding per operation."""
import numpy as np

import pointnet_ref as ref

F32, F64 = np.float32, np.float64
TILE = 64
GROUPS = 32  # FX3D_POINTNET_STAT_GROUPS
BN_ORDER = (["stn.bn1", "stn.bn2", "stn.bn3", "stn.bn4", "conv_block1.bn"] + ["fstn.bn1", "fstn.bn2", "fstn.bn3", "fstn.bn4"]
            + ["feat.bn1", "feat.bn2", "feat.bn3", "feat.bn4"])
DENSE_BN = ("stn.bn4", "fstn.bn4", "feat.bn3", "feat.bn4")


def point_sums(v):
    """v (B, N, C) Float32 -> (S1, S2) (C,) Float64 in the header's order for a convolution's BatchNorm."""
    B, N, C = v.shape
    nt = (N + TILE - 1) // TILE
    with np.errstate(all="ignore"):
        d = np.zeros((B, nt * TILE, C), F64)
        d[:, :N] = v
        d = d.reshape(B, nt, 8, 2, 4, C)  # row p = 8 q + 4 h + i of its tile
        s1, s2 = np.zeros((B, nt, 2, C), F64), np.zeros((B, nt, 2, C), F64)
        for q in range(8):
            for i in range(4):  # ascending p within chain h
                x = d[:, :, q, :, i, :]
                s1 = s1 + x
                s2 = s2 + x * x  # exact product
        t1, t2 = s1[:, :, 0] + s1[:, :, 1], s2[:, :, 0] + s2[:, :, 1]  # (B, nt, C): the tile sums
        out = []
        for t in (t1, t2):
            T = B * nt
            rows = (T + GROUPS - 1) // GROUPS
            f = np.zeros((rows * GROUPS, C), F64)
            f[:T] = t.reshape(T, C)  # t = tile + nt b
            f = f.reshape(rows, GROUPS, C)
            chains = np.zeros((GROUPS, C), F64)
            for k in range(rows):
                chains = chains + f[k]
            s = np.zeros(C, F64)
            for g in range(GROUPS):
                s = s + chains[g]
            out.append(s)
    return out[0], out[1]


def dense_sums(v):
    """v (B, C) Float32 -> (S1, S2) (C,) Float64: one chain over the clouds in ascending b."""
    with np.errstate(all="ignore"):
        d = v.astype(F64)
        s1, s2 = np.zeros(v.shape[1], F64), np.zeros(v.shape[1], F64)
        for b in range(v.shape[0]):
            s1 = s1 + d[b]
            s2 = s2 + d[b] * d[b]
    return s1, s2


def raw_var(s1, s2, m):
    """S2 / m - mu64 mu64 in Float64, the variance before the clamp: on a constant channel pure rounding residue of either sign."""
    with np.errstate(all="ignore"):
        dm = F64(m)
        mu64 = s1 / dm
        return s2 / dm - mu64 * mu64


def mean_var(s1, s2, m):
    """(mu, var) Float32 from the Float64 sums over m values per channel."""
    with np.errstate(all="ignore"):
        mu64 = s1 / F64(m)
        var64 = raw_var(s1, s2, m)
        var64 = np.where(var64 < 0, F64(0), var64)  # a NaN stays
        return mu64.astype(F32), var64.astype(F32)


def running_update(run_mu, run_var, mu, var, m, momentum):
    """Flux's BatchNorm after the step, Float32, one rounding per operation."""
    mtm = F32(momentum)
    with np.errstate(all="ignore"):
        keep = F32(F32(1) - mtm)
        new_mu = ((keep * run_mu).astype(F32) + (mtm * mu).astype(F32)).astype(F32)
        factor = F32(F32(mtm * F32(m)) / F32(m - 1))
        new_var = ((keep * run_var).astype(F32) + (factor * var).astype(F32)).astype(F32)
    return new_mu, new_var


class _Train:
    """The parameters with every BatchNorm's mu / sigma2 replaced, as the layers run, by the batch statistics."""

    def __init__(self, P, momentum):
        self.P, self.Q, self.momentum = P, dict(P), momentum
        self.batch_stats, self.running, self.bn_inputs, self.raw_var = {}, {}, {}, {}

    def bn(self, v, name):
        v = np.asarray(v, F32)
        if v.ndim == 3:
            s1, s2 = point_sums(v)
            m = v.shape[0] * v.shape[1]
        else:
            s1, s2 = dense_sums(v)
            m = v.shape[0]
        mu, var = mean_var(s1, s2, m)
        self.raw_var[name] = raw_var(s1, s2, m)
        self.bn_inputs[name] = v
        self.batch_stats[name + ".mu"], self.batch_stats[name + ".sigma2"] = mu, var
        self.running[name + ".mu"], self.running[name + ".sigma2"] = running_update(
            np.asarray(self.P[name + ".mu"], F32), np.asarray(self.P[name + ".sigma2"], F32), mu, var, m, self.momentum)
        self.Q[name + ".mu"], self.Q[name + ".sigma2"] = mu, var
        return ref.batchnorm(v, self.Q, name)


def _stn_stage(x, t, name, K):
    P, r = t.P, {}
    r["a1"] = t.bn(ref.relu(ref.conv(x, P, f"{name}.conv1")), f"{name}.bn1")
    r["a2"] = t.bn(ref.relu(ref.conv(r["a1"], P, f"{name}.conv2")), f"{name}.bn2")
    r["a3"] = t.bn(ref.relu(ref.conv(r["a2"], P, f"{name}.conv3")), f"{name}.bn3")
    r["max"] = ref.jmax(r["a3"], axis=1)
    r["d1"] = ref.relu(ref.dense(r["max"], P, f"{name}.dense1"))
    r["d2"] = t.bn(ref.relu(ref.dense(r["d1"], P, f"{name}.dense2")), f"{name}.bn4")
    r["d3"] = ref.dense(r["d2"], P, f"{name}.dense3")
    B = x.shape[0]
    r["T"] = np.ascontiguousarray(np.transpose(r["d3"].reshape(B, K, K), (1, 2, 0)))
    return r


def forward_train(X, P, dropout=None, momentum=0.1):
    """X (3, N, B) with B >= 2, P: name -> array in Flux's shapes (its mu / sigma2 are the running statistics), dropout: None
    or (256, B) multipliers.  Returns every intermediate; ``logits``, ``stn``, ``fstn``, ``pooled`` and ``probs`` laid out as the
    library returns them; ``batch_stats`` and ``running``: name -> (C,) with the ``...bnK.mu`` / ``.sigma2`` names; ``bn_inputs``:
    BatchNorm name -> what it was given; ``raw_var``: BatchNorm name -> (C,) Float64, the variance before the clamp."""
    X = np.asarray(X, F32)
    assert X.ndim == 3 and X.shape[2] >= 2
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, 3)
    t, r = _Train(P, momentum), {}
    r["stn_stage"] = _stn_stage(x, t, "stn", 3)
    r["stn"] = r["stn_stage"]["T"]
    r["x_t"] = ref.apply_transform(x, r["stn"])
    r["h"] = ref.relu(t.bn(ref.conv(r["x_t"], P, "conv_block1.conv"), "conv_block1.bn"))
    r["fstn_stage"] = _stn_stage(r["h"], t, "fstn", 64)
    r["fstn"] = r["fstn_stage"]["T"]
    r["h_t"] = ref.apply_transform(r["h"], r["fstn"])
    r["feat_a1"] = t.bn(ref.relu(ref.conv(r["h_t"], P, "feat.conv1")), "feat.bn1")
    r["feat_a2"] = t.bn(ref.conv(r["feat_a1"], P, "feat.conv2"), "feat.bn2")
    pooled = ref.jmax(r["feat_a2"], axis=1)  # (B, 1024)
    r["feat_d1"] = t.bn(ref.relu(ref.dense(pooled, P, "feat.dense1")), "feat.bn3")
    drop = ref.relu(ref.dense(r["feat_d1"], P, "feat.dense2"))
    if dropout is not None:
        mask = np.asarray(dropout, F32)
        assert mask.shape == (256, X.shape[2]), mask.shape
        with np.errstate(all="ignore"):
            drop = (drop * mask.T).astype(F32)
    r["feat_drop"] = drop
    r["feat_d2"] = t.bn(drop, "feat.bn4")
    logits = ref.relu(ref.dense(r["feat_d2"], P, "cls"))
    r["pooled"] = np.asfortranarray(pooled.T)
    r["logits"] = np.asfortranarray(logits.T)
    r["probs"] = ref.softmax32(r["logits"])
    r["batch_stats"], r["running"], r["bn_inputs"], r["raw_var"] = t.batch_stats, t.running, t.bn_inputs, t.raw_var
    assert [k[:-3] for k in t.batch_stats if k.endswith(".mu")] == BN_ORDER  # the BatchNorms ran in the layout's order
    return r


def flat_stats(named):
    """name -> (C,) as the library's flat statistics buffer: per BatchNorm in forward order mu (C), then sigma2 (C)."""
    return np.concatenate([np.asarray(named[f"{bn}.{f}"], F32) for bn in BN_ORDER for f in ("mu", "sigma2")])
