"""Host restatement of include/flux3d_hip.h "Training step": fx3d_crossentropy, fx3d_dropout_mask and fx3d_adam_step, and the map
from a model's flat statistics buffer to the mu / sigma2 slots of its flat parameter buffer.  Numpy only: numpy rounds every
operation once and fuses nothing, and its Float64 division and square root are IEEE's, which is what the header asks of the device."""
import numpy as np

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64


def crossentropy(probs, labels):
    """(loss, glogits, counts) of fx3d_crossentropy for probs (num_classes, B) Float32 and B integer labels: loss a Float64, glogits
    (num_classes, B) Float32, counts int32 (first maxima that are the label, labels out of range).  log is numpy's."""
    probs = np.asarray(probs, F32)
    nc, B = probs.shape
    y = np.asarray(labels).astype(np.int64)
    assert y.shape == (B,)
    inside = (y >= 0) & (y < nc)
    onehot = np.zeros((nc, B), F32)
    onehot[y[inside], np.flatnonzero(inside)] = 1
    with np.errstate(all="ignore"):
        glogits = np.asfortranarray(((probs - onehot).astype(F32) / F32(B)).astype(F32))
        total = F64(0.0)
        for b in range(B):  # one chain in ascending b
            total = total + (np.log(F64(probs[y[b], b])) if inside[b] else F64(np.nan))
        loss = F64(-total) / F64(B)
    best, pbest = np.zeros(B, np.int64), probs[0].copy()
    for o in range(1, nc):  # the first maximum: only a strictly larger value moves it
        take = probs[o] > pbest
        best[take], pbest[take] = o, probs[o][take]
    return loss, glogits, np.array([np.count_nonzero(inside & (best == y)), np.count_nonzero(~inside)], np.int32)


def adam_step(x, g, m, v, betap, eta=0.001, beta=(0.9, 0.999), eps=1e-8, running=None, stat_map=None, dtype=F32):
    """One fx3d_adam_step: (x, m, v, betap) after the step, new arrays.  ``dtype``: the type of the arrays -- Float32 is the
    library's mixed-precision form (Float64 hyper-parameters over Float32 arrays, each line of the header rounded to Float32 where it
    is stored); Float64 makes every rounding to ``dtype`` the identity, which is plain Float64 ADAM."""
    T = dtype
    x, g, m, v = (np.asarray(a, T) for a in (x, g, m, v))
    b1, b2, eta, eps = F64(beta[0]), F64(beta[1]), F64(eta), F64(eps)
    bp1, bp2 = F64(betap[0]), F64(betap[1])
    with np.errstate(all="ignore"):
        m = ((b1 * m.astype(F64)) + ((F64(1) - b1) * g.astype(F64))).astype(T)
        gg = (g * g).astype(T)  # the product in the arrays' own type
        v = ((b2 * v.astype(F64)) + ((F64(1) - b2) * gg.astype(F64))).astype(T)
        delta = (((m.astype(F64) / (F64(1) - bp1)) / (np.sqrt(v.astype(F64) / (F64(1) - bp2)) + eps)) * eta).astype(T)
        x = (x - delta).astype(T)
    if stat_map is not None:
        x[np.asarray(stat_map)] = np.asarray(running, T)
    return x, m, v, np.array([bp1 * b1, bp2 * b2], F64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of counter words; the key is two scalars.  Four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(w, U64)) & U64(0xFFFFFFFF) for w in (c0, c1, c2, c3)]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(w, shape).copy() for w in c]
    k0, k1, mask = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF, U64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c[0], U64(0xCD9E8D57) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ U64(k0), p1 & mask, (p0 >> U64(32)) ^ c[3] ^ U64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [w.astype(U32) for w in c]


def dropout_mask(n, p, seed, counter=0, stream_id=0):
    """fx3d_dropout_mask: n Float32 multipliers.  ``counter``: the value of the device counter added to ``seed``."""
    n, p = int(n), float(p)
    key = (int(seed) + int(counter)) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((n + 3) // 4, dtype=U64)
    words = np.stack(philox4x32_10(q, stream_id, 0, 0, key & 0xFFFFFFFF, key >> 32), axis=1).reshape(-1)[:n]  # element e: word e mod 4 of block e div 4
    u = ((words >> U32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)
    return np.where(u.astype(F64) > p, F32(1.0 / (1.0 - p)), F32(0.0)).astype(F32)


def stat_map(model):
    """int32 (nstat,): for every element of a model's flat statistics buffer (per BatchNorm mu (C), then sigma2 (C)) its index in
    the flat parameter buffer, from the model's ``_stat_slots``."""
    out = []
    for _, C, at, flat in model._stat_slots():
        assert at == len(out)
        out.extend(range(flat, flat + 2 * C))
    return np.array(out, np.int32)
