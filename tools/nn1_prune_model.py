#!/usr/bin/env python3
"""A numpy model of which lane tiles the pruned nearest-neighbour kernel runs (nn1_f16_kernel<.., PRUNE>, csrc/chamfer.hip),
so that finer pruning can be priced without a GPU.

The kernel's rule, in exact arithmetic (its rounding margins -- a few per cent of a squared radius -- are left out):
  * candidates and queries are ordered along the Hilbert curve kHilbertCell through an 8 x 8 x 8 grid over their own bounding
    boxes (index order inside a cell); 64 consecutive candidates are a lane tile with a box, 32 consecutive queries a group
    with a box (one wave's queries of a pass);
  * phase 0 runs the tiles whose box meets the group's box (none does: the nearest ones);
  * phase 1 runs the tiles whose box lies within the LARGEST upper bound of a nearest distance that phase 0 gave a query of
    the group.
Variants priced beside it:
  true      the same cut with every query's TRUE nearest distance: the floor of any rule that cuts per group with tile boxes
            (more phases, progressive re-cuts)
  sub2/sub4 points inside a cell ordered by 2^3 / 4^3 sub-cells (Morton) instead of by index
  g16/g8/g4 the group's 32 queries tested as sub-groups of 16 / 8 / 4 with boxes and bounds of their own; the wave runs a tile
            that any sub-group keeps

  python tools/nn1_prune_model.py [--n 4096] [--seeds 3]
prints the mean number of lane tiles kept per wave-pass (of n / 64) for uniform, unit-sphere and Gaussian clouds."""
import argparse
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, GROUP = 64, 32


def hilbert_cells():
    """kHilbertCell of chamfer.hip: the cell t = ux | uy << 3 | uz << 6 at every position of the curve."""
    src = open(os.path.join(ROOT, "flux3d.jl_amd", "csrc", "chamfer.hip")).read()
    body = re.search(r"kHilbertCell\[512\]\s*=\s*\{([^}]*)\}", src).group(1)
    cells = np.array([int(v) for v in body.replace("\n", " ").split(",") if v.strip()], dtype=np.int64)
    assert cells.size == 512 and np.array_equal(np.sort(cells), np.arange(512))
    return cells


def curve_order(p, sub=1):
    """Stable order of the points p (n, 3) along the curve; sub > 1: Morton order of sub^3 sub-cells inside a cell."""
    pos = np.empty(512, dtype=np.int64)
    pos[hilbert_cells()] = np.arange(512)
    lo, hi = p.min(0), p.max(0)
    inv = np.where(hi > lo, 8.0 / np.where(hi > lo, hi - lo, 1.0), 0.0)
    f = (p - lo) * inv
    u = np.clip(np.floor(f), 0, 7).astype(np.int64)
    key = pos[u[:, 0] | (u[:, 1] << 3) | (u[:, 2] << 6)]
    if sub > 1:
        s = np.clip(np.floor((f - u) * sub), 0, sub - 1).astype(np.int64)
        m = np.zeros(len(p), dtype=np.int64)
        for b in range(int(np.log2(sub))):
            for d in range(3):
                m |= ((s[:, d] >> b) & 1) << (3 * b + d)
        key = key * sub ** 3 + m
    return np.argsort(key, kind="stable")


def box_gap2(lo_a, hi_a, lo_b, hi_b):
    """Squared distance between boxes a (A, 3) and b (T, 3): (A, T)."""
    g = np.maximum(np.maximum(lo_b[None] - hi_a[:, None], lo_a[:, None] - hi_b[None]), 0.0)
    return (g * g).sum(-1)


def keep_masks(q, c, sub=1, group=GROUP):
    """(wave-passes, lane tiles) masks of the tiles a wave runs: under the current rule, under the true-distance rule."""
    q, c = q[curve_order(q, sub)], c[curve_order(c, sub)]
    nq, nc = len(q), len(c)
    assert nq % GROUP == 0 and nc % TILE == 0, "whole groups and lane tiles only"
    nt, nw = nc // TILE, nq // GROUP
    ct = c.reshape(nt, TILE, 3)
    tlo, thi = ct.min(1), ct.max(1)
    d2 = ((q * q).sum(1)[:, None] + (c * c).sum(1)[None]) - 2.0 * (q @ c.T)   # (nq, nc), Float64: exact enough to rank tiles
    tmin = np.maximum(d2, 0.0).reshape(nq, nt, TILE).min(2)                   # a query's nearest distance^2 inside every tile
    dtrue = tmin.min(1)
    ns = nq // group                                                          # (sub-)groups with a box and a bound of their own
    qs = q.reshape(ns, group, 3)
    bd = box_gap2(qs.min(1), qs.max(1), tlo, thi)                             # (ns, nt)
    todo0 = bd == 0.0
    none = ~todo0.any(1)
    todo0[none] = bd[none] == bd[none].min(1, keepdims=True)
    tq = tmin.reshape(ns, group, nt)
    bound0 = np.where(todo0[:, None, :], tq, np.inf).min(2)                   # (ns, group): after phase 0
    keep_cur = todo0 | (bd <= bound0.max(1)[:, None])
    keep_true = bd <= dtrue.reshape(ns, group).max(1)[:, None]
    per = GROUP // group                                                      # the wave runs what any of its sub-groups keeps
    return keep_cur.reshape(nw, per, nt).any(1), keep_true.reshape(nw, per, nt).any(1)


def tiles_kept(q, c, **kw):
    """Mean lane tiles kept per wave-pass: (current rule, true-distance rule, lane tiles of the cloud)."""
    cur, true = keep_masks(q, c, **kw)
    return cur.sum(1).mean(), true.sum(1).mean(), cur.shape[1]


def cloud(kind, rng, n):
    if kind == "uniform":
        return rng.random((n, 3))
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) if kind == "sphere" else v


VARIANTS = [("current", dict()), ("sub2", dict(sub=2)), ("sub4", dict(sub=4)), ("g16", dict(group=16)), ("g8", dict(group=8)),
            ("g4", dict(group=4))]


def table(n=4096, seeds=3):
    """{kind: {"tiles": lane tiles, variant: mean tiles kept, "true": ... under the true-distance rule}}"""
    out = {}
    for kind in ("uniform", "sphere", "gaussian"):
        acc = {}
        for s in range(seeds):
            rng = np.random.default_rng(1000 + s)
            q, c = cloud(kind, rng, n), cloud(kind, rng, n)
            for name, kw in VARIANTS:
                cur, true, nt = tiles_kept(q, c, **kw)
                acc.setdefault(name, []).append(cur)
                if name == "current":
                    acc.setdefault("true", []).append(true)
        out[kind] = {k: float(np.mean(v)) for k, v in acc.items()}
        out[kind]["tiles"] = nt
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=3)
    a = ap.parse_args()
    t = table(a.n, a.seeds)
    cols = ["current", "true", "sub2", "sub4", "g16", "g8", "g4"]
    print(f"lane tiles kept per wave-pass, {a.n} x {a.n} points, mean of {a.seeds} seeds")
    print(f"{'cloud':<10}{'tiles':>6}" + "".join(f"{c:>9}" for c in cols))
    for kind, r in t.items():
        print(f"{kind:<10}{r['tiles']:>6}" + "".join(f"{r[c]:>9.2f}" for c in cols))


if __name__ == "__main__":
    main()
