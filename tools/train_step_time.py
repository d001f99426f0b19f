#!/usr/bin/env python3
"""One training step of PointNet and DGCNN (train_step, include/flux3d_hip.h "Training step") beside its parts, in one process.

Per shape -- PointNet 32 x 1024 and 2 x 64, DGCNN 32 x 1024 with K = 20 and 2 x 64 with K = 10, 40 classes -- the eager
``train_step`` and the captured replay (fx.TrainStepGraph, dropout drawn on the device) beside ``forward_train``,
``flat_grad_train`` (forward given) and the existing ``crossentropy_grad_train`` on the same arrays.  Per kernel: fx3d_crossentropy,
fx3d_dropout_mask and fx3d_adam_step at the model's parameter count, the ADAM launches' algorithmic GB/s (28 bytes per element)
beside fx3d_momentum_step (20 bytes per element) at the same n and beside the 6.3 TB/s tools/hbm_roofline.py takes as achievable.

Every figure: device events on the stream around --reps calls after --warmup calls, the median over --rounds rounds with min and
max; the calls of a shape alternate within a round.  One JSON line per shape and one for the kernels; all of it also goes to
profiles/train_step_time.txt.

  python tools/train_step_time.py [--rounds 5] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flux3d_jl_amd as fx  # noqa: E402
from flux3d_jl_amd import _lib  # noqa: E402
import dgcnn_ref  # noqa: E402
import pointnet_ref  # noqa: E402

NC = 40
SHAPES = (("pointnet", 1024, 32, 0), ("pointnet", 64, 2, 0), ("dgcnn", 1024, 32, 20), ("dgcnn", 64, 2, 10))
HBM_ACHIEVABLE = 6300.0  # GB/s (tools/hbm_roofline.py, tools/ubench_hbm.hip)


def timed(call, reps, s=None):
    e0, e1 = fx.Event(), fx.Event()
    e0.record(s)
    for _ in range(reps):
        call()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_ms(e1) / reps


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def model_of(kind, N, K, seed):
    if kind == "pointnet":
        return fx.PointNet(NC).load(pointnet_ref.random_params(NC, seed=seed))
    return fx.DGCNN(NC, K, N).load(dgcnn_ref.random_params(NC, seed=seed))


def setup(kind, N, B, K):
    rng = np.random.default_rng(2)
    X = np.asfortranarray(rng.standard_normal((3, N, B)).astype(np.float32))
    labels = rng.integers(0, NC, B)
    glogits = np.asfortranarray(rng.standard_normal((NC, B)).astype(np.float32))
    parts, eager, replayed = model_of(kind, N, K, 10), model_of(kind, N, K, 10), model_of(kind, N, K, 10)
    xd, gd, yd = fx.gpu(X), fx.gpu(glogits), fx.gpu(labels.astype(np.int32))
    fwd = parts.forward_train(xd, intermediates=True)
    opt, counter = fx.ADAM(), fx.gpu(np.zeros(1, np.uint64))
    graph = fx.TrainStepGraph(replayed, fx.ADAM(), X, labels, seed=1)
    calls = {"train_step": lambda: eager.train_step(xd, yd, opt, dropout=("device", 1, counter)),
             "forward_train": lambda: parts.forward_train(xd),
             "flat_grad_train": lambda: parts.flat_grad_train(xd, gd, fwd=fwd),
             "crossentropy_grad_train": lambda: parts.crossentropy_grad_train(xd, labels)}
    return calls, graph, eager.param_count


def kernels(n, B, rounds, reps, warmup):
    """The three new kernels and fx3d_momentum_step at n elements / a (NC, B) problem, ms per call."""
    rng = np.random.default_rng(3)
    x, g, m, v = (fx.gpu(rng.standard_normal(n).astype(np.float32)) for _ in range(4))
    m2, v2 = fx.gpu(np.zeros(n, np.float32)), fx.gpu(np.zeros(n, np.float32))
    bp = fx.gpu(np.array([0.9, 0.999]))
    probs, labels = fx.gpu(np.full((NC, B), 1.0 / NC, np.float32)), fx.gpu(np.zeros(B, np.int32))
    gl, loss, counts = fx.DeviceArray.empty((NC, B), np.float32), fx.DeviceArray.empty((1,), np.float64), fx.DeviceArray.empty((2,), np.int32)
    mask = fx.DeviceArray.empty((512, B), np.float32)
    calls = {"adam_step": lambda: _lib.call("fx3d_adam_step", n, 1e-3, 0.9, 0.999, 1e-8, g.ptr, m2.ptr, v2.ptr, bp.ptr, x.ptr, None, None, 0, None),
             "momentum_step": lambda: _lib.call("fx3d_momentum_step", n, 0.9, 1e-3, g.ptr, v.ptr, m.ptr, None),
             "crossentropy": lambda: _lib.call("fx3d_crossentropy", probs.ptr, labels.ptr, NC, B, gl.ptr, loss.ptr, counts.ptr, None),
             "dropout_mask": lambda: _lib.call("fx3d_dropout_mask", mask.size, 0.5, 1, None, 0, mask.ptr, None)}
    for call in calls.values():
        for _ in range(warmup):
            call()
    fx.synchronize()
    res = {k: [] for k in calls}
    for _ in range(rounds):
        for k, call in calls.items():
            res[k].append(timed(call, reps))
    out = {k + "_ms": summary(v) for k, v in res.items()}
    out["adam_gbs"] = round(28 * n / (out["adam_step_ms"]["median"] * 1e-3) / 1e9, 1)
    out["momentum_gbs"] = round(20 * n / (out["momentum_step_ms"]["median"] * 1e-3) / 1e9, 1)
    out["hbm_achievable_gbs"] = HBM_ACHIEVABLE
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert fx.functional(), "train_step_time.py needs a GPU"
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    counts = {}
    for kind, N, B, K in SHAPES:
        calls, graph, counts[kind] = setup(kind, N, B, K)
        for call in calls.values():
            for _ in range(a.warmup):
                call()
        for _ in range(a.warmup):
            graph.step()
        fx.synchronize()
        graph.synchronize()
        res = {}
        for _ in range(a.rounds):
            for k, call in calls.items():
                res.setdefault(k, []).append(timed(call, a.reps))
            with fx.stream(graph.stream):
                res.setdefault("graph_replay", []).append(timed(graph.step, a.reps, graph.stream))
        s = {k + "_ms": summary(v) for k, v in res.items()}
        s["config"] = f"{kind} {B} x {N}" + (f", K = {K}" if K else "") + f", {NC} classes, {counts[kind]} parameters"
        s["ratio_train_step_over_forward_plus_grad"] = round(
            s["train_step_ms"]["median"] / (s["forward_train_ms"]["median"] + s["flat_grad_train_ms"]["median"]), 3)
        s["ratio_replay_over_train_step"] = round(s["graph_replay_ms"]["median"] / s["train_step_ms"]["median"], 3)
        emit(s)
        del calls, graph
    for kind, n in counts.items():
        k = kernels(n, 32, a.rounds, a.reps, a.warmup)
        k["config"] = f"kernels at {kind}'s {n} parameters, B = 32"
        emit(k)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "train_step_time.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
