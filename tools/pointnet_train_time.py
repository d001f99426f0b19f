#!/usr/bin/env python3
"""The PointNet training-mode forward (fx.PointNet.forward_train, fx3d_pointnet_forward_train) beside the test-mode
fx3d_pointnet_forward of the same shapes, in the same run: 32 x 1024 and 2 x 64, 40 classes, a seeded dropout mask on the device.
Per round (stn, fstn, feat) the call runs one statistics pass per point BatchNorm with its finishing kernel, the test-mode point
kernel as the closing pass, and the heads split at their BatchNorms with the dense statistics in between: 32 launches.

One process; --rounds rounds, each visiting every configuration in turn.  A visit takes, with the library's own events around
the kernels' launches (fx3d_profile_enable), --kreps forward calls and then --kreps training-mode calls in windows of their own
(the closing passes carry the point kernel's label, so the two calls cannot share a window); a label's figure is the sum of its
launches per call.  Then device events around --reps calls each of the forward and the new call, alternating (time per call,
profiling off).  Reported per configuration: medians over the rounds with min and max, and the ratio.  The new call is first
compared with the host restatement tests/pointnet_train_ref.py on the 2 x 64 batch, bit for bit.  One JSON line per configuration.

  python tools/pointnet_train_time.py [--rounds 5] [--reps 200] [--kreps 20] [--warmup 5]
"""
import argparse
import ctypes as C
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
import pointnet_ref  # noqa: E402
import pointnet_train_ref  # noqa: E402

NC = 40
SHAPES = ((32, 1024), (2, 64))   # (B, N)
FORWARD = ("pointnet_points", "pointnet_head")
# label -> what it is; launches per call: 6, 3, 9, 3, 7, 4
TRAIN = {"pointnet_train_stats": "statistics passes below the 1024-channel layer", "pointnet_train_stats_last": "statistics passes of the 1024-channel layer",
         "pointnet_train_finish": "finishing kernels", "pointnet_points": "closing passes", "pointnet_train_head": "heads",
         "pointnet_train_dense_stats": "dense statistics"}
CALLS = ("forward_call", "train_call")


def label_ms_per_call(name, calls):
    avg, cnt = C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), None, None, C.byref(cnt))
    assert cnt.value > 0 and cnt.value % calls == 0, (name, cnt.value)
    return avg.value * cnt.value / calls


def per_call(fn, reps):
    e0, e1 = fx.Event(), fx.Event()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1) / reps


def visit(fwd, train, reps, kreps):
    """ms per call of every label of one visit (the forward's, then the new call's), then ms per call of the two calls."""
    ms = []
    for fn, labels in ((fwd, FORWARD), (train, tuple(TRAIN))):
        _lib.call("fx3d_profile_enable", 1)
        for _ in range(kreps):
            fn()
        fx.synchronize()
        ms += [label_ms_per_call(k, kreps) for k in labels]
        _lib.call("fx3d_profile_enable", 0)
    return ms + [per_call(f, reps) for f in (fwd, train)]


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--kreps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert fx.functional(), "pointnet_train_time.py needs a GPU"
    P = pointnet_ref.random_params(NC, seed=NC)
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)  # noqa: E731
    configs = []
    for B, N in SHAPES:
        m = fx.PointNet(NC).load(P)
        X = np.asfortranarray(np.random.default_rng(2).standard_normal((3, N, B)).astype(np.float32))
        mask = fx.PointNet.dropout_mask(B, seed=3)
        xd, md = fx.gpu(X), fx.gpu(mask)
        if N * B <= 128:
            got = m.forward_train(xd, dropout=md, intermediates=True)
            want = pointnet_train_ref.forward_train(X, P, dropout=mask)
            same = all(np.array_equal(bits(got[k].to_host()), bits(want[k])) for k in ("logits", "stn", "fstn", "pooled")) and all(
                np.array_equal(bits(got[s][k].to_host()), bits(want[s][k])) for s in ("batch_stats", "running") for k in want[s])
            print(json.dumps({"config": f"pointnet_train {B} x {N}", "num_classes": NC,
                              "equals_the_restatement_bit_for_bit": bool(same)}), flush=True)
            assert same
        configs.append((f"{B} x {N}", (lambda m=m, xd=xd: m.forward(xd)), (lambda m=m, xd=xd, md=md: m.forward_train(xd, dropout=md))))
    for _, fwd, train in configs:
        for _ in range(a.warmup):
            fwd()
            train()
    fx.synchronize()
    keys = tuple("forward:" + k for k in FORWARD) + tuple("train:" + k for k in TRAIN) + CALLS
    res = {}
    for _ in range(a.rounds):
        for shape, fwd, train in configs:
            for key, v in zip(keys, visit(fwd, train, a.reps, a.kreps)):
                res.setdefault((shape, key), []).append(v)
    for shape, _, _ in configs:
        s = {k: summary(res[(shape, k)]) for k in keys}
        call, fwd = s["train_call"]["median"], s["forward_call"]["median"]
        line = {"config": f"pointnet_train {shape}", "num_classes": NC}
        line.update({k + "_ms_per_call": s[k] for k in keys if k not in CALLS})
        line.update({k + "_ms": s[k] for k in CALLS})
        line.update({"train_call_breakdown_ms": {TRAIN[k]: s["train:" + k]["median"] for k in TRAIN},
                     "stats_pass_of_the_1024_layer_over_closing_pass": round(
                         s["train:pointnet_train_stats_last"]["median"] / s["train:pointnet_points"]["median"], 3),
                     "ratio_train_call_over_forward_call": round(call / fwd, 3)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
