#!/usr/bin/env python3
"""The PointNet training-mode adjoint (fx.PointNet.flat_grad_train, fx3d_pointnet_grad_train) beside its two neighbours, the
test-mode adjoint (flat_grad, fx3d_pointnet_grad) and the training-mode forward (forward_train), of the same shapes in the same
run: 32 x 1024 and 2 x 64, 40 classes.  The new call is given the batch statistics of a forward_train run once before the timing
(fwd=), so a call is fx3d_pointnet_grad_train plus the 26 small device copies that gather the statistics' views into one buffer.

One process; --rounds rounds, each visiting every configuration in turn.  A visit ALTERNATES the three calls, call by call,
--kreps of each, with the library's own events around the kernels' launches (fx3d_profile_enable), so that all see the same clock;
a label's figure is the average of its launches, times the label's launches per call (LAUNCHES).  Then device events around --reps
calls of each (time per call).  Reported per configuration: medians over the rounds with min and max, and the ratios.  The new call
is first compared with the host restatement tests/pointnet_grad_train_ref.py on the first two clouds, bit for bit.  One JSON line
per configuration.

  python tools/pointnet_grad_train_time.py [--rounds 5] [--reps 10] [--kreps 10] [--warmup 3]
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
import pointnet_grad_train_ref  # noqa: E402
import pointnet_ref  # noqa: E402

NC = 40
SHAPES = ((32, 1024), (2, 64))   # (B, N)
# the new call's labels and how many launches (groups of launches under one label) of each one call makes
LAUNCHES = {"pointnet_gt_head": 3, "pointnet_gt_last_bwd": 3, "pointnet_gt_last_pgrad": 3, "pointnet_gt_sums": 6,
            "pointnet_gt_finish": 6, "pointnet_gt_layer_bwd": 6, "pointnet_gt_reduce": 9}
KERNELS = tuple(LAUNCHES)
CALLS = ("grad_call", "forward_train_call", "grad_train_call")


def kernel_ms(name):
    avg, cnt = C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), None, None, C.byref(cnt))
    assert cnt.value > 0, name
    return avg.value


def per_call(fn, reps):
    e0, e1 = fx.Event(), fx.Event()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1) / reps


def visit(calls, reps, kreps):
    """The labels' ms per launch of one visit, then ms per call of the three calls."""
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(kreps):
        for fn in calls:
            fn()
    fx.synchronize()
    ms = [kernel_ms(k) for k in KERNELS]
    _lib.call("fx3d_profile_enable", 0)
    return ms + [per_call(f, reps) for f in calls]


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert fx.functional(), "pointnet_grad_train_time.py needs a GPU"
    P = pointnet_ref.random_params(NC, seed=NC)
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)  # noqa: E731
    configs = []
    for B, N in SHAPES:
        m = fx.PointNet(NC).load(P)
        rng = np.random.default_rng(2)
        X = np.asfortranarray(rng.standard_normal((3, N, B)).astype(np.float32))
        glogits = np.asfortranarray(rng.standard_normal((NC, B)).astype(np.float32))
        xd, gd = fx.gpu(X), fx.gpu(glogits)
        x0, g0 = np.asfortranarray(X[:, :, :2]), np.asfortranarray(glogits[:, :2])
        got, gx = m.flat_grad_train(fx.gpu(x0), fx.gpu(g0))
        G, wx, _ = pointnet_grad_train_ref.grad_train(x0, P, g0)
        same = bool(np.array_equal(bits(got.to_host()), bits(pointnet_grad_train_ref.flat(G)))
                    and np.array_equal(bits(gx.to_host()), bits(wx)))
        print(json.dumps({"config": f"pointnet_grad_train {B} x {N}", "num_classes": NC,
                          "first_two_clouds_equal_the_restatement_bit_for_bit": same}), flush=True)
        assert same
        fwd = m.forward_train(xd, intermediates=True)
        configs.append((f"{B} x {N}", ((lambda m=m, xd=xd, gd=gd: m.flat_grad(xd, gd)), (lambda m=m, xd=xd: m.forward_train(xd)),
                                       (lambda m=m, xd=xd, gd=gd, fwd=fwd: m.flat_grad_train(xd, gd, fwd=fwd)))))
    for _, calls in configs:
        for _ in range(a.warmup):
            for fn in calls:
                fn()
    fx.synchronize()
    res = {}
    for _ in range(a.rounds):
        for shape, calls in configs:
            for key, v in zip(KERNELS + CALLS, visit(calls, a.reps, a.kreps)):
                res.setdefault((shape, key), []).append(v)
    for shape, _ in configs:
        s = {k: summary(res[(shape, k)]) for k in KERNELS + CALLS}
        call = s["grad_train_call"]["median"]
        per = {k: round(LAUNCHES[k] * s[k]["median"], 4) for k in KERNELS}
        line = {"config": f"pointnet_grad_train {shape}", "num_classes": NC}
        line.update({k + "_ms_per_launch": s[k] for k in KERNELS})
        line.update({k + "_ms": s[k] for k in CALLS})
        line.update({"labels_ms_per_grad_train_call": per,
                     "largest_label_share_of_the_call": {max(per, key=per.get): round(max(per.values()) / call, 4)},
                     "ratio_grad_train_call_over_grad_call": round(call / s["grad_call"]["median"], 3),
                     "ratio_grad_train_call_over_forward_train_call": round(call / s["forward_train_call"]["median"], 3)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
