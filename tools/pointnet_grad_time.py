#!/usr/bin/env python3
"""The PointNet adjoint (fx.PointNet.flat_grad, fx3d_pointnet_grad) beside fx3d_pointnet_forward of the same shapes, in the same
run: 32 x 1024 and 2 x 64, 40 classes.  The call runs the forward's three rounds itself (with the winners per tile), then per
round the head's adjoint, the trunk's adjoint, the last convolution's sums, the head's sums over the clouds and the chains over
the tile partials.

One process; --rounds rounds, each visiting every configuration in turn.  A visit ALTERNATES the forward and the new call, call
by call, --kreps of each, with the library's own events around the kernels' launches (fx3d_profile_enable), so that both see the
same clock; a label's figure is the average of its launches (three per call: one per round of the network; the head's sums and the
chains over the partials are several small launches under one label each).  Then device events around --reps calls each of the
forward and the new call (time per call).  Reported per configuration: medians over the rounds with min and max, and the ratios.
The new call is first compared with the host restatement tests/pointnet_grad_ref.py on the first cloud, bit for bit.  One JSON
line per configuration.

  python tools/pointnet_grad_time.py [--rounds 5] [--reps 10] [--kreps 10] [--warmup 3]
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
import pointnet_grad_ref  # noqa: E402
import pointnet_ref  # noqa: E402

NC = 40
SHAPES = ((32, 1024), (2, 64))   # (B, N)
ADJOINT = ("pointnet_points_win", "pointnet_head_bwd", "pointnet_trunk_bwd", "pointnet_conv3_pgrad", "pointnet_head_pgrad",
           "pointnet_grad_reduce")   # three launches (groups of launches) of each per call
KERNELS = ("pointnet_points", "pointnet_head") + ADJOINT
CALLS = ("forward_call", "grad_call")


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


def visit(fwd, grad, reps, kreps):
    """The labels' ms per launch of one visit, then ms per call of the two calls."""
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(kreps):
        fwd()
        grad()
    fx.synchronize()
    ms = [kernel_ms(k) for k in KERNELS]
    _lib.call("fx3d_profile_enable", 0)
    return ms + [per_call(f, reps) for f in (fwd, grad)]


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert fx.functional(), "pointnet_grad_time.py needs a GPU"
    P = pointnet_ref.random_params(NC, seed=NC)
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)  # noqa: E731
    configs = []
    for B, N in SHAPES:
        m = fx.PointNet(NC).load(P)
        rng = np.random.default_rng(2)
        X = np.asfortranarray(rng.standard_normal((3, N, B)).astype(np.float32))
        glogits = np.asfortranarray(rng.standard_normal((NC, B)).astype(np.float32))
        xd, gd = fx.gpu(X), fx.gpu(glogits)
        x0, g0 = np.asfortranarray(X[:, :, :1]), np.asfortranarray(glogits[:, :1])
        got, gx = m.flat_grad(fx.gpu(x0), fx.gpu(g0))
        G, wx, _ = pointnet_grad_ref.grad(x0, P, g0)
        same = bool(np.array_equal(bits(got.to_host()), bits(pointnet_grad_ref.flat(G))) and np.array_equal(bits(gx.to_host()), bits(wx)))
        print(json.dumps({"config": f"pointnet_grad {B} x {N}", "num_classes": NC,
                          "first_cloud_equals_the_restatement_bit_for_bit": same}), flush=True)
        assert same
        configs.append((f"{B} x {N}", (lambda m=m, xd=xd: m.forward(xd)), (lambda m=m, xd=xd, gd=gd: m.flat_grad(xd, gd))))
    for _, fwd, grad in configs:
        for _ in range(a.warmup):
            fwd()
            grad()
    fx.synchronize()
    res = {}
    for _ in range(a.rounds):
        for shape, fwd, grad in configs:
            for key, v in zip(KERNELS + CALLS, visit(fwd, grad, a.reps, a.kreps)):
                res.setdefault((shape, key), []).append(v)
    for shape, _, _ in configs:
        s = {k: summary(res[(shape, k)]) for k in KERNELS + CALLS}
        call, fwd = s["grad_call"]["median"], s["forward_call"]["median"]
        heads = 3 * s["pointnet_head_bwd"]["median"]
        line = {"config": f"pointnet_grad {shape}", "num_classes": NC}
        line.update({k + "_ms_per_launch": s[k] for k in KERNELS})
        line.update({k + "_ms": s[k] for k in CALLS})
        line.update({"labels_ms_per_grad_call": {k: round(3 * s[k]["median"], 4) for k in ADJOINT},
                     "head_adjoints_share_of_the_grad_call": round(heads / call, 4),
                     "ratio_grad_call_over_forward_call": round(call / fwd, 3)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
