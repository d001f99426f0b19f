#!/usr/bin/env python3
"""The DGCNN adjoint (fx.DGCNN.flat_grad, fx3d_dgcnn_grad) beside fx3d_dgcnn_forward and the two fx3d_edgeconv_grad calls of the
same shapes, in the same run: 32 x 1024 with K = 20 and 40 classes, and 2 x 64 with K = 10.  What is new in the call is its tail
-- the argmax recomputation of conv_3, the head's adjoint, the two gathers, the sums over the clouds --; the yardsticks are the
forward's conv_3 kernel, which the recomputation repeats with a compare in place of the maximum, and the forward itself.

One process; --rounds rounds, each visiting every configuration in turn.  A visit ALTERNATES the forward, the two stages' own
fx3d_edgeconv_grad calls and the new call (given the forward's intermediates, with gx) call by call, --kreps of each, with the
library's own events around the kernels' launches (fx3d_profile_enable), so that all see the same clock.  Then device events
around --reps calls each of the forward, the two EdgeConv.flat_grad calls together, and the new call with and without the
forward's intermediates (time per call).  Reported per configuration: medians over the rounds with min and max, and the ratios.
The new call is first compared with the host restatement tests/dgcnn_grad_ref.py on the first cloud, bit for bit.  One JSON line
per configuration.

  python tools/dgcnn_grad_time.py [--rounds 5] [--reps 10] [--kreps 10] [--warmup 3]
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
import dgcnn_grad_ref  # noqa: E402
import dgcnn_ref  # noqa: E402

NC = 40
SHAPES = ((32, 1024, 20), (2, 64, 10))   # (B, N, K)
TAIL = ("dgcnn_argmax", "dgcnn_head_bwd", "dgcnn_gx2", "dgcnn_conv3_pgrad", "dgcnn_dense_pgrad")
KERNELS = ("dgcnn_conv3", "dgcnn_head") + TAIL + ("edgeconv_pgrad", "edgeconv_pgrad_finish")
CALLS = ("forward_call", "two_edgeconv_grad_calls", "grad_call_given_the_forward", "grad_call_with_its_own_forward")


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


def visit(fwd, stages, grad, alone, reps, kreps):
    """The kernels' ms of one visit (the forward's conv_3 and head, the tail's five, the parameter adjoint's two: the average of
    a launch over both stages), then ms per call of the four calls."""
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(kreps):
        fwd()
        stages()
        grad()
    fx.synchronize()
    ms = [kernel_ms(k) for k in KERNELS]
    _lib.call("fx3d_profile_enable", 0)
    return ms + [per_call(f, reps) for f in (fwd, stages, grad, alone)]


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert fx.functional(), "dgcnn_grad_time.py needs a GPU"
    P = dgcnn_ref.random_params(NC, seed=NC)
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)  # noqa: E731
    configs = []
    for B, N, K in SHAPES:
        dg = fx.DGCNN(NC, K, N).load(P)
        rng = np.random.default_rng(2)
        xd = fx.gpu(np.asfortranarray(rng.standard_normal((3, N, B)).astype(np.float32)))
        glogits = np.asfortranarray(rng.standard_normal((NC, B)).astype(np.float32))
        gd = fx.gpu(glogits)
        f = dg.forward(xd, intermediates=True)
        # the first cloud against the restatement, fed the device's own forward
        one = {k: np.asfortranarray(v.to_host()[..., :1]) for k, v in f.items()}
        x0 = np.asfortranarray(xd.to_host()[:, :, :1])
        got, gx = dg.flat_grad(fx.gpu(x0), fx.gpu(np.asfortranarray(glogits[:, :1])), fwd={k: fx.gpu(v) for k, v in one.items()})
        G, wx, _, _ = dgcnn_grad_ref.grad(x0, P, K, glogits[:, :1], one)
        same = bool(np.array_equal(bits(got.to_host()), bits(dgcnn_grad_ref.flat(G))) and np.array_equal(bits(gx.to_host()), bits(wx)))
        print(json.dumps({"config": f"dgcnn_grad {B} x {N}", "K": K, "num_classes": NC,
                          "first_cloud_equals_the_restatement_bit_for_bit": same}), flush=True)
        assert same
        _, _, mid = dg.flat_grad(xd, gd, fwd=f, intermediates=True)
        ec1 = fx.EdgeConv(dgcnn_grad_ref.L1, K).load(dgcnn_grad_ref.stage_params(P, "ec1"))
        ec2 = fx.EdgeConv(dgcnn_grad_ref.L2, K).load(dgcnn_grad_ref.stage_params(P, "ec2"))

        def stages(ec1=ec1, ec2=ec2, xd=xd, f=f, mid=mid):
            ec2.flat_grad(f["x1"], mid["gx2"], f["idx2"], f["x2"])
            ec1.flat_grad(xd, mid["gx1"], f["idx1"], f["x1"])

        configs.append((f"{B} x {N}", K, (lambda dg=dg, xd=xd: dg.forward(xd, intermediates=True)), stages,
                        (lambda dg=dg, xd=xd, gd=gd, f=f: dg.flat_grad(xd, gd, fwd=f)),
                        (lambda dg=dg, xd=xd, gd=gd: dg.flat_grad(xd, gd))))
    for _, _, fwd, stages, grad, alone in configs:
        for _ in range(a.warmup):
            fwd()
            stages()
            grad()
            alone()
    fx.synchronize()
    res = {}
    for _ in range(a.rounds):
        for shape, _, fwd, stages, grad, alone in configs:
            for key, v in zip(KERNELS + CALLS, visit(fwd, stages, grad, alone, a.reps, a.kreps)):
                res.setdefault((shape, key), []).append(v)
    for shape, K, _, _, _, _ in configs:
        s = {k: summary(res[(shape, k)]) for k in KERNELS + CALLS}
        tail = sum(s[k]["median"] for k in TAIL)
        call = s["grad_call_given_the_forward"]["median"]
        line = {"config": f"dgcnn_grad {shape}", "K": K, "num_classes": NC}
        line.update({k + "_kernel_ms": s[k] for k in KERNELS})
        line.update({k + "_ms": s[k] for k in CALLS})
        line.update({"tail_kernels_ms": round(tail, 4),
                     "ratio_argmax_recomputation_over_forward_conv3_kernel": round(s["dgcnn_argmax"]["median"] / s["dgcnn_conv3"]["median"], 3),
                     "tail_share_of_the_grad_call": round(tail / call, 4),
                     "ratio_grad_call_over_forward_call": round(call / s["forward_call"]["median"], 3),
                     "ratio_grad_call_over_two_edgeconv_grad_calls": round(call / s["two_edgeconv_grad_calls"]["median"], 3)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
