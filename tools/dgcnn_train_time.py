#!/usr/bin/env python3
"""The DGCNN training-mode forward (fx.DGCNN.forward_train, fx3d_dgcnn_forward_train) beside the test-mode fx3d_dgcnn_forward of
the same shapes, in the same run: 32 x 1024 with K = 20 and 2 x 64 with K = 10, 40 classes, seeded dropout masks on the device.
Per EdgeConv stage the call runs one statistics pass per BatchNorm with its finishing kernel and the test-mode edgeconv_kernel
as the closing pass; conv_3 gets a statistics pass, a finishing kernel and the test-mode maxima kernel; the head is split at
its two BatchNorms with the dense statistics in between: 20 launches besides the two neighbour searches.

One process; --rounds rounds, each visiting every configuration in turn.  A visit takes, with the library's own events around
the kernels' launches (fx3d_profile_enable), --kreps forward calls and then --kreps training-mode calls in windows of their own;
a label's figure is the sum of its launches per call.  Then device events around --reps calls each of the forward and the new
call, alternating (time per call, profiling off).  Reported per configuration: medians over the rounds with min and max, each
stage's last-layer statistics pass over the unchanged closing kernel of the same stage in the same run (the yardstick), and the
whole call over DGCNN.forward.  The new call is first compared with the host restatement tests/dgcnn_train_ref.py on the 2 x 64
batch, bit for bit.  One JSON line per configuration.

  python tools/dgcnn_train_time.py [--rounds 5] [--reps 50] [--kreps 10] [--warmup 3]
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
import dgcnn_ref  # noqa: E402
import dgcnn_train_ref  # noqa: E402

NC = 40
SHAPES = ((32, 1024, 20), (2, 64, 10))   # (B, N, K)
FORWARD = ("knn", "dgcnn_edgeconv1", "dgcnn_edgeconv2", "dgcnn_conv3", "dgcnn_head")
# label -> what it is; launches per call: the two searches', 2, 1, 1, 1, 1, 1, 1, 1, 6, 3, 2
TRAIN = {"knn": "both neighbour searches",
         "dgcnn_train_ec1_stats": "EdgeConv1 statistics passes of bn1, bn2", "dgcnn_train_ec1_stats_last": "EdgeConv1 statistics pass of bn3",
         "dgcnn_train_ec1_closing": "EdgeConv1 closing pass",
         "dgcnn_train_ec2_stats": "EdgeConv2 statistics pass of bn1", "dgcnn_train_ec2_stats_last": "EdgeConv2 statistics pass of bn2",
         "dgcnn_train_ec2_closing": "EdgeConv2 closing pass",
         "dgcnn_train_conv3_stats": "conv_3 statistics pass", "dgcnn_train_conv3_closing": "conv_3 closing pass",
         "dgcnn_train_finish": "finishing kernels", "dgcnn_train_head": "head", "dgcnn_train_dense_stats": "dense statistics"}
CALLS = ("forward_call", "train_call")
BITWISE = ("logits", "x1", "x2", "pooled")


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert fx.functional(), "dgcnn_train_time.py needs a GPU"
    P = dgcnn_ref.random_params(NC, seed=1)
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)  # noqa: E731
    configs = []
    for B, N, K in SHAPES:
        m = fx.DGCNN(NC, K, N).load(P)
        X = np.asfortranarray(np.random.default_rng(2).standard_normal((3, N, B)).astype(np.float32))
        masks = fx.DGCNN.dropout_masks(B, seed=3)
        xd, md = fx.gpu(X), tuple(fx.gpu(k) for k in masks)
        if N * B <= 128:
            got = m.forward_train(xd, dropout=md, intermediates=True)
            want = dgcnn_train_ref.forward_train(X, P, K, dropout=masks)
            same = all(np.array_equal(bits(got[k].to_host()), bits(want[k])) for k in BITWISE + ("idx1", "idx2")) and all(
                np.array_equal(bits(got[s][k].to_host()), bits(want[s][k])) for s in ("batch_stats", "running") for k in want[s])
            print(json.dumps({"config": f"dgcnn_train {B} x {N}, K = {K}", "num_classes": NC,
                              "equals_the_restatement_bit_for_bit": bool(same)}), flush=True)
            assert same
        configs.append((f"{B} x {N}, K = {K}", (lambda m=m, xd=xd: m.forward(xd)),
                        (lambda m=m, xd=xd, md=md: m.forward_train(xd, dropout=md))))
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
        med = lambda k: s["train:" + k]["median"]  # noqa: E731
        call, fwd = s["train_call"]["median"], s["forward_call"]["median"]
        line = {"config": f"dgcnn_train {shape}", "num_classes": NC}
        line.update({k + "_ms_per_call": s[k] for k in keys if k not in CALLS})
        line.update({k + "_ms": s[k] for k in CALLS})
        line.update({"train_call_breakdown_ms": {TRAIN[k]: med(k) for k in TRAIN},
                     "ec1_stats_pass_of_bn3_over_ec1_closing_pass": round(med("dgcnn_train_ec1_stats_last") / med("dgcnn_train_ec1_closing"), 3),
                     "ec1_stats_passes_of_bn1_bn2_over_ec1_closing_pass": round(med("dgcnn_train_ec1_stats") / med("dgcnn_train_ec1_closing"), 3),
                     "ec2_stats_pass_of_bn2_over_ec2_closing_pass": round(med("dgcnn_train_ec2_stats_last") / med("dgcnn_train_ec2_closing"), 3),
                     "ec2_stats_pass_of_bn1_over_ec2_closing_pass": round(med("dgcnn_train_ec2_stats") / med("dgcnn_train_ec2_closing"), 3),
                     "conv3_stats_pass_over_conv3_closing_pass": round(med("dgcnn_train_conv3_stats") / med("dgcnn_train_conv3_closing"), 3),
                     "closing_passes_over_the_forward_s_own": {
                         "ec1": round(med("dgcnn_train_ec1_closing") / s["forward:dgcnn_edgeconv1"]["median"], 3),
                         "ec2": round(med("dgcnn_train_ec2_closing") / s["forward:dgcnn_edgeconv2"]["median"], 3)},
                     "ratio_train_call_over_forward_call": round(call / fwd, 3)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
