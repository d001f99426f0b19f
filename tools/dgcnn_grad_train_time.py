#!/usr/bin/env python3
"""The DGCNN training-mode adjoint (fx.DGCNN.flat_grad_train, fx3d_dgcnn_grad_train) beside its yardsticks in the same run, 40
classes, at 32 x 1024 with K = 20 and at 2 x 64 with K = 10.

The yardsticks are existing kernels, never the code under test:
  conv_3's dense input gradient (dgcnn_gt_conv3_bwd) against dgcnn_conv3_stats_kernel of DGCNN.forward_train: the same tile and the
    same 256 x 1024 contraction; expected 2.0 x by MFMA count (the contraction plus the way back), allowed 1.25 x that;
  conv_3's dense dW (dgcnn_gt_conv3_pgrad) against one launch of pointnet_gt_last_pgrad_kernel of PointNet.grad_train at the same
    N x B (its three launches -- stn, fstn, feat -- are the same 128 x 1024 contraction; the label's sum over 3): expected 2.0 x for
    twice the input channels, allowed 1.25 x that;
  the two stage calls inside the new call against EdgeConv.flat_grad_train alone on the same arrays: the same kernels.

One process; --rounds rounds, each visiting both shapes in turn.  A visit has two parts, each with the library's own events around
the kernels' launches (fx3d_profile_enable), a label's figure being its sum per call.  Part one ALTERNATES DGCNN.grad,
DGCNN.forward_train, PointNet.grad_train and the new call (given the forward) call by call, --kreps of each: the only
edgeconv_grad_train_* launches in it are the new call's two stages.  Part two alternates the two stages' EdgeConv.flat_grad_train
alone on x1 / gx2 and X / gx1.  Then device events around --reps calls of the new entry, of DGCNN.grad and of
DGCNN.forward_train.  Reported per shape: medians over the rounds with min and max, and the ratios.  Before timing the new call
on the first two clouds is compared with the host restatement tests/dgcnn_grad_train_ref.py bit for bit.  One JSON line per
shape.  For a per-kernel table run it under `rocprofv3 --kernel-trace --stats -- python tools/dgcnn_grad_train_time.py` in a run of
its own.

  python tools/dgcnn_grad_train_time.py [--rounds 5] [--reps 10] [--kreps 10] [--warmup 3]
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
import dgcnn_grad_train_ref as gref  # noqa: E402
import dgcnn_ref  # noqa: E402
import pointnet_ref  # noqa: E402

NC = 40
SHAPES = ((1024, 32, 20), (64, 2, 10))   # N, B, K
TAIL = ("dgcnn_gt_argmax", "dgcnn_gt_head", "dgcnn_gt_conv3_bwd", "dgcnn_gt_conv3_pgrad", "dgcnn_gt_reduce")
STAGE = ("edgeconv_grad_train_sums_last", "edgeconv_grad_train_sums_3", "edgeconv_grad_train_sums_2", "edgeconv_grad_train_sums_1",
         "edgeconv_grad_train_finish", "edgeconv_grad_train_closing", "edgeconv_grad_train_reduce")
YARD = ("dgcnn_train_conv3_stats", "pointnet_gt_last_pgrad")


def label_ms(name, calls):
    """The label's launches of the visit, summed, per call (0 for a label that was not launched)."""
    avg, cnt = C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), None, None, C.byref(cnt))
    return avg.value * cnt.value / calls if cnt.value > 0 else 0.0


def profiled(calls, kreps, labels):
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(kreps):
        for call in calls:
            call()
    fx.synchronize()
    ms = {k: label_ms(k, kreps) for k in labels}
    _lib.call("fx3d_profile_enable", 0)
    return ms


def timed(call, reps):
    e0, e1 = fx.Event(), fx.Event()
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1) / reps


def visit(c, reps, kreps):
    ms = profiled((c["grad"], c["forward_train"], c["pointnet"], c["new"]), kreps, TAIL + STAGE + YARD)
    ms["stages_in_the_call"] = sum(ms.pop(k) for k in STAGE)
    alone = profiled((c["ec2"], c["ec1"]), kreps, STAGE)
    ms["stages_alone"] = sum(alone.values())
    ms["call"] = timed(c["new"], reps)
    ms["grad_call"] = timed(c["grad"], reps)
    ms["forward_train_call"] = timed(c["forward_train"], reps)
    return ms


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def setup(N, B, K, P, PP):
    dg = fx.DGCNN(NC, K, N).load(P)
    pn = fx.PointNet(NC).load(PP)
    rng = np.random.default_rng(2)
    X = np.asfortranarray(rng.standard_normal((3, N, B)).astype(np.float32))
    glogits = np.asfortranarray(rng.standard_normal((NC, B)).astype(np.float32))
    # the first two clouds against the restatement, bit for bit
    x0, g0 = fx.gpu(np.asfortranarray(X[:, :, :2])), fx.gpu(np.asfortranarray(glogits[:, :2]))
    f0 = dg.forward_train(x0, intermediates=True)
    got, gx = dg.flat_grad_train(x0, g0, fwd=f0)
    h0 = {k: ({n: w.to_host() for n, w in v.items()} if isinstance(v, dict) else v.to_host()) for k, v in f0.items()}
    G, wx, _, _ = gref.grad_train(X[:, :, :2], P, K, glogits[:, :2], h0)
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)  # noqa: E731
    same = bool(np.array_equal(bits(got.to_host()), bits(gref.flat(G))) and np.array_equal(bits(gx.to_host()), bits(wx)))
    print(json.dumps({"shape": f"{B} x {N}", "K": K, "first_two_clouds_equal_the_restatement_bit_for_bit": same}), flush=True)
    assert same
    xd, gd = fx.gpu(X), fx.gpu(glogits)
    fwd = dg.forward_train(xd, intermediates=True)
    test_fwd = dg.forward(xd, intermediates=True)
    pfwd = pn.forward_train(xd, intermediates=True)
    _, _, mid = dg.flat_grad_train(xd, gd, fwd=fwd, intermediates=True)
    own = lambda d, name: {k[len(name) + 1:]: v for k, v in d.items() if k.startswith(name + ".")}  # noqa: E731
    ec2 = fx.EdgeConv(gref.L2, K).load(own(P, "ec2"))
    ec1 = fx.EdgeConv(gref.L1, K).load(own(P, "ec1"))
    f2 = {"out": fwd["x2"], "idx": fwd["idx2"], "batch_stats": own(fwd["batch_stats"], "ec2")}
    f1 = {"out": fwd["x1"], "idx": fwd["idx1"], "batch_stats": own(fwd["batch_stats"], "ec1")}
    return {"new": lambda: dg.flat_grad_train(xd, gd, fwd=fwd), "grad": lambda: dg.flat_grad(xd, gd, fwd=test_fwd),
            "forward_train": lambda: dg.forward_train(xd), "pointnet": lambda: pn.flat_grad_train(xd, gd, fwd=pfwd),
            "ec2": lambda: ec2.flat_grad_train(fwd["x1"], mid["gx2"], fwd=f2), "ec1": lambda: ec1.flat_grad_train(xd, mid["gx1"], fwd=f1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert fx.functional(), "dgcnn_grad_train_time.py needs a GPU"
    P, PP = dgcnn_ref.random_params(NC, seed=NC), pointnet_ref.random_params(NC, seed=10)
    configs = [(shape, setup(*shape, P, PP)) for shape in SHAPES]
    for _, c in configs:
        for _ in range(a.warmup):
            for call in c.values():
                call()
    fx.synchronize()
    res = {}
    for _ in range(a.rounds):
        for shape, c in configs:
            for key, v in visit(c, a.reps, a.kreps).items():
                res.setdefault((shape, key), []).append(v)
    for shape, _ in configs:
        N, B, K = shape
        s = {k: summary(v) for (sh, k), v in res.items() if sh == shape}
        stats, pgrad = s["dgcnn_train_conv3_stats"]["median"], s["pointnet_gt_last_pgrad"]["median"] / 3
        print(json.dumps({"config": f"dgcnn_grad_train {B} x {N}, K = {K}, {NC} classes",
                          "tail_ms": {k: s[k] for k in TAIL},
                          "conv3_stats_kernel_ms": s["dgcnn_train_conv3_stats"],
                          "pointnet_last_pgrad_ms_per_launch": round(pgrad, 4),
                          "ratio_conv3_bwd_over_conv3_stats": round(s["dgcnn_gt_conv3_bwd"]["median"] / stats, 3),
                          "ratio_conv3_pgrad_over_pointnet_last_pgrad": round(s["dgcnn_gt_conv3_pgrad"]["median"] / pgrad, 3),
                          "expected_each": 2.0, "allowed_each": 2.5,
                          "stages_in_the_call_ms": s["stages_in_the_call"], "stages_alone_ms": s["stages_alone"],
                          "ratio_stages_in_the_call_over_alone": round(s["stages_in_the_call"]["median"] / s["stages_alone"]["median"], 3),
                          "grad_train_call_ms": s["call"], "grad_call_ms": s["grad_call"], "forward_train_call_ms": s["forward_train_call"],
                          "ratio_call_over_grad": round(s["call"]["median"] / s["grad_call"]["median"], 3),
                          "ratio_call_over_forward_train": round(s["call"]["median"] / s["forward_train_call"]["median"], 3)}), flush=True)


if __name__ == "__main__":
    main()
