#!/usr/bin/env python3
"""stnKD(K) on the device (fx.stnKD, fx3d_stnkd_forward / fx3d_stnkd_forward_train): time per call at 32 x 1024 for K = 3, 6, 64
and 128, test mode and training mode, beside PointNet's own forward in the same run -- whose stn and fstn rounds are this layer at
K = 3 and K = 64 on kernels frozen at those widths.

Per workload: --rounds rounds of device events around --reps calls after a warm-up; the row gives the median round and the
spread (smallest and largest round), which is the run's own noise: two numbers closer than that are not told apart.  One JSON
line per workload.

Per kernel: run one workload alone under the kernel trace, which names every instantiation,

  rocprofv3 --kernel-trace --stats -d DIR -o r -- python tools/stnkd_time.py --trace 3        (or 6, 64, 128, pointnet)
  python tools/rocprof_summary.py stats DIR/r_results.db

pointnet_points_kernel<3, false> is the run-time-K point kernel; in the `pointnet` trace <0, false> is the stn round's (the same
work as K = 3) and <1, false> the fstn round's (conv_block1 in front of the work of K = 64); pointnet_head_kernel<false> is the
head of both (in the `pointnet` trace the mean of the (3, 3) and the (64, 64) head).  Tracing adds to the event times: the two
kinds of run are kept apart.

  python tools/stnkd_time.py [--reps 100] [--warmup 10] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flux3d_jl_amd as fx  # noqa: E402
import pointnet_ref as ref  # noqa: E402

N, B, NUM_CLASSES = 1024, 32, 40
KS = (3, 6, 64, 128)


def flop(K):
    """Algorithmic FLOP of one stnKD(K) forward at (N, B), 2 per multiply-add."""
    return 2 * ((K * 64 + 64 * 128 + 128 * 1024) * N * B + (1024 * 512 + 512 * 256 + 256 * K * K) * B)


def rounds_ms(call, reps, warmup, rounds):
    for _ in range(warmup):
        call()
    fx.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = fx.Event(), fx.Event()
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_ms(e1) / reps)
    return sorted(out)


def row(what, ms, **more):
    r = {"workload": what, "shape": f"{B} x {N}", "ms_per_call": round(ms[len(ms) // 2], 4), "smallest_round": round(ms[0], 4),
         "largest_round": round(ms[-1], 4), "spread_percent": round(100 * (ms[-1] - ms[0]) / ms[len(ms) // 2], 2)}
    r.update(more)
    print(json.dumps(r), flush=True)


def layer(K):
    """stnKD(K) with PointNet's own stn / fstn parameters where K is theirs, and its input on the device."""
    if K in (3, 64):
        m = fx.stnKD.from_pointnet(fx.PointNet(NUM_CLASSES).load(ref.random_params(NUM_CLASSES, seed=NUM_CLASSES)), "stn" if K == 3 else "fstn")
    else:
        m = fx.stnKD(K, seed=K)
    x = fx.gpu(np.asfortranarray(np.random.default_rng(K).standard_normal((K, N, B)).astype(np.float32)))
    return m, x


def pointnet():
    m = fx.PointNet(NUM_CLASSES).load(ref.random_params(NUM_CLASSES, seed=NUM_CLASSES))
    x = fx.gpu(np.asfortranarray(np.random.default_rng(2).standard_normal((3, N, B)).astype(np.float32)))
    return m, x


def trace(what, reps):
    """One workload alone, for the kernel trace: `reps` forwards, then (a layer) `reps` training-mode forwards."""
    if what == "pointnet":
        m, x = pointnet()
        for _ in range(reps):
            m(x)
    else:
        m, x = layer(int(what))
        for _ in range(reps):
            m(x)
        for _ in range(reps):
            m.forward_train(x)
    fx.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", default=None, help="run one workload alone: pointnet, or a K")
    a = ap.parse_args()
    assert fx.functional(), "stnkd_time.py needs a GPU"
    if a.trace is not None:
        return trace(a.trace, a.reps)
    pm, px = pointnet()
    row("PointNet forward", rounds_ms(lambda: pm(px), a.reps, a.warmup, a.rounds), library=os.path.basename(fx.LIB_PATH))
    for K in KS:
        m, x = layer(K)
        ms = rounds_ms(lambda: m(x), a.reps, a.warmup, a.rounds)
        row(f"stnKD({K}) forward", ms, GFLOP=round(flop(K) / 1e9, 3), TFLOPs=round(flop(K) / (ms[len(ms) // 2] * 1e-3) / 1e12, 2))
        row(f"stnKD({K}) forward_train", rounds_ms(lambda: m.forward_train(x), a.reps, a.warmup, a.rounds))
    row("PointNet forward, again", rounds_ms(lambda: pm(px), a.reps, a.warmup, a.rounds), library=os.path.basename(fx.LIB_PATH))


if __name__ == "__main__":
    main()
