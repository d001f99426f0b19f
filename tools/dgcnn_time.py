#!/usr/bin/env python3
"""DGCNN inference on the device (fx.DGCNN, fx3d_dgcnn_forward): time per forward and per kernel at 32 x 1024 with K = 20 and
at 2 x 64 with K = 10, 40 classes, beside the same network in float32 with torch eager on the same device in the same call
(neighbours by cdist + topk; tests/dgcnn_torch_eval.py).

Per shape: device events around --reps forwards after a warm-up (time per forward), the library's own events around each
kernel's launches (fx3d_profile_enable: two neighbour searches, the two EdgeConv kernels, conv_3 and the head per forward),
the algorithmic FLOP of the layer table (2 FLOP per multiply-add: per edge row 6->32->64->64 and 128->128->256, per point
256->1024, per cloud the dense head; the searches are not counted) and its share of the 157.3 TFLOP/s Float32 matrix peak,
and torch's time for the same layers (figure, not target: torch's sums are not pinned to an order, and its float32 search
may break a near-tie the other way).  One JSON line per shape.  For the per-kernel table run it under
`rocprofv3 --kernel-trace --stats -- python tools/dgcnn_time.py` in a run of its own (tracing adds to the event times).

  python tools/dgcnn_time.py [--reps 50] [--warmup 5] [--no-torch]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flux3d_jl_amd as fx  # noqa: E402
from flux3d_jl_amd import _lib  # noqa: E402
import dgcnn_ref as ref  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
KERNELS = ("knn", "dgcnn_edgeconv1", "dgcnn_edgeconv2", "dgcnn_conv3", "dgcnn_head")


def flop(N, B, K, nc):
    per_edge = 6 * 32 + 32 * 64 + 64 * 64 + 128 * 128 + 128 * 256   # multiply-adds per (point, neighbour)
    per_point = 256 * 1024
    per_cloud = 1024 * 512 + 512 * 256 + 256 * nc
    return 2 * ((per_edge * K + per_point) * N * B + per_cloud * B)


def kernel_stats(name):
    avg, mn, mx, cnt = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), C.byref(mn), C.byref(mx), C.byref(cnt))
    return avg.value, cnt.value


def torch_forward_ms(X, P, K, reps, warmup):
    """tests/dgcnn_torch_eval.py in float32 on the device, eager: (ms per forward, probabilities (num_classes, B))."""
    try:
        import torch
    except ImportError:
        return None
    if not torch.cuda.is_available():
        return None
    import dgcnn_torch_eval
    out, run = dgcnn_torch_eval.forward(X, P, K, torch.float32, device="cuda", softmax=True)
    with torch.no_grad():
        for _ in range(warmup):
            out = run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            out = run()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out.cpu().numpy()


def measure(N, B, K, nc, reps, warmup, with_torch):
    P = ref.random_params(nc, seed=nc)
    m = fx.DGCNN(nc, K, N).load(P)
    X = np.asfortranarray(np.random.default_rng(2).standard_normal((3, N, B)).astype(np.float32))
    xd = fx.gpu(X)
    for _ in range(warmup):
        probs = m(xd)
    fx.synchronize()
    e0, e1 = fx.Event(), fx.Event()
    e0.record()
    for _ in range(reps):
        probs = m(xd)
    e1.record()
    e1.synchronize()
    fwd_ms = e0.elapsed_ms(e1) / reps
    _lib.call("fx3d_profile_enable", 1)
    n_prof = min(reps, 20)
    for _ in range(n_prof):
        m(xd)
    fx.synchronize()
    stats = {k: kernel_stats(k) for k in KERNELS}
    _lib.call("fx3d_profile_enable", 0)
    total = flop(N, B, K, nc)
    row = {"shape": f"{B} x {N}", "K": K, "num_classes": nc, "forward_ms": round(fwd_ms, 4)}
    for k, (avg, cnt) in stats.items():
        row[f"{k}_ms_per_forward"] = round(avg * cnt / n_prof, 4)   # (knn: both searches)
    row.update({"kernels_ms_per_forward": round(sum(avg * cnt for avg, cnt in stats.values()) / n_prof, 4),
                "GFLOP": round(total / 1e9, 3), "TFLOPs": round(total / (fwd_ms * 1e-3) / 1e12, 2),
                "share_of_f32_matrix_peak": round(total / (fwd_ms * 1e-3) / PEAK_F32_MATRIX, 4),
                "floor_us_at_peak": round(total / PEAK_F32_MATRIX * 1e6, 1)})
    if with_torch:
        t = torch_forward_ms(X, P, K, reps, warmup)
        if t is None:
            row["torch_eager_f32_forward_ms"] = None  # torch is missing or sees no device in this environment
        else:
            row["torch_eager_f32_forward_ms"] = round(t[0], 4)
            row["max_abs_probability_difference_to_torch"] = float(np.max(np.abs(t[1] - probs.to_host())))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert fx.functional(), "dgcnn_time.py needs a GPU"
    for N, B, K in ((1024, 32, 20), (64, 2, 10)):
        measure(N, B, K, 40, a.reps, a.warmup, not a.no_torch)


if __name__ == "__main__":
    main()
