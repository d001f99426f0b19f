#!/usr/bin/env python3
"""EdgeConv(layers, K) on the device (fx.EdgeConv, fx3d_edgeconv_forward) at 32 x 1024 with K = 20: time per call (search +
kernel) and per kernel for DGCNN's two stages, [3, 32, 64, 64] and [64, 128, 256], on DGCNN's inputs and parameters, and for
one shape DGCNN never runs, [64, 64, 128, 256].  (fx3d_dgcnn_forward runs the same kernel; tools/dgcnn_time.py times it there.)

One process; --rounds rounds, each visiting every configuration in turn, so that they share whatever else the host and the
device are doing.  Per visit: device events around --reps unprofiled calls (time per call), then the library's own events
around each kernel's launch over --kreps calls (fx3d_profile_enable; time per kernel).  After a warm-up of every
configuration.  Reported per configuration: the median over the rounds and their spread (min, max).  The outputs of the two
DGCNN shapes are first compared with DGCNN's x1 / x2 bit for bit.  One JSON line per configuration.  For a per-kernel table
run it under `rocprofv3 --kernel-trace --stats -- python tools/edgeconv_time.py` in a run of its own (tracing adds to the
event times).

  python tools/edgeconv_time.py [--rounds 5] [--reps 20] [--kreps 10] [--warmup 3] [--no-third]
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
import edgeconv_ref  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
N, B, K, NC = 1024, 32, 20, 40


def kernel_ms(name):
    avg, cnt = C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), None, None, C.byref(cnt))
    assert cnt.value > 0, name
    return avg.value


def flop(layers):
    cins = [2 * layers[0]] + layers[1:-1]
    return 2 * sum(ci * co for ci, co in zip(cins, layers[1:])) * K * N * B


def visit(run, reps, kreps):
    """(ms per call, ms per kernel launch) of one visit of a configuration."""
    e0, e1 = fx.Event(), fx.Event()
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    e1.synchronize()
    call_ms = e0.elapsed_ms(e1) / reps
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(kreps):
        run()
    fx.synchronize()
    ms = kernel_ms("edgeconv")
    _lib.call("fx3d_profile_enable", 0)
    return call_ms, ms


def summary(values):
    med = statistics.median(values)
    return {"median": round(med, 4), "min": round(min(values), 4), "max": round(max(values), 4),
            "spread": round((max(values) - min(values)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-third", action="store_true", help="leave [64, 64, 128, 256] out: it runs the instantiation of "
                    "[64, 128, 256], and a kernel trace groups by kernel name")
    a = ap.parse_args()
    assert fx.functional(), "edgeconv_time.py needs a GPU"
    P = dgcnn_ref.random_params(NC, seed=NC)
    dg = fx.DGCNN(NC, K, N).load(P)
    xd = fx.gpu(np.asfortranarray(np.random.default_rng(2).standard_normal((3, N, B)).astype(np.float32)))
    inter = dg.forward(xd, intermediates=True)
    x1 = inter["x1"]
    L1, L2, L3 = [3, 32, 64, 64], [64, 128, 256], [64, 64, 128, 256]
    own = lambda name: {k[len(name) + 1:]: v for k, v in P.items() if k.startswith(name + ".")}  # noqa: E731
    e1 = fx.EdgeConv(L1, K).load(own("ec1"))
    e2 = fx.EdgeConv(L2, K).load(own("ec2"))
    e3 = fx.EdgeConv(L3, K).load(edgeconv_ref.random_params(L3, seed=1))
    same = (np.array_equal(e1(xd).to_host().view(np.uint32), x1.to_host().view(np.uint32))
            and np.array_equal(e2(x1).to_host().view(np.uint32), inter["x2"].to_host().view(np.uint32)))
    print(json.dumps({"shape": f"{B} x {N}", "K": K, "outputs_equal_dgcnn_x1_x2_bit_for_bit": bool(same)}), flush=True)
    assert same
    configs = [(L1, lambda: e1(xd)), (L2, lambda: e2(x1)), (L3, lambda: e3(x1))][:2 if a.no_third else 3]
    for _, run in configs:
        for _ in range(a.warmup):
            run()
    fx.synchronize()
    calls, kern = {}, {}
    for _ in range(a.rounds):
        for layers, run in configs:
            call_ms, ms = visit(run, a.reps, a.kreps)
            calls.setdefault(str(layers), []).append(call_ms)
            kern.setdefault(str(layers), []).append(ms)
    for layers, _ in configs:
        k = summary(kern[str(layers)])
        print(json.dumps({"config": "edgeconv " + json.dumps(layers, separators=(",", ":")), "kernel_ms": k,
                          "call_ms_search_and_kernel": summary(calls[str(layers)]), "GFLOP": round(flop(layers) / 1e9, 3),
                          "kernel_TFLOPs": round(flop(layers) / (k["median"] * 1e-3) / 1e12, 2),
                          "kernel_share_of_f32_matrix_peak": round(flop(layers) / (k["median"] * 1e-3) / PEAK_F32_MATRIX, 4)}),
              flush=True)


if __name__ == "__main__":
    main()
