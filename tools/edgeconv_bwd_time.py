#!/usr/bin/env python3
"""The EdgeConv input adjoint (fx.EdgeConv.input_grad, fx3d_edgeconv_bwd) against the forward of the same shape in the same
run, at 32 x 1024 with K = 20: DGCNN's two stages, [3, 32, 64, 64] and [64, 128, 256], on DGCNN's inputs and parameters, and
[64, 64, 128, 256].  The yardstick is the forward: the adjoint recomputes it and walks back, twice the forward's MFMA work
plus the weight transposes.

One process; --rounds rounds, each visiting every configuration in turn.  A visit ALTERNATES forward and adjoint call by call,
--kreps of each, with the library's own events around the two kernels' launches (fx3d_profile_enable: "edgeconv" and
"edgeconv_bwd"), so that both see the same clock and neighbours on the device.  The neighbour lists and the forward's output are
given to both, so a call is the kernel (the adjoint's call also launches its small weight transpose, which is outside the
bracket).  Then device events around --reps adjoint calls (time per call).  Reported per configuration: medians over the rounds
with min and max, and the ratio adjoint / forward of the kernel medians.  The adjoint is first compared with the host
restatement tests/edgeconv_bwd_ref.py on the first cloud, bit for bit.  One JSON line per configuration.  For a per-kernel
table run it under `rocprofv3 --kernel-trace --stats -- python tools/edgeconv_bwd_time.py` in a run of its own.

  python tools/edgeconv_bwd_time.py [--rounds 5] [--reps 10] [--kreps 10] [--warmup 3]
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
import edgeconv_bwd_ref  # noqa: E402
import edgeconv_ref  # noqa: E402

N, B, K, NC = 1024, 32, 20, 40


def kernel_ms(name):
    avg, cnt = C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), None, None, C.byref(cnt))
    assert cnt.value > 0, name
    return avg.value


def flop(layers):
    cins = [2 * layers[0]] + layers[1:-1]
    return 2 * sum(ci * co for ci, co in zip(cins, layers[1:])) * K * N * B


def visit(fwd, bwd, reps, kreps):
    """(forward kernel ms, adjoint kernel ms, adjoint ms per call) of one visit of a configuration."""
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(kreps):
        fwd()
        bwd()
    fx.synchronize()
    f_ms, b_ms = kernel_ms("edgeconv"), kernel_ms("edgeconv_bwd")
    _lib.call("fx3d_profile_enable", 0)
    e0, e1 = fx.Event(), fx.Event()
    e0.record()
    for _ in range(reps):
        bwd()
    e1.record()
    e1.synchronize()
    return f_ms, b_ms, e0.elapsed_ms(e1) / reps


def summary(values):
    med = statistics.median(values)
    return {"median": round(med, 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert fx.functional(), "edgeconv_bwd_time.py needs a GPU"
    P = dgcnn_ref.random_params(NC, seed=NC)
    dg = fx.DGCNN(NC, K, N).load(P)
    rng = np.random.default_rng(2)
    xd = fx.gpu(np.asfortranarray(rng.standard_normal((3, N, B)).astype(np.float32)))
    x1 = dg.forward(xd, intermediates=True)["x1"]
    own = lambda name: {k[len(name) + 1:]: v for k, v in P.items() if k.startswith(name + ".")}  # noqa: E731
    configs = []
    for layers, params, x in (([3, 32, 64, 64], own("ec1"), xd), ([64, 128, 256], own("ec2"), x1),
                              ([64, 64, 128, 256], edgeconv_ref.random_params([64, 64, 128, 256], seed=1), x1)):
        m = fx.EdgeConv(layers, K).load(params)
        out, idx = m.forward(x, return_idx=True)
        gout = np.asfortranarray(rng.standard_normal((layers[-1], N, B)).astype(np.float32))
        g = fx.gpu(gout)
        got = m.input_grad(x, g, idx, out).to_host()[:, :, :1]
        want = edgeconv_bwd_ref.input_grad(x.to_host()[:, :, :1], params, layers, K, gout[:, :, :1], idx.to_host()[:, :, :1],
                                           out.to_host()[:, :, :1])
        same = bool(np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)))
        print(json.dumps({"config": json.dumps(layers, separators=(",", ":")), "shape": f"{B} x {N}", "K": K,
                          "first_cloud_equals_the_restatement_bit_for_bit": same}), flush=True)
        assert same
        configs.append((layers, (lambda m=m, x=x, idx=idx: m.forward(x, idx=idx)),
                        (lambda m=m, x=x, g=g, idx=idx, out=out: m.input_grad(x, g, idx, out))))
    for _, fwd, bwd in configs:
        for _ in range(a.warmup):
            fwd()
            bwd()
    fx.synchronize()
    res = {}
    for _ in range(a.rounds):
        for layers, fwd, bwd in configs:
            for key, v in zip(("fwd", "bwd", "call"), visit(fwd, bwd, a.reps, a.kreps)):
                res.setdefault((str(layers), key), []).append(v)
    for layers, _, _ in configs:
        f, b = summary(res[(str(layers), "fwd")]), summary(res[(str(layers), "bwd")])
        print(json.dumps({"config": "edgeconv_bwd " + json.dumps(layers, separators=(",", ":")), "forward_kernel_ms": f,
                          "adjoint_kernel_ms": b, "adjoint_call_ms": summary(res[(str(layers), "call")]),
                          "ratio_adjoint_over_forward": round(b["median"] / f["median"], 3),
                          "forward_GFLOP": round(flop(layers) / 1e9, 3),
                          "adjoint_kernel_TFLOPs_at_twice_the_forward_flop": round(2 * flop(layers) / (b["median"] * 1e-3) / 1e12, 2)}),
              flush=True)


if __name__ == "__main__":
    main()
