#!/usr/bin/env python3
"""The EdgeConv parameter adjoint (fx.EdgeConv.flat_grad, fx3d_edgeconv_grad) against the input adjoint and the forward of the
same shape in the same run, at 32 x 1024 with K = 20: DGCNN's two stages, [3, 32, 64, 64] and [64, 128, 256], on DGCNN's inputs
and parameters, and [64, 64, 128, 256].  The yardstick is the input adjoint: the new kernel is its chain plus the contraction
of every layer's upstream gradient with the layer's input, 3/2 of its MFMA work, times the passes over the tile list.

One process; --rounds rounds, each visiting every configuration in turn.  A visit ALTERNATES forward, input adjoint and the new
call (with gx) call by call, --kreps of each, with the library's own events around the kernels' launches (fx3d_profile_enable:
"edgeconv", "edgeconv_bwd", "edgeconv_pgrad" and "edgeconv_pgrad_finish", the two finishing kernels together), so that all see
the same clock.  The neighbour lists and the forward's output are given to all three, so a call is its kernels (and the small
weight transpose, outside the brackets).  Then device events around --reps calls of the new entry (time per call).  Reported
per configuration: medians over the rounds with min and max, and the ratios.  The new call is first compared with the host
restatement tests/edgeconv_pgrad_ref.py on the first cloud, bit for bit.  One JSON line per configuration.  For a per-kernel
table run it under `rocprofv3 --kernel-trace --stats -- python tools/edgeconv_pgrad_time.py` in a run of its own.

  python tools/edgeconv_pgrad_time.py [--rounds 5] [--reps 10] [--kreps 10] [--warmup 3]
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
import edgeconv_pgrad_ref  # noqa: E402
import edgeconv_ref  # noqa: E402

N, B, K, NC = 1024, 32, 20, 40
KERNELS = ("edgeconv", "edgeconv_bwd", "edgeconv_pgrad", "edgeconv_pgrad_finish")


def kernel_ms(name):
    avg, cnt = C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), None, None, C.byref(cnt))
    assert cnt.value > 0, name
    return avg.value


def visit(fwd, bwd, grad, reps, kreps):
    """(forward, input adjoint, new kernel, finishing kernels: kernel ms; the new call: ms per call) of one visit."""
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(kreps):
        fwd()
        bwd()
        grad()
    fx.synchronize()
    ms = [kernel_ms(k) for k in KERNELS]
    _lib.call("fx3d_profile_enable", 0)
    e0, e1 = fx.Event(), fx.Event()
    e0.record()
    for _ in range(reps):
        grad()
    e1.record()
    e1.synchronize()
    return ms + [e0.elapsed_ms(e1) / reps]


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert fx.functional(), "edgeconv_pgrad_time.py needs a GPU"
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
        one = lambda v: np.asfortranarray(v.to_host()[:, :, :1])  # noqa: E731
        x0, g0, i0, o0 = fx.gpu(one(x)), fx.gpu(np.asfortranarray(gout[:, :, :1])), fx.gpu(one(idx)), fx.gpu(one(out))
        got, gx = m.flat_grad(x0, g0, i0, o0)
        G, wx = edgeconv_pgrad_ref.grad(one(x), params, layers, K, gout[:, :, :1], one(idx), one(out))
        bits = lambda v: np.ascontiguousarray(v).view(np.uint32)  # noqa: E731
        same = bool(np.array_equal(bits(got.to_host()), bits(edgeconv_pgrad_ref.flat(G, layers)))
                    and np.array_equal(bits(gx.to_host()), bits(wx)))
        print(json.dumps({"config": json.dumps(layers, separators=(",", ":")), "shape": f"{B} x {N}", "K": K,
                          "first_cloud_equals_the_restatement_bit_for_bit": same}), flush=True)
        assert same
        configs.append((layers, (lambda m=m, x=x, idx=idx: m.forward(x, idx=idx)),
                        (lambda m=m, x=x, g=g, idx=idx, out=out: m.input_grad(x, g, idx, out)),
                        (lambda m=m, x=x, g=g, idx=idx, out=out: m.flat_grad(x, g, idx, out))))
    for _, fwd, bwd, grad in configs:
        for _ in range(a.warmup):
            fwd()
            bwd()
            grad()
    fx.synchronize()
    res = {}
    for _ in range(a.rounds):
        for layers, fwd, bwd, grad in configs:
            for key, v in zip(KERNELS + ("call",), visit(fwd, bwd, grad, a.reps, a.kreps)):
                res.setdefault((str(layers), key), []).append(v)
    for layers, _, _, _ in configs:
        s = {k: summary(res[(str(layers), k)]) for k in KERNELS + ("call",)}
        print(json.dumps({"config": "edgeconv_pgrad " + json.dumps(layers, separators=(",", ":")),
                          "forward_kernel_ms": s["edgeconv"], "input_adjoint_kernel_ms": s["edgeconv_bwd"],
                          "parameter_adjoint_kernel_ms": s["edgeconv_pgrad"], "finishing_kernels_ms": s["edgeconv_pgrad_finish"],
                          "parameter_adjoint_call_ms": s["call"],
                          "ratio_parameter_adjoint_over_input_adjoint": round(s["edgeconv_pgrad"]["median"] / s["edgeconv_bwd"]["median"], 3),
                          "ratio_parameter_adjoint_over_forward": round(s["edgeconv_pgrad"]["median"] / s["edgeconv"]["median"], 3)}),
              flush=True)


if __name__ == "__main__":
    main()
