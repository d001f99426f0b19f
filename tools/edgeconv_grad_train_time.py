#!/usr/bin/env python3
"""The EdgeConv training-mode adjoint (fx.EdgeConv.flat_grad_train, fx3d_edgeconv_grad_train) beside the input adjoint, the
test-mode parameter adjoint and the training-mode forward of the same shape in the same run, at 32 x 1024 with K = 20: DGCNN's two
stages, [3, 32, 64, 64] and [64, 128, 256], on DGCNN's inputs and parameters, and [64, 64, 128, 256].

The yardstick of a sums pass is the input adjoint's kernel: a pass does its contractions down to the stop layer plus one
recomputed forward slab per hidden layer it crosses, plus Float64 additions.  The yardstick of the closing pass is the test-mode
parameter adjoint's kernel.  The expected ratios are MFMA counts from the layer widths (f_l = cin_l cout_l per edge row):
  the input adjoint 2 sum f;  a sums pass that stops at s:  sum f + sum_{l > s} f_l + sum_{s <= l < L} f_l;
  the test-mode kernel 3 sum f per pass;  the closing pass 3 sum f + sum_{l < L} f_l per pass (passes: the tile lists' lengths).

One process; --rounds rounds, each visiting every configuration in turn.  A visit ALTERNATES EdgeConv.input_grad, EdgeConv.grad,
EdgeConv.forward_train and the new call (with gx, given the forward) call by call, --kreps of each, with the library's own
events around the kernels' launches (fx3d_profile_enable), so that all see the same clock; a label's figure is its sum per call.
Then device events around --reps calls of the new entry.  Reported per configuration: medians over the rounds with min and max,
and the ratios.  The new call is first compared with the host restatement tests/edgeconv_grad_train_ref.py on the first cloud,
bit for bit.  One JSON line per configuration.  For a per-kernel table run it under
`rocprofv3 --kernel-trace --stats -- python tools/edgeconv_grad_train_time.py` in a run of its own.

  python tools/edgeconv_grad_train_time.py [--rounds 5] [--reps 10] [--kreps 10] [--warmup 3]
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
import edgeconv_grad_train_ref  # noqa: E402
import edgeconv_ref  # noqa: E402

N, B, K, NC = 1024, 32, 20, 40
FORWARD = ("edgeconv_train_stats", "edgeconv_train_stats_last", "edgeconv_train_finish", "edgeconv_train_closing")
SUMS = ("edgeconv_grad_train_sums_last", "edgeconv_grad_train_sums_3", "edgeconv_grad_train_sums_2", "edgeconv_grad_train_sums_1")
OTHER = ("edgeconv_bwd", "edgeconv_pgrad", "edgeconv_grad_train_closing", "edgeconv_grad_train_finish", "edgeconv_grad_train_reduce")


def label_ms(name, calls):
    """The label's launches of the visit, summed, per call (0 for a label that was not launched)."""
    avg, cnt = C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), None, None, C.byref(cnt))
    return avg.value * cnt.value / calls if cnt.value > 0 else 0.0


def visit(calls, new, reps, kreps):
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(kreps):
        for call in calls:
            call()
    fx.synchronize()
    ms = {k: label_ms(k, kreps) for k in FORWARD + SUMS + OTHER}
    _lib.call("fx3d_profile_enable", 0)
    e0, e1 = fx.Event(), fx.Event()
    e0.record()
    for _ in range(reps):
        new()
    e1.record()
    e1.synchronize()
    ms["call"] = e0.elapsed_ms(e1) / reps
    ms["forward_train"] = sum(ms[k] for k in FORWARD)
    return ms


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def expected(layers):
    """The MFMA counts of the module docstring: (per sums pass, last first, over the input adjoint; the closing pass over the
    test-mode kernel, one pass each)."""
    f = [(2 * layers[0] if i == 1 else layers[i - 1]) * layers[i] for i in range(1, len(layers))]
    L, tot = len(f), sum(f)
    sums = {}
    for s in range(L, 0, -1):
        sums["last" if s == L else str(s)] = round((tot + sum(f[s:]) + sum(f[s - 1:L - 1])) / (2 * tot), 3)
    return sums, round((3 * tot + sum(f[:L - 1])) / (3 * tot), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert fx.functional(), "edgeconv_grad_train_time.py needs a GPU"
    P = dgcnn_ref.random_params(NC, seed=NC)
    dg = fx.DGCNN(NC, K, N).load(P)
    rng = np.random.default_rng(2)
    xd = fx.gpu(np.asfortranarray(rng.standard_normal((3, N, B)).astype(np.float32)))
    x1 = dg.forward_train(xd, intermediates=True)["x1"]
    own = lambda name: {k[len(name) + 1:]: v for k, v in P.items() if k.startswith(name + ".")}  # noqa: E731
    configs = []
    for layers, params, x in (([3, 32, 64, 64], own("ec1"), xd), ([64, 128, 256], own("ec2"), x1),
                              ([64, 64, 128, 256], edgeconv_ref.random_params([64, 64, 128, 256], seed=1), x1)):
        m = fx.EdgeConv(layers, K).load(params)
        gout = np.asfortranarray(rng.standard_normal((layers[-1], N, B)).astype(np.float32))
        g = fx.gpu(gout)
        one = lambda v: np.asfortranarray(v.to_host()[:, :, :1])  # noqa: E731
        x0, g0 = fx.gpu(one(x)), fx.gpu(np.asfortranarray(gout[:, :, :1]))
        f0 = m.forward_train(x0, intermediates=True)
        got, gx = m.flat_grad_train(x0, g0, fwd=f0)
        stats = {k: v.to_host() for k, v in f0["batch_stats"].items()}
        G, wx = edgeconv_grad_train_ref.grad(one(x), params, layers, K, gout[:, :, :1], stats, f0["idx"].to_host(), f0["out"].to_host())
        bits = lambda v: np.ascontiguousarray(v).view(np.uint32)  # noqa: E731
        same = bool(np.array_equal(bits(got.to_host()), bits(edgeconv_grad_train_ref.flat(G, layers)))
                    and np.array_equal(bits(gx.to_host()), bits(wx)))
        print(json.dumps({"config": json.dumps(layers, separators=(",", ":")), "shape": f"{B} x {N}", "K": K,
                          "first_cloud_equals_the_restatement_bit_for_bit": same}), flush=True)
        assert same
        out, idx = m.forward(x, return_idx=True)
        fwd = m.forward_train(x, idx=idx, intermediates=True)
        new = lambda m=m, x=x, g=g, fwd=fwd: m.flat_grad_train(x, g, fwd=fwd)  # noqa: E731
        configs.append((layers, ((lambda m=m, x=x, g=g, idx=idx, out=out: m.input_grad(x, g, idx, out)),
                                 (lambda m=m, x=x, g=g, idx=idx, out=out: m.flat_grad(x, g, idx, out)),
                                 (lambda m=m, x=x, idx=idx: m.forward_train(x, idx=idx)), new), new))
    for _, calls, _ in configs:
        for _ in range(a.warmup):
            for call in calls:
                call()
    fx.synchronize()
    res = {}
    for _ in range(a.rounds):
        for layers, calls, new in configs:
            for key, v in visit(calls, new, a.reps, a.kreps).items():
                res.setdefault((str(layers), key), []).append(v)
    for layers, _, _ in configs:
        s = {k: summary(v) for (name, k), v in res.items() if name == str(layers)}
        bwd, pgrad = s["edgeconv_bwd"]["median"], s["edgeconv_pgrad"]["median"]
        want_sums, want_closing = expected(layers)
        passes = {k.rsplit("_", 1)[1]: s[k] for k in SUMS if s[k]["median"] > 0}
        print(json.dumps({"config": "edgeconv_grad_train " + json.dumps(layers, separators=(",", ":")),
                          "input_adjoint_kernel_ms": s["edgeconv_bwd"], "parameter_adjoint_kernel_ms": s["edgeconv_pgrad"],
                          "forward_train_kernels_ms": s["forward_train"],
                          "sums_pass_ms": passes, "finishing_kernels_ms": s["edgeconv_grad_train_finish"],
                          "closing_pass_ms": s["edgeconv_grad_train_closing"], "reduce_ms": s["edgeconv_grad_train_reduce"],
                          "grad_train_call_ms": s["call"],
                          "ratio_sums_pass_over_input_adjoint": {k: round(v["median"] / bwd, 3) for k, v in passes.items()},
                          "expected_from_mfma_counts": want_sums,
                          "ratio_closing_pass_over_parameter_adjoint": round(s["edgeconv_grad_train_closing"]["median"] / pgrad, 3),
                          "expected_per_pass_from_mfma_counts": want_closing,
                          "ratio_call_over_forward_train": round(s["call"]["median"] / s["forward_train"]["median"], 3)}), flush=True)


if __name__ == "__main__":
    main()
