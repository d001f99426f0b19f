#!/usr/bin/env python3
"""Vertex / face normals and their adjoints on the device, per call, beside the numpy restatement of the reference's CPU
method (tests/normals_ref.py) -- at B = 8 teapots (the reference's benchmarks/triangle_mesh.jl mesh) and at the bandwidth-bound
jittered 1400 x 1400-cell sheet (1.96 M vertices, 3.92 M faces: the shape of tools/hbm_roofline.py).

Per op: the host-clock time of one call ended by a device synchronisation (median of --reps), the kernel time from the
library's own HIP events around the launches (fx3d_profile_enable), the algorithmic bytes over the kernel
time, and the restatement's time for the same result.  Every device result is checked bit for bit against the restatement.
One JSON line per (mesh, op).

  python tools/normals_time.py [--reps 20] [--only teapot8|sheet]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flux3d_jl_amd as fx  # noqa: E402
from flux3d_jl_amd import _lib  # noqa: E402
import normals_ref as ref  # noqa: E402


def algorithmic_bytes(op, V, F):
    """Bytes the algorithm must move once: int32 table rowptr (V+1) / entries (3F), int32 faces (3F), Float32 (3,*) arrays."""
    return {"verts_normals": 12 * V + 4 * V + 12 * F + 12 * F + 12 * V,           # verts, rowptr, entries, faces, normals
            "faces_normals": 12 * V + 12 * F + 12 * F,                               # verts, faces, normals
            "verts_normals_bwd": (4 * V + 12 * F + 12 * F + 12 * V + 12 * V + 12 * V)  # g_raw pass: + gout, g_raw
            + (4 * V + 12 * F + 12 * F + 3 * F + 12 * V + 12 * V + 12 * V),            # gather: + mask, g_raw, gverts
            "faces_normals_bwd": (12 * F + 12 * V + 12 * F + 12 * F)                  # g_raw pass: faces, verts, gout, g_raw
            + (4 * V + 12 * F + 12 * F + 12 * V + 12 * F + 12 * V)}[op]              # gather: table, faces, verts, g_raw, gverts


def kernel_ms(name, fn, reps):
    _lib.call("fx3d_profile_enable", 1)
    for _ in range(reps):
        fn()
    fx.synchronize()
    avg, mn, mx, cnt = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int64(0)
    _lib.call("fx3d_profile_kernel_stats", name.encode(), C.byref(avg), C.byref(mn), C.byref(mx), C.byref(cnt))
    _lib.call("fx3d_profile_enable", 0)
    return avg.value, mn.value


def call_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        fx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), r


def same_bits(a, b):
    an, bn = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(an, bn) and np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn]))


def measure(name, m, reps, host_reps):
    v, f = m.get_verts_packed_host(), np.asfortranarray(m.get_faces_packed().astype(np.int64) - m.index_base)
    V, F = v.shape[1], f.shape[1]
    rng = np.random.default_rng(1)
    g, gf = (np.asfortranarray(rng.standard_normal(s).astype(np.float32)) for s in ((3, V), (3, F)))
    gd, gfd = fx.gpu(g), fx.gpu(gf)
    out = fx.DeviceArray.empty((3, V), np.float32)
    ops = {"verts_normals": (lambda: fx.compute_verts_normals_packed(m), lambda: ref.verts_normals(v, f)),
           "faces_normals": (lambda: fx.compute_faces_normals_packed(m), lambda: ref.faces_normals(v, f)),
           "verts_normals_bwd": (lambda: fx.compute_verts_normals_grad(m, gd, out=out), lambda: ref.verts_normals_bwd(v, f, g)),
           "faces_normals_bwd": (lambda: fx.compute_faces_normals_grad(m, gfd, out=out), lambda: ref.faces_normals_bwd(v, f, gf))}
    for op, (dev, host) in ops.items():
        for _ in range(3):
            r = dev()
        fx.synchronize()
        got = r.to_host()
        t_host, want = host_ms(host, host_reps)
        k_avg, k_min = kernel_ms(op, dev, reps)
        nb = algorithmic_bytes(op, V, F)
        print(json.dumps({"mesh": name, "op": op, "V": V, "F": F, "bit_identical": same_bits(got, want),
                          "call_ms": round(call_ms(dev, reps), 4), "kernel_ms": round(k_avg, 4), "kernel_min_ms": round(k_min, 4),
                          "algorithmic_MB": round(nb / 1e6, 2), "GBps": round(nb / (k_avg * 1e-3) / 1e9, 1),
                          "host_restatement_ms": round(t_host, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["teapot8", "sheet"])
    a = ap.parse_args()
    assert fx.functional(), "normals_time.py needs a GPU"
    if a.only in (None, "teapot8"):
        t = os.path.join(ROOT, "tests", "golden", "teapot.obj")
        measure("teapot x 8", fx.gpu(fx.load_trimesh(*([t] * 8))), a.reps, 5)
    if a.only in (None, "sheet"):
        v, f = ref.sheet(1400, 1400)
        measure("sheet 1400^2", fx.gpu(fx.TriMesh([v], [f], index_base=0)), a.reps, 1)


if __name__ == "__main__":
    main()
