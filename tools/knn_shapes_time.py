#!/usr/bin/env python3
"""Self-kNN graphs over a spread of (D, N, B, k) outside the BASELINE configs: per-call device time and pairs per second --
a check for launch-plan cliffs (few clouds with many rows, wide features).  The feature-space rows cover knn_mfma_kernel's three
filter modes: behind the pre-pass at D = 16, 32, 64, 128, the block's own fp16 image (option knn_no_prepass) at D = 64, the Float32
GEMM at M > 4096 per slice or cloud."""
import os, sys, numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tools"))
import flux3d_jl_amd as fx
from bench_ops import gpu_time
rng = np.random.default_rng(5)
for D, N, B, k, nopre in [(3, 1024, 32, 20, 0), (3, 4096, 8, 20, 0), (3, 16384, 1, 20, 0), (3, 16384, 4, 20, 0), (3, 32768, 1, 16, 0),
                          (64, 1024, 32, 20, 0), (64, 4096, 4, 20, 0), (64, 8192, 1, 20, 0), (16, 2048, 8, 10, 0), (128, 1024, 8, 20, 0),
                          (32, 1024, 32, 20, 0), (128, 1024, 32, 20, 0), (64, 1024, 32, 20, 1)]:
    x = fx.gpu(np.asfortranarray(rng.standard_normal((D, N, B)).astype(np.float32)))
    try:
        with fx._lib.option("knn_no_prepass", nopre):
            mn, md = gpu_time(lambda: fx.knn(x, k, drop_first=True, return_dist=False), reps=10, inner=4)
        print(f"D={D:<3d} N=M={N:<6d} B={B:<3d} k={k:<3d}{' no pre-pass' if nopre else ''} min {mn:9.1f} us   {B*N*N/mn/1e6:8.3f} T pairs/s", flush=True)
    except Exception as e:
        print(D, N, B, k, nopre, "ERR", str(e)[:100])
