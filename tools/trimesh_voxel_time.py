#!/usr/bin/env python3
"""trimesh_to_voxel (fx3d_trimesh_to_voxel) device time per call beside the host restatement of the reference's _voxelize
(tests/trimesh_voxel_ref.py) on the same meshes: the reference's own test case (teapot + sphere, res 28, B = 2), each of
the 8 committed ModelNet meshes alone at res 32 and 64, and all 8 as one ragged batch at res 32, 64 and 128.  Every device
grid is checked bit for bit against the restatement before it is timed.  The device time is event-timed over back-to-back
calls with a device-side error counter (no read-back inside the timed region); it includes the grid's zeroing."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flux3d_jl_amd as fx  # noqa: E402
from bench_ops import gpu_time  # noqa: E402
import trimesh_voxel_ref as ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def case(name, meshes, res, rows):
    verts, faces = [v for v, _ in meshes], [f for _, f in meshes]
    m = fx.gpu(fx.TriMesh(verts, faces))
    t0 = time.perf_counter()
    exp = ref.trimesh_to_voxel(verts, faces, res)
    host_us = (time.perf_counter() - t0) * 1e6
    bad = fx.DeviceArray.zeros((1,), np.uint32)
    got = fx.trimesh_to_voxel(m, res, bad=bad).to_host()
    assert int(bad.to_host()[0]) == 0 and np.array_equal(got, exp), name
    us_min, us_med = gpu_time(lambda: fx.trimesh_to_voxel(m, res, bad=bad), reps=20, inner=8)
    points = sum(ref.voxelize(v, f, res, return_stats=True)[2] for v, f in meshes)
    row = dict(case=name, B=len(meshes), res=res, faces=int(sum(f.shape[1] for f in faces)), points=int(points),
               voxels=int(exp.sum()), device_us_min=round(us_min, 1), device_us_median=round(us_med, 1),
               host_restatement_us=round(host_us, 0))
    rows.append(row)
    print(f"{name:28s} B={row['B']} res={res:4d} faces={row['faces']:6d} points={points:9d} voxels={row['voxels']:7d}  "
          f"device {us_min:9.1f} us (median {us_med:9.1f})   host restatement {host_us:12.0f} us", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--json", help="also write the rows to this file")
    a = ap.parse_args()
    assert fx.functional(), "needs a GPU"
    rows = []
    ref_meshes = [fx.load_obj(os.path.join(GOLDEN, n)) for n in ("teapot.obj", "sphere.obj")]
    case("teapot+sphere (reference)", ref_meshes, 28, rows)
    mn = ref.modelnet_meshes(GOLDEN)
    for res in (32, 64):
        for name, v, f in mn:
            case(name, [(v, f)], res, rows)
    for res in (32, 64, 128):
        case("ModelNet batch of 8", [(v, f) for _, v, f in mn], res, rows)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump({"device": fx.device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
