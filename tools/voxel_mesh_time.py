#!/usr/bin/env python3
"""voxel_to_trimesh with algo :Exact (fx3d_voxel_mesh_count + fx3d_voxel_mesh_emit) device time per call beside the host
restatement of the reference's _voxel_exact (tests/voxel_mesh_ref.py) on the same grids: the reference's test grid (res 32,
B = 2, thresh 0.9), a full 128^3 grid, a 128^3 checkerboard (K = 1 048 576), and the 8 committed ModelNet meshes voxelised
on the device at 64 and 128 as one batch.  Every mesh is checked bit for bit against the restatement before it is timed.

device us: both phases with vertices and device faces, event-timed over back-to-back calls (no read-back inside the timed
region: the counts of the checked call size the buffers).  call ms: trimesh_from_voxels end to end on the host clock,
its count read-back included.  emit bytes: 96 B of vertices + 144 B of faces per cube.
``--only checker128 --reps N``: just that case's two phases N times (for a kernel trace of its own)."""
import argparse
import ctypes as C
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
from flux3d_jl_amd import _lib  # noqa: E402
from bench_ops import gpu_time  # noqa: E402
import trimesh_voxel_ref as tvref  # noqa: E402
import voxel_mesh_ref as ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def phases(vox, thresh, K):
    """A closure running count + emit into fixed buffers sized from the known counts."""
    res, B = vox.shape[0], vox.shape[3]
    nb = C.c_size_t(0)
    _lib.call("fx3d_voxel_mesh_workspace_bytes", res, B, C.byref(nb))
    ws = fx.DeviceArray.empty((nb.value,), np.uint8)
    counts = fx.DeviceArray.empty((2 * B,), np.int64)
    total, Fmax = int(K.sum()), 12 * int(K.max())
    verts = fx.DeviceArray.empty((3, 8 * total), np.float32)
    faces = fx.DeviceArray.empty((3, Fmax, B), np.int32)

    def run():
        st = fx.current_stream().handle
        _lib.call("fx3d_voxel_mesh_count", vox.ptr, res, B, float(np.float32(thresh)), counts.ptr, counts.ptr + 8 * B,
                  ws.ptr, ws.nbytes, st)
        _lib.call("fx3d_voxel_mesh_emit", res, B, total, verts.ptr, faces.ptr, Fmax, ws.ptr, ws.nbytes, st)
    return run


def case(name, vox_host, thresh, rows, vox_dev=None):
    vox_dev = vox_dev if vox_dev is not None else fx.DeviceArray.from_host(vox_host)
    t0 = time.perf_counter()
    ev, ef = ref.voxel_to_trimesh(vox_host, np.float32(thresh))
    host_us = (time.perf_counter() - t0) * 1e6
    m = fx.trimesh_from_voxels(vox_dev, thresh, "Exact")
    got = m.get_verts_packed().to_host()
    assert np.array_equal(got, np.concatenate(ev, axis=1)), name
    for i, f in enumerate(m.get_faces_list()):
        assert np.array_equal(f, ef[i]), (name, i)
    K = m._verts_len // 8
    us_min, us_med = gpu_time(phases(vox_dev, thresh, K), reps=20, inner=8)
    fx.synchronize()
    call = []
    for _ in range(10):
        t0 = time.perf_counter()
        fx.trimesh_from_voxels(vox_dev, thresh, "Exact").get_verts_packed()
        fx.synchronize()
        call.append((time.perf_counter() - t0) * 1e3)
    res, B = vox_host.shape[0], vox_host.shape[3]
    emit_bytes = 240 * int(K.sum())
    row = dict(case=name, B=B, res=res, cubes=int(K.sum()), in_bytes=int(vox_host.nbytes), emit_bytes=emit_bytes,
               device_us_min=round(us_min, 1), device_us_median=round(us_med, 1), call_ms_min=round(min(call), 3),
               host_restatement_us=round(host_us, 0))
    rows.append(row)
    print(f"{name:32s} B={B} res={res:4d} cubes={row['cubes']:8d} in={vox_host.nbytes / 1e6:7.1f} MB "
          f"emit={emit_bytes / 1e6:7.1f} MB  device {us_min:8.1f} us (median {us_med:8.1f})  call {min(call):7.3f} ms  "
          f"host restatement {host_us:11.0f} us", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--json", help="also write the rows to this file")
    ap.add_argument("--only", choices=["checker128"], help="run one case's two phases --reps times, nothing else")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    assert fx.functional(), "needs a GPU"
    if a.only == "checker128":
        vox = fx.DeviceArray.from_host(ref.checkerboard(128))
        K = np.array([128 ** 3 // 2])
        run = phases(vox, 0.5, K)
        for _ in range(a.reps):
            run()
        fx.synchronize()
        return
    rows = []
    case("reference test grid (thr 0.9)", ref.reference_test_grid(), 0.9, rows)
    case("full 128^3", np.ones((128, 128, 128, 1), np.float32, order="F"), 0.5, rows)
    case("checkerboard 128^3", ref.checkerboard(128), 0.5, rows)
    mn = tvref.modelnet_meshes(GOLDEN)
    m = fx.gpu(fx.TriMesh([v for _, v, _ in mn], [f for _, _, f in mn]))
    for res in (64, 128):
        grid = fx.trimesh_to_voxel(m, res)
        case(f"ModelNet batch of 8, res {res}", grid.to_host(), 0.5, rows, vox_dev=grid)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump({"device": fx.device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
