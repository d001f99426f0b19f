#!/usr/bin/env python3
"""Mesh topology on the two routes, per table and in one run: the host builders of csrc/topology.cpp with their uploads (what
TriMesh.dev() did for every mesh before csrc/topology_dev.hip, restated here from the same public pieces) against the device
build (what it does now for a device mesh).  Meshes: the sheets of tests/normals_ref.sheet at 1400 x 1400, 350 x 350 and
40 x 40 cells, eight teapots, and a device-born 128^3 checker grid (trimesh_from_voxels).  Per table: the host clock from the
call to the synchronised result, the device time between two events around the call (device route; it contains the count
read-back), and the algorithmic bytes (tables read + tables written, once each) over that device time.  For the device-born
mesh also the time from a fresh mesh to the first laplacian_loss and to the first compute_verts_normals_packed on either route.

    python tools/topology_time.py [--only NAME] [--route host|device] [--reps N]
For the per-kernel table run it under `rocprofv3 --kernel-trace --stats -- python tools/topology_time.py --only sheet1400
--route device` in a run of its own (tracing adds to the times) and summarise with tools/rocprof_summary.py."""
import argparse
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
from flux3d_jl_amd.rep import index_upload  # noqa: E402
from normals_ref import sheet  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
TABLES = ("faces_packed", "edges", "laplacian", "vf_padded", "vf_packed")


def sheet_mesh(n):
    v, f = sheet(n, n)
    return lambda: fx.gpu(fx.TriMesh([v], [f + 1]))


def teapots():
    v, f = fx.load_obj(os.path.join(G, "teapot.obj"))
    return lambda: fx.gpu(fx.TriMesh([v] * 8, [f] * 8))


def checker_grid(res=128):
    i, j, k = np.meshgrid(*[np.arange(res)] * 3, indexing="ij")
    vox = fx.gpu(np.asfortranarray((((i + j + k) % 2) == 0).astype(np.float32)[..., None]))
    return lambda: fx.trimesh_from_voxels(vox, 0.5, "Exact")


MESHES = {"sheet1400": lambda: sheet_mesh(1400), "sheet350": lambda: sheet_mesh(350), "sheet40": lambda: sheet_mesh(40),
          "teapot8": teapots, "grid128": checker_grid}


def host_table(m, table):
    """One table on the host route: build from the host faces, upload into the mesh's device cache."""
    d, b = m._topo_dev, m.index_base
    V = int(np.sum(m._verts_len))
    if table == "faces_packed":  # (a device-born mesh builds its host face lists here)
        d["faces_packed"] = index_upload(m.get_faces_packed(), b, limit=V)
        if "faces_padded" not in d:
            d["faces_padded"] = index_upload(m.get_faces_padded(), b, clamp_pad=True, limit=int(m.V))
    elif table == "edges":
        m.get_faces_list()
        d["edges"] = index_upload(m.get_edges_packed(), b, limit=V)
    elif table == "laplacian":
        m.get_faces_list()
        for n, a in zip(("lap_rowptr", "lap_colind", "lap_vals"), m.get_laplacian_packed()):
            d[n] = fx.DeviceArray.from_host(a)
    else:
        if table == "vf_padded":
            fp = np.asfortranarray(m.get_faces_padded().astype(np.int64) - b).astype(np.int32)
            fp[fp < 0] = 0
            fp, fl, Vm, Fm, B, pre = np.asfortranarray(fp), np.ascontiguousarray(m._faces_len, dtype=np.int32), int(m.V), int(m.F), int(m.N), "vf_"
        else:
            fp = np.asfortranarray(m.get_faces_packed().astype(np.int64) - b).astype(np.int32)
            Vm, Fm, B, pre = V, fp.shape[1], 1, "vf_packed_"
            fl = np.array([Fm], np.int32)
        rowptr, ent = np.zeros((Vm + 1, B), np.int32, order="F"), np.zeros((3 * Fm, B), np.int32, order="F")
        _lib.call("fx3d_build_vertex_faces", fp.ctypes.data, fl.ctypes.data, Vm, Fm, B, rowptr.ctypes.data, ent.ctypes.data)
        d[pre + "rowptr"], d[pre + "ent"] = fx.DeviceArray.from_host(rowptr), fx.DeviceArray.from_host(ent)


def device_table(m, table):
    for n in {"faces_packed": ("faces_packed",), "edges": ("edges",), "laplacian": ("lap_rowptr",), "vf_padded": ("vf_rowptr",),
              "vf_packed": ("vf_packed_rowptr",)}[table]:
        m.dev(n)


def table_bytes(m, table):
    V, Vm, F, Fm, B = int(np.sum(m._verts_len)), int(m.V), int(np.sum(m._faces_len)), int(m.F), int(m.N)
    if table == "faces_packed":
        return 24 * F
    if table == "edges":
        return 12 * F + 8 * m.dev("edges").shape[0]
    if table == "laplacian":
        return 8 * m.dev("edges").shape[0] + 4 * (V + 1) + 8 * m.dev("lap_colind").shape[0]
    if table == "vf_padded":
        return 12 * Fm * B + 4 * (Vm + 1) * B + 12 * Fm * B
    return 12 * F + 4 * (V + 1) + 12 * F


def timed(fn):
    fx.synchronize()
    e0, e1 = fx.Event(), fx.Event()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    fx.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_ms(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(MESHES))
    ap.add_argument("--route", choices=("host", "device"))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    routes = [a.route] if a.route else ["host", "device"]
    for name in ([a.only] if a.only else list(MESHES)):
        fresh = MESHES[name]()
        born = name == "grid128"
        for route in routes:
            build = host_table if route == "host" else device_table
            best = {}
            for _ in range(a.reps if route == "device" else 1):  # (the host route takes seconds on the large meshes: once)
                m = fresh()
                if not born:
                    m.dev("faces_packed"), m.dev("faces_padded"), m.dev("faces_len")  # uploads both routes share
                for t in TABLES[0 if born else 1:]:
                    wall, dev_ms = timed(lambda: build(m, t))
                    if t not in best or wall < best[t][0]:
                        best[t] = (wall, dev_ms)
            for t, (wall, dev_ms) in best.items():
                row = {"mesh": name, "V": int(np.sum(m._verts_len)), "F": int(np.sum(m._faces_len)), "B": int(m.N), "route": route,
                       "table": t, "wall_ms": round(wall, 3)}
                if route == "device":
                    by = table_bytes(m, t)
                    row.update(device_ms=round(dev_ms, 3), algorithmic_MB=round(by / 1e6, 2), GBps=round(by / dev_ms / 1e6, 1))
                print(json.dumps(row), flush=True)
            print(json.dumps({"mesh": name, "route": route, "table": "all", "wall_ms": round(sum(w for w, _ in best.values()), 3)}), flush=True)
        if born:
            for route in routes:
                for op, tables, call in (("laplacian_loss", ("faces_packed", "edges", "laplacian"), lambda m: fx.laplacian_loss(m)),
                                         ("compute_verts_normals_packed", ("faces_packed", "vf_packed"),
                                          lambda m: fx.compute_verts_normals_packed(m))):
                    m = fresh()

                    def first():
                        if route == "host":
                            for t in tables:
                                host_table(m, t)
                        call(m)
                    wall, _ = timed(first)
                    print(json.dumps({"mesh": name, "route": route, "first_result_of": op, "wall_ms": round(wall, 3)}), flush=True)


if __name__ == "__main__":
    main()
