"""The device topology entry points (csrc/topology_dev.hip) where no device is needed: size queries, the ABI table, the
no-fallback rule, and the host mesh's unchanged route."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = {"fx3d_edges_dev_workspace_bytes", "fx3d_edges_dev_count", "fx3d_edges_dev_emit", "fx3d_laplacian_dev_workspace_bytes",
       "fx3d_laplacian_dev_csr", "fx3d_vertex_faces_dev_workspace_bytes", "fx3d_vertex_faces_dev",
       "fx3d_faces_padded_to_packed_dev_workspace_bytes", "fx3d_faces_padded_to_packed_dev"}


def test_workspace_queries_grow_with_the_mesh(fx):
    q = fx._lib.query_bytes
    sizes = [1, 2, 63, 64, 1000, 4096, 4097, 100000, 3000000]
    for V in (1, 7, 5000, 2000000):
        e = [q("fx3d_edges_dev_workspace_bytes", F, V) for F in sizes]
        lap = [q("fx3d_laplacian_dev_workspace_bytes", E, V) for E in sizes]
        vf = [q("fx3d_vertex_faces_dev_workspace_bytes", min(V, 1 << 20), F, 2) for F in sizes]
        for got in (e, lap, vf):
            assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])), got
    for F in sizes:  # and with V at a fixed F
        lap = [q("fx3d_laplacian_dev_workspace_bytes", F, V) for V in sizes]
        assert all(a <= b for a, b in zip(lap, lap[1:]))
    pk = [q("fx3d_faces_padded_to_packed_dev_workspace_bytes", B) for B in (1, 2, 100, 100000)]
    assert pk[0] > 0 and all(a <= b for a, b in zip(pk, pk[1:]))


def test_workspace_queries_refuse_the_limits(fx):
    lib, n = fx._lib.load(), C.c_size_t(0)
    assert lib.fx3d_edges_dev_workspace_bytes((1 << 31) // 3 + 1, 10, C.byref(n)) != 0      # 3F >= 2^31
    assert lib.fx3d_edges_dev_workspace_bytes((1 << 31) // 3, 10, C.byref(n)) == 0
    assert lib.fx3d_edges_dev_workspace_bytes(0, 10, C.byref(n)) != 0 and lib.fx3d_edges_dev_workspace_bytes(10, 0, C.byref(n)) != 0
    assert lib.fx3d_laplacian_dev_workspace_bytes(1 << 30, 1, C.byref(n)) != 0             # 2E + V >= 2^31
    assert lib.fx3d_laplacian_dev_workspace_bytes(0, 0, C.byref(n)) != 0
    assert lib.fx3d_vertex_faces_dev_workspace_bytes(10, 1 << 29, 1, C.byref(n)) != 0      # Fmax >= 2^29
    assert lib.fx3d_vertex_faces_dev_workspace_bytes(10, (1 << 29) - 1, 1, C.byref(n)) == 0


def test_signatures_match_the_header(fx):
    hdr = open(os.path.join(ROOT, "include", "flux3d_hip.h")).read()
    for name in sorted(NEW):
        m = re.search(r"FX3D_API\s+fx3d_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        assert len(fx._lib.SIGNATURES[name]) == len(m.group(1).split(",")), name


def test_no_cpu_fallback(fx):
    """Without a device the compute entry points return an error status: nothing is built on the host in their place.
    (Skipped on a box with a GPU, like test_host.test_no_cpu_fallback.)"""
    if fx.functional():
        pytest.skip("GPU present")
    lib, q = fx._lib.load(), fx._lib.query_bytes
    F, V, B = 4, 6, 1
    buf = np.zeros(max(q("fx3d_edges_dev_workspace_bytes", F, V), q("fx3d_laplacian_dev_workspace_bytes", 3 * F, V),
                       q("fx3d_vertex_faces_dev_workspace_bytes", V, F, B)), np.uint8)
    a = np.zeros(64, np.int64)  # well-formed arguments that stand in for device memory: no launch ever reads them
    p, w = a.ctypes.data, buf.ctypes.data
    assert lib.fx3d_edges_dev_count(p, F, V, p, p, w, buf.nbytes, None) != 0
    assert lib.fx3d_edges_dev_emit(p, F, V, 5, p, p, w, buf.nbytes, None) != 0
    assert lib.fx3d_laplacian_dev_csr(p, 3 * F, V, p, p, p, p, p, w, buf.nbytes, None) != 0
    assert lib.fx3d_vertex_faces_dev(p, p, V, F, B, p, p, p, w, buf.nbytes, None) != 0
    assert lib.fx3d_faces_padded_to_packed_dev(p, p, p, F, B, F, p, w, buf.nbytes, None) != 0
    assert not a.any()


def test_host_mesh_keeps_the_host_builders(fx, monkeypatch):
    from flux3d_jl_amd import rep
    names, real = [], rep._lib.call

    def recorder(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(rep._lib, "call", recorder)
    faces = np.asfortranarray(np.array([[1, 2, 3], [2, 3, 4], [3, 4, 5], [1, 1, 5]], np.int64).T)
    m = fx.TriMesh([np.zeros((3, 6), np.float32)], [faces])
    e, f2e, (rowptr, colind, vals) = m.get_edges_packed(), m.get_faces_to_edges_packed(), m.get_laplacian_packed()
    assert names == ["fx3d_build_edges_packed", "fx3d_build_laplacian_csr"] and not any("_dev" in n for n in names)
    assert e.tolist() == [[1, 1], [1, 2], [1, 3], [1, 5], [2, 3], [2, 4], [3, 4], [3, 5], [4, 5]]
    assert f2e.tolist() == [[5, 3, 2], [7, 6, 5], [9, 8, 7], [4, 4, 1]] and e.dtype == f2e.dtype == np.int64
    assert len(colind) == 2 * 9 + 6 - 2 and rowptr[-1] == len(vals) and rowptr[6] - rowptr[5] == 1
