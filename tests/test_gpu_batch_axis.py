"""Every entry point with a batch argument at the first batch sizes that do not fit in 16 bits (DESIGN.md 2 "Batch axis").

About fifty launches put the batch on the grid's y, which ends at 65535; the rest of the GPU suite stops at B = 1025.  Each
family below runs at B = 65535, 65536 and 65537 (the last is no multiple of 8: the matrix-core kernels' padded batch then holds
blocks that belong to no cloud), or at 32767 and 32768 where the limit is on 2 B or on B x slices.  ``LIMITS`` names, for every
``FX3D_API`` function of include/flux3d_hip.h with an ``int32_t B`` parameter, the largest B its argument check accepts (with
every other size at its smallest) and what this file does with it; tests/test_batch_axis_host.py holds the table complete and
equal to the header's "Batch axis:" notes without a GPU.  A case ends in one of two ways, decided by the code and the header:

  it runs     every cloud has random data of its own, the outputs are pre-filled with 0xFF bytes (-1 as an index, NaN as a float)
              and placed between 0xA5 pads (tests/misaligned.py), a workspace has exactly the queried size between guard pads
              (tests/dirty_ws.py, filled with 0xFF).  Indices and per-point values equal the family's reference bit for bit -- the
              oracle, the tests/*_ref.py restatements, integer numpy -- and a loss is within LOSS_RTOL of the oracle's Float64 sum.
              Where the reference is a Python loop per mesh (fx3d_trimesh_to_voxel, the voxel mesher) every cloud of the wide call
              is compared with the same clouds run 64 at a time, and the reference is taken on SAMPLE;
  it refuses  FX3D_ERR_INVALID_ARG, a message that names B, not one byte of an input, an output, the workspace or a pad changed
              (every buffer has the size the call would need), and the same entry point straight afterwards at B = 2 returns
              FX3D_OK with the reference's answer: no stale launch error waits for the next FX3D_LAUNCH_CHECK.

No case is run in the expectation that a launch fails: the refusals were read in the argument checks first.
Not run here, and said so in LIMITS: a refusal needs buffers of the size the call would take, and at B = 65536 the workspaces of
fx3d_pointnet_grad(_train) and fx3d_dgcnn_grad(_train) are 14 to 80 GB; their size queries, which go through the same size check,
are held by tests/test_batch_axis_host.py.  The split plan's two-launch finalisation (B <= 32767) needs clouds of thousands of
points.  Device memory: most cases stay below 0.5 GB and every array below about 135 MB; the exceptions are workspaces the entry
points themselves size.  A run: fx3d_knn_ws behind the pre-pass at B = 65537 and the wide slices at B = 32767, 1.4 and 1.5 GB
(21.5 KB per candidate cloud, M = 64 being the smallest the kernel takes).  A refusal, which gets the size the call would
need: fx3d_pointnet_forward 1.3 GB, fx3d_dgcnn_forward_train 1.6 GB and, the largest of the file, fx3d_pointnet_forward_train
2.5 GB.  Those above 256 MB are filled and checked on the device (Scratch), but for the wide slices.

Two things the fixes rest on were read, not observed, since each fix was made before the first run of its case: that the parent's
fx3d_knn_ws launched its two pre-pass kernels with B on the grid's y (so that at B >= 65536 neither could be configured and the
search ran on an image nobody built), and that hipGetLastError still reports such a failed configuration after a later launch
succeeded.  The Mfma cases of test_knn_routes and the B = 2 call that follows every refusal are what decides here."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_families as fam
import dirty_ws as dirty
import misaligned as mis
import transforms_ref as tref
from abi_families import I, _abi, _bits_equal, _first_diff, _rand, _randn
from test_gpu_hardening import LOSS_RTOL

pytestmark = pytest.mark.gpu

INVALID = -1                      # FX3D_ERR_INVALID_ARG
WIDE = (65535, 65536, 65537)
GRID_Y = 65535
U, Y, CH = "unbounded", 65535, (1 << 29) - 1   # CH: B * 2 * ceil(max(N, M) / 256) < 2^30 at one tile
RUN, REFUSE, QUERY, HOST = "runs at 65535, 65536 and 65537", "runs at 65535, refused at 65536", "a size query: tests/test_batch_axis_host.py", \
    "host code, no launch"


def SAMPLE(B):
    return [b for b in (0, 1, 7, 8, 65534, 65535, 65536, B - 1) if b < B]


# entry point: (largest accepted B, what this file does with it)
LIMITS = {
    "fx3d_nn1": (CH, RUN), "fx3d_chamfer_fwd": (CH, RUN), "fx3d_chamfer_fwd_bwd": (CH, RUN), "fx3d_chamfer_bwd": (CH, RUN),
    "fx3d_chamfer_sums": (CH, "fx3d_chamfer_fwd's driver; its two-launch split form refuses B > 32767 up front: untested, it needs clouds "
                              "of thousands of points at that B"),
    "fx3d_nn1_plan_describe": (U, "asserted in every nn1 case"),
    "fx3d_chamfer_workspace_bytes": (U, QUERY), "fx3d_chamfer_fwd_bwd_workspace_bytes": (U, QUERY),
    "fx3d_chamfer_sampled_bwd_workspace_bytes": (U, QUERY), "fx3d_chamfer_pairwise_workspace_bytes": (U, QUERY),
    "fx3d_chamfer_sampled_bwd": (CH, "not run: the batch lies on the grid's x, as in fx3d_chamfer_bwd"),
    "fx3d_chamfer_sampled_bwd_step": (CH, "not run: as fx3d_chamfer_sampled_bwd"),
    "fx3d_chamfer_sampled_bwd_step_reg": (CH, "not run: as fx3d_chamfer_sampled_bwd"),
    "fx3d_chamfer_loss_pairwise_f32": (CH, "not run: the batch lies on the grid's x"),
    "fx3d_transform_plan_describe": (Y, QUERY), "fx3d_transform_workspace_bytes": (Y, QUERY),
    "fx3d_segment_minmax": (Y, REFUSE), "fx3d_normalize": (Y, REFUSE), "fx3d_realign": (Y, REFUSE), "fx3d_rotate": (Y, REFUSE),
    "fx3d_knn": (U, RUN + " on the matrix-core routes; " + REFUSE + " on the others"),
    "fx3d_knn_ws": (U, RUN + " on the matrix-core routes, the pre-pass included; " + REFUSE + " on the others; wide slices at 32767 and 32768 (the plain "
                         "slices, M / S >= 512, would need 0.5 GB of clouds at that B: not run)"),
    "fx3d_knn_workspace_bytes": (U, "queried in every fx3d_knn_ws case"),
    "fx3d_knn_gather": (U, RUN), "fx3d_edge_features_bwd": (U, RUN),
    "fx3d_edge_features": (U, RUN + " at layout 0; layout 1 " + REFUSE),
    "fx3d_edgeconv_graph": (U, RUN + " fused (F = 3); unfused " + REFUSE),
    "fx3d_faces_areas_padded": (U, "not run: a grid-stride kernel"),
    "fx3d_sample_points_explicit": (U, RUN), "fx3d_sample_points": (U, RUN + "; with the multi-block CDF " + REFUSE),
    "fx3d_sample_points_cdf": (U, RUN + "; multi-block through fx3d_sample_points"),
    "fx3d_sample_points_draw": (U, RUN), "fx3d_sample_points_workspace_bytes": (U, QUERY),
    "fx3d_sample_points_cdf_pair": (U, "not run: fx3d_sample_points_cdf's launch with two batches"),
    "fx3d_sample_points_draw_pair": (U, "not run: fx3d_sample_points_draw's launch with two batches"),
    "fx3d_sample_points_draw_pair_reg": (U, "not run: fx3d_sample_points_draw's launch with two batches"),
    "fx3d_sample_points_bwd": ((1 << 26) - 1, RUN),
    "fx3d_build_vertex_faces": (U, HOST + "; builds the ordered adjoint's table at 65537"),
    "fx3d_packed_to_padded": (U, RUN), "fx3d_padded_to_packed": (U, RUN),
    "fx3d_voxel_workspace_bytes": (U, QUERY), "fx3d_pointcloud_to_voxel": (Y, REFUSE),
    "fx3d_trimesh_voxel_workspace_bytes": (U, QUERY), "fx3d_trimesh_to_voxel": (Y, REFUSE),
    "fx3d_voxel_mesh_workspace_bytes": (1 << 24, QUERY), "fx3d_voxel_mesh_count": (1 << 24, RUN), "fx3d_voxel_mesh_emit": (1 << 24, RUN),
    "fx3d_chamfer_distance_host": (U, HOST), "fx3d_knn_host": (U, HOST), "fx3d_sample_points_host": (U, HOST),
    "fx3d_vertex_faces_dev_workspace_bytes": (((1 << 31) - 1) // 3, QUERY), "fx3d_vertex_faces_dev": (((1 << 31) - 1) // 3, RUN),
    "fx3d_faces_padded_to_packed_dev_workspace_bytes": (U, QUERY), "fx3d_faces_padded_to_packed_dev": (U, RUN),
    "fx3d_crossentropy": (U, RUN),
}
_BIG = "refusal not run: a workspace of the size the call would take is %s at B = 65536; the size query refuses through the same check"
_COUPLED = ("refused at 65536; no run at 65535: batch statistics and parameter gradients couple all clouds, so narrow batches say "
            "nothing, and the restatement of 65535 clouds takes tens of seconds")
for _net, _entry, _what in (
        ("pointnet", "forward", "refused at 65536; no run at 65535: the workspace is 1.3 GB"),
        ("pointnet", "forward_train", "refused at 65536; no run at 65535: the workspace is 2.5 GB"),
        ("pointnet", "grad", _BIG % "42 GB"), ("pointnet", "grad_train", _BIG % "43 GB"),
        ("dgcnn", "forward", "test mode: runs at 65535 against narrow batches and the restatement on SAMPLE, refused at 65536"),
        ("dgcnn", "forward_train", "refused at 65536; no run at 65535: the workspace is 1.6 GB"),
        ("dgcnn", "grad", _BIG % "15 GB"), ("dgcnn", "grad_train", _BIG % "79 GB"),
        ("edgeconv", "forward", "test mode: runs at 65535 against narrow batches and the restatement on SAMPLE, refused at 65536"),
        ("edgeconv", "bwd", "runs at 65535 against narrow batches and the restatement on SAMPLE, refused at 65536"),
        ("edgeconv", "forward_train", _COUPLED), ("edgeconv", "grad", _COUPLED), ("edgeconv", "grad_train", _COUPLED)):
    _stem = {"forward": "", "forward_train": "_train", "bwd": "_bwd", "grad": "_grad", "grad_train": "_grad_train"}[_entry]
    LIMITS[f"fx3d_{_net}_{_entry}"] = (Y, _what)
    LIMITS[f"fx3d_{_net}{_stem}_workspace_bytes"] = (Y, QUERY)


@pytest.fixture(autouse=True)
def fresh_nullable():
    fam.NULLABLE.clear()


# ---------------------------------------------------------------------------------------------------------------- the drivers
def _sync(fx, what):
    try:
        fx.synchronize()
    except fx.Flux3DHipError as e:  # a fault: nothing more is started on the device
        pytest.exit(f"{what}: {e}", returncode=3)


def Out(name, shape, dtype=np.float32):
    """An output, every byte 0xFF before the call: -1 as an index, NaN as a float -- an element left unwritten shows."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return fam.Arr(name, np.full(n, 0xFF, np.uint8).view(dtype).reshape(shape, order="F"), out=True)


def Counter(name, shape, dtype=np.uint32):
    """A counter the header asks the caller to zero (fx3d_trimesh_to_voxel's bad_dev): an output that starts at 0."""
    a = fam.O(name, shape, dtype)
    a.zeroed = True
    return a


def _sentinel(a):
    return Out(a.name, a.host.shape, a.host.dtype) if a.out and not getattr(a, "zeroed", False) else a


def _place(fx, arrs):
    return {a.name: mis.place(fx, a.host, 0, output=a.out) for a in arrs}


class Scratch:
    """dirty_ws.Workspace's surface for a workspace of a gigabyte: exactly `nbytes` bytes at a 256-byte aligned address between
    guard pads of dirty_ws.GUARD 0xA5 bytes, filled on the device (ONES: 0xFF bytes; INF: 0x7F bytes -- 3.4e38 as a Float32,
    2.1e9 as an index) and read back in pieces, so that no copy of it ever stands on the host."""
    PIECE = 64 << 20

    def __init__(self, fx, nbytes):
        self.fx, self.nbytes, self.byte = fx, int(nbytes), None
        self.buf = fx.DeviceArray.empty((self.nbytes + 2 * dirty.GUARD,), np.uint8)
        assert self.buf.ptr % dirty.ALIGN == 0
        fx._lib.call("fx3d_memset", self.buf.ptr, mis.OUTPUT_BYTE, self.buf.nbytes, None)
        self.ptr = self.buf.ptr + dirty.GUARD

    def fill(self, pattern):
        self.byte = {"ONES": 0xFF, "INF": 0x7F}[pattern]
        self.fx._lib.call("fx3d_memset", self.ptr, self.byte, self.nbytes, None)

    def _piece(self, at, n):
        return self.fx.DeviceArray(self.buf.ptr + at, (n,), np.uint8, owned=False, keep=self.buf).to_host()

    def check(self, what=""):
        for at in (0, dirty.GUARD + self.nbytes):
            assert np.all(self._piece(at, dirty.GUARD) == mis.OUTPUT_BYTE), f"workspace of {self.nbytes} bytes, {what}: pad bytes written"

    def unchanged(self):
        return all(np.all(self._piece(dirty.GUARD + at, min(self.PIECE, self.nbytes - at)) == self.byte) for at in range(0, self.nbytes, self.PIECE))


class _Guarded(dirty.Workspace):
    def fill(self, pattern):
        super().fill(pattern)
        self.pattern = pattern

    def unchanged(self):
        return _bits_equal(self.image(), dirty.fill_bytes(self.nbytes, self.pattern))


def _workspace(fx, nbytes, guarded=False):
    return _Guarded(fx, nbytes) if guarded or nbytes <= (256 << 20) else Scratch(fx, nbytes)


def hold(fx, call, arrs, ws_bytes=0, skip=(), check=None, guarded=False):
    """One run of `call` (tests/abi_families.py's driver surface): outputs pre-filled 0xFF between 0xA5 pads, the workspace of
    exactly `ws_bytes` bytes filled 0xFF between guard pads (`guarded`: dirty_ws.Workspace whatever the size); {output: host
    result}, all pads checked."""
    arrs = [_sentinel(a) for a in arrs]
    placed = _place(fx, arrs)
    ws = _workspace(fx, ws_bytes, guarded)
    ws.fill("ONES")
    call(fam.Ptrs(**{n: p.ptr for n, p in placed.items()}), ws.ptr, ws.nbytes)
    _sync(fx, "wide batch")
    ws.check("wide batch")
    out = {}
    for a in arrs:
        if a.out:
            placed[a.name].check_pads(a.name)
            out[a.name] = placed[a.name].to_host()
    if check:
        check(out)
    return out


def refused(fx, call, arrs, ws_bytes=0):
    """`call` is refused with FX3D_ERR_INVALID_ARG and a message that names B, and has written nothing: inputs, outputs
    (pre-filled 0xFF), the workspace (the INF fill) and every pad are as they were."""
    arrs = [_sentinel(a) for a in arrs]
    placed = _place(fx, arrs)
    ws = _workspace(fx, ws_bytes)
    ws.fill("INF")
    with pytest.raises(fx.Flux3DHipError) as ei:
        call(fam.Ptrs(**{n: p.ptr for n, p in placed.items()}), ws.ptr, ws.nbytes)
    assert ei.value.code == INVALID, ei.value
    assert re.search(r"\bB\b", str(ei.value)), ei.value
    _sync(fx, "after a refusal")
    ws.check("refused")
    assert ws.unchanged(), "the workspace was written by a refused call"
    for a in arrs:
        assert _bits_equal(placed[a.name].to_host(), a.host), (a.name, "written by a refused call")
        if a.out:
            placed[a.name].check_pads(a.name)


def _same(got, want, what):
    assert _bits_equal(np.asfortranarray(got), np.asfortranarray(want, dtype=got.dtype)), (what, "differing / first:", _first_diff(
        np.asfortranarray(got), np.asfortranarray(want, dtype=got.dtype)))


def run_or_refuse(fx, B, limit, case):
    """`case(B, drive)` states the family at batch size B through `drive` (hold's surface) and compares what it returns with its
    reference.  B within `limit`: it runs.  Beyond: it is refused, then runs at B = 2."""
    if limit == U or B <= limit:
        case(B, hold)
        return

    class _Refused(Exception):
        pass

    def drive(fx_, call, arrs, ws_bytes=0, skip=(), check=None):
        refused(fx_, call, arrs, ws_bytes)
        raise _Refused
    with pytest.raises(_Refused):
        case(B, drive)
    case(2, hold)


# ------------------------------------------------------------------------------------------------------------ nn1 and chamfer
def _plan(fx, N, M, B, D):
    buf = C.create_string_buffer(512)
    fx._lib.call("fx3d_nn1_plan_describe", N, M, B, D, buf, 512)
    return dict(kv.split("=") for kv in buf.value.decode().split())


def _nn_shape(fx, kernel, B):
    """(N = M, D) of the smallest clouds `kernel` takes at this B."""
    if kernel == "f16":
        N = next(n for n in range(4, 4097) if _plan(fx, n, n, B, 3)["kernel"] == "f16")
        assert N * B * 12 < 100e6, N
        return N, 3
    return {"tiny": (4, 3), "small_d": (5, 2), "generic": (5, 8)}[kernel]


_NN_REF = {}


def _nn_case(fx, oracle, kernel, B):
    """Clouds and the oracle's answers for one kernel and batch size, computed once for the four entry points."""
    if (kernel, B) not in _NN_REF:
        N, D = _nn_shape(fx, kernel, B)
        x, y = _rand((D, N, B), 11 * N + D), _rand((D, N, B), 13 * N + D)
        ox, oy, odx, ody = oracle.nn1(x, y, want_dist=True)
        w1, w2, gout = 0.7, 1.3, 2.0
        _NN_REF[(kernel, B)] = (N, D, x, y, ox, oy, odx, ody, oracle.chamfer_distance(x, y, w1, w2), oracle.chamfer_bwd(x, y, ox, oy, w1, w2, gout))
    return _NN_REF[(kernel, B)]


@pytest.mark.parametrize("B", WIDE)
@pytest.mark.parametrize("kernel", ["tiny", "f16", "small_d", "generic"])
@pytest.mark.parametrize("entry", ["nn1", "chamfer_fwd", "chamfer_fwd_bwd", "chamfer_bwd"])
def test_nn1_and_chamfer(gpu_fx, oracle, entry, kernel, B):
    fx = gpu_fx
    N, D, x, y, ox, oy, odx, ody, oloss, (ogx, ogy) = _nn_case(fx, oracle, kernel, B)
    M = N
    assert _plan(fx, N, M, B, D)["kernel"] == kernel
    w1, w2, gout = 0.7, 1.3, 2.0
    idx = [Out("idx_x", (N, B), np.int32), Out("idx_y", (M, B), np.int32)]
    if entry == "nn1":
        r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_nn1")(p.x, N, p.y, M, B, D, p.idx_x, p.idx_y, p.dmin_x, p.dmin_y, None),
                 [I("x", x), I("y", y)] + idx + [Out("dmin_x", (N, B)), Out("dmin_y", (M, B))])
        _same(r["dmin_x"], odx, "dmin_x"), _same(r["dmin_y"], ody, "dmin_y")
    elif entry == "chamfer_bwd":
        r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_chamfer_bwd")(p.x, N, p.y, M, B, D, p.idx_x, p.idx_y, w1, w2, gout, B, p.gx, p.gy, None),
                 [I("x", x), I("y", y), I("idx_x", ox), I("idx_y", oy), Out("gx", (D, N, B)), Out("gy", (D, M, B))])
    elif entry == "chamfer_fwd":
        nb = fx._lib.query_bytes("fx3d_chamfer_workspace_bytes", N, M, B, D)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_chamfer_fwd")(p.x, N, p.y, M, B, D, w1, w2, p.loss, None, p.idx_x, p.idx_y, ws, n, None),
                 [I("x", x), I("y", y), Out("loss", (1,))] + idx, nb)
    else:
        nb = fx._lib.query_bytes("fx3d_chamfer_fwd_bwd_workspace_bytes", N, M, B, D)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_chamfer_fwd_bwd")(p.x, N, p.y, M, B, D, w1, w2, gout, B, p.loss, None, p.gx, p.gy,
                                                                     p.idx_x, p.idx_y, ws, n, None),
                 [I("x", x), I("y", y), Out("loss", (1,)), Out("gx", (D, N, B)), Out("gy", (D, M, B))] + idx, nb)
    if "idx_x" in r:
        _same(r["idx_x"], ox, "idx_x"), _same(r["idx_y"], oy, "idx_y")
    if "gx" in r:
        _same(r["gx"], ogx, "gx"), _same(r["gy"], ogy, "gy")
    if "loss" in r:
        assert np.isclose(r["loss"][0], oloss, rtol=LOSS_RTOL, atol=0), (r["loss"][0], oloss)


def test_nn1_and_chamfer_through_the_python_layer(gpu_fx, oracle):
    """fx.nearest_neighbors and fx.chamfer_distance at B = 65537 (the tiny kernel's clouds)."""
    fx = gpu_fx
    N, D, x, y, ox, oy, odx, ody, _, _ = _nn_case(fx, oracle, "tiny", 65537)
    ix, iy, dx, dy = fx.nearest_neighbors(x, y, return_dist=True)
    _same(ix.to_host(), ox, "idx_x"), _same(iy.to_host(), oy, "idx_y"), _same(dx.to_host(), odx, "dmin_x"), _same(dy.to_host(), ody, "dmin_y")
    loss, ix, iy = fx.chamfer_distance(x, y, w1=0.7, w2=1.3, return_indices=True)
    _same(ix.to_host(), ox, "idx_x"), _same(iy.to_host(), oy, "idx_y")
    assert np.isclose(loss, oracle.chamfer_distance(x, y, 0.7, 1.3), rtol=LOSS_RTOL, atol=0)


# ------------------------------------------------------------------------------------------------------------------------ kNN
# route (csrc/knn.hip: knn_route): (D, M, k, options, the batch is on the grid's y).  N = 2 queries per cloud.
KNN_ROUTES = {
    "F16D3": (3, 64, 4, {}, False),                          # D = 3, the smallest M knn_f16_d3_shape_ok accepts
    "Mfma": (4, 64, 4, {}, False),                           # with the workspace: behind the pre-pass
    "WaveD3": (3, 8, 4, {}, True),
    "WaveGeneric_d2": (2, 8, 4, {}, True),
    "WaveGeneric_d4_no_mfma": (4, 64, 4, {"knn_no_mfma": 1}, True),
    "Select": (3, 80, 65, {}, True),                         # k > 64
}
_KNN_REF = {}


def _knn_ref(oracle, D, N, M, B, k):
    if (D, M, B, k) not in _KNN_REF:
        x, y = _randn((D, N, B), 100 * D + k), _randn((D, M, B), 100 * D + k + 1)
        _KNN_REF[(D, M, B, k)] = (x, y) + tuple(oracle.knn(x, k, y=y, drop_first=False))
    return _KNN_REF[(D, M, B, k)]


def _knn_case(fx, oracle, entry, D, M, k, N=2, expect_ws=None):
    def case(B, drive):
        x, y, oi, od = _knn_ref(oracle, D, N, M, B, k)
        arrs = [I("x", x), I("y", y), Out("idx", (k, N, B), np.int32), Out("dist", (k, N, B))]
        if entry == "fx3d_knn":
            r = drive(fx, lambda p, ws, nb: _abi(fx, entry)(p.x, N, p.y, M, B, D, k, 0, p.idx, p.dist, None), arrs)
        else:
            nb = fx._lib.query_bytes("fx3d_knn_workspace_bytes", N, M, B, D, k, 0)
            assert expect_ws is None or B == 2 or (nb > 0) == expect_ws, nb
            r = drive(fx, lambda p, ws, n: _abi(fx, entry)(p.x, N, p.y, M, B, D, k, 0, p.idx, p.dist, ws if n else None, n, None), arrs, nb)
        _same(r["idx"], oi, "idx"), _same(r["dist"], od, "dist")
    return case


@pytest.mark.parametrize("B", WIDE)
@pytest.mark.parametrize("route", list(KNN_ROUTES))
@pytest.mark.parametrize("entry", ["fx3d_knn", "fx3d_knn_ws"])
def test_knn_routes(gpu_fx, oracle, fx_option, entry, route, B):
    """The matrix-core routes run at all three sizes -- fx3d_knn_ws on the Mfma route behind its pre-pass, whose two kernels had
    the cloud on the grid's y --; the others run at 65535 and are refused at 65536."""
    D, M, k, opts, in_y = KNN_ROUTES[route]
    if in_y and B > GRID_Y + 1:
        return                                # (one refusal per route: at 65536)
    for o, v in opts.items():
        fx_option(o, v)
    # (the size query is a function of the shape alone: under knn_no_mfma it still asks for the pre-pass slabs, which the call
    #  then leaves alone)
    run_or_refuse(gpu_fx, B, GRID_Y if in_y else U, _knn_case(gpu_fx, oracle, entry, D, M, k, expect_ws=True if D == 4 else False))


@pytest.mark.parametrize("B", [32767, 32768])
def test_knn_wide_slices_on_both_sides_of_their_limit(gpu_fx, oracle, B):
    """D = 4, M = 128, k = 33: two verified slices of 32 while B x 2 <= 65535, the wave kernel on the whole clouds beyond; the
    size query and the call change sides together, and the answer is the oracle's on both."""
    fx = gpu_fx
    nb = fx._lib.query_bytes("fx3d_knn_workspace_bytes", 2, 128, B, 4, 33, 0)
    with fx._lib.option("knn_slices", 1):
        unsliced = fx._lib.query_bytes("fx3d_knn_workspace_bytes", 2, 128, B, 4, 33, 0)
    assert unsliced == 0 and (nb > 0) == (B == 32767), (nb, unsliced)
    _knn_case(fx, oracle, "fx3d_knn_ws", 4, 128, 33)(B, lambda *a, **k: hold(*a, guarded=True, **k))   # dirty_ws.Workspace, exact size


def _graph_x(F, N, B, K):
    x = _randn((F, N, B), 7 * F + K + N)
    idx = np.asfortranarray(np.random.default_rng(N + K).integers(0, N, (K, N, B)).astype(np.int32))
    return x, idx


@pytest.mark.parametrize("B", WIDE)
def test_gather_and_edge_features_with_their_adjoint(gpu_fx, oracle, B):
    """F = 3, N = 2, K = 1, any neighbour list: fx3d_knn_gather, fx3d_edge_features at layout 0 and its adjoint at both layouts are
    grid-stride kernels; layout 1 of fx3d_edge_features has the cloud on the grid's y."""
    fx, F, N, K = gpu_fx, 3, 2, 1

    def gather(B, drive):
        x, idx = _graph_x(F, N, B, K)
        r = drive(fx, lambda p, ws, nb: _abi(fx, "fx3d_knn_gather")(p.x, N, B, F, K, p.idx, p.out, None), [I("x", x), I("idx", idx), Out("out", (F, K, N, B))])
        _same(r["out"], oracle.knn_gather(x, idx), "knn_gather")

    def features(layout):
        def case(B, drive):
            x, idx = _graph_x(F, N, B, K)
            oshape = (2 * F, K, N, B) if layout == 0 else (K * N, 2 * F, B)
            r = drive(fx, lambda p, ws, nb: _abi(fx, "fx3d_edge_features")(p.x, N, B, F, K, p.idx, layout, p.out, None),
                      [I("x", x), I("idx", idx), Out("out", oshape)])
            _same(r["out"], oracle.edge_features(x, idx, layout), ("edge_features", layout))
        return case

    def adjoint(layout):
        def case(B, drive):
            g = _randn((2 * F, K, N, B) if layout == 0 else (K * N, 2 * F, B), 31 * F + K + layout)
            r = drive(fx, lambda p, ws, nb: _abi(fx, "fx3d_edge_features_bwd")(p.gout, N, B, F, K, layout, p.gx, None), [I("gout", g), Out("gx", (F, N, B))])
            _same(r["gx"], oracle.edge_features_bwd(g, F, N, B, K, layout), ("edge_features_bwd", layout))
        return case
    run_or_refuse(fx, B, U, gather)
    run_or_refuse(fx, B, U, features(0))
    if B <= GRID_Y + 1:
        run_or_refuse(fx, B, GRID_Y, features(1))
    for layout in (0, 1):
        run_or_refuse(fx, B, U, adjoint(layout))


def _edgeconv_graph_case(fx, oracle, F, N, K, layout):
    def case(B, drive):
        x = _randn((F, N, B), 7 * F + K + N)
        oshape = (2 * F, K, N, B) if layout == 0 else (K * N, 2 * F, B)
        r = drive(fx, lambda p, ws, nb: _abi(fx, "fx3d_edgeconv_graph")(p.x, N, B, F, K, layout, p.idx, p.out, None),
                  [I("x", x), Out("idx", (K, N, B), np.int32), Out("out", oshape)])
        idx = oracle.knn(x, K, drop_first=True, want_dist=False)
        _same(r["idx"], idx, "idx"), _same(r["out"], oracle.edge_features(x, idx, layout), "out")
    return case


@pytest.mark.parametrize("B,layout", [(65535, 0), (65536, 0), (65537, 0), (65537, 1)])
def test_edgeconv_graph_fused(gpu_fx, oracle, B, layout):
    """F = 3, N = 64, K = 1: the search and the features in the D = 3 matrix-core kernel, the batch in the grid's x."""
    run_or_refuse(gpu_fx, B, U, _edgeconv_graph_case(gpu_fx, oracle, 3, 64, 1, layout))


@pytest.mark.parametrize("B,layout", [(65535, 0), (65535, 1), (65536, 0), (65536, 1)])
def test_edgeconv_graph_unfused(gpu_fx, oracle, fx_option, B, layout):
    """F = 3, N = 8, K = 1 with edgeconv_unfused: fx3d_knn on the D = 3 wave kernel (the batch on the grid's y), then
    fx3d_edge_features."""
    fx_option("edgeconv_unfused", 1)
    run_or_refuse(gpu_fx, B, GRID_Y, _edgeconv_graph_case(gpu_fx, oracle, 3, 8, 1, layout))


def test_edgeconv_graph_refuses_layout_1_before_its_search_runs(gpu_fx, oracle, fx_option):
    """F = 4, N = 64 at layout 1: the search is the feature-space matrix-core kernel, which takes 65536 clouds, the features'
    layout-1 kernel does not -- the refusal comes before the search writes idx."""
    fx_option("edgeconv_unfused", 1)
    run_or_refuse(gpu_fx, 65536, GRID_Y, _edgeconv_graph_case(gpu_fx, oracle, 4, 64, 1, 1))


# ------------------------------------------------------------------------------------------------- conversions and the sampler
@pytest.mark.parametrize("B", WIDE[:2])
def test_pointcloud_to_voxel(gpu_fx, oracle, B):
    """res = 2, N = 3.  The parent cleared `voxels` and ran cloud_range_kernel before the launch that cannot take 65536 clouds."""
    run_or_refuse(gpu_fx, B, GRID_Y, lambda B_, drive: fam.pointcloud_to_voxel(gpu_fx, oracle, drive, 2, N=3, B=B_))


def _narrow(B, chunk=64):
    return [(b0, min(chunk, B - b0)) for b0 in range(0, B, chunk)]


@pytest.mark.parametrize("B", WIDE[:2])
def test_trimesh_to_voxel(gpu_fx, B):
    """One triangle per mesh, res = 2.  The wide batch against the same meshes 64 at a time, tests/trimesh_voxel_ref.py on SAMPLE."""
    import trimesh_voxel_ref
    fx, res, Vmax, Fmax = gpu_fx, 2, 3, 1

    def case(B, drive):
        verts = _rand((3, Vmax, B), 5)
        vlen, flen = np.full(B, 3, np.int32), np.ones(B, np.int32)
        faces = np.asfortranarray(np.broadcast_to(np.arange(3, dtype=np.int32).reshape(3, 1, 1), (3, Fmax, B)))
        nb = fx._lib.query_bytes("fx3d_trimesh_voxel_workspace_bytes", Vmax, Fmax, min(B, GRID_Y), res)
        nb = -(-nb * B // min(B, GRID_Y))       # (refused: the last accepted size, scaled)
        vox_elems = res ** 3

        def at(p, ws, n, b0, nb_, vox):
            _abi(fx, "fx3d_trimesh_to_voxel")(p.verts + 36 * b0, Vmax, p.vlen + 4 * b0, p.faces + 12 * b0, Fmax, p.flen + 4 * b0, nb_, res,
                                              vox + 4 * vox_elems * b0, p.bad, ws, n, None)
        arrs = [I("verts", verts), I("vlen", vlen), I("faces", faces), I("flen", flen), Out("vox", (res, res, res, B)), Counter("bad", (1,)),
                Out("vox_narrow", (res, res, res, B))]

        def call(p, ws, n):
            at(p, ws, n, 0, B, p.vox)
            if B > 64:
                for b0, nb_ in _narrow(B):
                    at(p, ws, n, b0, nb_, p.vox_narrow)
        r = drive(fx, call, arrs, nb)
        assert r["bad"][0] == 0
        if B > 64:
            _same(r["vox"], r["vox_narrow"], "wide against narrow batches")
        s = SAMPLE(B)
        want = trimesh_voxel_ref.trimesh_to_voxel([verts[:, :, b] for b in s], [faces[:, :, b] for b in s], res, index_base=0)
        _same(r["vox"][..., s], want, "reference on the sample")
    run_or_refuse(fx, B, GRID_Y, case)


@pytest.mark.parametrize("B", WIDE)
def test_voxel_mesh_count_and_emit(gpu_fx, B):
    """res = 1: a grid is one voxel, a mesh one cube or nothing.  tests/voxel_mesh_ref.py on SAMPLE, the cube's 8 vertices and 12
    faces in every occupied grid against the sample's."""
    import voxel_mesh_ref
    fx, res = gpu_fx, 1
    vox = np.asfortranarray(np.random.default_rng(3).random((res, res, res, B), dtype=np.float32))
    occ = vox.reshape(B) >= np.float32(0.5)     # (an empty grid: K = 0, where the reference throws)
    K = int(occ.sum())
    nb = fx._lib.query_bytes("fx3d_voxel_mesh_workspace_bytes", res, B)
    arrs = [I("vox", vox), Out("cubes", (B,), np.int64), Out("bad", (B,), np.uint32), Out("verts", (3, 8 * K)), Out("faces", (3, 12, B), np.int32)]

    def call(p, ws, n):
        _abi(fx, "fx3d_voxel_mesh_count")(p.vox, res, B, 0.5, p.cubes, p.bad, ws, n, None)
        _abi(fx, "fx3d_voxel_mesh_emit")(res, B, K, p.verts, p.faces, 12, ws, n, None)
    r = hold(fx, call, arrs, nb)
    assert np.array_equal(r["cubes"], occ.astype(np.int64)) and not r["bad"].any()
    first = np.concatenate([[0], np.cumsum(occ)])                 # cubes before grid b
    cube_v = cube_f = None
    for b in SAMPLE(B):
        if occ[b]:
            ev, ef = voxel_mesh_ref.voxel_to_trimesh(np.asfortranarray(vox[..., b]), np.float32(0.5))
            cube_v, cube_f = np.asarray(ev[0], np.float32), ef[0].astype(np.int64) - 1
            _same(r["verts"][:, 8 * first[b]:8 * first[b] + 8], cube_v, ("verts", b))
            assert np.array_equal(r["faces"][:, :, b], cube_f), b
        else:
            assert not r["faces"][:, :, b].any(), b
    assert cube_v is not None and 0 < K < B
    # every grid is the same single voxel: all cubes are the sample's cube
    _same(r["verts"], np.tile(cube_v, (1, K)), "every cube")
    assert np.array_equal(r["faces"][:, :, occ], np.broadcast_to(cube_f[:, :, None], (3, 12, K))) and not r["faces"][:, :, ~occ].any()


def _meshes(B):
    """Vmax = 4, Fmax = 2: a quad's two triangles in the even meshes, its first alone in the odd ones; vertices random per mesh."""
    verts = _rand((3, 4, B), 21)
    flen = (2 - np.arange(B) % 2).astype(np.int32)
    faces = np.zeros((3, 2, B), np.int32, order="F")
    faces[:, 0, :] = np.array([0, 1, 2], np.int32)[:, None]
    faces[:, 1, ::2] = np.array([0, 2, 3], np.int32)[:, None]
    return verts, faces, flen


@pytest.mark.parametrize("B", WIDE)
def test_sampler_and_its_adjoint(gpu_fx, oracle, B):
    """One or two faces per mesh, n = 2 samples: fx3d_sample_points, fx3d_sample_points_cdf + _draw, fx3d_sample_points_explicit and
    the ordered fx3d_sample_points_bwd against the oracle."""
    from test_gpu_topology import host_vertex_faces
    fx, n, seed, Vmax, Fmax = gpu_fx, 2, 11, 4, 2
    verts, faces, flen = _meshes(B)
    out, fi, r1, r2 = oracle.sample_points_seeded(verts, faces, flen, n, seed, return_draws=True)
    nb = fx._lib.query_bytes("fx3d_sample_points_workspace_bytes", Fmax, B)
    mesh = [I("verts", verts), I("faces", faces), I("flen", flen)]
    outs = [Out("out", (3, n, B)), Out("fi", (n, B), np.int32), Out("r1", (n, B)), Out("r2", (n, B))]

    def cdf_draw(p, ws, nn):
        _abi(fx, "fx3d_sample_points_cdf")(p.verts, Vmax, p.faces, Fmax, p.flen, B, 1e-6, ws, nn, None)
        _abi(fx, "fx3d_sample_points_draw")(p.verts, Vmax, p.faces, Fmax, p.flen, B, n, seed, None, ws, nn, p.out, p.fi, p.r1, p.r2, None)
    for call in (lambda p, ws, nn: _abi(fx, "fx3d_sample_points")(p.verts, Vmax, p.faces, Fmax, p.flen, B, n, 1e-6, seed, p.out, p.fi, p.r1, p.r2,
                                                                  ws, nn, None), cdf_draw):
        r = hold(fx, call, mesh + outs, nb)
        _same(r["out"], out, "out"), _same(r["fi"], fi, "fi"), _same(r["r1"], r1, "r1"), _same(r["r2"], r2, "r2")
    draws = [I("fi", fi), I("r1", r1), I("r2", r2)]
    r = hold(fx, lambda p, ws, nn: _abi(fx, "fx3d_sample_points_explicit")(p.verts, Vmax, p.faces, Fmax, B, n, p.fi, p.r1, p.r2, p.out, None),
             mesh[:2] + draws + [Out("out", (3, n, B))])
    _same(r["out"], oracle.sample_points_explicit(verts, faces, fi, r1, r2), "explicit")
    vfr, vfe = host_vertex_faces(fx._lib, faces, flen, Vmax)
    g = _randn((3, n, B), 4)
    r = hold(fx, lambda p, ws, nn: _abi(fx, "fx3d_sample_points_bwd")(p.faces, Vmax, Fmax, B, n, p.fi, p.r1, p.r2, p.gout, p.gverts, 0, p.vfr, p.vfe, None),
             [I("faces", faces)] + draws + [I("gout", g), I("vfr", vfr), I("vfe", vfe), Out("gverts", (3, Vmax, B))])
    _same(r["gverts"], oracle.sample_points_bwd(faces, flen, Vmax, fi, r1, r2, g), "gverts")


@pytest.mark.parametrize("B", WIDE[:2])
def test_sampler_multi_block_cdf(gpu_fx, oracle, fx_option, B):
    """The CDF built by several blocks per mesh (cdf_multiblock_from lowered to one face) has the meshes on the grid's y."""
    fx, n, seed, Vmax, Fmax = gpu_fx, 2, 11, 4, 2
    fx_option("cdf_multiblock_from", 1)

    def case(B, drive):
        verts, faces, flen = _meshes(B)
        nb = fx._lib.query_bytes("fx3d_sample_points_workspace_bytes", Fmax, B)
        r = drive(fx, lambda p, ws, nn: _abi(fx, "fx3d_sample_points")(p.verts, Vmax, p.faces, Fmax, p.flen, B, n, 1e-6, seed, p.out, p.fi, p.r1, p.r2,
                                                                      ws, nn, None),
                  [I("verts", verts), I("faces", faces), I("flen", flen), Out("out", (3, n, B)), Out("fi", (n, B), np.int32), Out("r1", (n, B)),
                   Out("r2", (n, B))], nb)
        out, fi, r1, r2 = oracle.sample_points_seeded(verts, faces, flen, n, seed, return_draws=True)
        _same(r["out"], out, "out"), _same(r["fi"], fi, "fi"), _same(r["r1"], r1, "r1"), _same(r["r2"], r2, "r2")
    run_or_refuse(fx, B, GRID_Y, case)


@pytest.mark.parametrize("B", WIDE)
def test_packed_and_padded_vertices(gpu_fx, B):
    """Meshes of 1 or 2 vertices, Vmax = 2: one device copy per mesh each way."""
    fx, Vmax = gpu_fx, 2
    vlen = (1 + np.arange(B) % 2).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(vlen)])
    packed = _rand((3, int(off[-1])), 8)
    padded = np.zeros((3, Vmax, B), np.float32, order="F")
    padded[:, 0, :] = packed[:, off[:-1]]
    padded[:, 1, 1::2] = packed[:, off[1:-1:2] + 1]
    lens = vlen.ctypes.data
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_packed_to_padded")(p.packed, lens, B, Vmax, p.padded, None), [I("packed", packed), Out("padded", (3, Vmax, B))])
    _same(r["padded"], padded, "padded")
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_padded_to_packed")(p.padded, lens, B, Vmax, p.packed, None), [I("padded", padded), Out("packed", packed.shape)])
    _same(r["packed"], packed, "packed")


@pytest.mark.parametrize("B", WIDE)
def test_topology_tables_on_the_device(gpu_fx, B):
    """fx3d_vertex_faces_dev against the host builder, fx3d_faces_padded_to_packed_dev against integer numpy."""
    from test_gpu_topology import host_vertex_faces
    fx, Vmax, Fmax = gpu_fx, 4, 2
    _, faces, flen = _meshes(B)
    hvr, hve = host_vertex_faces(fx._lib, faces, flen, Vmax)
    nb = fx._lib.query_bytes("fx3d_vertex_faces_dev_workspace_bytes", Vmax, Fmax, B)
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_vertex_faces_dev")(p.faces, p.flen, Vmax, Fmax, B, p.vfr, p.vfe, p.bad, ws, n, None),
             [I("faces", faces), I("flen", flen), Out("vfr", (Vmax + 1, B), np.int32), Out("vfe", (3 * Fmax, B), np.int32), Out("bad", (1,), np.uint32)], nb)
    assert r["bad"][0] == 0
    _same(r["vfr"], hvr, "vf_rowptr"), _same(r["vfe"], hve, "vf_ent")
    nverts = (3 + (flen == 2)).astype(np.int32)
    voff = np.concatenate([[0], np.cumsum(nverts)[:-1]]).astype(np.int32)
    keep = (np.arange(Fmax)[:, None] < flen[None, :])                      # (Fmax, B)
    want = (faces + voff[None, None, :]).transpose(0, 2, 1)[:, keep.T]     # mesh by mesh, face by face
    sumF = int(flen.sum())
    nb = fx._lib.query_bytes("fx3d_faces_padded_to_packed_dev_workspace_bytes", B)
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_faces_padded_to_packed_dev")(p.faces, p.flen, p.nverts, Fmax, B, sumF, p.packed, ws, n, None),
             [I("faces", faces), I("flen", flen), I("nverts", nverts), Out("packed", (3, sumF), np.int32)], nb)
    _same(r["packed"], want, "packed faces")


# ----------------------------------------------------------------------------------------------------------------- transforms
@pytest.mark.parametrize("B", WIDE[:2])
@pytest.mark.parametrize("entry", ["fx3d_segment_minmax", "fx3d_normalize", "fx3d_realign", "fx3d_rotate"])
def test_transforms(gpu_fx, entry, B):
    """(3, 2, B) clouds: a segment is a row of the grid's y."""
    fx, D, n = gpu_fx, 3, 2

    def case(B, drive):
        x = _randn((D, n, B), 1000 * D + n) + np.float32(3.0)
        nb = fx._lib.query_bytes("fx3d_transform_workspace_bytes", D, n, min(B, GRID_Y))
        smin, smax = tref.jmin(x, 1)[:, 0, :], tref.jmax(x, 1)[:, 0, :]
        if entry == "fx3d_segment_minmax":
            r = drive(fx, lambda p, ws, n_: _abi(fx, entry)(p.x, D, n, B, None, 0, p.mn, p.mx, ws if n_ else None, n_, None),
                      [I("x", x), Out("mn", (D, B)), Out("mx", (D, B))], nb)
            assert tref.same_bits(r["mn"], smin) and tref.same_bits(r["mx"], smax)
        elif entry == "fx3d_normalize":
            r = drive(fx, lambda p, ws, n_: _abi(fx, entry)(p.x, D, n, B, None, 0, p.y, p.c, p.s, ws if n_ else None, n_, None),
                      [I("x", x), Out("y", x.shape), Out("c", (D, B)), Out("s", (D, B))], nb)
            wc, wsd = tref.pcloud_stats(x)
            assert tref.within_ulp(r["c"], wc) and tref.within_ulp(r["s"], wsd)
            assert tref.same_bits(r["y"], tref.pcloud_normalize(x, r["c"], r["s"]))
        elif entry == "fx3d_realign":
            tmin, tmax = np.full((D, 1), -2.0, np.float32), np.linspace(1, 3, D, dtype=np.float32).reshape(D, 1)
            r = drive(fx, lambda p, ws, n_: _abi(fx, entry)(p.x, D, n, B, None, p.smin, p.smax, p.tmin, p.tmax, p.y, None),
                      [I("x", x), I("smin", smin), I("smax", smax), I("tmin", tmin), I("tmax", tmax), Out("y", x.shape)])
            assert tref.same_bits(r["y"], tref.pcloud_realign(x, tmin, tmax))
        else:
            Rb = _randn((3, 3, B), 6)
            r = drive(fx, lambda p, ws, n_: _abi(fx, entry)(p.x, n * B, n, B, None, None, p.R, p.y, None), [I("x", x), I("R", Rb), Out("y", x.shape)])
            assert tref.same_bits(r["y"], tref.pcloud_rotate(x, Rb))
    run_or_refuse(fx, B, GRID_Y, case)


# --------------------------------------------------------------------------------------------------------------------- models
def test_crossentropy(gpu_fx):
    """One block walks the batch: 65537 columns of 3 classes against tests/train_step_ref.py."""
    import train_step_ref
    fx, nc, B = gpu_fx, 3, 65537
    rng = np.random.default_rng(9)
    probs = rng.random((nc, B), dtype=np.float32) + np.float32(0.05)
    probs = np.asfortranarray(probs / probs.sum(axis=0, keepdims=True, dtype=np.float32))
    labels = rng.integers(0, nc, B).astype(np.int32)
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_crossentropy")(p.probs, p.labels, nc, B, p.glogits, p.loss, p.counts, None),
             [I("probs", probs), I("labels", labels), Out("glogits", (nc, B)), Out("loss", (1,), np.float64), Out("counts", (2,), np.int32)])
    loss, glogits, counts = train_step_ref.crossentropy(probs, labels)
    _same(r["glogits"], glogits, "glogits")
    assert np.array_equal(r["counts"], counts) and counts[1] == 0 and 0 < counts[0] < B, (r["counts"], counts)
    # the log is the device's: tests/test_gpu_train_step.py's bound, one rounding of the running Float64 sum per column
    bound = (B + 4) * 2.0 ** -53 * np.abs(np.log(probs[labels, np.arange(B)].astype(np.float64))).max()
    assert abs(r["loss"][0] - loss) <= bound, (r["loss"][0], loss, bound)


def _count(fx, name, *args):
    n = C.c_int64(0)
    fx._lib.call(name, *args, C.byref(n))
    return n.value


def _scaled(fx, query, args_at):
    """The workspace a refused call would need: the size queried at B = 65535, scaled to 65536."""
    return -(-fx._lib.query_bytes(query, *args_at(GRID_Y)) * (GRID_Y + 1) // GRID_Y)


EDGE_LAYERS = [3, 32]


def _edgeconv_forward_case(fx):
    """fx3d_edgeconv_forward, layers [3, 32], K = 1, N = 2 (each point's neighbour is the other one)."""
    import edgeconv_ref
    L, nl, K, N = (C.c_int32 * 2)(*EDGE_LAYERS), 2, 1, 2
    P = edgeconv_ref.random_params(EDGE_LAYERS, 5)
    params = fx.EdgeConv(EDGE_LAYERS, K).load(P).flat_params()

    def case(B, drive):
        x = _randn((3, N, B), 77)
        nb = fx._lib.query_bytes("fx3d_edgeconv_workspace_bytes", L, nl, K, N, min(B, GRID_Y))
        nb = -(-nb * B // min(B, GRID_Y))
        arrs = [I("params", params), I("x", x), Out("out", (32, N, B)), Out("idx", (K, N, B), np.int32), Out("out_narrow", (32, N, B)),
                Out("idx_narrow", (K, N, B), np.int32)]

        def at(p, ws, n, b0, nb_, out, idx):
            _abi(fx, "fx3d_edgeconv_forward")(p.params, L, nl, K, p.x + 4 * 3 * N * b0, N, nb_, None, out + 4 * 32 * N * b0, idx + 4 * K * N * b0, ws, n, None)

        def call(p, ws, n):
            at(p, ws, n, 0, B, p.out, p.idx)
            if B > 64:
                for b0, nb_ in _narrow(B):
                    at(p, ws, n, b0, nb_, p.out_narrow, p.idx_narrow)
        r = drive(fx, call, arrs, nb)
        if B > 64:
            _same(r["out"], r["out_narrow"], "wide against narrow batches"), _same(r["idx"], r["idx_narrow"], "idx, wide against narrow")
        s = SAMPLE(B)
        idx, out = edgeconv_ref.forward(np.asfortranarray(x[:, :, s]), P, EDGE_LAYERS, K)
        assert np.array_equal(r["idx"][:, :, s], idx)
        assert tref.same_bits(np.asfortranarray(r["out"][:, :, s]).ravel(order="F"), np.asarray(out, np.float32).ravel(order="F"))
    return case


@pytest.mark.parametrize("B", WIDE[:2])
def test_edgeconv_forward(gpu_fx, B):
    run_or_refuse(gpu_fx, B, GRID_Y, _edgeconv_forward_case(gpu_fx))


def _edgeconv_bwd_case(fx):
    """fx3d_edgeconv_bwd with idx = out = NULL (the search and the forward run first, into the workspace): the input gradient is
    a cloud's own, so narrow batches give the same bits."""
    import edgeconv_bwd_ref
    import edgeconv_ref
    L, nl, K, N, cL = (C.c_int32 * 2)(*EDGE_LAYERS), 2, 1, 2, EDGE_LAYERS[-1]
    P = edgeconv_ref.random_params(EDGE_LAYERS, 5)
    params = fx.EdgeConv(EDGE_LAYERS, K).load(P).flat_params()

    def case(B, drive):
        x, gout = _randn((3, N, B), 77), _randn((cL, N, B), 78)
        nb = fx._lib.query_bytes("fx3d_edgeconv_bwd_workspace_bytes", L, nl, K, N, min(B, GRID_Y))
        nb = -(-nb * B // min(B, GRID_Y))

        def at(p, ws, n, b0, nb_, gx):
            _abi(fx, "fx3d_edgeconv_bwd")(p.params, L, nl, K, p.x + 4 * 3 * N * b0, N, nb_, None, None, p.gout + 4 * cL * N * b0, gx + 4 * 3 * N * b0,
                                          ws, n, None)

        def call(p, ws, n):
            at(p, ws, n, 0, B, p.gx)
            if B > 64:
                for b0, nb_ in _narrow(B):
                    at(p, ws, n, b0, nb_, p.gx_narrow)
        r = drive(fx, call, [I("params", params), I("x", x), I("gout", gout), Out("gx", (3, N, B)), Out("gx_narrow", (3, N, B))], nb)
        if B > 64:
            _same(r["gx"], r["gx_narrow"], "wide against narrow batches")
        s = SAMPLE(B)
        xs, gs = np.asfortranarray(x[:, :, s]), np.asfortranarray(gout[:, :, s])
        idx, out = edgeconv_ref.forward(xs, P, EDGE_LAYERS, K)
        want = edgeconv_bwd_ref.input_grad(xs, P, EDGE_LAYERS, K, gs, idx, out)
        assert tref.same_bits(np.asfortranarray(r["gx"][:, :, s]).ravel(order="F"), np.asarray(want, np.float32).ravel(order="F"))
    return case


@pytest.mark.parametrize("B", WIDE[:2])
def test_edgeconv_bwd(gpu_fx, B):
    run_or_refuse(gpu_fx, B, GRID_Y, _edgeconv_bwd_case(gpu_fx))


def _dgcnn_forward_case(fx):
    """fx3d_dgcnn_forward, K = 1, N = 2, 10 classes: probs and logits (the other outputs NULL: they live in the workspace)."""
    import dgcnn_ref
    nc, K, N = 10, 1, 2
    P = dgcnn_ref.random_params(nc, seed=3)
    params = fx.DGCNN(nc, K, npoints=N).load(P).flat_params()

    def case(B, drive):
        x = _randn((3, N, B), 27)
        nb = fx._lib.query_bytes("fx3d_dgcnn_workspace_bytes", N, min(B, GRID_Y), K, nc)
        nb = -(-nb * B // min(B, GRID_Y))
        arrs = [I("params", params), I("x", x)] + [Out(k, (nc, B)) for k in ("probs", "logits", "probs_narrow", "logits_narrow")]

        def at(p, ws, n, b0, nb_, probs, logits):
            _abi(fx, "fx3d_dgcnn_forward")(p.params, nc, K, p.x + 4 * 3 * N * b0, N, nb_, probs + 4 * nc * b0, logits + 4 * nc * b0, None, None, None,
                                           None, None, ws, n, None)

        def call(p, ws, n):
            at(p, ws, n, 0, B, p.probs, p.logits)
            if B > 64:
                for b0, nb_ in _narrow(B):
                    at(p, ws, n, b0, nb_, p.probs_narrow, p.logits_narrow)
        r = drive(fx, call, arrs, nb)
        if B > 64:
            _same(r["probs"], r["probs_narrow"], "probs, wide against narrow batches"), _same(r["logits"], r["logits_narrow"], "logits, wide against narrow")
        s = SAMPLE(B)
        want = dgcnn_ref.forward(np.asfortranarray(x[:, :, s]), P, K)
        assert tref.same_bits(np.asfortranarray(r["logits"][:, s]).ravel(order="F"), np.asarray(want["logits"], np.float32).ravel(order="F"))
    return case


@pytest.mark.parametrize("B", WIDE[:2])
def test_dgcnn_forward(gpu_fx, B):
    run_or_refuse(gpu_fx, B, GRID_Y, _dgcnn_forward_case(gpu_fx))


def _model_refusals(fx):
    """{entry point: (call(p, ws, n), arrays, workspace bytes, the family's run at B = 2)} at B = 65536 with every optional
    argument NULL and every other buffer of the size the call would take."""
    B, nc = GRID_Y + 1, 10
    out = {}
    # PointNet, N = 1
    N = 1
    pp = np.zeros(_count(fx, "fx3d_pointnet_param_count", nc), np.float32)
    ps = np.zeros(_count(fx, "fx3d_pointnet_stat_count"), np.float32)
    x1 = _randn((3, N, B), 1)
    out["fx3d_pointnet_forward"] = (
        lambda p, ws, n: _abi(fx, "fx3d_pointnet_forward")(p.params, nc, p.x, N, B, p.probs, None, None, None, None, ws, n, None),
        [I("params", pp), I("x", x1), Out("probs", (nc, B))], _scaled(fx, "fx3d_pointnet_workspace_bytes", lambda b: (N, b, nc)),
        lambda: fam.pointnet(fx, hold, "forward"))
    out["fx3d_pointnet_forward_train"] = (
        lambda p, ws, n: _abi(fx, "fx3d_pointnet_forward_train")(p.params, nc, p.x, N, B, None, 0.1, p.probs, None, None, None, None, p.stats, None, ws, n, None),
        [I("params", pp), I("x", x1), Out("probs", (nc, B)), Out("stats", ps.shape)], _scaled(fx, "fx3d_pointnet_train_workspace_bytes", lambda b: (N, b, nc)),
        lambda: fam.pointnet(fx, hold, "forward_train"))
    # DGCNN, N = 2, K = 1
    N, K = 2, 1
    dp = np.zeros(_count(fx, "fx3d_dgcnn_param_count", nc), np.float32)
    ds = np.zeros(_count(fx, "fx3d_dgcnn_stat_count"), np.float32)
    x2 = _randn((3, N, B), 2)
    out["fx3d_dgcnn_forward"] = (
        lambda p, ws, n: _abi(fx, "fx3d_dgcnn_forward")(p.params, nc, K, p.x, N, B, p.probs, None, None, None, None, None, None, ws, n, None),
        [I("params", dp), I("x", x2), Out("probs", (nc, B))], _scaled(fx, "fx3d_dgcnn_workspace_bytes", lambda b: (N, b, K, nc)),
        lambda: fam.dgcnn(fx, hold, "forward"))
    out["fx3d_dgcnn_forward_train"] = (
        lambda p, ws, n: _abi(fx, "fx3d_dgcnn_forward_train")(p.params, nc, K, p.x, N, B, None, None, 0.1, p.probs, None, None, None, None, None, None,
                                                             p.stats, None, ws, n, None),
        [I("params", dp), I("x", x2), Out("probs", (nc, B)), Out("stats", ds.shape)], _scaled(fx, "fx3d_dgcnn_train_workspace_bytes", lambda b: (N, b, K, nc)),
        lambda: fam.dgcnn(fx, hold, "forward_train"))
    # EdgeConv [3, 32], N = 2, K = 1
    L, nl, cL = (C.c_int32 * 2)(*EDGE_LAYERS), 2, EDGE_LAYERS[-1]
    ep = np.zeros(_count(fx, "fx3d_edgeconv_param_count", L, nl), np.float32)
    es = np.zeros(_count(fx, "fx3d_edgeconv_stat_count", L, nl), np.float32)
    gout, eout, idx = _randn((cL, N, B), 3), _randn((cL, N, B), 4), np.zeros((K, N, B), np.int32)
    name = "3_32_64_64"
    q = lambda stem: _scaled(fx, f"fx3d_edgeconv{stem}_workspace_bytes", lambda b: (L, nl, K, N, b))  # noqa: E731
    out["fx3d_edgeconv_forward_train"] = (
        lambda p, ws, n: _abi(fx, "fx3d_edgeconv_forward_train")(p.params, L, nl, K, p.x, N, B, None, 0.1, p.out, None, p.stats, None, ws, n, None),
        [I("params", ep), I("x", x2), Out("out", (cL, N, B)), Out("stats", es.shape)], q("_train"), lambda: fam.edgeconv(fx, hold, name, "forward_train"))
    out["fx3d_edgeconv_bwd"] = (
        lambda p, ws, n: _abi(fx, "fx3d_edgeconv_bwd")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, p.gout, p.gx, ws, n, None),
        [I("params", ep), I("x", x2), I("idx", idx), I("out", eout), I("gout", gout), Out("gx", (3, N, B))], q("_bwd"), lambda: fam.edgeconv(fx, hold, name, "bwd"))
    out["fx3d_edgeconv_grad"] = (
        lambda p, ws, n: _abi(fx, "fx3d_edgeconv_grad")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, p.gout, p.gparams, p.gx, ws, n, None),
        [I("params", ep), I("x", x2), I("idx", idx), I("out", eout), I("gout", gout), Out("gparams", ep.shape), Out("gx", (3, N, B))], q("_grad"),
        lambda: fam.edgeconv(fx, hold, name, "grad"))
    out["fx3d_edgeconv_grad_train"] = (
        lambda p, ws, n: _abi(fx, "fx3d_edgeconv_grad_train")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, p.stats, p.gout, p.gparams, p.gx, ws, n, None),
        [I("params", ep), I("x", x2), I("idx", idx), I("out", eout), I("stats", es), I("gout", gout), Out("gparams", ep.shape), Out("gx", (3, N, B))],
        q("_grad_train"), lambda: fam.edgeconv(fx, hold, name, "grad_train"))
    return out


# (fx3d_edgeconv_forward, fx3d_edgeconv_bwd and fx3d_dgcnn_forward: refused in the tests above, next to their runs)
MODEL_REFUSALS = ["fx3d_pointnet_forward", "fx3d_pointnet_forward_train", "fx3d_dgcnn_forward_train",
                  "fx3d_edgeconv_forward_train", "fx3d_edgeconv_grad", "fx3d_edgeconv_grad_train"]


@pytest.mark.parametrize("entry", MODEL_REFUSALS)
def test_model_entry_points_refuse_65536_clouds(gpu_fx, entry):
    """The size check of every model entry point comes before its first launch; the same entry point then runs tests/abi_families.py's
    case at B = 2 against its restatement."""
    call, arrs, nb, at_two = _model_refusals(gpu_fx)[entry]
    refused(gpu_fx, call, arrs, nb)
    at_two()
