"""Every entry point that takes ``(ws, ws_bytes)`` on dirty scratch of exactly the queried size (DESIGN.md 2.2 "What a call may
assume about its workspace").

A caller of the C ABI hands over recycled memory of exactly ``*_workspace_bytes()`` bytes.  The rest of the GPU suite never
does: its scratch is zero or what the same entry point left, at least 4096 bytes, with nothing checked behind it.  Each case
here runs one family of tests/abi_families.py -- the same call and the same reference as tests/test_gpu_alignment.py -- through
``hold`` below, which places the workspace with tests/dirty_ws.py and makes the call once per fill, ZERO, STALE, INF, ONES:

  * ZERO: outputs equal the family's reference exactly as the family's own test checks it (the family asserts that on what
    ``hold`` returns);
  * STALE, INF, ONES: every output bit-equal to the ZERO run, NaN payloads included (the float-atomic routes: the family's bound);
  * after EVERY C-ABI call -- each call of a carried pair, the fill going in before the first only -- the guard pads around the
    workspace intact; after the run the pads around every output intact and every input unwritten.

Each entry point runs at the alignment file's shape and at a ragged one (padded rows, a tail tile).  ``test_refusal`` gives every
entry point ``queried - 1`` bytes, NULL and, where the header promises it, ``ws + 16``: the documented status, and not one byte
of an output (pre-filled 0xA5) or of the workspace changed; the documented fall-backs give the full call's bits.
tests/test_dirty_ws_host.py holds the table complete against ``_lib.SIGNATURES`` without a GPU."""
import numpy as np
import pytest

import abi_families as fam
import dirty_ws as dirty
import misaligned as mis
from abi_families import _bits_equal, _first_diff

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = -1, -6   # FX3D_ERR_INVALID_ARG, FX3D_ERR_WORKSPACE (include/flux3d_hip.h)


@pytest.fixture(autouse=True)
def fresh_nullable():
    fam.NULLABLE.clear()


# ---------------------------------------------------------------------------------------------------------------- the driver
def _sync(fx, what):
    try:
        fx.synchronize()
    except fx.Flux3DHipError as e:  # a fault: nothing more is started on the device
        pytest.exit(f"{what}: {e}", returncode=3)


REORDERED = ("faces", "edges")   # (3, F[, B]) faces, columns reversed; (E, 2) edges, rows reversed (CSR offsets, lengths, lists stay)
KEPT = ("params", "stats")   # a model's parameters and batch statistics stay what they are in the run that leaves STALE: a valid model


def _place(fx, arrs, prime=False, poison=False):
    """Every array at an aligned address between pads.  `prime`: the inputs of the run that leaves STALE behind;  `poison`: outputs
    pre-filled 0xA5 (a refused call must leave them so)."""
    placed = {}
    for a in arrs:
        host = a.host
        if prime and not a.out and a.name not in KEPT:
            host = dirty.other_inputs(host)
            if a.name in REORDERED and host.ndim >= 2:   # other index inputs that stay in range: the same faces / edges in reverse order
                host = np.asfortranarray(np.flip(host, axis=1 if a.name == "faces" else 0))
        if poison and a.out:
            host = np.full(host.nbytes, mis.OUTPUT_BYTE, np.uint8).view(host.dtype).reshape(host.shape, order="F")
        placed[a.name] = (mis.place(fx, host, 0, output=a.out), np.asfortranarray(host))
    return placed


def _run(fx, call, arrs, ws, what, prime=False):
    """The call on `ws` as it is: {output name: host result}; the workspace's guard pads checked after every C-ABI call the closure
    makes and at the end, the outputs' pads and the inputs' contents at the end."""
    placed = _place(fx, arrs, prime)

    def after(name):
        _sync(fx, f"{what}: {name}")
        ws.check(f"{what}, after {name}")
    fam.Calls.after = after
    try:
        call(fam.Ptrs(**{n: p.ptr for n, (p, _) in placed.items()}), ws.ptr, ws.nbytes)
    finally:
        fam.Calls.after = None
    _sync(fx, what)
    ws.check(what)
    out = {}
    for a in arrs:
        p, host = placed[a.name]
        if a.out:
            p.check_pads(f"{a.name} ({what})")
            out[a.name] = p.to_host()
        else:
            assert _bits_equal(p.to_host(), host), f"input {a.name} was written ({what})"
    return out


def hold(fx, call, arrs, ws_bytes=0, skip=(), check=None):
    """`call` on a workspace of exactly `ws_bytes` bytes under every fill of dirty_ws.PATTERNS, in that order: all outputs bit-equal
    to the ZERO run's (`check`: instead, every run through the family's bound).  Returns the ZERO run's results for the
    comparison with the family's reference.  A call without a workspace (a 0-byte query: NULL) runs once."""
    ws = dirty.Workspace(fx, ws_bytes)
    if ws.nbytes == 0:
        base = _run(fx, call, arrs, ws, "no workspace")
        if check:
            check(base)
        return base
    base = None
    for pattern in dirty.patterns(ws, prime=lambda: _run(fx, call, arrs, ws, "the run that leaves STALE", prime=True)):
        got = _run(fx, call, arrs, ws, pattern)
        if check:
            check(got)
        elif base is not None:
            for k, want in base.items():
                assert _bits_equal(got[k], want), (pattern, k, "elements differing from the ZERO run / first:", _first_diff(got[k], want))
        base = base or got
    return base


# ------------------------------------------------------------------------------------------------------------------ the cases
class Case:
    """One family at one shape.  `entries`: the workspace-taking entry points (and the later calls of their carried pairs) it
    runs;  `queries`: the size queries it makes;  `refuse`: {entry: status} -- the case is also the entry's refusal case."""

    def __init__(self, name, run, entries, queries, refuse=None):
        self.name, self.run, self.entries, self.queries, self.refuse = name, run, tuple(entries), tuple(queries), dict(refuse or {})

    def __repr__(self):
        return self.name


def _smallest_transform_n(fx, D, B=2):
    """The smallest n whose fx3d_transform_workspace_bytes(D, n, B) is positive (short clouds reduce in one block: no scratch)."""
    n = 1
    while fx._lib.query_bytes("fx3d_transform_workspace_bytes", D, n, B) == 0:
        n *= 2
        assert n <= 1 << 24
    lo, hi = n // 2, n     # query(lo) == 0 < query(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if fx._lib.query_bytes("fx3d_transform_workspace_bytes", D, mid, B) else (mid, hi)
    assert fx._lib.query_bytes("fx3d_transform_workspace_bytes", D, hi, B) > 0 == fx._lib.query_bytes("fx3d_transform_workspace_bytes", D, hi - 1, B)
    return hi


def _transforms(fx, oracle, opt, hold_, D, plus):
    fam.transforms_dense(fx, hold_, D, _smallest_transform_n(fx, D) + plus, only_ws=True)


def _models_without(family, *args, **kw):
    """The model entry point with every output given, then with its optional outputs NULL (those then live in the workspace): the
    outputs it still gives are the full call's bits (the family holds them to the restatement; probs through the full call)."""
    def run(fx, oracle, opt, hold_):
        full = {}

        def keep(fx_, call, arrs, ws_bytes=0, skip=(), check=None):
            full.update(hold_(fx_, call, arrs, ws_bytes, skip, check))
            return full
        family(fx, keep, *args, **{k: v for k, v in kw.items() if k not in ("without", "null_inputs")})
        part = {}

        def keep2(fx_, call, arrs, ws_bytes=0, skip=(), check=None):
            part.update(hold_(fx_, call, arrs, ws_bytes, skip, check))
            return part
        family(fx, keep2, *args, **kw)
        assert part and set(part) <= set(full)
        for k, v in part.items():
            assert _bits_equal(v, full[k]), (k, _first_diff(v, full[k]))
    return run


def _fwd_bwd_idx_null(shape):
    """fx3d_chamfer_fwd_bwd with every output, then with idx_x = idx_y = NULL: loss, gx and gy bit-equal."""
    def run(fx, oracle, opt, hold_):
        def family(fx_, h, **kw):
            fam.nn1_and_chamfer(fx_, oracle, opt, h, shape, "chamfer_fwd_bwd", **kw)
        _models_without(family, without=("idx_x", "idx_y"))(fx, oracle, opt, hold_)
    return run


CH, CHQ = "fx3d_chamfer_fwd", "fx3d_chamfer_workspace_bytes"
MODEL_OPTIONAL = {   # the optional outputs of each model entry point (include/flux3d_hip.h)
    "pointnet": {"forward": ("logits", "stn", "fstn", "pooled"), "forward_train": ("logits", "stn", "fstn", "pooled", "running"),
                 "grad": ("gx", "gstn", "gfstn", "gh", "gxt"), "grad_train": ("gx", "gstn", "gfstn", "gh", "gxt")},
    "dgcnn": {"forward": ("logits", "idx1", "x1", "idx2", "x2", "pooled"), "forward_train": ("logits", "idx1", "x1", "idx2", "x2", "pooled", "running"),
              "grad": ("gx", "gx2", "gx1"), "grad_train": ("gx", "gx2", "gx1")},
    "edgeconv": {"forward_train": ("running",), "grad": ("gx",), "grad_train": ("gx",)},
}


def _cases():
    out = []

    def add(name, run, entries, queries, refuse=None):
        out.append(Case(name, run, entries, queries, refuse))
    # ---- chamfer
    for shape in ("1024", "split_plan", "r257_d3", "r130_d2", "r130_d64"):
        first = shape == "1024"
        add(f"chamfer_fwd-{shape}", lambda fx, o, opt, h, s=shape: fam.nn1_and_chamfer(fx, o, opt, h, s, "chamfer_fwd"), [CH], [CHQ],
            {CH: WORKSPACE} if first else None)
        add(f"chamfer_fwd_bwd-{shape}", lambda fx, o, opt, h, s=shape: fam.nn1_and_chamfer(fx, o, opt, h, s, "chamfer_fwd_bwd"),
            ["fx3d_chamfer_fwd_bwd"], ["fx3d_chamfer_fwd_bwd_workspace_bytes"], {"fx3d_chamfer_fwd_bwd": WORKSPACE} if first else None)
        if True:   # (the split plan too: its finalise launch writes the sums)
            add(f"chamfer_sums-{shape}", lambda fx, o, opt, h, s=shape: fam.chamfer_sums_and_finalize(fx, o, opt, h, s),
                ["fx3d_chamfer_sums", "fx3d_chamfer_finalize", "fx3d_chamfer_finalize_many"], [CHQ], {"fx3d_chamfer_sums": WORKSPACE} if first else None)
    for shape in ("1024", "r257_d3"):   # idx_x = idx_y = NULL: the indices the adjoint dereferences live in the workspace
        add(f"chamfer_fwd_bwd-{shape}-idx_null", _fwd_bwd_idx_null(shape), ["fx3d_chamfer_fwd_bwd"], ["fx3d_chamfer_fwd_bwd_workspace_bytes"])
    for N, M, B, D in ((1024, 1024, 2, 3), (257, 131, 3, 3), (130, 77, 2, 2), (130, 77, 2, 64)):
        for e in ("fx3d_chamfer_fwd_sharded", "fx3d_chamfer_fwd_sharded_async"):
            add(f"{e[5:]}-{N}x{M}x{B}_d{D}", lambda fx, o, opt, h, e=e, a=(N, M, B, D): fam.chamfer_sharded(fx, o, h, e, *a), [e], [CHQ],
                {e: WORKSPACE} if N == 1024 else None)
    for N, M, B in ((1024, 1024, 2), (65, 33, 3)):
        add(f"chamfer_pairwise-{N}x{M}x{B}", lambda fx, o, opt, h, a=(N, M, B): fam.chamfer_pairwise(fx, o, h, *a), ["fx3d_chamfer_loss_pairwise_f32"],
            ["fx3d_chamfer_pairwise_workspace_bytes"], {"fx3d_chamfer_loss_pairwise_f32": WORKSPACE} if N == 1024 else None)
    SB = "fx3d_chamfer_sampled_bwd"
    for n in (100, 257):
        add(f"chamfer_sampled_bwd-ragged3_n{n}", lambda fx, o, opt, h, n=n: fam.chamfer_sampled_bwd(fx, o, h, n), [SB], [SB + "_workspace_bytes"],
            {SB: WORKSPACE} if n == 100 else None)
        add(f"chamfer_sampled_bwd_step-equalv3_n{n}", lambda fx, o, opt, h, n=n: fam.chamfer_sampled_bwd_step(fx, o, h, n), [SB + "_step"],
            [SB + "_workspace_bytes"], {SB + "_step": WORKSPACE} if n == 100 else None)
    DPR, SR = "fx3d_sample_points_draw_pair_reg", SB + "_step_reg"
    # which of the passengers' entry points takes (and so refuses) each of the four workspaces
    takes = {"cdf_a": {DPR: WORKSPACE}, "cdf_t": {DPR: WORKSPACE}, "adjoint": {SR: WORKSPACE}, "reg": {DPR: WORKSPACE, SR: WORKSPACE}}
    for which in ("cdf_a", "cdf_t", "adjoint", "reg"):
        add(f"fit_regularisers_as_passengers-{which}", lambda fx, o, opt, h, w=which: fam.fit_regularisers_as_passengers(fx, o, h, w),
            ["fx3d_sample_points_cdf_pair", DPR, SR],
            ["fx3d_sample_points_workspace_bytes", SB + "_workspace_bytes", "fx3d_mesh_losses_workspace_bytes"], takes[which])
    # V = 4506, E = 13 500: the draw launch's trailing blocks store several Float64 partials each into fx3d_mesh_reg.ws
    for which in ("adjoint", "reg"):
        add(f"fit_regularisers_as_passengers-{which}-v4506",
            lambda fx, o, opt, h, w=which: fam.fit_regularisers_as_passengers(fx, o, h, w, kind="equalv3_v1502"),
            ["fx3d_sample_points_cdf_pair", DPR, SR],
            ["fx3d_sample_points_workspace_bytes", SB + "_workspace_bytes", "fx3d_mesh_losses_workspace_bytes"])
    # ---- kNN: the fall-backs are the refusal (a short, NULL or misaligned workspace is fx3d_knn)
    for case in ("d64_prepass", "d64_slices2", "d64_slices_n300_m2048", "d64_verified_k40"):
        add(f"knn_ws-{case}", lambda fx, o, opt, h, c=case: fam.knn(fx, o, opt, h, c, "fx3d_knn_ws"), ["fx3d_knn_ws"], ["fx3d_knn_workspace_bytes"])
    # ---- conversions and voxels
    for D in (3, 4):
        for plus in (0, 1):
            add(f"transforms-d{D}-smallest_n+{plus}", lambda fx, o, opt, h, a=(D, plus): _transforms(fx, o, opt, h, *a),
                ["fx3d_normalize", "fx3d_segment_minmax"], ["fx3d_transform_workspace_bytes"],
                {"fx3d_normalize": WORKSPACE, "fx3d_segment_minmax": WORKSPACE} if (D, plus) == (3, 0) else None)
    add("transforms-ragged_segments_3_1_2_chunks", lambda fx, o, opt, h: fam.transforms_ragged_segments(fx, h),
        ["fx3d_normalize", "fx3d_segment_minmax"], ["fx3d_transform_workspace_bytes"])
    NB = ["fx3d_verts_normals_bwd", "fx3d_faces_normals_bwd"]
    for kind in ("teapot_sphere", "sphere_v50"):
        add(f"normals-{kind}", lambda fx, o, opt, h, k=kind: fam.mesh_normals_and_adjoints(fx, h, k), NB, ["fx3d_normals_workspace_bytes"],
            {e: WORKSPACE for e in NB} if kind == "teapot_sphere" else None)
    for t in ("upload_uint32", "upload_int64"):
        for count in (None, 1027):
            add(f"index_{t}-{count or 'all'}", lambda fx, o, opt, h, a=(t, count): fam.mesh_faces_through_index_convert_and_upload(fx, h, *a),
                ["fx3d_index_upload"], ["fx3d_index_upload_workspace_bytes"], {"fx3d_index_upload": WORKSPACE} if (t, count) == ("upload_uint32", None) else None)
    for res, N, B in ((8, 1024, 2), (8, 85, 3)):
        add(f"pointcloud_to_voxel-res{res}_n{N}_b{B}", lambda fx, o, opt, h, a=(res, N, B): fam.pointcloud_to_voxel(fx, o, h, *a), ["fx3d_pointcloud_to_voxel"],
            ["fx3d_voxel_workspace_bytes"], {"fx3d_pointcloud_to_voxel": INVALID} if N == 1024 else None)
    for kind in ("teapot_sphere", "ragged3"):
        add(f"trimesh_to_voxel-res8-{kind}", lambda fx, o, opt, h, k=kind: fam.trimesh_to_voxel(fx, h, 8, k), ["fx3d_trimesh_to_voxel"],
            ["fx3d_trimesh_voxel_workspace_bytes"], {"fx3d_trimesh_to_voxel": INVALID} if kind == "teapot_sphere" else None)
    VM = ["fx3d_voxel_mesh_count", "fx3d_voxel_mesh_emit"]
    for extra, fill in ((0, 0.4), (3, 0.07)):
        add(f"voxel_to_trimesh-extra{extra}_fill{fill}", lambda fx, o, opt, h, a=(extra, fill): fam.voxel_to_trimesh_exact(fx, h, *a), VM,
            ["fx3d_voxel_mesh_workspace_bytes"], {e: INVALID for e in VM} if extra == 0 else None)
    # ---- mesh losses
    ML = ["fx3d_edge_loss", "fx3d_laplacian_loss", "fx3d_mesh_losses", "fx3d_mesh_losses_bwd"]
    for kind in ("teapot_sphere", "sphere_v1502"):
        add(f"mesh_losses-{kind}", lambda fx, o, opt, h, k=kind: fam.mesh_losses_and_adjoints(fx, o, h, k, only_ws=True, reuse=((1, True), (0, True), (0, False))),
            ML, ["fx3d_mesh_loss_workspace_bytes", "fx3d_mesh_losses_workspace_bytes"], {e: WORKSPACE for e in ML} if kind == "teapot_sphere" else None)
    # ---- sampling and topology
    SP = ["fx3d_sample_points", "fx3d_sample_points_cdf", "fx3d_sample_points_draw", "fx3d_sample_points_cdf_pair", "fx3d_sample_points_draw_pair"]
    # (sphere_f7688: above 7680 padded faces the one-block CDF kernel works in the workspace itself, columns F .. Fp included)
    for kind, n in (("teapot_sphere", 500), ("ragged3", 100), ("sphere_f7688", 100)):
        add(f"sampling-{kind}_n{n}", lambda fx, o, opt, h, a=(kind, n): fam.mesh_sampling_and_ordered_adjoint(fx, o, h, *a, only_ws=True), SP,
            ["fx3d_sample_points_workspace_bytes"], {e: WORKSPACE for e in SP} if n == 500 else None)
    TP = ["fx3d_edges_dev_count", "fx3d_edges_dev_emit", "fx3d_laplacian_dev_csr", "fx3d_vertex_faces_dev", "fx3d_faces_padded_to_packed_dev"]
    for kind in ("teapot_sphere", "sphere_v102", "ragged3"):
        add(f"topology-{kind}", lambda fx, o, opt, h, k=kind: fam.mesh_topology_tables(fx, h, k), TP,
            ["fx3d_edges_dev_workspace_bytes", "fx3d_laplacian_dev_workspace_bytes", "fx3d_vertex_faces_dev_workspace_bytes",
             "fx3d_faces_padded_to_packed_dev_workspace_bytes"], {e: INVALID for e in TP} if kind == "teapot_sphere" else None)
    # ---- models: the alignment file's shape (every output given: the refusal case) and N = 130 (three tiles, the last ragged), K = 5
    for entry in ("forward", "forward_train", "grad", "grad_train"):
        stem = {"forward": "", "forward_train": "_train", "grad": "_grad", "grad_train": "_grad_train"}[entry]
        e, q = f"fx3d_pointnet_{entry}", f"fx3d_pointnet{stem}_workspace_bytes"
        add(f"pointnet_{entry}-n64", lambda fx, o, opt, h, en=entry: fam.pointnet(fx, h, en), [e], [q], {e: INVALID})
        add(f"pointnet_{entry}-n130-and_optional_outputs_null", _models_without(fam.pointnet, entry, N=130, without=MODEL_OPTIONAL["pointnet"][entry]), [e], [q])
        e, q = f"fx3d_dgcnn_{entry}", f"fx3d_dgcnn{stem}_workspace_bytes"
        add(f"dgcnn_{entry}-n64_k10", lambda fx, o, opt, h, en=entry: fam.dgcnn(fx, h, en), [e], [q], {e: INVALID})
        add(f"dgcnn_{entry}-n130_k5-and_optional_outputs_null", _models_without(fam.dgcnn, entry, N=130, K=5, without=MODEL_OPTIONAL["dgcnn"][entry]), [e], [q])
    add("dgcnn_grad-n130_k5-forward_into_the_workspace",
        _models_without(fam.dgcnn, "grad", N=130, K=5, null_inputs=("idx1", "x1", "idx2", "x2", "pooled")),
        ["fx3d_dgcnn_grad"], ["fx3d_dgcnn_grad_workspace_bytes"])
    for name in fam.EDGECONV_LAYERS:
        for entry in ("forward", "forward_idx", "forward_train", "bwd", "grad", "grad_train"):
            stem = {"forward": "", "forward_idx": "", "forward_train": "_train", "bwd": "_bwd", "grad": "_grad", "grad_train": "_grad_train"}[entry]
            e, q = "fx3d_edgeconv_" + entry.replace("forward_idx", "forward"), f"fx3d_edgeconv{stem}_workspace_bytes"
            add(f"edgeconv_{entry}-{name}-n64_k4", lambda fx, o, opt, h, a=(name, entry): fam.edgeconv(fx, h, *a), [e], [q],
                {e: INVALID} if name == "3_32_64_64" and entry != "forward_idx" else None)
            if entry in ("bwd", "grad", "grad_train"):   # idx NULL: the search runs again; out NULL: the forward runs first, into the workspace
                for null in (("out",), ("idx",), ("idx", "out")):
                    add(f"edgeconv_{entry}-{name}-n130_k5-{'_'.join(null)}_null",
                        _models_without(fam.edgeconv, name, entry, N=130, K=5, null_inputs=null), [e], [q])
            if entry not in MODEL_OPTIONAL["edgeconv"]:
                add(f"edgeconv_{entry}-{name}-n130_k5", lambda fx, o, opt, h, a=(name, entry): fam.edgeconv(fx, h, *a, N=130, K=5), [e], [q])
            else:
                add(f"edgeconv_{entry}-{name}-n130_k5-and_optional_outputs_null",
                    _models_without(fam.edgeconv, name, entry, N=130, K=5, without=MODEL_OPTIONAL["edgeconv"][entry]), [e], [q])
    return out


CASES = _cases()
# refusal alone: with a weight of zero the regularisers' adjoint is a launch of its own, which must not run before the sampling
# adjoint's short workspace is refused
REFUSAL_ONLY = [Case("fit_regularisers_as_passengers-adjoint-w_lap_0",
                     lambda fx, o, opt, h: fam.fit_regularisers_as_passengers(fx, o, h, "adjoint", w_lap=0.0),
                     ["fx3d_chamfer_sampled_bwd_step_reg"], [], {"fx3d_chamfer_sampled_bwd_step_reg": WORKSPACE})]
# the workspaces the header asks 256-byte alignment for and refuses otherwise (FX3D_ERR_INVALID_ARG): checked at ws + 16;
# fx3d_pointnet_forward / _forward_train ask for 16 bytes (ws + 16 is valid: checked at ws + 4)
ALIGNED_256 = {e for c in CASES for e in c.refuse if e.startswith(("fx3d_dgcnn_", "fx3d_edgeconv_", "fx3d_pointnet_grad"))}
ALIGNED_16 = {"fx3d_pointnet_forward", "fx3d_pointnet_forward_train"}
# held elsewhere: the pruned chamfer tier by tests/test_gpu_pruned.py::test_pruned_workspace_sizes_and_poisoned_scratch
CITED = {"fx3d_chamfer_fwd (pruned tier)": "tests/test_gpu_pruned.py::test_pruned_workspace_sizes_and_poisoned_scratch"}


@pytest.fixture(scope="module")
def world_size_1(gpu_fx):
    """The communicator of the sharded cases, bootstrapped once (seconds of RCCL start-up that belong to no case)."""
    return fam._comm(gpu_fx)


@pytest.mark.parametrize("case", [c for c in CASES if "sharded" in c.name], ids=repr)
def test_dirty_exact_size_workspace_sharded(gpu_fx, oracle, fx_option, world_size_1, case):
    test_dirty_exact_size_workspace(gpu_fx, oracle, fx_option, case)


@pytest.mark.parametrize("case", [c for c in CASES if "sharded" not in c.name], ids=repr)
def test_dirty_exact_size_workspace(gpu_fx, oracle, fx_option, case):
    called = set()
    fam.Calls.before = called.add
    fam.QUERIED.clear()
    try:
        case.run(gpu_fx, oracle, fx_option, hold)
    finally:
        fam.Calls.before = None
    assert set(case.entries) <= called, (set(case.entries) - called, "the case no longer makes the calls it is listed for")
    assert set(case.queries) <= fam.QUERIED, set(case.queries) - fam.QUERIED


# ------------------------------------------------------------------------------------------------------------------- refusal
class _Refused(Exception):
    pass


def _refuse(fx, call, arrs, nb, want, seen):
    """Every workspace-taking call of the closure with a short, a NULL and (where the header promises a refusal) a misaligned
    workspace: the status of `want`, no byte of an output (pre-filled 0xA5) or of the workspace changed."""
    for mode, shift, size in (("queried - 1", 0, nb - 1), ("NULL", None, nb), ("ws + 16", 16, nb), ("ws + 4", 4, nb)):
        ws = dirty.Workspace(fx, nb + 16)
        ws.fill("INF")
        before = ws.image()
        placed = _place(fx, arrs, poison=True)
        got, made = {}, []

        def before_call(name):
            if name not in want:
                return False       # a call without a workspace (a pair's finalisation) has nothing to refuse: not made
            if (shift == 16 and name not in ALIGNED_256) or (shift == 4 and name not in ALIGNED_16):
                return False

        def refused(name, e):
            got[name] = e.code
            return True
        fam.Calls.before, fam.Calls.refused, fam.Calls.after = before_call, refused, made.append
        try:
            call(fam.Ptrs(**{n: p.ptr for n, (p, _) in placed.items()}), None if shift is None else ws.ptr + shift, size)
        finally:
            fam.Calls.before = fam.Calls.refused = fam.Calls.after = None
        _sync(fx, mode)
        accepted = [n for n in made if n not in got]
        assert not accepted, (mode, accepted, "took a workspace it documents to refuse")
        for name, code in got.items():
            assert code == want[name], (mode, name, code, want[name], fx._lib.last_error())
            seen.setdefault(name, set()).add(mode)
        ws.check(mode)
        assert _bits_equal(ws.image(), before), (mode, "the workspace was written by a refused call")
        for a in arrs:
            p, host = placed[a.name]
            assert _bits_equal(p.to_host(), host), (mode, a.name, "written by a refused call")
            if a.out:
                p.check_pads(f"{a.name} ({mode})")


@pytest.mark.parametrize("case", [c for c in CASES if c.refuse] + REFUSAL_ONLY, ids=repr)
def test_refusal(gpu_fx, oracle, fx_option, world_size_1, case):
    """The family runs once per `hold` it makes: the holds before the k-th run plainly (on a zeroed workspace, so that the family
    gets the results its assertions need), the k-th is refused in every way and ends the run."""
    seen, done = {}, 0
    while True:
        count = [0]

        def hold_(fx, call, arrs, ws_bytes=0, skip=(), check=None):
            count[0] += 1
            if count[0] > done and int(ws_bytes) > 0:
                _refuse(fx, call, arrs, int(ws_bytes), case.refuse, seen)
                raise _Refused
            ws = dirty.Workspace(fx, ws_bytes)
            ws.fill("ZERO")
            got = _run(fx, call, arrs, ws, "plain")
            if check:
                check(got)
            return got
        try:
            case.run(gpu_fx, oracle, fx_option, hold_)
        except _Refused:
            done = count[0]
            continue
        break
    for e in case.refuse:
        need = {"queried - 1", "NULL"} | ({"ws + 16"} if e in ALIGNED_256 else set()) | ({"ws + 4"} if e in ALIGNED_16 else set())
        assert seen.get(e, set()) >= need, (e, seen.get(e), need)


def test_fall_backs_give_the_full_call_bits(gpu_fx, oracle, fx_option):
    """fx3d_knn_ws with a short, a NULL or a misaligned workspace is fx3d_knn; fx3d_chamfer_fwd with the partial sums' size alone
    (fx3d_chamfer_workspace_bytes under nn1_prune = 0) runs the pruned shape unpruned: the full call's bits either way."""
    fx = gpu_fx
    from abi_families import I, O, _abi, _randn, _rand, _ws
    for case in ("d64_prepass", "d64_slices_n300_m2048"):
        D, N, M, B, k, drop, _, _ = {**fam.KNN_CASES, **fam.KNN_SLICED}[case]
        x = _randn((D, N, B), 100 * D + k)
        y = x.copy(order="F") if drop else _randn((D, M, B), 100 * D + k + 1)
        nb = _ws(fx, "fx3d_knn_workspace_bytes", N, M, B, D, k, drop)
        assert nb > 0
        arrs = [I("x", x), I("y", y), O("idx", (k, N, B), np.int32), O("dist", (k, N, B))]
        got = {}
        for mode, shift, size in (("full", 0, nb), ("queried - 1", 0, nb - 1), ("NULL", None, nb), ("ws + 16", 16, nb)):
            ws = dirty.Workspace(fx, nb + 16)
            ws.fill("ONES")
            got[mode] = _run(fx, lambda p, w, n: _abi(fx, "fx3d_knn_ws")(p.x, N, p.y, M, B, D, k, drop, p.idx, p.dist, None if shift is None else w + shift,
                                                                          size, None), arrs, ws, f"{case} {mode}")
        oi, od = oracle.knn(x, k, y=y, drop_first=bool(drop))
        assert np.array_equal(got["full"]["idx"], oi) and np.array_equal(got["full"]["dist"], od)
        for mode, r in got.items():
            assert _bits_equal(r["idx"], got["full"]["idx"]) and _bits_equal(r["dist"], got["full"]["dist"]), (case, mode)
    N, M, B, D = fam.NN_SHAPES["pruned"][:4]
    full = _ws(fx, "fx3d_chamfer_workspace_bytes", N, M, B, D)
    with fx._lib.option("nn1_prune", 0):
        sums_only = _ws(fx, "fx3d_chamfer_workspace_bytes", N, M, B, D)
    assert 0 < sums_only < full
    x, y = _rand((D, N, B), 11 * N + B + D), _rand((D, M, B), 13 * M + B + D)
    arrs = [I("x", x), I("y", y), O("loss", (1,)), O("idx_x", (N, B), np.int32), O("idx_y", (M, B), np.int32)]
    got = {}
    for size in (full, full - 1, sums_only):
        ws = dirty.Workspace(fx, size)
        ws.fill("ONES")
        got[size] = _run(fx, lambda p, w, n: _abi(fx, "fx3d_chamfer_fwd")(p.x, N, p.y, M, B, D, 0.7, 1.3, p.loss, None, p.idx_x, p.idx_y, w, n, None),
                         arrs, ws, f"chamfer tiers, {size} bytes")
    ox, oy, _ = oracle.nn1_allcores(x, y, threads=16)
    assert np.array_equal(got[full]["idx_x"], ox) and np.array_equal(got[full]["idx_y"], oy)
    for size, r in got.items():
        for k2 in ("idx_x", "idx_y", "loss"):
            assert _bits_equal(r[k2], got[full][k2]), (size, k2)
