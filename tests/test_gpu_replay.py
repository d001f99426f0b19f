"""Every capturable entry point as a replayed graph (DESIGN.md "Capture and replay").

Graph replay is how the library is meant to be used: the fit_mesh iteration and train_step are replayed hipGraphs, and
include/flux3d_hip.h marks every entry point that takes a stream with a "Capture:" note.  A replay is another program than an
eager call: every address is baked in, every host argument is frozen, every host-side decision was made at record time, the
workspace holds what the previous replay left and a capture-owned arrival counter (csrc/runtime.hip: ticket_slot) is used again
by every replay of its graph.  Each case here runs one family of tests/abi_families.py -- the same call and the same reference
as tests/test_gpu_alignment.py and tests/test_gpu_workspace.py -- through ``hold`` below, on a created stream, arrays between
pads (tests/misaligned.py, offset 0), the workspace a dirty_ws.Workspace of exactly the queried size between guard pads:

  1. eager A    the call on the family's inputs, arrays and workspace of its own: the warm-up the header asks for, and E_A;
  2. record     the closure captured on the stream; outputs and workspace pre-filled 0xFF; not one byte of either may change
                (recording runs nothing); the workspace is filled 0xFF again;
  3. replay A   every output bit-equal to E_A;
  4. replay B   the record arrays' inputs overwritten in place with dirty_ws.other_inputs (the workspace file's REORDERED and KEPT
                rules; a device seed word, ADVANCED, moved on as fx3d_counter_add moves it), outputs 0xFF again, the workspace as
                step 3 left it; while the replay runs, the same call is enqueued
                eagerly on B on a second stream, arrays and workspace of its own (runtime.hip: eager and captured launches never
                share a counter); the replay's outputs bit-equal to that eager E_B;
  5. replay A   the A inputs restored, outputs 0xFF, the workspace filled with dirty_ws' INF words: bit-equal to E_A.  THIS is what
                ``hold`` returns: the family compares replayed bits with its reference (the oracle, the *_ref.py restatements, the
                golden answers; LOSS_RTOL is the one tolerance, as everywhere).

After every launch the guard pads of the workspace and the pads of the outputs are intact and the inputs unwritten.  ``check=``
(the two float-atomic scatter adjoints): every run goes through the family's bound instead of a bit comparison, and because that
bound is stated against the reference of the family's own inputs, step 4 keeps them (the gather forms of the same adjoints, bit
for bit, take the changed data).  A closure with a host read between two of its calls (SPLIT_AFTER) is captured call by call, one
graph each, replayed in order with a synchronisation between; any other closure is captured whole.

What an output starts a run with: 0xFF bytes, on the eager arrays too (a byte the call does not write is then equal on both
sides), except for the arrays a call reads as well as writes -- those the family gives initial contents (a base gradient, an
optimiser's state, an in-place transform, a seed counter) and the caller-zeroed counters of the header (CALLER_ZEROED) -- which
start every run from those contents (step 4: from other_inputs of them).

What the file found: behind the rest of the GPU suite -- alone it passed -- a hipMemsetAsync recorded by the capture
replayed with a stale fill value (voxels that should be 0 held the bits 0x00007F6F, ``bad`` held 0x40404040, 1024 of the 1027 bytes
of an fx3d_memset of 0x5A held garbage), at "replay A against eager A" in test_pointcloud_to_voxel, test_trimesh_to_voxel,
test_mesh_topology_tables[teapot_sphere], test_mesh_losses_and_adjoints[teapot_sphere] and the fx3d_memset case.  The library now
clears with a kernel of its own (csrc/runtime.hip: fill_bytes), so that no launching entry point records a memset node.

``CAPTURE`` names, for every FX3D_API function that takes a stream, the case that replays it or the reason it cannot be captured;
tests/test_replay_host.py holds it complete against the header and ``_lib.SIGNATURES`` and equal to the header's "Capture:" notes.
``test_capture_owned_counters_across_a_chunk_boundary`` runs tests/replay_counters_child.py in a process of its own."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_families as fam
import dirty_ws as dirty
import misaligned as mis
from abi_families import I, O, _abi, _bits_equal, _first_diff, _rand, _randn
from conftest import ROOT
from test_gpu_workspace import KEPT, REORDERED, _smallest_transform_n

pytestmark = pytest.mark.gpu

# the header: "caller-zeroed device counter" (missing_dev, bad_dev) -- read and added to, so zero before every launch
CALLER_ZEROED = ("bad", "missing")
# the calls after which the caller reads the device before it can make the next (cubes_dev / count_dev size the emit call's outputs;
# fx3d_sample_points_cdf is the prepared form whose CDF a host keeps across many draws): the closure's captures end there
SPLIT_AFTER = ("fx3d_voxel_mesh_count", "fx3d_edges_dev_count", "fx3d_sample_points_cdf")
RECORD_BYTE = 0xFF
# device words a recorded call reads so that a replay can differ from the last (the sampler's seed_dev): other_inputs leaves an
# integer array as it is, so step 4 advances these by ADVANCE, as fx3d_counter_add does between the replays of the fit iteration
ADVANCED, ADVANCE = ("seed_dev",), 2
STEP4 = {}            # the last hold's step 4: {"start": what every array held when the replay on B began, "got": its outputs}

CAPTURED = set()     # the entry points recorded into a graph by the running test
SERIAL = [False]      # the running family owns further scratch that every run of it shares: the eager B call then follows the replay
_STREAMS = []


def _streams(fx):
    """The capture stream and the stream of the concurrent eager call: two for the whole file."""
    if not _STREAMS:
        _STREAMS.extend([fx.Stream.create(), fx.Stream.create()])
    return _STREAMS


@pytest.fixture(autouse=True)
def replayed_what_the_table_says(request):
    """Every entry point whose CAPTURE row names the running test must have been recorded by it."""
    fam.NULLABLE.clear()
    CAPTURED.clear()
    SERIAL[0] = False
    yield
    want = {e for e, (kind, what) in CAPTURE.items() if kind == "replayed" and what == request.node.name}
    assert want <= CAPTURED, (sorted(want - CAPTURED), "named in CAPTURE for this case and not recorded by it")


# ---------------------------------------------------------------------------------------------------------------- the driver
def _sync(fx, stream, what):
    try:
        stream.synchronize()
    except fx.Flux3DHipError as e:  # a fault: nothing more is started on the device
        pytest.exit(f"{what}: {e}", returncode=3)


def _state(a):
    """An output the call also reads: it starts every run from its contents, not from 0xFF."""
    return a.out and (a.name in CALLER_ZEROED or bool(np.count_nonzero(a.host)))


def _contents(a, other):
    """What array `a` holds when a run starts (`other`: the B run)."""
    host = a.host
    if a.out and not _state(a):
        return np.full(host.nbytes, RECORD_BYTE, np.uint8).view(host.dtype).reshape(host.shape, order="F")
    if other and a.name not in KEPT:
        host = dirty.other_inputs(host)
        if a.name in REORDERED and host.ndim >= 2:   # other index inputs that stay in range: the same faces / edges in reverse order
            host = np.asfortranarray(np.flip(host, axis=1 if a.name == "faces" else 0))
        if a.name in ADVANCED:
            host = host + host.dtype.type(ADVANCE)
    return np.asfortranarray(host)


class _Arrays:
    """One set of placed arrays and a workspace: the record set, or an eager call's own."""

    def __init__(self, fx, arrs, ws_bytes):
        self.fx, self.arrs = fx, arrs
        self.placed = {a.name: mis.place(fx, _contents(a, False), 0, output=a.out) for a in arrs}
        self.ws = dirty.Workspace(fx, ws_bytes)
        self.start = {a.name: _contents(a, False) for a in arrs}

    def load(self, other):
        for a in self.arrs:
            self.start[a.name] = _contents(a, other)
            self.placed[a.name].arr.copy_(self.start[a.name])

    def ptrs(self):
        return fam.Ptrs(**{n: p.ptr for n, p in self.placed.items()})

    def check(self, what):
        """Guard pads, output pads, inputs unwritten."""
        self.ws.check(what)
        for a in self.arrs:
            p = self.placed[a.name]
            if a.out:
                p.check_pads(f"{a.name} ({what})")
            else:
                assert _bits_equal(p.to_host(), self.start[a.name]), f"input {a.name} was written ({what})"

    def results(self, what):
        self.check(what)
        return {a.name: self.placed[a.name].to_host() for a in self.arrs if a.out}

    def untouched(self, ws_image, what):
        """Recording runs nothing: every output and the workspace still hold what they held."""
        for a in self.arrs:
            if a.out:
                assert _bits_equal(self.placed[a.name].to_host(), self.start[a.name]), (what, a.name, "written while recording")
        assert _bits_equal(self.ws.image(), ws_image), (what, "the workspace was written while recording")


def _eager(fx, call, arrays, stream, what, wait=True):
    """The plain call on `arrays`, on `stream`."""
    def after(name):
        if wait:
            _sync(fx, stream, f"{what}: {name}")
            arrays.ws.check(f"{what}, after {name}")
    fam.Calls.stream, fam.Calls.after = stream.handle, after
    try:
        call(arrays.ptrs(), arrays.ws.ptr, arrays.ws.nbytes)
    finally:
        fam.Calls.stream = fam.Calls.after = None
    if wait:
        _sync(fx, stream, what)


def _record(fx, call, arrays, stream):
    """The closure captured on `stream`: one graph, or one per stretch between the calls of SPLIT_AFTER."""
    lib, graphs, is_open = fx._lib, [], [False]

    def begin():
        lib.call("fx3d_graph_begin_capture", stream.handle)
        is_open[0] = True

    def end():
        h = C.c_void_p()
        is_open[0] = False
        lib.call("fx3d_graph_end_capture", stream.handle, C.byref(h))
        g = fx.Graph()
        g.handle, g.stream = h.value, stream
        graphs.append(g)

    def after(name):
        CAPTURED.add(name)
        if name in SPLIT_AFTER:
            end()
            begin()
    fam.Calls.stream, fam.Calls.after = stream.handle, after
    begin()
    try:
        call(arrays.ptrs(), arrays.ws.ptr, arrays.ws.nbytes)
        end()
    finally:
        fam.Calls.stream = fam.Calls.after = None
        if is_open[0]:   # a call was refused while recording: the stream must not stay in capture mode
            h = C.c_void_p()
            if lib.load().fx3d_graph_end_capture(stream.handle, C.byref(h)) == 0:
                lib.load().fx3d_graph_destroy(h)
    return graphs


def _replay(fx, graphs, arrays, stream, what, then=None):
    """Launch the graphs in order, a synchronisation and the pad checks after each.  `then`: called right after the (last) launch,
    before anything waits for it."""
    for i, g in enumerate(graphs):
        g.launch(stream)
        if then and i == len(graphs) - 1:
            then()
        _sync(fx, stream, f"{what}, graph {i + 1} of {len(graphs)}")
        arrays.ws.check(f"{what}, after graph {i + 1} of {len(graphs)}")
    return arrays.results(what)


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert _bits_equal(got[k], want[k]), (what, k, "elements differing / first:", _first_diff(got[k], want[k]))


def hold(fx, call, arrs, ws_bytes=0, skip=(), check=None):
    """The five steps of the module's docstring.  Returns the outputs of the last replay."""
    st, st2 = _streams(fx)
    ws_bytes = int(ws_bytes)
    # 1. eager A
    a = _Arrays(fx, arrs, ws_bytes)
    a.ws.fill("ONES")
    _eager(fx, call, a, st, "eager A")
    e_a = a.results("eager A")
    if check:
        check(e_a)
    # 2. record
    rec = _Arrays(fx, arrs, ws_bytes)
    rec.ws.fill("ONES")
    image = rec.ws.image()
    graphs = _record(fx, call, rec, st)
    _sync(fx, st, "after recording")
    rec.untouched(image, "record")
    rec.ws.fill("ONES")
    # 3. replay on A
    got = _replay(fx, graphs, rec, st, "replay A")
    if check:
        check(got)
    else:
        _same(got, e_a, "replay A against eager A")
    # 4. replay on B, an eager call on B in flight beside it
    other = not check
    b = _Arrays(fx, arrs, ws_bytes)
    b.load(other)
    b.ws.fill("ONES")
    rec.load(other)
    concurrent = not SERIAL[0]
    got = _replay(fx, graphs, rec, st, "replay B", then=(lambda: _eager(fx, call, b, st2, "eager B", wait=False)) if concurrent else None)
    if not concurrent:
        _eager(fx, call, b, st2, "eager B")
    _sync(fx, st2, "eager B")
    e_b = b.results("eager B")
    STEP4.clear()
    STEP4.update(start=dict(rec.start), got=got)
    if check:
        check(got), check(e_b)
    else:
        _same(got, e_b, "replay B against eager B")
    # 5. replay on A again, the workspace full of +Inf words
    rec.load(False)
    rec.ws.fill("INF")
    got = _replay(fx, graphs, rec, st, "replay A again")
    if check:
        check(got)
    else:
        _same(got, e_a, "replay A again against eager A")
    return got


# ------------------------------------------------------------------------------------------------------------------ the cases
NN = fam.NN_CASES + [("r130_d64", "chamfer_fwd"), ("r130_d64", "chamfer_fwd_bwd")]


@pytest.mark.parametrize("shape,entry", NN, ids=[f"{s}-{e}" for s, e in NN])
def test_nn1_and_chamfer(gpu_fx, oracle, fx_option, shape, entry):
    fam.nn1_and_chamfer(gpu_fx, oracle, fx_option, hold, shape, entry)


@pytest.mark.parametrize("shape", ["tiny", "1024", "split_plan"])
def test_chamfer_sums_and_finalize(gpu_fx, oracle, fx_option, shape):
    fam.chamfer_sums_and_finalize(gpu_fx, oracle, fx_option, hold, shape)


def test_chamfer_pairwise(gpu_fx, oracle):
    fam.chamfer_pairwise(gpu_fx, oracle, hold)


def test_chamfer_backward_long_inverse_lists(gpu_fx, oracle):
    fam.chamfer_backward_long_inverse_lists(gpu_fx, oracle, hold)


KNN = [(c, e) for c in fam.KNN_CASES for e in ("fx3d_knn", "fx3d_knn_ws")] + [(c, "fx3d_knn_ws") for c in fam.KNN_SLICED]


@pytest.mark.parametrize("case,entry", KNN, ids=[f"{c}-{e}" for c, e in KNN])
def test_knn(gpu_fx, oracle, fx_option, case, entry):
    fam.knn(gpu_fx, oracle, fx_option, hold, case, entry)


@pytest.mark.parametrize("F,K", [(3, 4), (4, 5), (64, 4)], ids=["f3_k4", "f4_k5", "f64_k4"])
def test_graph_features(gpu_fx, oracle, fx_option, F, K):
    fam.graph_features(gpu_fx, oracle, fx_option, hold, F, K)


@pytest.mark.parametrize("D,n", [(3, 1027), (4, 1024)], ids=["d3_n1027", "d4_n1024"])
def test_transforms_dense(gpu_fx, D, n):
    fam.transforms_dense(gpu_fx, hold, D, n)


@pytest.mark.parametrize("D", [3, 4])
def test_transforms_with_scratch(gpu_fx, D):
    """The smallest cloud whose reduction takes a workspace, plus one point: two launches, partials carried in the scratch."""
    n = _smallest_transform_n(gpu_fx, D) + 1
    assert gpu_fx._lib.query_bytes("fx3d_transform_workspace_bytes", D, n, 2) > 0
    fam.transforms_dense(gpu_fx, hold, D, n, only_ws=True)


def test_transforms_ragged_segments(gpu_fx):
    fam.transforms_ragged_segments(gpu_fx, hold)


@pytest.mark.parametrize("res", [8, 32])
def test_pointcloud_to_voxel(gpu_fx, oracle, res):
    fam.pointcloud_to_voxel(gpu_fx, oracle, hold, res)


@pytest.mark.parametrize("res", [8, 28])
def test_trimesh_to_voxel(gpu_fx, res):
    fam.trimesh_to_voxel(gpu_fx, hold, res)


@pytest.mark.parametrize("extra,fill", [(0, 0.4), (3, 0.07)], ids=["extra0", "extra3"])
def test_voxel_to_trimesh_exact(gpu_fx, extra, fill):
    fam.voxel_to_trimesh_exact(gpu_fx, hold, extra, fill)


@pytest.mark.parametrize("index_type", ["int32", "uint32", "int64"])
def test_mesh_faces_through_index_convert(gpu_fx, index_type):
    fam.mesh_faces_through_index_convert_and_upload(gpu_fx, hold, index_type)


def test_mesh_face_areas(gpu_fx, oracle):
    fam.mesh_face_areas(gpu_fx, oracle, hold)


@pytest.mark.parametrize("kind", ["teapot_sphere", "sphere_v1502"])
def test_mesh_losses_and_adjoints(gpu_fx, oracle, kind):
    fam.mesh_losses_and_adjoints(gpu_fx, oracle, hold, kind, only_ws=kind != "teapot_sphere", reuse=((1, True), (0, True), (0, False)))


@pytest.mark.parametrize("kind,n", [("teapot_sphere", 500), ("sphere_f7688", 100)], ids=["teapot_sphere_n500", "sphere_f7688_n100"])
def test_mesh_sampling_and_ordered_adjoint(gpu_fx, oracle, kind, n):
    SERIAL[0] = True   # the pair forms: the family owns the other side's workspace, shared by every run
    fam.mesh_sampling_and_ordered_adjoint(gpu_fx, oracle, hold, kind, n, only_ws=kind != "teapot_sphere")


def test_sampling_with_its_device_seed(gpu_fx, oracle):
    """fx3d_sample_points_draw and fx3d_sample_points_draw_pair with a non-NULL seed_dev, the one sampler argument that exists for
    replay ("a captured graph replays with fresh samples"): the draws are those of seed + *seed_dev as the device holds it WHEN THE
    GRAPH RUNS.  Step 4 advances the word (ADVANCED) along with the other inputs, so a draw that read *seed_dev when it was
    enqueued, froze it or ignored it differs from the eager call there; and the replays on A, on B and on A again are held to
    oracle.sample_points_seeded at seed + *seed_dev on the inputs each of them ran on.  One closed mesh (no padded faces, so that
    the face list in reverse order is a mesh too); seed + *seed_dev crosses 2^32, both halves of the key take part."""
    fx = gpu_fx
    d = fam._mesh(fx, "sphere_v50")
    assert d.B == 1 and d.F == d.Fmax
    n, seed, dev = 300, 11, 2 ** 32 - 7
    nb = fam._ws(fx, "fx3d_sample_points_workspace_bytes", d.Fmax, d.B)
    mesh = [I("verts", d.vp), I("faces", d.fp), I("flen", d.flen), I("seed_dev", np.array([dev], np.uint64))]
    outs = [O("out", (3, n, d.B)), O("fi", (n, d.B), np.int32), O("r1", (n, d.B)), O("r2", (n, d.B))]

    def holds(got, start, names=("out", "fi", "r1", "r2"), verts="verts", plus=0, what=""):
        key = seed + plus + int(start["seed_dev"][0])
        want = oracle.sample_points_seeded(start[verts], start["faces"], d.flen, n, key, return_draws=True)
        for k, w in zip(names, want):
            assert _bits_equal(got[k], w), (what, k, key, _first_diff(got[k], w))

    def cdf_draw(p, ws, nn):
        _abi(fx, "fx3d_sample_points_cdf")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, 1e-6, ws, nn, None)
        _abi(fx, "fx3d_sample_points_draw")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, n, seed, p.seed_dev, ws, nn, p.out, p.fi, p.r1, p.r2, None)
    a_start = {a.name: a.host for a in mesh}
    r = hold(fx, cdf_draw, mesh + outs, nb)
    assert int(STEP4["start"]["seed_dev"][0]) == dev + ADVANCE
    holds(r, a_start, what="draw, replay A again")
    holds(STEP4["got"], STEP4["start"], what="draw, replay B")
    assert not _bits_equal(STEP4["got"]["fi"], r["fi"])
    # the pair form: this mesh and the same mesh scaled, seeds `seed` and `seed` + 1, seed_dev added to both
    SERIAL[0] = True   # the other side's workspace is this test's own, shared by every run
    vp2 = np.asfortranarray(d.vp * np.float32(1.5))
    other = fx.DeviceArray.zeros((max(nb, 256),), np.uint8)
    pair_in = mesh + [I("verts2", vp2)]

    def pair(p, ws, nn):
        _abi(fx, "fx3d_sample_points_cdf_pair")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, ws, nn,
                                                 p.verts2, d.Vmax, p.faces, d.Fmax, p.flen, d.B, other.ptr, nn, 1e-6, None)
        _abi(fx, "fx3d_sample_points_draw_pair")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, n, seed, ws, nn, p.out, p.fi, p.r1, p.r2,
                                                  p.verts2, d.Vmax, p.faces, d.Fmax, p.flen, d.B, n, seed + 1, other.ptr, nn, p.out2, None, None, None,
                                                  p.seed_dev, None)
    a_start = {a.name: a.host for a in pair_in}
    r = hold(fx, pair, pair_in + outs + [O("out2", (3, n, d.B))], nb)
    for got, start, what in ((r, a_start, "pair, replay A again"), (STEP4["got"], STEP4["start"], "pair, replay B")):
        holds(got, start, what=what)
        holds(got, start, names=("out2",), verts="verts2", plus=1, what=what)


def test_mesh_normals_and_adjoints(gpu_fx):
    fam.mesh_normals_and_adjoints(gpu_fx, hold)


@pytest.mark.parametrize("kind", ["teapot_sphere", "ragged3"])
def test_mesh_topology_tables(gpu_fx, kind):
    fam.mesh_topology_tables(gpu_fx, hold, kind)


def test_chamfer_sampled_bwd(gpu_fx, oracle):
    fam.chamfer_sampled_bwd(gpu_fx, oracle, hold)


def test_chamfer_sampled_bwd_step(gpu_fx, oracle):
    fam.chamfer_sampled_bwd_step(gpu_fx, oracle, hold)


@pytest.mark.parametrize("which,kind", [("adjoint", "equalv3"), ("reg", "equalv3"), ("reg", "equalv3_v1502")],
                         ids=["adjoint", "reg", "reg-v4506"])
def test_fit_regularisers_as_passengers(gpu_fx, oracle, which, kind):
    SERIAL[0] = True   # three of the four workspaces are the family's own, shared by every run
    fam.fit_regularisers_as_passengers(gpu_fx, oracle, hold, which, kind=kind)


@pytest.mark.parametrize("entry", ["forward", "forward_train", "grad", "grad_train"])
def test_pointnet(gpu_fx, entry):
    fam.pointnet(gpu_fx, hold, entry)


EC = [(n, e) for n in fam.EDGECONV_LAYERS for e in ("forward", "forward_idx", "forward_train", "bwd", "grad", "grad_train")]


@pytest.mark.parametrize("name,entry", EC, ids=[f"{n}-{e}" for n, e in EC])
def test_edgeconv(gpu_fx, name, entry):
    fam.edgeconv(gpu_fx, hold, name, entry)


@pytest.mark.parametrize("entry", ["forward", "forward_train", "grad", "grad_train"])
def test_dgcnn(gpu_fx, entry):
    fam.dgcnn(gpu_fx, hold, entry)


def test_elementwise_copies_and_the_training_step(gpu_fx):
    """The entry points no family of tests/abi_families.py states: the fit loop's element-wise kernels and copies against
    tests/fit_chain_ref.py and numpy, the training step's three against tests/train_step_ref.py (the loss to the device's log, by
    the bound of tests/test_gpu_train_step.py)."""
    import fit_chain_ref as fc
    import train_step_ref as ts
    fx, n = gpu_fx, 1027
    x, y, z, g = _randn((n,), 1), _randn((n,), 2), _randn((n,), 3), _randn((n,), 4)
    v0, base = _randn((n,), 5) * np.float32(0.1), _randn((n,), 6)
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_lincomb")(n, 0.7, p.x, -1.3, p.y, 2.5, p.z, p.out, None), [I("x", x), I("y", y), I("z", z), O("out", (n,))])
    assert _bits_equal(r["out"], fc.lincomb(0.7, x, -1.3, y, 2.5, z))
    rho, eta = 0.9, 0.7
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_momentum_step")(n, rho, eta, p.g, p.v, p.x, None), [I("g", g), O("v", (n,), init=v0), O("x", (n,), init=x)])
    v1, x1, o1 = fc.momentum_step(rho, eta, g, v0, x, base)
    assert _bits_equal(r["v"], v1) and _bits_equal(r["x"], x1)
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_momentum_step_offset")(n, rho, eta, p.g, p.v, p.x, p.base, p.out, p.ctr, 2, None),
             [I("g", g), I("base", base), O("v", (n,), init=v0), O("x", (n,), init=x), O("out", (n,)), O("ctr", (1,), np.uint64, init=[2 ** 32 - 1])])
    assert _bits_equal(r["v"], v1) and _bits_equal(r["x"], x1) and _bits_equal(r["out"], o1) and int(r["ctr"][0]) == 2 ** 32 + 1
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_counter_add")(p.ctr, 3, None), [O("ctr", (1,), np.uint64, init=[2 ** 32 - 2])])
    assert int(r["ctr"][0]) == 2 ** 32 + 1
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_memset")(p.dst, 0x5A, n, None), [O("dst", (n,), np.uint8)])
    assert np.all(r["dst"] == 0x5A)
    # fill_bytes at odd addresses and lengths: 13 head bytes, 61 whole 16-byte lines and 12 tail bytes; 5 bytes that reach no line;
    # 16 bytes across two lines.  Every byte around stays 0xFF
    for at, count in ((3, 1001), (5, 5), (9, 16)):
        r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_memset")(p.dst + at, 0x5A, count, None), [O("dst", (n,), np.uint8)])
        want = np.full(n, RECORD_BYTE, np.uint8)
        want[at:at + count] = 0x5A
        assert np.array_equal(r["dst"], want), (at, count, np.flatnonzero(r["dst"] != want)[:5])
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_memcpy_d2d")(p.dst, p.src, 4 * n, None), [I("src", x), O("dst", (n,))])
    assert _bits_equal(r["dst"], x)
    # three meshes of 5, 3 and 7 vertices: verts_len is a HOST array, read while recording (frozen, as every host argument)
    vlen, Vmax = np.array([5, 3, 7], np.int64), 7
    packed = _rand((3, int(vlen.sum())), 8)
    padded = fc.packed_to_padded(packed, vlen, Vmax)
    lens = vlen.ctypes.data
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_packed_to_padded")(p.packed, lens, 3, Vmax, p.padded, None), [I("packed", packed), O("padded", (3, Vmax, 3))])
    assert _bits_equal(r["padded"], padded)
    # (the columns behind a mesh's length never reach the packed array: NaN there must not show)
    full = np.asfortranarray(np.where(padded == 0, np.float32(np.nan), padded))
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_padded_to_packed")(p.padded, lens, 3, Vmax, p.packed, None), [I("padded", full), O("packed", packed.shape)])
    assert _bits_equal(r["packed"], fc.padded_to_packed(full, vlen)) and _bits_equal(r["packed"], packed)
    # ---- the training step
    nc, B = 10, 7
    e = np.exp(_randn((nc, B), 9).astype(np.float64))
    probs = np.asfortranarray((e / e.sum(axis=0)).astype(np.float32))
    labels = np.array([3, 0, 9, 10, 2, -1, 5], np.int32)   # two of them outside [0, nc)
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_crossentropy")(p.probs, p.labels, nc, B, p.glogits, p.loss, p.counts, None),
             [I("probs", probs), I("labels", labels), O("glogits", (nc, B)), O("loss", (1,), np.float64), O("counts", (2,), np.int32)])
    loss, gl, counts = ts.crossentropy(probs, labels)
    assert _bits_equal(r["glogits"], gl) and np.array_equal(r["counts"], counts) and np.isnan(loss) and np.isnan(r["loss"][0])
    inside = np.array([3, 0, 9, 1, 2, 8, 5], np.int32)
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_crossentropy")(p.probs, p.labels, nc, B, p.glogits, p.loss, p.counts, None),
             [I("probs", probs), I("labels", inside), O("glogits", (nc, B)), O("loss", (1,), np.float64), O("counts", (2,), np.int32)])
    loss, gl, counts = ts.crossentropy(probs, inside)
    assert _bits_equal(r["glogits"], gl) and np.array_equal(r["counts"], counts)
    # (tests/test_gpu_train_step.py: B rounded additions of logs known to 1 ulp each, the negation and the division)
    bound = (B + 4) * 2.0 ** -53 * np.abs(np.log(probs[inside, np.arange(B)].astype(np.float64))).max()
    assert abs(r["loss"][0] - loss) <= bound, (r["loss"][0], loss, bound)
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_dropout_mask")(n, 0.3, 77, p.ctr, 2, p.out, None),
             [I("ctr", np.array([2 ** 32 - 5], np.uint64)), O("out", (n,))])
    assert _bits_equal(r["out"], ts.dropout_mask(n, 0.3, 77, counter=2 ** 32 - 5, stream_id=2))
    m0, s0 = _randn((n,), 10) * np.float32(0.01), np.abs(_randn((n,), 11)) * np.float32(0.01)
    bp0, hyper = np.array([0.9 ** 3, 0.999 ** 3], np.float64), dict(eta=1e-3, beta=(0.9, 0.999), eps=1e-8)
    running, smap = _randn((5,), 12), np.array([0, 17, 1026, 1027, -1], np.int32)   # (the last two are outside [0, n): skipped)
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_adam_step")(n, hyper["eta"], *hyper["beta"], hyper["eps"], p.g, p.m, p.v, p.betap, p.x, p.running,
                                                               p.stat_map, 5, None),
             [I("g", g), I("running", running), I("stat_map", smap), O("m", (n,), init=m0), O("v", (n,), init=s0), O("betap", (2,), np.float64, init=bp0),
              O("x", (n,), init=x)])
    x2, m2, s2, bp2 = ts.adam_step(x, g, m0, s0, bp0, running=running[:3], stat_map=smap[:3], **hyper)
    assert _bits_equal(r["x"], x2) and _bits_equal(r["m"], m2) and _bits_equal(r["v"], s2) and _bits_equal(r["betap"], bp2)


# ------------------------------------------------------------------------------------------- capture-owned counters, one process
def test_capture_owned_counters_across_a_chunk_boundary(gpu_fx):
    """tests/replay_counters_child.py in a fresh process (the capture-owned counters are process-wide: the counts are exact only
    where nothing was captured before), ended by `timeout` if it does not end itself."""
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "replay_counters_child.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "REPLAY_COUNTERS_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------------------ the CAPTURE table
def _replayed(case):
    return ("replayed", case)


HOST_COPY = "copies to the host"
HOST_CODE = "host code"
COLLECTIVE = "collective"
NN_, KNN_, GF, TD = "test_nn1_and_chamfer", "test_knn", "test_graph_features[f4_k5]", "test_transforms_dense[d3_n1027]"
SEEDED = "test_sampling_with_its_device_seed"   # (seed_dev NULL: test_mesh_sampling_and_ordered_adjoint; _draw_pair_reg: REG)
SUMS, LOSSES, SAMPLING = "test_chamfer_sums_and_finalize[split_plan]", "test_mesh_losses_and_adjoints[teapot_sphere]", "test_mesh_sampling_and_ordered_adjoint[teapot_sphere_n500]"
NORMALS, TOPO, REG, ELEM = "test_mesh_normals_and_adjoints", "test_mesh_topology_tables[ragged3]", "test_fit_regularisers_as_passengers[reg-v4506]", "test_elementwise_copies_and_the_training_step"
# {entry point: ("replayed", the case of this file that records and replays it) or (the kind of reason, the reason as read in the code)}
CAPTURE = {
    "fx3d_memcpy_h2d": (HOST_COPY, "runtime.hip: hipMemcpyAsync from pageable host memory, then hipStreamSynchronize"),
    "fx3d_memcpy_d2h": (HOST_COPY, "runtime.hip: hipMemcpyAsync to the host, then hipStreamSynchronize"),
    "fx3d_memcpy_d2d": _replayed(ELEM),
    "fx3d_memset": _replayed(ELEM),
    "fx3d_stream_destroy": (HOST_CODE, "runtime.hip: hipStreamDestroy, no work enqueued"),
    "fx3d_stream_sync": (HOST_CODE, "runtime.hip: hipStreamSynchronize, illegal on a capturing stream"),
    "fx3d_graph_begin_capture": (HOST_CODE, "runtime.hip: hipStreamBeginCapture, the capture itself"),
    "fx3d_graph_end_capture": (HOST_CODE, "runtime.hip: hipStreamEndCapture and hipGraphInstantiate, the capture itself"),
    "fx3d_graph_launch": (HOST_CODE, "runtime.hip: hipGraphLaunch, the replay itself (a graph inside a graph is not attempted: captures here are single-stream)"),
    "fx3d_event_record": (HOST_CODE, "runtime.hip: hipEventRecord, the fork / join of a two-stream capture (captures here are single-stream)"),
    "fx3d_stream_wait_event": (HOST_CODE, "runtime.hip: hipStreamWaitEvent, the fork / join of a two-stream capture (captures here are single-stream)"),
    "fx3d_counter_add": _replayed(ELEM),
    "fx3d_nn1": _replayed(NN_ + "[tiny-nn1]"),
    "fx3d_chamfer_sums": _replayed(SUMS), "fx3d_chamfer_finalize": _replayed(SUMS), "fx3d_chamfer_finalize_many": _replayed(SUMS),
    "fx3d_segment_minmax": _replayed("test_transforms_ragged_segments"), "fx3d_normalize": _replayed("test_transforms_ragged_segments"),
    "fx3d_realign": _replayed(TD), "fx3d_rotate": _replayed(TD), "fx3d_scale_translate": _replayed(TD),
    "fx3d_chamfer_fwd": _replayed(NN_ + "[pruned-chamfer_fwd]"),
    "fx3d_chamfer_bwd": _replayed("test_chamfer_backward_long_inverse_lists"),
    "fx3d_chamfer_fwd_bwd": _replayed(NN_ + "[split_plan-chamfer_fwd_bwd]"),
    "fx3d_chamfer_sampled_bwd": _replayed("test_chamfer_sampled_bwd"),
    "fx3d_chamfer_sampled_bwd_step": _replayed("test_chamfer_sampled_bwd_step"),
    "fx3d_sample_points_draw_pair_reg": _replayed(REG), "fx3d_chamfer_sampled_bwd_step_reg": _replayed(REG),
    "fx3d_knn": _replayed(KNN_ + "[d3_k20-fx3d_knn]"), "fx3d_knn_ws": _replayed(KNN_ + "[d64_verified_k40-fx3d_knn_ws]"),
    "fx3d_knn_gather": _replayed(GF), "fx3d_edge_features": _replayed(GF), "fx3d_edge_features_bwd": _replayed(GF), "fx3d_edgeconv_graph": _replayed(GF),
    "fx3d_index_convert": _replayed("test_mesh_faces_through_index_convert[int64]"),
    "fx3d_index_upload": (HOST_COPY, "mesh.hip: hipMemcpyAsync from the caller's pageable array into the workspace, then hipStreamSynchronize"),
    "fx3d_faces_areas_packed": _replayed("test_mesh_face_areas"), "fx3d_faces_areas_padded": _replayed("test_mesh_face_areas"),
    "fx3d_verts_normals_packed": _replayed(NORMALS), "fx3d_verts_normals_bwd": _replayed(NORMALS),
    "fx3d_faces_normals_packed": _replayed(NORMALS), "fx3d_faces_normals_bwd": _replayed(NORMALS),
    "fx3d_sample_points_explicit": _replayed(SAMPLING), "fx3d_sample_points": _replayed(SAMPLING), "fx3d_sample_points_cdf": _replayed(SAMPLING),
    "fx3d_sample_points_draw": _replayed(SEEDED), "fx3d_sample_points_cdf_pair": _replayed(SAMPLING), "fx3d_sample_points_draw_pair": _replayed(SEEDED),
    "fx3d_sample_points_bwd": _replayed(SAMPLING),
    "fx3d_lincomb": _replayed(ELEM), "fx3d_momentum_step": _replayed(ELEM), "fx3d_momentum_step_offset": _replayed(ELEM),
    "fx3d_packed_to_padded": _replayed(ELEM), "fx3d_padded_to_packed": _replayed(ELEM),
    "fx3d_edge_loss": _replayed(LOSSES), "fx3d_edge_loss_bwd": _replayed(LOSSES), "fx3d_edge_loss_bwd_adj": _replayed(LOSSES),
    "fx3d_laplacian_loss": _replayed(LOSSES), "fx3d_laplacian_loss_bwd": _replayed(LOSSES), "fx3d_laplacian_loss_bwd_sym": _replayed(LOSSES),
    "fx3d_mesh_losses": _replayed(LOSSES), "fx3d_mesh_losses_bwd": _replayed(LOSSES),
    "fx3d_pointcloud_to_voxel": _replayed("test_pointcloud_to_voxel[32]"), "fx3d_trimesh_to_voxel": _replayed("test_trimesh_to_voxel[28]"),
    "fx3d_voxel_mesh_count": _replayed("test_voxel_to_trimesh_exact[extra3]"), "fx3d_voxel_mesh_emit": _replayed("test_voxel_to_trimesh_exact[extra3]"),
    "fx3d_chamfer_loss_pairwise_f32": _replayed("test_chamfer_pairwise"),
    "fx3d_comm_allreduce_sum_f64": (COLLECTIVE, "comm.cpp: an RCCL all-reduce; not attempted (one device per run, and a collective inside a capture is another question)"),
    "fx3d_comm_allreduce_max_f64": (COLLECTIVE, "comm.cpp: an RCCL all-reduce; not attempted"),
    "fx3d_chamfer_fwd_sharded": (COLLECTIVE, "comm.cpp: the sums' RCCL all-reduce between the kernel and the loss; not attempted"),
    "fx3d_chamfer_fwd_sharded_async": (COLLECTIVE, "comm.cpp: the all-reduce on a second stream behind an event; not attempted"),
    "fx3d_edges_dev_count": _replayed(TOPO), "fx3d_edges_dev_emit": _replayed(TOPO), "fx3d_laplacian_dev_csr": _replayed(TOPO),
    "fx3d_vertex_faces_dev": _replayed(TOPO), "fx3d_faces_padded_to_packed_dev": _replayed(TOPO),
    "fx3d_pointnet_forward": _replayed("test_pointnet[forward]"), "fx3d_pointnet_grad": _replayed("test_pointnet[grad]"),
    "fx3d_pointnet_forward_train": _replayed("test_pointnet[forward_train]"), "fx3d_pointnet_grad_train": _replayed("test_pointnet[grad_train]"),
    "fx3d_dgcnn_forward": _replayed("test_dgcnn[forward]"), "fx3d_dgcnn_grad": _replayed("test_dgcnn[grad]"),
    "fx3d_dgcnn_forward_train": _replayed("test_dgcnn[forward_train]"), "fx3d_dgcnn_grad_train": _replayed("test_dgcnn[grad_train]"),
    "fx3d_edgeconv_forward": _replayed("test_edgeconv[3_32_64_64-forward]"), "fx3d_edgeconv_bwd": _replayed("test_edgeconv[3_32_64_64-bwd]"),
    "fx3d_edgeconv_grad": _replayed("test_edgeconv[64_128_256-grad]"), "fx3d_edgeconv_forward_train": _replayed("test_edgeconv[64_128_256-forward_train]"),
    "fx3d_edgeconv_grad_train": _replayed("test_edgeconv[64_128_256-grad_train]"),
    "fx3d_crossentropy": _replayed(ELEM), "fx3d_dropout_mask": _replayed(ELEM), "fx3d_adam_step": _replayed(ELEM),
}
