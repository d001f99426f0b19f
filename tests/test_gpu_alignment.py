"""Every kernel family on pointers aligned to 4 bytes only (DESIGN.md "Pointer alignment of caller arrays").

The rest of the GPU suite allocates every array from the pool: 256-byte aligned.  A caller of the C ABI passes slabs of odd-N
clouds, ``ptr + 12 * off``, ``ptr + 4 * at``, Julia views and torch slices, and about twenty host and kernel sites choose a code
path from the low four bits of such a pointer.  Each case here makes the same C-ABI call twice -- on arrays placed by
tests/misaligned.py at offsets 4 / 8 / 12 from a 16-byte boundary (each array argument alone at 4, then all together at 4, 8 and
12) and on aligned copies -- and asserts

  * every output bit-equal between the two (pointer alignment must not change a bit);
  * the 0xA5 pads around every placed output untouched (a vector store's head or tail running over);
  * the aligned result equal to the family's reference exactly as the family's own test checks it (the oracle, the tests/*_ref.py
    restatements, the golden known answers).  The one tolerance is LOSS_RTOL, chamfer loss against the oracle, as everywhere.

The families -- each one's call and reference -- are stated once, in tests/abi_families.py, and shared with
tests/test_gpu_workspace.py; this file is the driver (`hold`) and the case tables.

Sizes are multiples of 4, so that an aligned base means every cloud of the batch is aligned and the offset flips all of them:
that is what reaches the `D % 4 == 0 && aligned` branches, which odd sizes on aligned bases never do.  The library cannot
report its route at run time; that these shapes reach the scalar fall-backs is shown by value mutations of those fall-backs on
scratch builds (same section)."""
import numpy as np
import pytest

import abi_families as fam
import misaligned as mis
from abi_families import LOSS_RTOL, _abi, _bits_equal, _first_diff, _rand, _randn, _ws

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fresh_nullable():
    fam.NULLABLE.clear()


# ---------------------------------------------------------------------------------------------------------------- the driver
def _run(fx, call, arrs, case, ws_bytes=0):
    """The call on arrays placed by `case` ({name: offset}; absent: aligned): {output name: host result}, pads checked."""
    # (an int64 / uint64 array sits at its own alignment: offsets 4 and 12 become 0 and 8)
    placed = {a.name: mis.place(fx, a.host, case.get(a.name, 0) // max(a.host.itemsize, 4) * max(a.host.itemsize, 4), output=a.out)
              for a in arrs}
    ws = fx.DeviceArray.zeros((max(int(ws_bytes), 256),), np.uint8)
    assert ws.ptr % 256 == 0
    call(fam.Ptrs(**{n: p.ptr for n, p in placed.items()}), ws.ptr, int(ws_bytes))
    try:
        fx.synchronize()
    except fx.Flux3DHipError as e:  # a fault: nothing more is started on the device
        pytest.exit(f"{mis.case_id(case)}: {e}", returncode=3)
    out = {}
    for a in arrs:
        p = placed[a.name]
        if a.out:
            p.check_pads(f"{a.name} {mis.case_id(case)}")
            out[a.name] = p.to_host()
        else:
            assert _bits_equal(p.to_host(), a.host), f"input {a.name} was written ({mis.case_id(case)})"
    return out


def hold(fx, call, arrs, ws_bytes=0, skip=(), check=None):
    """Run `call` aligned and on every pointer pattern of its array arguments (but those in `skip`, which stay aligned): all
    outputs bit-equal to the aligned call's.  Returns the aligned results for the comparison with the family's reference.
    `check(results)`: for the few routes whose sums have no fixed order (float atomics) -- instead of the bit comparison, every
    placement's results go through the family's own bound against its reference."""
    base = _run(fx, call, arrs, {}, ws_bytes)
    if check:
        check(base)
    for case in mis.cases([a.name for a in arrs if a.name not in skip]):
        got = _run(fx, call, arrs, case, ws_bytes)
        if check:
            check(got)
            continue
        for k, want in base.items():
            assert _bits_equal(got[k], want), (mis.case_id(case), k, "elements differing / first:", _first_diff(got[k], want))
    return base


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("shape,entry", fam.NN_CASES)
def test_nn1_and_chamfer(gpu_fx, oracle, fx_option, shape, entry):
    fam.nn1_and_chamfer(gpu_fx, oracle, fx_option, hold, shape, entry)


def test_chamfer_backward_long_inverse_lists(gpu_fx, oracle):
    fam.chamfer_backward_long_inverse_lists(gpu_fx, oracle, hold)


@pytest.mark.parametrize("entry", ["fx3d_knn", "fx3d_knn_ws"])
@pytest.mark.parametrize("case", list(fam.KNN_CASES))
def test_knn(gpu_fx, oracle, fx_option, case, entry):
    fam.knn(gpu_fx, oracle, fx_option, hold, case, entry)


@pytest.mark.parametrize("K", [4, 5])
@pytest.mark.parametrize("F", [3, 4, 64])
def test_graph_features(gpu_fx, oracle, fx_option, F, K):
    fam.graph_features(gpu_fx, oracle, fx_option, hold, F, K)


@pytest.mark.parametrize("n", [1024, 1025, 1026, 1027])
@pytest.mark.parametrize("D", [3, 4])
def test_transforms_dense(gpu_fx, D, n):
    fam.transforms_dense(gpu_fx, hold, D, n)


def test_transforms_ragged_mesh_batch_as_a_slab_of_a_longer_packed_array(gpu_fx):
    fam.transforms_ragged_mesh_batch_as_a_slab_of_a_longer_packed_array(gpu_fx)


@pytest.mark.parametrize("res", [8, 32])
def test_pointcloud_to_voxel(gpu_fx, oracle, res):
    fam.pointcloud_to_voxel(gpu_fx, oracle, hold, res)


@pytest.mark.parametrize("res", [8, 28])
def test_trimesh_to_voxel(gpu_fx, res):
    fam.trimesh_to_voxel(gpu_fx, hold, res)


@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_voxel_to_trimesh_exact(gpu_fx, extra):
    fam.voxel_to_trimesh_exact(gpu_fx, hold, extra)


@pytest.mark.parametrize("index_type", ["int32", "uint32", "int64", "upload_uint32", "upload_int64"])
def test_mesh_faces_through_index_convert_and_upload(gpu_fx, index_type):
    fam.mesh_faces_through_index_convert_and_upload(gpu_fx, hold, index_type)


def test_mesh_face_areas(gpu_fx, oracle):
    fam.mesh_face_areas(gpu_fx, oracle, hold)


def test_mesh_losses_and_adjoints(gpu_fx, oracle):
    fam.mesh_losses_and_adjoints(gpu_fx, oracle, hold)


def test_mesh_sampling_and_ordered_adjoint(gpu_fx, oracle):
    fam.mesh_sampling_and_ordered_adjoint(gpu_fx, oracle, hold)


def test_mesh_normals_and_adjoints(gpu_fx):
    fam.mesh_normals_and_adjoints(gpu_fx, hold)


def test_mesh_topology_tables(gpu_fx):
    fam.mesh_topology_tables(gpu_fx, hold)


@pytest.mark.parametrize("entry", ["forward", "forward_train", "grad", "grad_train"])
def test_pointnet(gpu_fx, entry):
    fam.pointnet(gpu_fx, hold, entry)


@pytest.mark.parametrize("entry", ["forward", "forward_idx", "forward_train", "bwd", "grad", "grad_train"])
@pytest.mark.parametrize("name", list(fam.EDGECONV_LAYERS))
def test_edgeconv(gpu_fx, name, entry):
    fam.edgeconv(gpu_fx, hold, name, entry)


@pytest.mark.parametrize("entry", ["forward", "forward_train", "grad"])
def test_dgcnn(gpu_fx, entry):
    fam.dgcnn(gpu_fx, hold, entry)


# ------------------------------------------------------------------------------------------------ capture and replay
def test_capture_and_replay_on_misaligned_pointers(gpu_fx, oracle):
    """One chamfer forward and one kNN (with scratch: the pre-pass shape, pushed off it by the offsets) recorded into a graph on
    arrays placed at 4, 12 and 8 bytes off: the replay's outputs are the eager call's bits, and the pads stay intact."""
    fx = gpu_fx
    N, M, B = 1024, 1024, 2
    x, y = _rand((3, N, B), 1), _rand((3, M, B), 2)
    D, n, k = 64, 256, 20
    f = _randn((D, n, B), 3)
    nbc, nbk = _ws(fx, "fx3d_chamfer_workspace_bytes", N, M, B, 3), _ws(fx, "fx3d_knn_workspace_bytes", n, n, B, D, k, 1)
    assert nbk > 0
    px, py, pf = mis.place(fx, x, 4), mis.place(fx, y, 12), mis.place(fx, f, 8)

    def outputs():
        return dict(loss=mis.place(fx, np.zeros(1, np.float32), 4, output=True), ix=mis.place(fx, np.zeros((N, B), np.int32), 8, output=True),
                    iy=mis.place(fx, np.zeros((M, B), np.int32), 12, output=True), idx=mis.place(fx, np.zeros((k, n, B), np.int32), 4, output=True),
                    dist=mis.place(fx, np.zeros((k, n, B), np.float32), 12, output=True))
    wsc, wsk = fx.DeviceArray.zeros((nbc,), np.uint8), fx.DeviceArray.zeros((nbk,), np.uint8)

    def enqueue(o, s):
        _abi(fx, "fx3d_chamfer_fwd")(px.ptr, N, py.ptr, M, B, 3, 0.7, 1.3, o["loss"].ptr, None, o["ix"].ptr, o["iy"].ptr, wsc.ptr, nbc, s)
        _abi(fx, "fx3d_knn_ws")(pf.ptr, n, pf.ptr, n, B, D, k, 1, o["idx"].ptr, o["dist"].ptr, wsk.ptr, nbk, s)
    eager = outputs()
    enqueue(eager, None)
    fx.synchronize()
    st = fx.Stream.create()
    rec = outputs()
    enqueue(rec, st.handle)   # warm-up on the capture stream
    st.synchronize()
    g = fx.Graph()
    with g.capture(st):
        enqueue(rec, st.handle)
    for o in rec.values():    # the recording itself ran nothing: wipe what the warm-up wrote
        o.arr.copy_(np.zeros(o.arr.shape, o.arr.dtype))
    g.launch(st)
    st.synchronize()
    for name in eager:
        eager[name].check_pads(name)
        rec[name].check_pads(name + " (replay)")
        assert _bits_equal(rec[name].to_host(), eager[name].to_host()), name
    ox, oy = oracle.nn1(x, y)
    assert np.array_equal(eager["ix"].to_host(), ox) and np.array_equal(eager["iy"].to_host(), oy)
    assert np.isclose(eager["loss"].to_host()[0], oracle.chamfer_distance(x, y, 0.7, 1.3), rtol=LOSS_RTOL, atol=0)
    oi, od = oracle.knn(f, k, drop_first=True)
    assert np.array_equal(eager["idx"].to_host(), oi) and np.array_equal(eager["dist"].to_host(), od)
