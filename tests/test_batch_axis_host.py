"""The case table of tests/test_gpu_batch_axis.py against the header: every ``FX3D_API`` function with an ``int32_t B`` parameter has
a row with the largest B it accepts, the header's "Batch axis:" note next to the function states the same limit, and the size
queries -- host code -- accept that B and refuse the next.  No device."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "flux3d_hip.h")
NEAR = 80   # lines between a note and the declaration it speaks of: "next to its entry point" (a group shares one note)


def _header():
    with open(HEADER) as fh:
        return fh.read()


def _batched_entry_points(text):
    """{name: line of its declaration} of the functions with a batch argument (B; B0 and B1 of the pair forms)."""
    out = {}
    for m in re.finditer(r"FX3D_API fx3d_status (fx3d_\w+)\(([^;]*?)\);", text, re.S):
        if re.search(r"\bint32_t B[01]?\b", m.group(2)):
            out[m.group(1)] = text.count("\n", 0, m.start()) + 1
    return out


def _notes(text):
    """{name: [(limit, line)]} from the comments that hold "Batch axis:": each ``fx3d_a, fx3d_b: B <= n`` or ``...: unbounded``."""
    out = {}
    for c in re.finditer(r"/\*(.*?)\*/", text, re.S):
        if "Batch axis:" not in c.group(1):
            continue
        line = text.count("\n", 0, c.start()) + 1
        body = re.sub(r"\s*\n\s*\*\s*", " ", c.group(1).split("Batch axis:", 1)[1])
        for m in re.finditer(r"((?:fx3d_\w+(?:, )?)+): (?:B <= (\d+)|(unbounded))\b", body):
            for name in m.group(1).split(", "):
                out.setdefault(name, []).append((int(m.group(2)) if m.group(2) else "unbounded", line))
    return out


def test_the_note_parser_reads_groups_and_both_kinds_of_limit():
    text = "/* x.\n * Batch axis: fx3d_a,\n * fx3d_b: B <= 65535 -- as fx3d_c.  fx3d_d: unbounded -- why. */\n/* fx3d_e: B <= 3 */"
    assert _notes(text) == {"fx3d_a": [(65535, 1)], "fx3d_b": [(65535, 1)], "fx3d_d": [("unbounded", 1)]}
    decl = "FX3D_API fx3d_status fx3d_a(int32_t N,\n int32_t B);\nFX3D_API fx3d_status fx3d_b(int64_t B);\nFX3D_API fx3d_status fx3d_c(int32_t B0, int32_t B1);"
    assert _batched_entry_points(decl) == {"fx3d_a": 1, "fx3d_c": 4}


def test_every_entry_point_with_a_batch_argument_has_a_row_and_the_header_states_its_limit():
    import test_gpu_batch_axis as tb
    text = _header()
    entries, notes = _batched_entry_points(text), _notes(text)
    assert len(entries) >= 81
    assert set(tb.LIMITS) == set(entries), (sorted(set(entries) - set(tb.LIMITS)), sorted(set(tb.LIMITS) - set(entries)))
    for name, (limit, what) in tb.LIMITS.items():
        assert limit == "unbounded" or (isinstance(limit, int) and limit >= 1), (name, limit)
        assert isinstance(what, str) and what, name
        assert name in notes, f"{name}: no 'Batch axis:' note in the header"
        assert len(notes[name]) == 1, (name, notes[name])
        stated, line = notes[name][0]
        assert stated == limit, (name, "the header says", stated, "the table", limit)
        assert abs(entries[name] - line) <= NEAR, (name, "declared at line", entries[name], "its note at line", line)
    assert set(notes) <= set(entries), sorted(set(notes) - set(entries))


def test_no_case_is_skipped_or_expected_to_fail():
    import test_gpu_batch_axis as tb
    with open(tb.__file__) as fh:
        text = fh.read()
    for word in ("pytest.skip", "mark.skip", "xfail", "importorskip"):
        assert word not in text, word
    for obj in vars(tb).values():
        assert all(m.name in ("gpu", "parametrize") for m in getattr(obj, "pytestmark", [])), obj


# the size queries and plan descriptions with a batch argument: the arguments in front of and behind B, every size at its smallest
_L2 = (C.c_int32 * 2)(3, 32)
QUERIES = {
    "fx3d_chamfer_workspace_bytes": ((1, 1), (1,)), "fx3d_chamfer_fwd_bwd_workspace_bytes": ((1, 1), (1,)),
    "fx3d_chamfer_sampled_bwd_workspace_bytes": ((1, 1), ()), "fx3d_chamfer_pairwise_workspace_bytes": ((1, 1), (1,)),
    "fx3d_transform_workspace_bytes": ((3, 2), ()), "fx3d_knn_workspace_bytes": ((2, 64), (4, 4, 0)),
    "fx3d_sample_points_workspace_bytes": ((2,), ()), "fx3d_voxel_workspace_bytes": ((), ()),
    "fx3d_trimesh_voxel_workspace_bytes": ((3, 1), (2,)), "fx3d_voxel_mesh_workspace_bytes": ((1,), ()),
    "fx3d_vertex_faces_dev_workspace_bytes": ((1, 1), ()), "fx3d_faces_padded_to_packed_dev_workspace_bytes": ((), ()),
    "fx3d_pointnet_workspace_bytes": ((1,), (10,)), "fx3d_pointnet_train_workspace_bytes": ((1,), (10,)),
    "fx3d_pointnet_grad_workspace_bytes": ((1,), (10,)), "fx3d_pointnet_grad_train_workspace_bytes": ((1,), (10,)),
    "fx3d_dgcnn_workspace_bytes": ((2,), (1, 10)), "fx3d_dgcnn_train_workspace_bytes": ((2,), (1, 10)),
    "fx3d_dgcnn_grad_workspace_bytes": ((2,), (1, 10)), "fx3d_dgcnn_grad_train_workspace_bytes": ((2,), (1, 10)),
    "fx3d_edgeconv_workspace_bytes": ((_L2, 2, 1, 2), ()), "fx3d_edgeconv_train_workspace_bytes": ((_L2, 2, 1, 2), ()),
    "fx3d_edgeconv_bwd_workspace_bytes": ((_L2, 2, 1, 2), ()), "fx3d_edgeconv_grad_workspace_bytes": ((_L2, 2, 1, 2), ()),
    "fx3d_edgeconv_grad_train_workspace_bytes": ((_L2, 2, 1, 2), ()),
}


def test_the_query_table_is_complete():
    import test_gpu_batch_axis as tb
    assert set(QUERIES) == {n for n in tb.LIMITS if n.endswith("_workspace_bytes")}


@pytest.mark.parametrize("query", sorted(QUERIES))
def test_size_queries_accept_their_limit_and_refuse_the_next_batch(fx, query):
    """The model and transform queries go through the size check of their entry points (the adjoints' refusals, whose workspaces
    are tens of gigabytes at 65536 clouds, are held here)."""
    import test_gpu_batch_axis as tb
    limit, _ = tb.LIMITS[query]
    front, back = QUERIES[query]
    for B in (2, 65535, 65536, 65537) + (() if limit == "unbounded" else (limit, limit + 1)):
        if limit == "unbounded" or B <= limit:
            assert fx._lib.query_bytes(query, *front, B, *back) >= 0, (query, B)
            continue
        with pytest.raises(fx.Flux3DHipError) as ei:
            fx._lib.query_bytes(query, *front, B, *back)
        assert ei.value.code == tb.INVALID, (query, B, ei.value)
        if limit == 65535:
            assert re.search(r"\bB\b", str(ei.value)), ei.value


@pytest.mark.parametrize("B,ok", [(65535, True), (65536, False)])
def test_transform_plan_describe(fx, B, ok):
    buf = C.create_string_buffer(256)
    if ok:
        fx._lib.call("fx3d_transform_plan_describe", 3, 2, B, buf, 256)
        assert b"plan=" in buf.value
    else:
        with pytest.raises(fx.Flux3DHipError) as ei:
            fx._lib.call("fx3d_transform_plan_describe", 3, 2, B, buf, 256)
        assert ei.value.code == -1 and re.search(r"\bB\b", str(ei.value))


def test_nn1_plan_describe_takes_a_wide_batch(fx):
    buf = C.create_string_buffer(512)
    fx._lib.call("fx3d_nn1_plan_describe", 4, 4, 65537, 3, buf, 512)
    assert b"kernel=tiny" in buf.value and b"grid=131074" in buf.value   # 2 B blocks: the batch in the grid's x
