"""stnKD(K) as a layer of its own, the part that needs no GPU: the new header's declarations against the loader's table and
the library's exports (and nothing of it in flux3d_hip.h or _lib.SIGNATURES), the header's Capture and Batch-axis notes, every
refusal before any device work with its status and the offending value in the message, the size queries at their limits, the
parameter count against the layer table, the restatement tests/stnkd_ref.py against torch in float64 (eval mode and
batch_norm(training=True); tests/stnkd_torch_eval.py), and the Python argument errors."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import stnkd_ref as sref
from conftest import ROOT

F32 = np.float32
INVALID, UNSUPPORTED = -1, -5  # FX3D_ERR_INVALID_ARG, FX3D_ERR_UNSUPPORTED
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "include", "flux3d_hip_layers.h")
MAIN_HEADER = os.path.join(ROOT, "include", "flux3d_hip.h")
NAMES = ("fx3d_stnkd_param_count", "fx3d_stnkd_workspace_bytes", "fx3d_stnkd_forward", "fx3d_stnkd_train_workspace_bytes",
         "fx3d_stnkd_forward_train")
MOMENTUM = 0.1


def _text(path):
    with open(path) as fh:
        return fh.read()


def _declared(text):
    """{name: [parameter, ...]} of the header's FX3D_API functions."""
    return {m.group(1): [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
            for m in re.finditer(r"FX3D_API\s+fx3d_status\s+(fx3d_\w+)\s*\(([^;]*?)\);", text, re.S)}


def _notes(text, word, kinds):
    """{name: kind} from the comments that hold ``word``: each ``fx3d_a, fx3d_b: kind`` (the parsers of tests/test_replay_host.py
    and tests/test_batch_axis_host.py)."""
    out = {}
    for c in re.finditer(r"/\*(.*?)\*/", text, re.S):
        if word not in c.group(1):
            continue
        body = re.sub(r"\s*\n\s*\*\s*", " ", c.group(1).split(word, 1)[1])
        for m in re.finditer(r"((?:fx3d_\w+(?:, )?)+): (%s)" % kinds, body):
            for name in m.group(1).split(", "):
                assert name not in out, (name, "has two notes")
                out[name] = m.group(2)
    return out


def test_the_header_the_loader_and_the_library_name_the_same_functions(fx):
    from flux3d_jl_amd import _lib
    decl = _declared(_text(HEADER))
    assert set(decl) == set(NAMES) == set(_lib.LAYER_SIGNATURES), set(decl) ^ set(_lib.LAYER_SIGNATURES)
    lib = ctypes.CDLL(fx.LIB_PATH)
    loaded = _lib.load()
    for name, params in decl.items():
        assert hasattr(lib, name), f"{name} is not exported"
        sig = _lib.LAYER_SIGNATURES[name]
        assert len(sig) == len(params), (name, len(sig), params)
        fn = getattr(loaded, name)
        assert fn.argtypes == sig and fn.restype is _lib.c_i32, name  # bound by load(), so _lib.call / query_bytes find them
        for ctype, p in zip(sig, params):
            if re.match(r"int32_t\s+\w+$", p):
                assert ctype is _lib.c_i32, (name, p)
            elif re.match(r"float\s+\w+$", p):
                assert ctype is _lib.c_f32, (name, p)
            elif re.match(r"size_t\s+\w+$", p):
                assert ctype is _lib.sz, (name, p)
            elif re.match(r"fx3d_stream_t\s+\w+$", p) or re.match(r"(const\s+)?(float|void)\s*\*\s*\w+$", p):
                assert ctype is _lib.vp, (name, p)
            else:
                assert re.match(r"(int64_t|size_t)\s*\*\s*\w+$", p) and ctype not in (_lib.c_i32, _lib.c_f32, _lib.sz, _lib.vp), (name, p)
    for name in ("fx3d_stnkd_forward", "fx3d_stnkd_forward_train"):  # the stream last
        assert re.match(r"fx3d_stream_t\s+\w+$", decl[name][-1]), name
    assert '#include "flux3d_hip.h"' in _text(HEADER)


def test_the_main_header_and_its_table_hold_no_stnkd_name():
    from flux3d_jl_amd import _lib
    assert "fx3d_stnkd" not in _text(MAIN_HEADER).lower()  # (its prose names PointNet's stnKD(3) / stnKD(64) blocks)
    assert not [n for n in _lib.SIGNATURES if "stnkd" in n.lower()]
    assert not set(_lib.SIGNATURES) & set(_lib.LAYER_SIGNATURES)


def test_the_header_carries_the_notes_of_its_streamed_and_batched_functions():
    text = _text(HEADER)
    decl = _declared(text)
    streamed = {n for n, ps in decl.items() if any(re.match(r"fx3d_stream_t\s+\w+$", p) for p in ps)}
    batched = {n for n, ps in decl.items() if any(re.match(r"int32_t B$", p) for p in ps)}
    assert streamed == {"fx3d_stnkd_forward", "fx3d_stnkd_forward_train"}
    assert batched == set(NAMES) - {"fx3d_stnkd_param_count"}
    capture = _notes(text, "Capture:", "replayed|copies to the host|host code|collective")
    assert capture == {n: "replayed" for n in streamed}, capture
    axis = _notes(text, "Batch axis:", r"B <= \d+|unbounded")
    assert axis == {n: "B <= 65535" for n in batched}, axis
    for word in ("src/models/pointnet.jl:3-20", "fmaf(x[c], W[c,o], acc)", "1 <= K <= 128", "FX3D_ERR_UNSUPPORTED",
                 "tests/stnkd_ref.py", "FX3D_POINTNET_STAT_GROUPS"):
        assert word in text, word


def test_the_header_is_plain_c(tmp_path):
    import shutil
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "use.c"
    src.write_text('#include "flux3d_hip_layers.h"\nint main(void) { return FX3D_STNKD_STAT_COUNT == 2944 && FX3D_STNKD_MAX_K == 128 ? 0 : 1; }\n')
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)


@pytest.mark.parametrize("K", [1, 3, 5, 64, 128])
def test_param_count_is_the_layer_table(fx, K):
    from flux3d_jl_amd import _lib, models
    count = ctypes.c_int64(0)
    _lib.call("fx3d_stnkd_param_count", K, ctypes.byref(count))
    spec = [(name[1:], kind, ch) for name, kind, ch in models._stn_spec("", K)]
    assert [n for n, _, _ in spec] == ["conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "dense1", "dense2", "bn4", "dense3"]
    want = sum(ch[0] * ch[1] + ch[1] if kind != "bn" else 4 * ch for _, kind, ch in spec)
    assert count.value == want == sum(int(np.prod(s)) for s in sref.param_shapes(K).values())
    assert models.stnkd_param_shapes(K) == sref.param_shapes(K) and list(models.stnkd_param_shapes(K)) == list(sref.param_shapes(K))
    m = fx.stnKD(K)
    assert m.param_count == want and m.flat_params().size == want
    assert [n for n, *_ in m._stat_slots()] == list(sref.BN_ORDER)


def test_the_pointnet_slices_are_stnkd_buffers(fx):
    """layout_stn walks both: the stn.* / fstn.* slice of a PointNet's flat buffer is the flat buffer of from_pointnet's layer."""
    net = fx.PointNet(10, seed=3)
    rng = np.random.default_rng(4)
    net.load({k: rng.standard_normal(v.shape).astype(F32) for k, v in net.params.items()})
    flat, names = net.flat_params(), list(net._shapes())
    offset, at = {}, 0
    for n in names:
        offset[n] = at
        at += net.params[n].size
    for which, K in (("stn", 3), ("fstn", 64)):
        layer = fx.stnKD.from_pointnet(net, which)
        assert layer.K == K
        mine = layer.flat_params()
        start = offset[f"{which}.conv1.weight"]
        assert np.array_equal(mine.view(np.uint32), flat[start:start + mine.size].view(np.uint32)), which
        layer.params["conv1.bias"][0] += 1  # a copy, not a view of the network's arrays
        assert net.params[f"{which}.conv1.bias"][0] != layer.params["conv1.bias"][0]


def test_the_c_entry_points_refuse_before_any_device_work(fx):
    """No call here has arguments that would pass the checks: the dummy pointers are never dereferenced."""
    from flux3d_jl_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(4096)
    nb, count = ctypes.c_size_t(0), ctypes.c_int64(0)

    def fwd(K=5, N_=64, B_=2, params=dummy, x=dummy, out=dummy, pooled=None, ws=dummy, ws_bytes=1 << 40):
        return lib.fx3d_stnkd_forward(params, K, x, N_, B_, out, pooled, ws, ws_bytes, None)

    def train(K=5, N_=64, B_=2, params=dummy, x=dummy, momentum=0.1, out=dummy, pooled=None, stats=dummy, running=None, ws=dummy,
              ws_bytes=1 << 40):
        return lib.fx3d_stnkd_forward_train(params, K, x, N_, B_, momentum, out, pooled, stats, running, ws, ws_bytes, None)

    def size(N_=64, B_=2, K=5, out=ctypes.byref(nb), train_=False):
        return (lib.fx3d_stnkd_train_workspace_bytes if train_ else lib.fx3d_stnkd_workspace_bytes)(N_, B_, K, out)

    def says(*words):
        msg = _lib.last_error()
        return all(w in msg for w in words)

    # NULL required pointers
    assert lib.fx3d_stnkd_param_count(5, None) == INVALID and says("NULL")
    assert size(out=None) == INVALID and says("NULL") and size(out=None, train_=True) == INVALID and says("NULL")
    for k in ("params", "x", "out", "ws"):
        assert fwd(**{k: None}) == INVALID and says("fx3d_stnkd_forward", "NULL"), k
    for k in ("params", "x", "out", "stats", "ws"):
        assert train(**{k: None}) == INVALID and says("fx3d_stnkd_forward_train", "NULL"), k
    # K outside [1, 128]: unsupported, the value in the message
    for K in (0, -1, 129, 1 << 20):
        assert lib.fx3d_stnkd_param_count(K, ctypes.byref(count)) == UNSUPPORTED and says("fx3d_stnkd_param_count", f"got {K}"), K
        assert fwd(K=K) == UNSUPPORTED and says("fx3d_stnkd_forward", "[1, 128]", f"got {K}"), K
        assert train(K=K) == UNSUPPORTED and says("fx3d_stnkd_forward_train", f"got {K}"), K
        assert size(K=K) == UNSUPPORTED and says("fx3d_stnkd_workspace_bytes", f"got {K}"), K
        assert size(K=K, train_=True) == UNSUPPORTED and says("fx3d_stnkd_train_workspace_bytes", f"got {K}"), K
    # the sizes
    for kw, words in ((dict(N_=0), ("N=0",)), (dict(B_=0), ("B=0",)), (dict(B_=65536, N_=8), ("B", "65536"))):
        assert fwd(**kw) == INVALID and says("fx3d_stnkd_forward", *words), kw
        assert train(**kw) == INVALID and says("fx3d_stnkd_forward_train", *words), kw
        assert train(**kw, pooled=dummy, running=dummy) == INVALID and says(*words), kw
        assert size(**kw) == INVALID and says("fx3d_stnkd_workspace_bytes", *words), kw
        assert size(**kw, train_=True) == INVALID and says("fx3d_stnkd_train_workspace_bytes", *words), kw
    assert train(B_=1) == INVALID and says("fx3d_stnkd_forward_train", "B >= 2", "got 1")
    assert size(B_=1, train_=True) == INVALID and says("fx3d_stnkd_train_workspace_bytes", "B >= 2", "got 1")
    assert size(B_=1) == 0  # test mode takes one cloud
    for mtm in (-0.1, 1.5, float("nan"), float("inf")):
        assert train(momentum=mtm) == INVALID and says("momentum"), mtm
    # the workspace: one byte short, or not 16-byte aligned
    assert size() == 0 and nb.value % 256 == 0 and nb.value >= 1024 * 1 * 2 * 4
    test_bytes = nb.value
    assert fwd(ws_bytes=test_bytes - 1) == INVALID and says("workspace", str(test_bytes), str(test_bytes - 1))
    assert fwd(ws=ctypes.c_void_p(4096 + 8), ws_bytes=test_bytes) == INVALID and says("16-byte aligned")
    assert size(train_=True) == 0 and nb.value >= test_bytes + 2 * 1024 * 1 * 2 * 8 + 256 * 2 * 4  # + the tile sums, relu(dense2)
    assert train(ws_bytes=nb.value - 1) == INVALID and says("workspace", str(nb.value))
    assert train(ws=ctypes.c_void_p(4096 + 8), ws_bytes=nb.value) == INVALID and says("16-byte aligned")


@pytest.mark.parametrize("query", ["fx3d_stnkd_workspace_bytes", "fx3d_stnkd_train_workspace_bytes"])
def test_size_queries_at_their_limits(fx, query):
    q = fx._lib.query_bytes
    assert q(query, 1, 65535, 128) > 0 and q(query, 1, 2, 1) > 0
    with pytest.raises(fx.Flux3DHipError) as ei:
        q(query, 1, 65536, 128)
    assert ei.value.code == INVALID and re.search(r"\bB\b", str(ei.value)) and "65536" in str(ei.value)
    with pytest.raises(fx.Flux3DHipError) as ei:
        q(query, 1, 65535, 129)
    assert ei.value.code == UNSUPPORTED and "129" in str(ei.value)
    # no (C, N, B) activation array in the workspace: it does not grow with K
    assert q(query, 1024, 32, 128) == q(query, 1024, 32, 1)


# ---- the restatement against torch ------------------------------------------------------------------------------------------------
N, B = 70, 4


def _split(flat):
    mu, var, at = [], [], 0
    for bn in sref.BN_ORDER:
        C = sref.BN_WIDTH[bn]
        mu.append(flat[at:at + C])
        var.append(flat[at + C:at + 2 * C])
        at += 2 * C
    assert at == flat.size == 2944
    return np.concatenate(mu), np.concatenate(var)


@pytest.mark.parametrize("K", [1, 5, 64])
def test_the_restatement_is_an_stnkd(K, tmp_path):
    """Against torch in float64, eval mode and batch_norm(training=True), with the bound of
    test_pointnet_train_host.py::test_the_restatement_is_a_pointnet_in_training_mode: the restatement's relative error is at most
    8 x torch-float32's, for both transforms, the batch means and variances and the updated running means and variances."""
    rng = np.random.default_rng(300 + K)
    X = rng.standard_normal((K, N, B)).astype(F32)
    P = sref.random_params(K, seed=K)
    ev, tr = sref.forward(X, P, K), sref.forward_train(X, P, K, momentum=MOMENTUM)
    assert ev["out"].shape == tr["out"].shape == (K, K, B) and ev["pooled"].shape == (1024, B)
    src, dst = os.path.join(str(tmp_path), "case.npz"), os.path.join(str(tmp_path), "torch.npz")
    np.savez(src, X=X, momentum=MOMENTUM, **P)
    subprocess.run([sys.executable, os.path.join(HERE, "stnkd_torch_eval.py"), src, dst], check=True, timeout=600)
    t = np.load(dst)
    got = {"eval": ev["out"], "train": tr["out"]}
    got["batch means"], got["batch variances"] = _split(sref.flat_stats(tr["batch_stats"]))
    got["running means"], got["running variances"] = _split(sref.flat_stats(tr["running"]))
    t64, t32 = {}, {}
    for d, tag in ((t64, "64"), (t32, "32")):
        d["eval"], d["train"] = t["eval" + tag], t["train" + tag]
        d["batch means"], d["batch variances"] = _split(t["stats" + tag])
        d["running means"], d["running variances"] = _split(t["running" + tag])
    assert not np.array_equal(t64["eval"], t64["train"])
    bad = []
    for key in got:
        assert got[key].shape == t64[key].shape, key
        scale = float(np.max(np.abs(t64[key])))
        err_ref = float(np.max(np.abs(got[key].astype(np.float64) - t64[key]))) / scale
        err_t32 = float(np.max(np.abs(t32[key].astype(np.float64) - t64[key]))) / scale
        print(f"  K={K} {key}: relative error of the restatement {err_ref:.3e}, of torch float32 {err_t32:.3e}")
        if not (err_t32 > 0 and err_ref <= 8 * err_t32):
            bad.append((key, err_ref, err_t32))
    assert not bad, bad


def test_the_restatement_is_pointnet_refs_stage():
    """On a PointNet's parameters the restatement is pointnet_ref's stn and fstn, bit for bit (it imports them: a renamed key
    or a transposed layout would show here)."""
    import pointnet_ref as ref
    P = ref.random_params(10, seed=5)
    X = np.random.default_rng(6).standard_normal((3, 66, 2)).astype(F32)
    whole = ref.forward(X, P)
    for which, K, x in (("stn", 3, X), ("fstn", 64, np.transpose(whole["h"], (2, 1, 0)))):
        mine = sref.forward(x, {k[len(which) + 1:]: v for k, v in P.items() if k.startswith(which + ".")}, K)
        assert np.array_equal(mine["out"].view(np.uint32), whole[which].view(np.uint32)), which


# ---- Python -----------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_before_any_device_call(fx):
    assert fx.stnKD is fx.models.stnKD
    for K in (0, 129, -3):
        with pytest.raises(ValueError, match=r"\[1, 128\]"):
            fx.stnKD(K)
    for K in (2.5, "3", None, True):
        with pytest.raises(TypeError, match="integer"):
            fx.stnKD(K)
    m = fx.stnKD(5)
    assert set(m.params) == set(sref.param_shapes(5)) and m.params["dense3.weight"].shape == (25, 256)
    with pytest.raises(ValueError, match="5 channels"):
        m.forward(np.zeros((3, 8, 2), F32))
    with pytest.raises(ValueError, match="5 channels"):
        m.forward_train(np.zeros((6, 8, 2), F32))
    with pytest.raises(ValueError, match="must be"):
        m.forward(np.zeros((5,), F32))
    with pytest.raises(ValueError, match="at least one point"):
        m.forward(np.zeros((5, 0, 2), F32))
    with pytest.raises(ValueError, match="PointCloud has 3 channels"):
        m.forward(fx.PointCloud(np.zeros((3, 8, 2), F32)))
    with pytest.raises(ValueError, match="at least two clouds"):
        m.forward_train(np.zeros((5, 8, 1), F32))
    with pytest.raises(ValueError, match="at least two clouds"):
        m.forward_train(np.zeros((5, 8), F32))
    for mtm in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            m.forward_train(np.zeros((5, 8, 2), F32), momentum=mtm)
    with pytest.raises(ValueError, match="do not match"):
        m.load({k: v for k, v in m.params.items() if k != "bn4.mu"})
    with pytest.raises(ValueError, match="dense3.weight must be"):
        m.load({**m.params, "dense3.weight": np.zeros((9, 256), F32)})
    with pytest.raises(TypeError, match="PointNet"):
        fx.stnKD.from_pointnet(m, "stn")
    with pytest.raises(ValueError, match="'stn' or 'fstn'"):
        fx.stnKD.from_pointnet(fx.PointNet(10), "feat")
