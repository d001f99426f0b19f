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

Sizes are multiples of 4, so that an aligned base means every cloud of the batch is aligned and the offset flips all of them:
that is what reaches the `D % 4 == 0 && aligned` branches, which odd sizes on aligned bases never do.  The library cannot
report its route at run time; that these shapes reach the scalar fall-backs is shown by value mutations of those fall-backs on
scratch builds (same section)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
import misaligned as mis
import transforms_ref as tref
from test_gpu_hardening import LOSS_RTOL

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the driver
class Arr:
    """One array argument: its name in the case table, its host contents (an output's initial contents), input or output."""

    def __init__(self, name, host, out=False):
        self.name, self.host, self.out = name, np.asfortranarray(host), out


def I(name, host, dtype=None):  # noqa: E743
    return Arr(name, np.asarray(host, dtype=dtype))


def O(name, shape, dtype=np.float32, init=None):  # noqa: E743
    return Arr(name, np.zeros(shape, dtype, order="F") if init is None else np.asarray(init, dtype), out=True)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _first_diff(a, b):
    """(how many elements differ in their bits, the first one's column-major position)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return ("shape / dtype", a.shape, a.dtype, b.shape, b.dtype)
    u = f"u{a.dtype.itemsize}"
    d = np.flatnonzero(np.asarray(a).ravel(order="F").view(u) != np.asarray(b).ravel(order="F").view(u))
    return (int(d.size), int(d[0])) if d.size else (0, -1)


def _run(fx, call, arrs, case, ws_bytes=0):
    """The call on arrays placed by `case` ({name: offset}; absent: aligned): {output name: host result}, pads checked."""
    # (an int64 / uint64 array sits at its own alignment: offsets 4 and 12 become 0 and 8)
    placed = {a.name: mis.place(fx, a.host, case.get(a.name, 0) // max(a.host.itemsize, 4) * max(a.host.itemsize, 4), output=a.out)
              for a in arrs}
    ws = fx.DeviceArray.zeros((max(int(ws_bytes), 256),), np.uint8)
    assert ws.ptr % 256 == 0
    call(SimpleNamespace(**{n: p.ptr for n, p in placed.items()}), ws.ptr, int(ws_bytes))
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


def _abi(fx, name):
    def f(*args):
        try:
            fx._lib.call(name, *args)
        except fx.Flux3DHipError as e:
            if e.code == -2:  # FX3D_ERR_HIP is sticky (a fault poisons the context): nothing more is started on the device
                pytest.exit(f"{name}: {e}", returncode=3)
            raise
    return f


def _ws(fx, query, *args):
    return fx._lib.query_bytes(query, *args)


def _rand(shape, seed, scale=1.0):
    return np.asfortranarray((np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(scale)))


def _randn(shape, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


# ------------------------------------------------------------------------------------- nn1, chamfer forward, fwd_bwd, backward
def _nn1_plan(fx, N, M, B, D):
    buf = C.create_string_buffer(512)
    fx._lib.call("fx3d_nn1_plan_describe", N, M, B, D, buf, 512)
    return dict(kv.split("=") for kv in buf.value.decode().split())


_NN_REF = {}


def _nn_reference(oracle, key, x, y, big):
    """Oracle indices (and distances: small shapes) of one shape, computed once and shared by the entry points' cases."""
    if key not in _NN_REF:
        if big:
            ox, oy, _ = oracle.nn1_allcores(x, y, threads=16)
            _NN_REF[key] = (ox, oy, None, None)
        else:
            _NN_REF[key] = oracle.nn1(x, y, want_dist=True)
    return _NN_REF[key]


# name: (N, M, B, D, options, what the plan must say, oracle over all cores)
NN_SHAPES = {
    "tiny": (64, 64, 2, 3, {}, dict(kernel="tiny"), False),
    "1024": (1024, 1024, 2, 3, {}, dict(), False),
    "mfma_filter": (4096, 4096, 2, 3, {}, dict(kernel="f16"), False),
    "split_plan": (5000, 5000, 1, 3, {}, dict(kernel="f16", split=True), True),
    "pruned": (4096, 4096, 17, 3, {}, dict(kernel="f16", nsplit="1", pruned=True), True),
    "exact_loop": (1024, 1024, 2, 3, {"nn1_variant": 0}, dict(kernel="small_d", variant="0"), False),
    "d2": (256, 256, 2, 2, {}, dict(kernel="small_d"), False),
    "d8": (256, 256, 2, 8, {}, dict(kernel="generic"), False),
}


# only the chamfer forward entry points prune: fx3d_nn1 and the adjoint at 4096 points are the mfma_filter case
NN_CASES = [(s, e) for s in NN_SHAPES for e in ("nn1", "chamfer_fwd", "chamfer_fwd_bwd", "chamfer_bwd")
            if not (s == "pruned" and e in ("nn1", "chamfer_bwd"))]


@pytest.mark.parametrize("shape,entry", NN_CASES)
def test_nn1_and_chamfer(gpu_fx, oracle, fx_option, shape, entry):
    fx = gpu_fx
    N, M, B, D, opts, want, big = NN_SHAPES[shape]
    for k, v in opts.items():
        fx_option(k, v)
    plan = _nn1_plan(fx, N, M, B, D)
    for k, v in want.items():
        if k == "split":
            assert int(plan["nsplit"]) > 1, plan
        elif k == "pruned":
            assert fx._lib.get_option("nn1_prune") == 1
            full = _ws(fx, "fx3d_chamfer_workspace_bytes", N, M, B, D)
            with fx._lib.option("nn1_prune", 0):
                assert full > _ws(fx, "fx3d_chamfer_workspace_bytes", N, M, B, D), "the shape no longer takes the pruned launch"
        else:
            assert plan[k] == v, plan
    x, y = _rand((D, N, B), 11 * N + B + D), _rand((D, M, B), 13 * M + B + D)
    ox, oy, odx, ody = _nn_reference(oracle, shape, x, y, big)
    w1, w2, gout = 0.7, 1.3, 2.0
    if entry == "nn1":
        arrs = [I("x", x), I("y", y), O("idx_x", (N, B), np.int32), O("idx_y", (M, B), np.int32), O("dmin_x", (N, B)), O("dmin_y", (M, B))]
        r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_nn1")(p.x, N, p.y, M, B, D, p.idx_x, p.idx_y, p.dmin_x, p.dmin_y, None), arrs)
        assert np.array_equal(r["idx_x"], ox) and np.array_equal(r["idx_y"], oy)
        if odx is not None:
            assert np.array_equal(r["dmin_x"], odx) and np.array_equal(r["dmin_y"], ody)
        return
    if entry == "chamfer_bwd":
        arrs = [I("x", x), I("y", y), I("idx_x", ox), I("idx_y", oy), O("gx", (D, N, B)), O("gy", (D, M, B))]
        r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_chamfer_bwd")(p.x, N, p.y, M, B, D, p.idx_x, p.idx_y, w1, w2, gout, B, p.gx, p.gy, None),
                 arrs)
        ogx, ogy = oracle.chamfer_bwd(x, y, ox, oy, w1, w2, gout)
        assert np.array_equal(r["gx"], ogx) and np.array_equal(r["gy"], ogy)
        return
    if big:
        with np.errstate(all="ignore"):
            oloss = oracle.chamfer_loss_pairwise(x, y, ox, oy, w1, w2)
    else:
        oloss = oracle.chamfer_distance(x, y, w1, w2)
    if entry == "chamfer_fwd":
        nb = _ws(fx, "fx3d_chamfer_workspace_bytes", N, M, B, D)
        arrs = [I("x", x), I("y", y), O("loss", (1,)), O("idx_x", (N, B), np.int32), O("idx_y", (M, B), np.int32)]
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_chamfer_fwd")(p.x, N, p.y, M, B, D, w1, w2, p.loss, None, p.idx_x, p.idx_y, ws, n, None),
                 arrs, nb)
    else:
        nb = _ws(fx, "fx3d_chamfer_fwd_bwd_workspace_bytes", N, M, B, D)
        arrs = [I("x", x), I("y", y), O("loss", (1,)), O("gx", (D, N, B)), O("gy", (D, M, B)), O("idx_x", (N, B), np.int32),
                O("idx_y", (M, B), np.int32)]
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_chamfer_fwd_bwd")(p.x, N, p.y, M, B, D, w1, w2, gout, B, p.loss, None, p.gx, p.gy,
                                                                     p.idx_x, p.idx_y, ws, n, None), arrs, nb)
        ogx, ogy = oracle.chamfer_bwd(x, y, ox, oy, w1, w2, gout)
        assert np.array_equal(r["gx"], ogx) and np.array_equal(r["gy"], ogy)
    assert np.array_equal(r["idx_x"], ox) and np.array_equal(r["idx_y"], oy)
    assert np.isclose(r["loss"][0], oloss, rtol=LOSS_RTOL, atol=0), (r["loss"][0], oloss)


def test_chamfer_backward_long_inverse_lists(gpu_fx, oracle):
    """The adjoint on index maps with long inverse lists (the "clusters" kind of test_gpu_parity's test of that name), D = 3."""
    fx = gpu_fx
    rng = np.random.default_rng(sum(map(ord, "clusters")) * 131 + 3)
    N, M, B, D = 6000, 9000, 3, 3
    x, y = _randn((D, N, B), 5), _randn((D, M, B), 6)
    ix = np.asfortranarray(rng.integers(0, 40, (N, B)).astype(np.int32) * 200)
    iy = np.asfortranarray(rng.integers(0, 30, (M, B)).astype(np.int32) * 199)
    arrs = [I("x", x), I("y", y), I("idx_x", ix), I("idx_y", iy), O("gx", (D, N, B)), O("gy", (D, M, B))]
    r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_chamfer_bwd")(p.x, N, p.y, M, B, D, p.idx_x, p.idx_y, 0.9, 1.1, 1.0, B, p.gx, p.gy, None), arrs)
    ogx, ogy = oracle.chamfer_bwd(x, y, ix, iy, 0.9, 1.1, 1.0)
    assert _bits_equal(r["gx"], ogx) and _bits_equal(r["gy"], ogy)


# ------------------------------------------------------------------------------------------------------------------------ kNN
# name: (D, N, M, B, k, drop, options, the workspace query must be positive: True, or None where the shape decides)
KNN_CASES = {
    "d3_k20": (3, 1024, 1024, 2, 20, 1, {}, None),
    "d3_k5": (3, 1024, 1024, 2, 5, 1, {}, None),
    "d3_kk64": (3, 1024, 1024, 2, 63, 1, {}, None),
    "d64_prepass": (64, 256, 256, 2, 20, 1, {}, True),
    "d8_prepass": (8, 256, 256, 2, 20, 1, {}, True),
    "d128_prepass": (128, 256, 256, 2, 20, 1, {}, True),
    "d64_slices2": (64, 1024, 1024, 2, 20, 1, {"knn_slices": 2}, True),
    "d4_select_k70": (4, 64, 332, 2, 70, 0, {}, None),
    "d64_no_mfma": (64, 256, 256, 2, 20, 1, {"knn_no_mfma": 1}, None),
}


@pytest.mark.parametrize("entry", ["fx3d_knn", "fx3d_knn_ws"])
@pytest.mark.parametrize("case", list(KNN_CASES))
def test_knn(gpu_fx, oracle, fx_option, case, entry):
    """x, y, idx and dist misaligned independently.  The pre-pass shapes are eligible for the F16Pre kernel when aligned; an
    offset x or y sends them to the F16 kernel (y aligned) or the F32-filter kernel (y not), an offset idx or dist to the
    scalar stores of the lists (k % 4 == 0)."""
    fx = gpu_fx
    D, N, M, B, k, drop, opts, wants_ws = KNN_CASES[case]
    for o, v in opts.items():
        fx_option(o, v)
    x = _randn((D, N, B), 100 * D + k)
    y = x.copy(order="F") if drop else _randn((D, M, B), 100 * D + k + 1)
    oi, od = oracle.knn(x, k, y=y, drop_first=bool(drop))
    arrs = [I("x", x), I("y", y), O("idx", (k, N, B), np.int32), O("dist", (k, N, B))]
    if entry == "fx3d_knn":
        r = hold(fx, lambda p, ws, nb: _abi(fx, entry)(p.x, N, p.y, M, B, D, k, drop, p.idx, p.dist, None), arrs)
    else:
        nb = _ws(fx, "fx3d_knn_workspace_bytes", N, M, B, D, k, drop)
        assert nb > 0 or not wants_ws, (case, nb)
        r = hold(fx, lambda p, ws, n: _abi(fx, entry)(p.x, N, p.y, M, B, D, k, drop, p.idx, p.dist, ws if n else None, n, None), arrs, nb)
    assert np.array_equal(r["idx"], oi), np.argwhere(r["idx"] != oi)[:5]
    assert np.array_equal(r["dist"], od)


# ------------------------------------------------------------------ knn_gather, edge_features, edge_features_grad, edgeconv_graph
@pytest.mark.parametrize("K", [4, 5])
@pytest.mark.parametrize("F", [3, 4, 64])
def test_graph_features(gpu_fx, oracle, fx_option, F, K):
    """N = 64, B = 2.  The layout-1 mlp4 kernel needs F % 4 == 0, (K N) % 4 == 0 and x, out, idx all aligned: F = 3 never takes
    it, F = 4 / 64 leave it for the one-position kernels as soon as one pointer moves.  (K N) % 4 is 0 for both K at N = 64, so
    K = 5 also runs at N = 63, where it is not and the second cloud of every array sits 12 bytes off whatever the base."""
    fx = gpu_fx
    for N in (64, 63) if K == 5 else (64,):
        B = 2
        x = _randn((F, N, B), 7 * F + K + N)
        idx = oracle.knn(x, K, drop_first=True, want_dist=False)
        arrs = [I("x", x), I("idx", idx), O("out", (F, K, N, B))]
        r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_knn_gather")(p.x, N, B, F, K, p.idx, p.out, None), arrs)
        assert _bits_equal(r["out"], oracle.knn_gather(x, idx))
        for layout in (0, 1):
            oshape = (2 * F, K, N, B) if layout == 0 else (K * N, 2 * F, B)
            arrs = [I("x", x), I("idx", idx), O("out", oshape)]
            r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_edge_features")(p.x, N, B, F, K, p.idx, layout, p.out, None), arrs)
            want = oracle.edge_features(x, idx, layout)
            assert _bits_equal(r["out"], want)
            g = _randn(oshape, 31 * F + K + layout)
            arrs = [I("gout", g), O("gx", (F, N, B))]
            r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_edge_features_bwd")(p.gout, N, B, F, K, layout, p.gx, None), arrs)
            assert _bits_equal(r["gx"], oracle.edge_features_bwd(g, F, N, B, K, layout))
            for unfused in (0, 1):
                fx_option("edgeconv_unfused", unfused)
                arrs = [I("x", x), O("idx", (K, N, B), np.int32), O("out", oshape)]
                r = hold(fx, lambda p, ws, nb: _abi(fx, "fx3d_edgeconv_graph")(p.x, N, B, F, K, layout, p.idx, p.out, None), arrs)
                assert np.array_equal(r["idx"], idx) and _bits_equal(r["out"], want), (layout, unfused)


# ----------------------------------------------------------------------------------------------------------------- transforms
def _vec(*v):
    return (C.c_float * len(v))(*[float(t) for t in v])


def _hold_map(fx, call, x, extra=(), ws_bytes=0, outs=()):
    """One transform out of place (x and y placed independently) and in place (y == x): both give the same bits."""
    arrs = [I("x", x)] + list(extra) + [O("y", x.shape)] + list(outs)
    r = hold(fx, lambda p, ws, nb: call(p, p.x, p.y, ws, nb), arrs, ws_bytes)
    arrs = list(extra) + [O("y", x.shape, init=x)] + list(outs)
    r2 = hold(fx, lambda p, ws, nb: call(p, p.y, p.y, ws, nb), arrs, ws_bytes)
    for k in r:
        assert _bits_equal(r[k], r2[k]), ("in place", k)
    return r


@pytest.mark.parametrize("n", [1024, 1025, 1026, 1027])
@pytest.mark.parametrize("D", [3, 4])
def test_transforms_dense(gpu_fx, D, n):
    """scale, translate, rotate (one matrix, one per cloud), both normalize forms, realign and segment_minmax through the C ABI on
    a (D, n, 2) cloud: map_range's "aligned middle" is taken from the element index, affine_kernel and rotate_kernel read and
    write 16 bytes at x + 4 q / x + 12 q whatever the address -- an odd n shifts the second cloud, the placement the first."""
    fx = gpu_fx
    B = 2
    x = _randn((D, n, B), 1000 * D + n) + np.float32(3.0)
    tot = D * n * B
    r = _hold_map(fx, lambda p, xi, yo, ws, nb: _abi(fx, "fx3d_scale_translate")(xi, tot, 0, _vec(1.7), yo, None), x)
    assert tref.same_bits(r["y"], tref.pcloud_scale(x, 1.7))
    if D == 3:
        t = (1.0, -2.0, 1e4)
        r = _hold_map(fx, lambda p, xi, yo, ws, nb: _abi(fx, "fx3d_scale_translate")(xi, tot, 1, _vec(*t), yo, None), x)
        assert tref.same_bits(r["y"].reshape(3, n * B, order="F"), tref.mesh_translate(x.reshape(3, n * B, order="F"), t))
        R, Rb = _randn((3, 3), 5), _randn((3, 3, B), 6)
        Rh = _vec(*R.reshape(-1, order="F"))
        r = _hold_map(fx, lambda p, xi, yo, ws, nb: _abi(fx, "fx3d_rotate")(xi, n * B, n, B, None, Rh, None, yo, None), x)
        assert tref.same_bits(r["y"], tref.pcloud_rotate(x, R))
        r = _hold_map(fx, lambda p, xi, yo, ws, nb: _abi(fx, "fx3d_rotate")(xi, n * B, n, B, None, None, p.R, yo, None), x, extra=[I("R", Rb)])
        assert tref.same_bits(r["y"], tref.pcloud_rotate(x, Rb))
    nb = _ws(fx, "fx3d_transform_workspace_bytes", D, n, B)
    wc, wsd = tref.pcloud_stats(x)
    for mode in (0, 1):
        r = _hold_map(fx, lambda p, xi, yo, ws, n_: _abi(fx, "fx3d_normalize")(xi, D, n, B, None, mode, yo, p.c, p.s, ws if n_ else None, n_, None),
                      x, ws_bytes=nb, outs=[O("c", (D, B)), O("s", (D, B))])
        assert tref.within_ulp(r["c"], wc) and tref.within_ulp(r["s"], wsd)
        if mode == 0:
            want = tref.pcloud_normalize(x, r["c"], r["s"])
        else:
            want = tref.mesh_normalize(x.reshape(D, n * B, order="F"), [n] * B, r["c"], r["s"]).reshape(D, n, B, order="F")
        assert tref.same_bits(r["y"], want), mode
    arrs = [I("x", x), O("mn", (D, B)), O("mx", (D, B))]
    r = hold(fx, lambda p, ws, n_: _abi(fx, "fx3d_segment_minmax")(p.x, D, n, B, None, 0, p.mn, p.mx, ws if n_ else None, n_, None), arrs, nb)
    smin, smax = tref.jmin(x, 1)[:, 0, :], tref.jmax(x, 1)[:, 0, :]
    assert tref.same_bits(r["mn"], smin) and tref.same_bits(r["mx"], smax)
    tmin, tmax = np.full((D, 1), -2.0, np.float32), np.linspace(1, 3, D, dtype=np.float32).reshape(D, 1)
    extra = [I("smin", smin), I("smax", smax), I("tmin", tmin), I("tmax", tmax)]
    r = _hold_map(fx, lambda p, xi, yo, ws, n_: _abi(fx, "fx3d_realign")(xi, D, n, B, None, p.smin, p.smax, p.tmin, p.tmax, yo, None), x, extra=extra)
    assert tref.same_bits(r["y"], tref.pcloud_realign(x, tmin, tmax))


def _teapot_sphere(fx):
    return fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj"))


def test_transforms_ragged_mesh_batch_as_a_slab_of_a_longer_packed_array(gpu_fx):
    """The teapot + sphere batch as columns [off, off + sum V) of a longer packed (3, *) array, off = 1, 2, 3 columns (12, 24, 36
    bytes: 12, 8 and 4 past a 16-byte boundary) -- what `v.ptr + 12 * off` and DeviceArray.slab hand to the kernels -- through
    the package's own in-place transforms."""
    fx = gpu_fx
    m = _teapot_sphere(fx)
    v = np.asfortranarray(m.get_verts_packed_host())
    lens = [int(t) for t in m._verts_len]
    V = v.shape[1]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Vmax = max(lens)
    Bm = len(lens)
    nb = _ws(fx, "fx3d_transform_workspace_bytes", 3, Vmax, Bm)
    R, Rb = _randn((3, 3), 8), _randn((3, 3, Bm), 9)
    Rh = _vec(*R.reshape(-1, order="F"))
    tmin, tmax = np.array([[-1.0], [0.0], [2.0]], np.float32), np.array([[1.0], [3.0], [2.5]], np.float32)
    smin, smax = tref.mesh_bounds_padded(v, lens)
    wc, wsd = tref.mesh_stats(v, lens)
    abi = lambda name: _abi(fx, name)  # noqa: E731
    ops = {
        "scale": (lambda p, xi, yo, ws, n: abi("fx3d_scale_translate")(xi, 3 * V, 0, _vec(0.25), yo, None), tref.mesh_scale(v, 0.25)),
        "translate": (lambda p, xi, yo, ws, n: abi("fx3d_scale_translate")(xi, 3 * V, 1, _vec(1.0, -2.0, 1e4), yo, None),
                      tref.mesh_translate(v, [1.0, -2.0, 1e4])),
        "rotate": (lambda p, xi, yo, ws, n: abi("fx3d_rotate")(xi, V, Vmax, Bm, p.seg, Rh, None, yo, None), tref.mesh_rotate(v, lens, R)),
        "rotate_b": (lambda p, xi, yo, ws, n: abi("fx3d_rotate")(xi, V, Vmax, Bm, p.seg, None, p.R, yo, None), tref.mesh_rotate(v, lens, Rb)),
        "realign": (lambda p, xi, yo, ws, n: abi("fx3d_realign")(xi, 3, Vmax, Bm, p.seg, p.smin, p.smax, p.tmin, p.tmax, yo, None),
                    tref.mesh_realign(v, lens, tmin, tmax)),
    }
    long = np.asfortranarray(np.concatenate([np.full((3, 4), np.nan, np.float32), v, np.full((3, 4), np.nan, np.float32)], axis=1))
    for off in (1, 2, 3):
        host = np.roll(long, off - 4, axis=1)   # v at columns [off, off + V)
        assert _bits_equal(np.ascontiguousarray(host[:, off:off + V]), np.ascontiguousarray(v))
        for name, (call, want) in ops.items():
            buf = fx.gpu(host)
            view = fx.DeviceArray(buf.ptr + 12 * off, (3, V), np.float32, owned=False, keep=buf)
            assert view.ptr % 16 == (12 * off) % 16
            aux = SimpleNamespace(seg=fx.gpu(seg), R=fx.gpu(Rb), smin=fx.gpu(smin), smax=fx.gpu(smax), tmin=fx.gpu(tmin), tmax=fx.gpu(tmax))
            call(SimpleNamespace(**{k: a.ptr for k, a in vars(aux).items()}), view.ptr, view.ptr, None, 0)
            fx.synchronize()
            got = buf.to_host()
            assert tref.same_bits(got[:, off:off + V], want), (name, off)
            rest = np.ones(host.shape[1], bool)
            rest[off:off + V] = False
            assert np.all(np.isnan(got[:, rest])), (name, off, "columns around the slab were written")
        for mode in (1, 0):
            buf = fx.gpu(host)
            c, s, segd = fx.DeviceArray.empty((3, Bm)), fx.DeviceArray.empty((3, Bm)), fx.gpu(seg)
            ws = fx.DeviceArray.zeros((max(nb, 256),), np.uint8)
            abi("fx3d_normalize")(buf.ptr + 12 * off, 3, Vmax, Bm, segd.ptr, mode, buf.ptr + 12 * off, c.ptr, s.ptr, ws.ptr if nb else None, nb, None)
            mn, mx = fx.DeviceArray.empty((3, Bm)), fx.DeviceArray.empty((3, Bm))
            buf2 = fx.gpu(host)
            abi("fx3d_segment_minmax")(buf2.ptr + 12 * off, 3, Vmax, Bm, segd.ptr, 1, mn.ptr, mx.ptr, ws.ptr if nb else None, nb, None)
            fx.synchronize()
            ch, sh = c.to_host(), s.to_host()
            assert tref.within_ulp(ch, wc) and tref.within_ulp(sh, wsd), (off, mode)
            if mode == 1:
                want = tref.mesh_normalize(v, lens, ch, sh)
            else:
                want = np.concatenate([tref.pcloud_normalize(v[:, a:b][:, :, None], ch[:, i:i + 1], sh[:, i:i + 1])[:, :, 0]
                                       for i, (a, b) in enumerate(zip(seg[:-1], seg[1:]))], axis=1)
            assert tref.same_bits(buf.to_host()[:, off:off + V], want), (off, mode)
            assert tref.same_bits(mn.to_host(), smin) and tref.same_bits(mx.to_host(), smax), off


# ---------------------------------------------------------------------------------------------------------------- conversions
@pytest.mark.parametrize("res", [8, 32])
def test_pointcloud_to_voxel(gpu_fx, oracle, res):
    fx = gpu_fx
    N, B = 1024, 2
    x = _rand((3, N, B), 77 + res)
    nb = _ws(fx, "fx3d_voxel_workspace_bytes", B)
    arrs = [I("x", x), O("vox", (res, res, res, B))]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointcloud_to_voxel")(p.x, N, B, res, p.vox, ws, n, None), arrs, nb)
    assert _bits_equal(r["vox"], oracle.pointcloud_to_voxel(x, res))


def _mesh(fx):
    """The teapot + sphere batch in every form the mesh entry points take (host arrays; int32 0-based indices)."""
    if not hasattr(_mesh, "d"):
        m = _teapot_sphere(fx)
        d = SimpleNamespace(m=m, B=m.N, Vmax=m.V, Fmax=m.F)
        d.v = np.asfortranarray(m.get_verts_packed_host())
        d.f = np.asfortranarray((m.get_faces_packed().astype(np.int64) - 1).astype(np.int32))
        d.vp = np.asfortranarray(m.get_verts_padded_host())
        d.fp = np.asfortranarray(np.maximum(m.get_faces_padded().astype(np.int64) - 1, 0).astype(np.int32))
        d.flen, d.vlen = np.asarray(m._faces_len, np.int32), np.asarray(m._verts_len, np.int32)
        d.V, d.F = d.v.shape[1], d.f.shape[1]
        d.e = np.asfortranarray((m.get_edges_packed().astype(np.int64) - 1).astype(np.int32))
        d.E = d.e.shape[0]
        d.rowptr, d.colind, d.vals = [np.ascontiguousarray(a) for a in m.get_laplacian_packed()]
        _mesh.d = d
    return _mesh.d


@pytest.mark.parametrize("res", [8, 28])
def test_trimesh_to_voxel(gpu_fx, res):
    import trimesh_voxel_ref
    fx, d = gpu_fx, _mesh(gpu_fx)
    nb = _ws(fx, "fx3d_trimesh_voxel_workspace_bytes", d.Vmax, d.Fmax, d.B, res)
    arrs = [I("verts", d.vp), I("vlen", d.vlen), I("faces", d.fp), I("flen", d.flen), O("vox", (res, res, res, d.B)),
            O("bad", (1,), np.uint32)]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_trimesh_to_voxel")(p.verts, d.Vmax, p.vlen, p.faces, d.Fmax, p.flen, d.B, res, p.vox, p.bad,
                                                                     ws, n, None), arrs, nb)
    assert r["bad"][0] == 0
    assert _bits_equal(r["vox"], trimesh_voxel_ref.trimesh_to_voxel(d.m.get_verts_list(), d.m.get_faces_list(), res))


@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_voxel_to_trimesh_exact(gpu_fx, extra):
    """fx3d_voxel_mesh_count + _emit with the caller's verts and faces outputs: vm_emit_kernel stores a cube's 24 floats as six
    float4 at verts + 24 s0 and, when Fmax % 4 == 0 (extra = 0), its 36 face ids as nine int4 -- at whatever address."""
    import voxel_mesh_ref
    fx = gpu_fx
    res, B = 8, 2
    rng = np.random.default_rng(70 + extra)
    vox = np.asfortranarray((rng.random((res, res, res, B)) < 0.4).astype(np.float32))
    ev, ef = voxel_mesh_ref.voxel_to_trimesh(vox, np.float32(0.5))
    K = np.array([f.shape[1] // 12 for f in ef])
    Fmax = 12 * int(K.max()) + extra
    nb = _ws(fx, "fx3d_voxel_mesh_workspace_bytes", res, B)
    arrs = [I("vox", vox), O("cubes", (B,), np.int64), O("bad", (B,), np.uint32), O("verts", (3, 8 * int(K.sum()))), O("faces", (3, Fmax, B), np.int32)]

    def call(p, ws, n):
        _abi(fx, "fx3d_voxel_mesh_count")(p.vox, res, B, 0.5, p.cubes, p.bad, ws, n, None)
        _abi(fx, "fx3d_voxel_mesh_emit")(res, B, int(K.sum()), p.verts, p.faces, Fmax, ws, n, None)
    r = hold(fx, call, arrs, nb)
    assert np.array_equal(r["cubes"], K) and not r["bad"].any()
    assert _bits_equal(r["verts"], np.asfortranarray(np.concatenate(ev, axis=1)))
    for i in range(B):
        assert np.array_equal(r["faces"][:, :12 * K[i], i], ef[i].astype(np.int64) - 1) and not r["faces"][:, 12 * K[i]:, i].any()


# ------------------------------------------------------------------------------------------------------------------ mesh path
@pytest.mark.parametrize("index_type", ["int32", "uint32", "int64", "upload_uint32", "upload_int64"])
def test_mesh_faces_through_index_convert_and_upload(gpu_fx, index_type):
    """The reference's 1-based UInt32 / Int64 face arrays to the library's int32 0-based form on the device, source and
    destination offset (fx3d_index_convert), and from the host through the staging workspace (fx3d_index_upload)."""
    fx, d = gpu_fx, _mesh(gpu_fx)
    dt = np.dtype(index_type.replace("upload_", ""))
    code = {"int32": 0, "uint32": 1, "int64": 2}[dt.name]
    src = np.asfortranarray(d.m.get_faces_padded().astype(dt))
    cnt = src.size
    if index_type.startswith("upload"):
        nb = _ws(fx, "fx3d_index_upload_workspace_bytes", code, cnt)
        arrs = [O("dst", src.shape, np.int32), O("bad", (1,), np.uint32)]
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_index_upload")(src.ctypes.data, code, 1, cnt, 1, d.Vmax, p.dst, p.bad, ws, n, None), arrs, nb)
    else:
        arrs = [I("src", src), O("dst", src.shape, np.int32), O("bad", (1,), np.uint32)]
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_index_convert")(p.src, code, 1, cnt, 1, d.Vmax, p.dst, p.bad, None), arrs)
    assert r["bad"][0] == 0 and np.array_equal(r["dst"], d.fp)


def test_mesh_face_areas(gpu_fx, oracle):
    fx, d = gpu_fx, _mesh(gpu_fx)
    arrs = [I("verts", d.v), I("faces", d.f), O("areas", (d.F,))]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_faces_areas_packed")(p.verts, d.V, p.faces, d.F, p.areas, None), arrs)
    assert _bits_equal(r["areas"], oracle.faces_areas_packed(d.v, d.f))
    arrs = [I("verts", d.vp), I("faces", d.fp), I("flen", d.flen), O("areas", (1, d.Fmax, d.B))]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_faces_areas_padded")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, p.areas, None), arrs)
    assert _bits_equal(r["areas"], oracle.faces_areas_padded(d.vp, d.fp, d.flen))


def test_mesh_losses_and_adjoints(gpu_fx, oracle):
    """laplacian_loss, edge_loss, the fused pair; their adjoints in the gather forms (bit for bit the oracle) and in the scatter
    forms, whose float atomics add in arrival order: no placement of those is bit-equal to another RUN of itself, so each is
    held to the family's bound against the oracle (test_gpu_parity / test_gpu_hardening: rtol 1e-4, atol 1e-9)."""
    fx, d = gpu_fx, _mesh(gpu_fx)
    r64, c64, e64 = d.rowptr.astype(np.int64), d.colind.astype(np.int64), d.e.astype(np.int64)
    target, gout = 0.05, 0.7
    ol, oe = oracle.laplacian_loss(d.v, r64, c64, d.vals), oracle.edge_loss(d.v, e64, target)
    glap, gedge = oracle.laplacian_loss_bwd(d.v, r64, c64, d.vals, gout), oracle.edge_loss_bwd(d.v, e64, target, gout)
    csr = [I("rowptr", d.rowptr), I("colind", d.colind), I("vals", d.vals)]
    nb = _ws(fx, "fx3d_mesh_loss_workspace_bytes", max(d.E, d.V))
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_laplacian_loss")(p.verts, d.V, p.rowptr, p.colind, p.vals, p.loss, None, ws, n, None),
             [I("verts", d.v)] + csr + [O("loss", (1,))], nb)
    assert np.isclose(r["loss"][0], ol, rtol=LOSS_RTOL, atol=0)
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edge_loss")(p.verts, d.V, p.edges, d.E, target, p.loss, None, ws, n, None),
             [I("verts", d.v), I("edges", d.e), O("loss", (1,))], nb)
    assert np.isclose(r["loss"][0], oe, rtol=LOSS_RTOL, atol=0)
    # gather forms
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_laplacian_loss_bwd_sym")(p.verts, d.V, p.rowptr, p.colind, p.vals, gout, p.g, 0, p.missing, None),
             [I("verts", d.v)] + csr + [O("g", (3, d.V)), O("missing", (1,), np.uint32)])
    assert _bits_equal(r["g"], glap) and r["missing"][0] == 0
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edge_loss_bwd_adj")(p.verts, d.V, p.rowptr, p.colind, d.E, target, gout, p.g, 0, None),
             [I("verts", d.v), I("rowptr", d.rowptr), I("colind", d.colind), O("g", (3, d.V))])
    assert _bits_equal(r["g"], gedge)
    # scatter forms (float atomics)
    close = lambda want: (lambda res: np.testing.assert_allclose(res["g"], want, rtol=1e-4, atol=1e-9))  # noqa: E731
    hold(fx, lambda p, ws, n: _abi(fx, "fx3d_laplacian_loss_bwd")(p.verts, d.V, p.rowptr, p.colind, p.vals, gout, p.g, 0, None),
         [I("verts", d.v)] + csr + [O("g", (3, d.V))], check=close(glap))
    hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edge_loss_bwd")(p.verts, d.V, p.edges, d.E, target, gout, p.g, 0, None),
         [I("verts", d.v), I("edges", d.e), O("g", (3, d.V))], check=close(gedge))
    # both losses in one launch, both adjoints in one gather launch, on top of a base gradient
    nb2 = _ws(fx, "fx3d_mesh_losses_workspace_bytes", d.V, d.E)
    base = _randn((3, d.V), 3)
    arrs = [I("verts", d.v)] + csr + [I("edges", d.e), O("lap", (1,)), O("edge", (1,)), O("total", (1,)), O("g", (3, d.V), init=base)]

    def call(p, ws, n):
        _abi(fx, "fx3d_mesh_losses")(p.verts, d.V, p.rowptr, p.colind, p.vals, p.edges, d.E, target, 0.1, 1.0, None, p.lap, p.edge, p.total, ws, n, None)
        _abi(fx, "fx3d_mesh_losses_bwd")(p.verts, d.V, p.rowptr, p.colind, p.vals, d.E, target, 0.1 * gout, gout, 1, p.g, 1, ws, n, None)
    r = hold(fx, call, arrs, nb2)
    assert np.isclose(r["lap"][0], ol, rtol=LOSS_RTOL, atol=0) and np.isclose(r["edge"][0], oe, rtol=LOSS_RTOL, atol=0)
    assert r["total"][0] == np.float32(np.float32(np.float32(0.1) * r["lap"][0]) + r["edge"][0])
    gl2 = oracle.laplacian_loss_bwd(d.v, r64, c64, d.vals, 0.1 * gout)
    assert _bits_equal(r["g"], ((base + gl2).astype(np.float32) + gedge).astype(np.float32))


def test_mesh_sampling_and_ordered_adjoint(gpu_fx, oracle):
    from test_gpu_topology import host_vertex_faces
    fx, d = gpu_fx, _mesh(gpu_fx)
    n, seed = 500, 11
    out, fi, r1, r2 = oracle.sample_points_seeded(d.vp, d.fp, d.flen, n, seed, return_draws=True)
    nb = _ws(fx, "fx3d_sample_points_workspace_bytes", d.Fmax, d.B)
    mesh = [I("verts", d.vp), I("faces", d.fp), I("flen", d.flen)]
    arrs = mesh + [O("out", (3, n, d.B)), O("fi", (n, d.B), np.int32), O("r1", (n, d.B)), O("r2", (n, d.B))]
    r = hold(fx, lambda p, ws, nn: _abi(fx, "fx3d_sample_points")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, n, 1e-6, seed, p.out, p.fi, p.r1,
                                                                   p.r2, ws, nn, None), arrs, nb)
    assert _bits_equal(r["out"], out) and np.array_equal(r["fi"], fi) and _bits_equal(r["r1"], r1) and _bits_equal(r["r2"], r2)
    arrs = [I("verts", d.vp), I("faces", d.fp), I("fi", fi), I("r1", r1), I("r2", r2), O("out", (3, n, d.B))]
    r = hold(fx, lambda p, ws, nn: _abi(fx, "fx3d_sample_points_explicit")(p.verts, d.Vmax, p.faces, d.Fmax, d.B, n, p.fi, p.r1, p.r2, p.out, None), arrs)
    assert _bits_equal(r["out"], oracle.sample_points_explicit(d.vp, d.fp, fi, r1, r2))
    ordered = C.c_int32(0)
    fx._lib.call("fx3d_sample_points_bwd_ordered", d.Fmax, n, C.byref(ordered))
    assert ordered.value == 1
    vfr, vfe = host_vertex_faces(fx._lib, d.fp, d.flen, d.Vmax)
    g, base = _randn((3, n, d.B), 4), _randn((3, d.Vmax, d.B), 5)
    for acc in (0, 1):
        arrs = [I("faces", d.fp), I("fi", fi), I("r1", r1), I("r2", r2), I("gout", g), I("vfr", vfr), I("vfe", vfe),
                O("gverts", (3, d.Vmax, d.B), init=base)]
        r = hold(fx, lambda p, ws, nn: _abi(fx, "fx3d_sample_points_bwd")(p.faces, d.Vmax, d.Fmax, d.B, n, p.fi, p.r1, p.r2, p.gout, p.gverts, acc,
                                                                           p.vfr, p.vfe, None), arrs)
        assert _bits_equal(r["gverts"], oracle.sample_points_bwd(d.fp, d.flen, d.Vmax, fi, r1, r2, g, base=base if acc else None))


def test_mesh_normals_and_adjoints(gpu_fx):
    import normals_ref
    from test_gpu_topology import host_vertex_faces
    fx, d = gpu_fx, _mesh(gpu_fx)
    f64 = np.asfortranarray(d.f.astype(np.int64))
    vfr, vfe = host_vertex_faces(fx._lib, d.f.reshape(3, d.F, 1, order="F"), [d.F], d.V)
    vfr, vfe = np.ascontiguousarray(vfr[:, 0]), np.ascontiguousarray(vfe[:, 0])
    mesh = [I("verts", d.v), I("faces", d.f), I("vfr", vfr), I("vfe", vfe)]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_verts_normals_packed")(p.verts, d.V, p.faces, d.F, p.vfr, p.vfe, p.normals, p.mask, None),
             mesh + [O("normals", (3, d.V)), O("mask", (3 * d.F,), np.uint8)])
    assert tref.same_bits(r["normals"], normals_ref.verts_normals(d.v, f64))
    mask = r["mask"]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_faces_normals_packed")(p.verts, d.V, p.faces, d.F, p.normals, None),
             [I("verts", d.v), I("faces", d.f), O("normals", (3, d.F))])
    assert tref.same_bits(r["normals"], normals_ref.faces_normals(d.v, f64))
    nb = _ws(fx, "fx3d_normals_workspace_bytes", d.V, d.F)
    base = _randn((3, d.V), 6)
    gv, gf = _randn((3, d.V), 7), _randn((3, d.F), 8)
    for acc in (0, 1):
        arrs = mesh + [I("mask", mask), I("gout", gv), O("g", (3, d.V), init=base)]
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_verts_normals_bwd")(p.verts, d.V, p.faces, d.F, p.vfr, p.vfe, p.mask, p.gout, p.g, acc, ws, n, None),
                 arrs, nb)
        assert tref.same_bits(r["g"], normals_ref.verts_normals_bwd(d.v, f64, gv, base=base if acc else None))
        arrs = mesh + [I("gout", gf), O("g", (3, d.V), init=base)]
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_faces_normals_bwd")(p.verts, d.V, p.faces, d.F, p.vfr, p.vfe, p.gout, p.g, acc, ws, n, None),
                 arrs, nb)
        assert tref.same_bits(r["g"], normals_ref.faces_normals_bwd(d.v, f64, gf, base=base if acc else None))


def test_mesh_topology_tables(gpu_fx):
    """csrc/topology_dev.hip against the host builders of csrc/topology.cpp, as tests/test_gpu_topology.py holds them."""
    from test_gpu_topology import host_edges, host_laplacian, host_vertex_faces
    fx, d = gpu_fx, _mesh(gpu_fx)
    he, hf2e = host_edges(fx._lib, d.f, d.V)
    assert np.array_equal(he, d.e)
    nb = _ws(fx, "fx3d_edges_dev_workspace_bytes", d.F, d.V)
    arrs = [I("faces", d.f), O("cnt", (1,), np.int64), O("bad", (1,), np.uint32), O("edges", (d.E, 2), np.int32), O("f2e", (d.F, 3), np.int32)]

    def edges(p, ws, n):
        _abi(fx, "fx3d_edges_dev_count")(p.faces, d.F, d.V, p.cnt, p.bad, ws, n, None)
        _abi(fx, "fx3d_edges_dev_emit")(p.faces, d.F, d.V, d.E, p.edges, p.f2e, ws, n, None)
    r = hold(fx, edges, arrs, nb)
    assert r["cnt"][0] == d.E and r["bad"][0] == 0 and np.array_equal(r["edges"], he) and np.array_equal(r["f2e"], hf2e)
    hr, hc, hv = host_laplacian(fx._lib, he, d.V)
    cap = 2 * d.E + d.V
    nb = _ws(fx, "fx3d_laplacian_dev_workspace_bytes", d.E, d.V)
    arrs = [I("edges", he), O("rowptr", (d.V + 1,), np.int32), O("colind", (cap,), np.int32), O("vals", (cap,)), O("nnz", (1,), np.int64),
            O("bad", (1,), np.uint32)]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_laplacian_dev_csr")(p.edges, d.E, d.V, p.rowptr, p.colind, p.vals, p.nnz, p.bad, ws, n, None), arrs, nb)
    nnz = int(r["nnz"][0])
    assert nnz == len(hc) and r["bad"][0] == 0 and np.array_equal(r["rowptr"], hr) and np.array_equal(r["colind"][:nnz], hc)
    assert _bits_equal(r["vals"][:nnz], hv)
    hvr, hve = host_vertex_faces(fx._lib, d.fp, d.flen, d.Vmax)
    nb = _ws(fx, "fx3d_vertex_faces_dev_workspace_bytes", d.Vmax, d.Fmax, d.B)
    arrs = [I("faces", d.fp), I("flen", d.flen), O("vfr", (d.Vmax + 1, d.B), np.int32), O("vfe", (3 * d.Fmax, d.B), np.int32), O("bad", (1,), np.uint32)]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_vertex_faces_dev")(p.faces, p.flen, d.Vmax, d.Fmax, d.B, p.vfr, p.vfe, p.bad, ws, n, None), arrs, nb)
    assert r["bad"][0] == 0 and np.array_equal(r["vfr"], hvr) and np.array_equal(r["vfe"], hve)
    nb = _ws(fx, "fx3d_faces_padded_to_packed_dev_workspace_bytes", d.B)
    arrs = [I("faces", d.fp), I("flen", d.flen), I("nverts", d.vlen), O("packed", (3, d.F), np.int32)]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_faces_padded_to_packed_dev")(p.faces, p.flen, p.nverts, d.Fmax, d.B, d.F, p.packed, ws, n, None),
             arrs, nb)
    assert np.array_equal(r["packed"], d.f)


# --------------------------------------------------------------------------------------------------------------------- models
def _flat_same(got, want, what):
    assert tref.same_bits(np.asarray(got).ravel(order="F"), np.asarray(want, np.float32).ravel(order="F")), what


def _pointnet_case(fx):
    if not hasattr(_pointnet_case, "c"):
        import pointnet_ref
        N, B, nc = 64, 2, 10
        P = pointnet_ref.random_params(nc, seed=10)
        m = fx.PointNet(nc).load(P)
        c = SimpleNamespace(N=N, B=B, nc=nc, P=P, params=m.flat_params(), X=_randn((3, N, B), 564), glogits=_randn((nc, B), 664),
                            dropout=np.asfortranarray(m.dropout_mask(B, 3), dtype=np.float32))
        n = C.c_int64(0)
        fx._lib.call("fx3d_pointnet_stat_count", C.byref(n))
        c.nstat = n.value
        _pointnet_case.c = c
    return _pointnet_case.c


@pytest.mark.parametrize("entry", ["forward", "forward_train", "grad", "grad_train"])
def test_pointnet(gpu_fx, entry):
    """PointNet at 2 x 64: X, params_dev, glogits, the dropout multipliers, the batch statistics and every output offset."""
    import pointnet_grad_ref
    import pointnet_grad_train_ref
    import pointnet_ref
    import pointnet_train_ref
    fx, c = gpu_fx, _pointnet_case(gpu_fx)
    N, B, nc = c.N, c.B, c.nc
    fwd_outs = [O("probs", (nc, B)), O("logits", (nc, B)), O("stn", (3, 3, B)), O("fstn", (64, 64, B)), O("pooled", (1024, B))]
    grad_outs = [O("gparams", (c.params.size,)), O("gx", (3, N, B)), O("gstn", (3, 3, B)), O("gfstn", (64, 64, B)), O("gh", (64, N, B)),
                 O("gxt", (3, N, B))]
    if entry == "forward":
        nb = _ws(fx, "fx3d_pointnet_workspace_bytes", N, B, nc)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointnet_forward")(p.params, nc, p.x, N, B, p.probs, p.logits, p.stn, p.fstn, p.pooled, ws, n, None),
                 [I("params", c.params), I("x", c.X)] + fwd_outs, nb)
        want = pointnet_ref.forward(c.X, c.P)
    elif entry == "forward_train":
        nb = _ws(fx, "fx3d_pointnet_train_workspace_bytes", N, B, nc)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointnet_forward_train")(p.params, nc, p.x, N, B, p.dropout, 0.1, p.probs, p.logits, p.stn, p.fstn,
                                                                              p.pooled, p.stats, p.running, ws, n, None),
                 [I("params", c.params), I("x", c.X), I("dropout", c.dropout)] + fwd_outs + [O("stats", (c.nstat,)), O("running", (c.nstat,))], nb)
        want = pointnet_train_ref.forward_train(c.X, c.P, c.dropout, 0.1)
        _flat_same(r["stats"], pointnet_train_ref.flat_stats(want["batch_stats"]), "batch_stats")
        _flat_same(r["running"], pointnet_train_ref.flat_stats(want["running"]), "running")
    if entry.startswith("forward"):
        for k in ("logits", "stn", "fstn", "pooled"):
            _flat_same(r[k], want[k], k)
        return
    if entry == "grad":
        nb = _ws(fx, "fx3d_pointnet_grad_workspace_bytes", N, B, nc)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointnet_grad")(p.params, nc, p.x, N, B, p.glogits, p.gparams, p.gx, p.gstn, p.gfstn, p.gh, p.gxt,
                                                                     ws, n, None),
                 [I("params", c.params), I("x", c.X), I("glogits", c.glogits)] + grad_outs, nb)
        grads, gx, mid = pointnet_grad_ref.grad(c.X, c.P, c.glogits)
        flat = pointnet_grad_ref.flat(grads)
    else:
        stats = pointnet_train_ref.flat_stats(pointnet_train_ref.forward_train(c.X, c.P, c.dropout, 0.1)["batch_stats"])
        nb = _ws(fx, "fx3d_pointnet_grad_train_workspace_bytes", N, B, nc)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointnet_grad_train")(p.params, nc, p.x, N, B, p.dropout, p.stats, p.glogits, p.gparams, p.gx,
                                                                           p.gstn, p.gfstn, p.gh, p.gxt, ws, n, None),
                 [I("params", c.params), I("x", c.X), I("dropout", c.dropout), I("stats", stats), I("glogits", c.glogits)] + grad_outs, nb)
        grads, gx, mid = pointnet_grad_train_ref.grad_train(c.X, c.P, c.glogits, c.dropout)
        flat = pointnet_grad_ref.flat(grads)
    _flat_same(r["gparams"], flat, "gparams")
    _flat_same(r["gx"], gx, "gx")
    for k in ("gstn", "gfstn", "gh", "gxt"):
        _flat_same(r[k], mid[k], k)


EDGECONV_LAYERS = {"3_32_64_64": [3, 32, 64, 64], "64_128_256": [64, 128, 256]}


def _edgeconv_case(fx, name):
    cache = _edgeconv_case.__dict__.setdefault("c", {})
    if name not in cache:
        import dgcnn_train_ref
        import edgeconv_ref
        layers, K, N, B = EDGECONV_LAYERS[name], 4, 64, 2
        P = edgeconv_ref.random_params(layers, 5)
        c = SimpleNamespace(layers=layers, K=K, N=N, B=B, P=P, params=fx.EdgeConv(layers, K).load(P).flat_params(),
                            X=_randn((layers[0], N, B), 77 + layers[0]), gout=_randn((layers[-1], N, B), 78 + layers[0]))
        c.lc = (C.c_int32 * len(layers))(*layers)
        c.idx, c.out = edgeconv_ref.forward(c.X, P, layers, K)
        c.train = dgcnn_train_ref.edgeconv_forward_train(c.X, P, layers, K, idx=c.idx, momentum=0.1)
        c.order = [f"bn{i}" for i in range(1, len(layers))]
        c.stats = dgcnn_train_ref.flat_stats(c.train["batch_stats"], c.order)
        cache[name] = c
    return cache[name]


@pytest.mark.parametrize("entry", ["forward", "forward_idx", "forward_train", "bwd", "grad", "grad_train"])
@pytest.mark.parametrize("name", list(EDGECONV_LAYERS))
def test_edgeconv(gpu_fx, name, entry):
    """EdgeConv [3, 32, 64, 64] and [64, 128, 256] at N = 64, B = 2, K = 4: X, params_dev, a given idx, out, gout, the batch
    statistics and every output offset."""
    import dgcnn_train_ref
    import edgeconv_bwd_ref
    import edgeconv_grad_train_ref
    import edgeconv_pgrad_ref
    fx, c = gpu_fx, _edgeconv_case(gpu_fx, name)
    L, nl, K, N, B = c.lc, len(c.layers), c.K, c.N, c.B
    F, cL, np_ = c.layers[0], c.layers[-1], c.params.size
    if entry in ("forward", "forward_idx"):
        nb = _ws(fx, "fx3d_edgeconv_workspace_bytes", L, nl, K, N, B)
        if entry == "forward":
            r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edgeconv_forward")(p.params, L, nl, K, p.x, N, B, None, p.out, p.idx, ws, n, None),
                     [I("params", c.params), I("x", c.X), O("out", (cL, N, B)), O("idx", (K, N, B), np.int32)], nb)
            assert np.array_equal(r["idx"], c.idx)
        else:
            r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edgeconv_forward")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, None, ws, n, None),
                     [I("params", c.params), I("x", c.X), I("idx", c.idx), O("out", (cL, N, B))], nb)
        _flat_same(r["out"], c.out, "out")
    elif entry == "forward_train":
        ns = C.c_int64(0)
        fx._lib.call("fx3d_edgeconv_stat_count", L, nl, C.byref(ns))
        assert ns.value == c.stats.size
        nb = _ws(fx, "fx3d_edgeconv_train_workspace_bytes", L, nl, K, N, B)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edgeconv_forward_train")(p.params, L, nl, K, p.x, N, B, p.idx, 0.1, p.out, None, p.stats, p.running,
                                                                              ws, n, None),
                 [I("params", c.params), I("x", c.X), I("idx", c.idx), O("out", (cL, N, B)), O("stats", (ns.value,)), O("running", (ns.value,))], nb)
        _flat_same(r["out"], c.train["out"], "out")
        _flat_same(r["stats"], c.stats, "batch_stats")
        _flat_same(r["running"], dgcnn_train_ref.flat_stats(c.train["running"], c.order), "running")
    elif entry == "bwd":
        nb = _ws(fx, "fx3d_edgeconv_bwd_workspace_bytes", L, nl, K, N, B)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edgeconv_bwd")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, p.gout, p.gx, ws, n, None),
                 [I("params", c.params), I("x", c.X), I("idx", c.idx), I("out", c.out), I("gout", c.gout), O("gx", (F, N, B))], nb)
        _flat_same(r["gx"], edgeconv_bwd_ref.input_grad(c.X, c.P, c.layers, K, c.gout, c.idx, c.out), "gx")
    elif entry == "grad":
        nb = _ws(fx, "fx3d_edgeconv_grad_workspace_bytes", L, nl, K, N, B)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edgeconv_grad")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, p.gout, p.gparams, p.gx, ws, n, None),
                 [I("params", c.params), I("x", c.X), I("idx", c.idx), I("out", c.out), I("gout", c.gout), O("gparams", (np_,)), O("gx", (F, N, B))], nb)
        G, gx = edgeconv_pgrad_ref.grad(c.X, c.P, c.layers, K, c.gout, c.idx, c.out)
        _flat_same(r["gparams"], edgeconv_pgrad_ref.flat(G, c.layers), "gparams")
        _flat_same(r["gx"], gx, "gx")
    else:
        out = np.asfortranarray(c.train["out"], dtype=np.float32)
        nb = _ws(fx, "fx3d_edgeconv_grad_train_workspace_bytes", L, nl, K, N, B)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edgeconv_grad_train")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, p.stats, p.gout, p.gparams, p.gx,
                                                                           ws, n, None),
                 [I("params", c.params), I("x", c.X), I("idx", c.idx), I("out", out), I("stats", c.stats), I("gout", c.gout), O("gparams", (np_,)),
                  O("gx", (F, N, B))], nb)
        G, gx = edgeconv_grad_train_ref.grad(c.X, c.P, c.layers, K, c.gout, c.train["batch_stats"], c.idx, out)
        _flat_same(r["gparams"], edgeconv_pgrad_ref.flat(G, c.layers), "gparams")
        _flat_same(r["gx"], gx, "gx")


def _dgcnn_case(fx):
    if not hasattr(_dgcnn_case, "c"):
        import dgcnn_ref
        N, B, K, nc = 64, 2, 10, 10
        P = dgcnn_ref.random_params(nc, seed=3)
        m = fx.DGCNN(nc, K, npoints=N).load(P)
        d4, d5 = m.dropout_masks(B, 7)
        c = SimpleNamespace(N=N, B=B, K=K, nc=nc, P=P, params=m.flat_params(), X=_randn((3, N, B), 91), glogits=_randn((nc, B), 92),
                            d4=np.asfortranarray(d4, dtype=np.float32), d5=np.asfortranarray(d5, dtype=np.float32))
        n = C.c_int64(0)
        fx._lib.call("fx3d_dgcnn_stat_count", C.byref(n))
        c.nstat = n.value
        c.fwd = dgcnn_ref.forward(c.X, P, K)
        _dgcnn_case.c = c
    return _dgcnn_case.c


@pytest.mark.parametrize("entry", ["forward", "forward_train", "grad"])
def test_dgcnn(gpu_fx, entry):
    """DGCNN at 2 x 64, K = 10.  x1 is the one array argument the header asks 16-byte alignment for (the forward entry points
    write it with 16-byte stores): it stays aligned, and a misaligned x1 is refused before any launch."""
    import dgcnn_grad_ref
    import dgcnn_ref
    import dgcnn_train_ref
    fx, c = gpu_fx, _dgcnn_case(gpu_fx)
    N, B, K, nc = c.N, c.B, c.K, c.nc
    outs = [O("probs", (nc, B)), O("logits", (nc, B)), O("idx1", (K, N, B), np.int32), O("x1", (64, N, B)), O("idx2", (K, N, B), np.int32),
            O("x2", (256, N, B)), O("pooled", (1024, B))]
    bitwise = ("logits", "x1", "x2", "pooled")
    if entry == "forward":
        nb = _ws(fx, "fx3d_dgcnn_workspace_bytes", N, B, K, nc)
        call = lambda p, ws, n: _abi(fx, "fx3d_dgcnn_forward")(p.params, nc, K, p.x, N, B, p.probs, p.logits, p.idx1, p.x1, p.idx2, p.x2, p.pooled,  # noqa: E731
                                                               ws, n, None)
        r = hold(fx, call, [I("params", c.params), I("x", c.X)] + outs, nb, skip=("x1",))
        want = c.fwd
        pd, xd, probs, x1 = fx.gpu(c.params), fx.gpu(c.X), fx.DeviceArray.empty((nc, B)), fx.DeviceArray.empty((64 * N * B + 4,))
        ws = fx.DeviceArray.empty((nb,), np.uint8)
        rc = fx._lib.load().fx3d_dgcnn_forward(pd.ptr, nc, K, xd.ptr, N, B, probs.ptr, None, None, x1.ptr + 4, None, None, None, ws.ptr, nb, None)
        assert rc == -1 and "x1" in fx._lib.last_error()
    elif entry == "forward_train":
        nb = _ws(fx, "fx3d_dgcnn_train_workspace_bytes", N, B, K, nc)
        call = lambda p, ws, n: _abi(fx, "fx3d_dgcnn_forward_train")(p.params, nc, K, p.x, N, B, p.d4, p.d5, 0.1, p.probs, p.logits, p.idx1, p.x1,  # noqa: E731
                                                                     p.idx2, p.x2, p.pooled, p.stats, p.running, ws, n, None)
        r = hold(fx, call, [I("params", c.params), I("x", c.X), I("d4", c.d4), I("d5", c.d5)] + outs + [O("stats", (c.nstat,)), O("running", (c.nstat,))],
                 nb, skip=("x1",))
        want = dgcnn_train_ref.forward_train(c.X, c.P, K, dropout=(c.d4, c.d5), momentum=0.1)
        _flat_same(r["stats"], dgcnn_train_ref.flat_stats(want["batch_stats"]), "batch_stats")
        _flat_same(r["running"], dgcnn_train_ref.flat_stats(want["running"]), "running")
    if entry.startswith("forward"):
        assert np.array_equal(r["idx1"], want["idx1"]) and np.array_equal(r["idx2"], want["idx2"])
        for k in bitwise:
            _flat_same(r[k], want[k], k)
        return
    f = c.fwd
    nb = _ws(fx, "fx3d_dgcnn_grad_workspace_bytes", N, B, K, nc)
    arrs = [I("params", c.params), I("x", c.X), I("idx1", f["idx1"], np.int32), I("x1", f["x1"], np.float32), I("idx2", f["idx2"], np.int32),
            I("x2", f["x2"], np.float32), I("pooled", f["pooled"], np.float32), I("glogits", c.glogits), O("gparams", (c.params.size,)), O("gx", (3, N, B)),
            O("gx2", (256, N, B)), O("gx1", (64, N, B))]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_dgcnn_grad")(p.params, nc, K, p.x, N, B, p.idx1, p.x1, p.idx2, p.x2, p.pooled, p.glogits, p.gparams, p.gx,
                                                              p.gx2, p.gx1, ws, n, None), arrs, nb)
    grads, gx, gx2, gx1 = dgcnn_grad_ref.grad(c.X, c.P, K, c.glogits, f)
    _flat_same(r["gparams"], dgcnn_grad_ref.flat(grads), "gparams")
    for k, w in (("gx", gx), ("gx2", gx2), ("gx1", gx1)):
        _flat_same(r[k], w, k)


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
