"""One statement of every kernel family's C-ABI call and of the reference it is held to.

tests/test_gpu_alignment.py (pointers aligned to 4 bytes only), tests/test_gpu_workspace.py (dirty, exact-size scratch) and
tests/test_gpu_replay.py (the call recorded into a graph and replayed, on the recorded and on other data) run the same families: each family builds its arrays, states the call as a closure ``call(p, ws, ws_bytes)`` over the placed
pointers, hands both to the ``hold`` driver of the file that runs it and compares what ``hold`` returns -- the outputs of the
plain call -- with the family's reference exactly as the family's own test checks it (the oracle, the tests/*_ref.py
restatements, the golden known answers; the one tolerance is LOSS_RTOL, chamfer loss against the oracle, as everywhere).

``hold(fx, call, arrs, ws_bytes=0, skip=(), check=None)`` is the driver's whole surface.  ``check(results)``: for the few
routes whose sums have no fixed order (float atomics) every run goes through the family's own bound instead of a bit comparison.
Shapes default to those of the alignment file; the workspace file also passes ragged ones."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
import transforms_ref as tref
from test_gpu_hardening import LOSS_RTOL


# ---------------------------------------------------------------------------------------------------------- shared by drivers
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


NULLABLE = set()   # the optional arguments the running test's family has left out on purpose (_but): only those may be missing
                   # from a Ptrs.  Both test files empty it before every test (`fresh_nullable`).


class Ptrs(SimpleNamespace):
    """{argument name: device pointer} as attributes; an optional argument a family left out on purpose (_but) is NULL, any
    other missing name is an error."""

    def __getattr__(self, name):
        if name.startswith("__") or name not in NULLABLE:
            raise AttributeError(name)
        return None


class Calls:
    """What a driver may hang on every C-ABI call a family makes through ``_abi``: ``before(name)`` / ``after(name)`` run around
    the call (the workspace driver checks its guard pads after each call of a carried pair), ``before`` returning False leaves the
    call out; ``refused(name, error)`` returning True swallows an error status other than FX3D_ERR_HIP (the refusal driver
    records it).  ``stream``: the families state every call on the default stream, a literal None as the last argument; a driver
    that runs them on a stream of its own (tests/test_gpu_replay.py: a capture needs a created stream) puts its handle here, and
    it takes the place of that trailing None wherever the entry point's last parameter is a pointer -- in every call a family
    makes through ``_abi`` that is the stream."""
    before = after = refused = stream = None


def _abi(fx, name):
    def f(*args):
        if Calls.stream is not None and args and args[-1] is None and fx._lib.SIGNATURES[name][-1] is fx._lib.vp:
            args = args[:-1] + (Calls.stream,)
        if Calls.before and Calls.before(name) is False:
            return
        try:
            fx._lib.call(name, *args)
        except fx.Flux3DHipError as e:
            if e.code == -2:  # FX3D_ERR_HIP is sticky (a fault poisons the context): nothing more is started on the device
                pytest.exit(f"{name}: {e}", returncode=3)
            if not (Calls.refused and Calls.refused(name, e)):
                raise
        if Calls.after:
            Calls.after(name)
    return f


def _ws(fx, query, *args):
    QUERIED.add(query)
    return fx._lib.query_bytes(query, *args)


QUERIED = set()   # the size queries made so far (the workspace file asserts that a case made the one it names)


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


# ragged shapes (the workspace file): padded rows and a tail tile in every layout; one split-plan shape is NN_SHAPES' own
NN_RAGGED = {
    "r257_d3": (257, 131, 3, 3, {}, dict(), False),
    "r130_d2": (130, 77, 2, 2, {}, dict(), False),
    "r130_d64": (130, 77, 2, 64, {}, dict(), False),
}


# only the chamfer forward entry points prune: fx3d_nn1 and the adjoint at 4096 points are the mfma_filter case
NN_CASES = [(s, e) for s in NN_SHAPES for e in ("nn1", "chamfer_fwd", "chamfer_fwd_bwd", "chamfer_bwd")
            if not (s == "pruned" and e in ("nn1", "chamfer_bwd"))]


def nn1_and_chamfer(fx, oracle, fx_option, hold, shape, entry, without=()):
    N, M, B, D, opts, want, big = {**NN_SHAPES, **NN_RAGGED}[shape]
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
        # (`without` idx_x, idx_y: the neighbour indices the adjoint dereferences then live in the workspace)
        arrs = [I("x", x), I("y", y), O("loss", (1,)), O("gx", (D, N, B)), O("gy", (D, M, B))] + _but(
            [O("idx_x", (N, B), np.int32), O("idx_y", (M, B), np.int32)], without)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_chamfer_fwd_bwd")(p.x, N, p.y, M, B, D, w1, w2, gout, B, p.loss, None, p.gx, p.gy,
                                                                     p.idx_x, p.idx_y, ws, n, None), arrs, nb)
        ogx, ogy = oracle.chamfer_bwd(x, y, ox, oy, w1, w2, gout)
        assert np.array_equal(r["gx"], ogx) and np.array_equal(r["gy"], ogy)
    for k, want_idx in (("idx_x", ox), ("idx_y", oy)):
        assert (k in r or k in NULLABLE) and (k not in r or np.array_equal(r[k], want_idx)), k
    assert np.isclose(r["loss"][0], oloss, rtol=LOSS_RTOL, atol=0), (r["loss"][0], oloss)


def chamfer_backward_long_inverse_lists(fx, oracle, hold):
    """The adjoint on index maps with long inverse lists (the "clusters" kind of test_gpu_parity's test of that name), D = 3."""
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


# the workspace file's candidate-slice shape: few queries, many candidates, so the plan cuts the candidates into slices
KNN_SLICED = {"d64_slices_n300_m2048": (64, 300, 2048, 2, 20, 0, {}, True),
              # 32 < k + drop in feature space: two slices of 32 entries each, the VERIFIED merge (flags, the interleaved copy of the
              # candidates) and the selection kernel for the flagged queries
              "d64_verified_k40": (64, 256, 256, 2, 40, 1, {}, True)}


def knn(fx, oracle, fx_option, hold, case, entry):
    """x, y, idx and dist misaligned independently.  The pre-pass shapes are eligible for the F16Pre kernel when aligned; an
    offset x or y sends them to the F16 kernel (y aligned) or the F32-filter kernel (y not), an offset idx or dist to the
    scalar stores of the lists (k % 4 == 0)."""
    D, N, M, B, k, drop, opts, wants_ws = {**KNN_CASES, **KNN_SLICED}[case]
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
        if case in KNN_SLICED:   # the candidate slices ask for scratch of their own: without them the query is another
            with fx._lib.option("knn_slices", 1):
                assert _ws(fx, "fx3d_knn_workspace_bytes", N, M, B, D, k, drop) != nb, "the shape no longer takes the candidate slices"
        r = hold(fx, lambda p, ws, n: _abi(fx, entry)(p.x, N, p.y, M, B, D, k, drop, p.idx, p.dist, ws if n else None, n, None), arrs, nb)
    assert np.array_equal(r["idx"], oi), np.argwhere(r["idx"] != oi)[:5]
    assert np.array_equal(r["dist"], od)


# ------------------------------------------------------------------ knn_gather, edge_features, edge_features_grad, edgeconv_graph
def graph_features(fx, oracle, fx_option, hold, F, K):
    """N = 64, B = 2.  The layout-1 mlp4 kernel needs F % 4 == 0, (K N) % 4 == 0 and x, out, idx all aligned: F = 3 never takes
    it, F = 4 / 64 leave it for the one-position kernels as soon as one pointer moves.  (K N) % 4 is 0 for both K at N = 64, so
    K = 5 also runs at N = 63, where it is not and the second cloud of every array sits 12 bytes off whatever the base."""
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


def _hold_map(fx, hold, call, x, extra=(), ws_bytes=0, outs=()):
    """One transform out of place (x and y placed independently) and in place (y == x): both give the same bits."""
    arrs = [I("x", x)] + list(extra) + [O("y", x.shape)] + list(outs)
    r = hold(fx, lambda p, ws, nb: call(p, p.x, p.y, ws, nb), arrs, ws_bytes)
    arrs = list(extra) + [O("y", x.shape, init=x)] + list(outs)
    r2 = hold(fx, lambda p, ws, nb: call(p, p.y, p.y, ws, nb), arrs, ws_bytes)
    for k in r:
        assert _bits_equal(r[k], r2[k]), ("in place", k)
    return r


def transforms_dense(fx, hold, D, n, only_ws=False):
    """scale, translate, rotate (one matrix, one per cloud), both normalize forms, realign and segment_minmax through the C ABI on
    a (D, n, 2) cloud: map_range's "aligned middle" is taken from the element index, affine_kernel and rotate_kernel read and
    write 16 bytes at x + 4 q / x + 12 q whatever the address -- an odd n shifts the second cloud, the placement the first.
    `only_ws`: the two entry points that take a workspace (normalize, segment_minmax) alone."""
    B = 2
    x = _randn((D, n, B), 1000 * D + n) + np.float32(3.0)
    tot = D * n * B
    if not only_ws:
        _transforms_maps(fx, hold, D, n, B, x, tot)
    nb = _ws(fx, "fx3d_transform_workspace_bytes", D, n, B)
    wc, wsd = tref.pcloud_stats(x)
    for mode in (0, 1):
        r = _hold_map(fx, hold, lambda p, xi, yo, ws, n_: _abi(fx, "fx3d_normalize")(xi, D, n, B, None, mode, yo, p.c, p.s, ws if n_ else None, n_, None),
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
    if only_ws:
        return
    tmin, tmax = np.full((D, 1), -2.0, np.float32), np.linspace(1, 3, D, dtype=np.float32).reshape(D, 1)
    extra = [I("smin", smin), I("smax", smax), I("tmin", tmin), I("tmax", tmax)]
    r = _hold_map(fx, hold, lambda p, xi, yo, ws, n_: _abi(fx, "fx3d_realign")(xi, D, n, B, None, p.smin, p.smax, p.tmin, p.tmax, yo, None), x, extra=extra)
    assert tref.same_bits(r["y"], tref.pcloud_realign(x, tmin, tmax))


def transforms_ragged_segments(fx, hold):
    """fx3d_segment_minmax and fx3d_normalize on a packed (3, sum n) stream of three segments of 3, 1 and 2 chunks: the grid is
    (3 chunks, 3 segments), a chunk past a segment's end stores no partial, and the fold reads its own segment's chunks only."""
    D, B = 3, 3
    buf = C.create_string_buffer(256)
    fx._lib.call("fx3d_transform_plan_describe", D, 1 << 20, B, buf, 256)
    cc = int(dict(kv.split("=") for kv in buf.value.decode().split())["chunk_cols"])
    n_max = 2 * cc + 7
    lens = [n_max, cc // 2, cc + 3]
    fx._lib.call("fx3d_transform_plan_describe", D, n_max, B, buf, 256)
    plan = dict(kv.split("=") for kv in buf.value.decode().split())
    assert plan["plan"] == "two_launch" and int(plan["nchunks"]) == 3, plan
    v = _randn((D, sum(lens)), 77) + np.float32(3.0)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nb = _ws(fx, "fx3d_transform_workspace_bytes", D, n_max, B)
    assert nb > 0
    for pad_zero, (smin, smax) in ((1, tref.mesh_bounds_padded(v, lens)),):
        arrs = [I("x", v), I("seg", seg), O("mn", (D, B)), O("mx", (D, B))]
        r = hold(fx, lambda p, ws, n_: _abi(fx, "fx3d_segment_minmax")(p.x, D, n_max, B, p.seg, pad_zero, p.mn, p.mx, ws, n_, None), arrs, nb)
        assert tref.same_bits(r["mn"], smin) and tref.same_bits(r["mx"], smax)
    wc, wsd = tref.mesh_stats(v, lens)
    arrs = [I("x", v), I("seg", seg), O("y", v.shape), O("c", (D, B)), O("s", (D, B))]
    r = hold(fx, lambda p, ws, n_: _abi(fx, "fx3d_normalize")(p.x, D, n_max, B, p.seg, 1, p.y, p.c, p.s, ws, n_, None), arrs, nb)
    assert tref.within_ulp(r["c"], wc) and tref.within_ulp(r["s"], wsd)
    assert tref.same_bits(r["y"], tref.mesh_normalize(v, lens, r["c"], r["s"]))


def _transforms_maps(fx, hold, D, n, B, x, tot):
    """scale, translate and rotate: no workspace."""
    r = _hold_map(fx, hold, lambda p, xi, yo, ws, nb: _abi(fx, "fx3d_scale_translate")(xi, tot, 0, _vec(1.7), yo, None), x)
    assert tref.same_bits(r["y"], tref.pcloud_scale(x, 1.7))
    if D == 3:
        t = (1.0, -2.0, 1e4)
        r = _hold_map(fx, hold, lambda p, xi, yo, ws, nb: _abi(fx, "fx3d_scale_translate")(xi, tot, 1, _vec(*t), yo, None), x)
        assert tref.same_bits(r["y"].reshape(3, n * B, order="F"), tref.mesh_translate(x.reshape(3, n * B, order="F"), t))
        R, Rb = _randn((3, 3), 5), _randn((3, 3, B), 6)
        Rh = _vec(*R.reshape(-1, order="F"))
        r = _hold_map(fx, hold, lambda p, xi, yo, ws, nb: _abi(fx, "fx3d_rotate")(xi, n * B, n, B, None, Rh, None, yo, None), x)
        assert tref.same_bits(r["y"], tref.pcloud_rotate(x, R))
        r = _hold_map(fx, hold, lambda p, xi, yo, ws, nb: _abi(fx, "fx3d_rotate")(xi, n * B, n, B, None, None, p.R, yo, None), x, extra=[I("R", Rb)])
        assert tref.same_bits(r["y"], tref.pcloud_rotate(x, Rb))

def _teapot_sphere(fx):
    return fx.load_trimesh(os.path.join(GOLDEN, "teapot.obj"), os.path.join(GOLDEN, "sphere.obj"))


def transforms_ragged_mesh_batch_as_a_slab_of_a_longer_packed_array(fx):
    """The teapot + sphere batch as columns [off, off + sum V) of a longer packed (3, *) array, off = 1, 2, 3 columns (12, 24, 36
    bytes: 12, 8 and 4 past a 16-byte boundary) -- what `v.ptr + 12 * off` and DeviceArray.slab hand to the kernels -- through
    the package's own in-place transforms."""
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
def pointcloud_to_voxel(fx, oracle, hold, res, N=1024, B=2):
    x = _rand((3, N, B), 77 + res)
    nb = _ws(fx, "fx3d_voxel_workspace_bytes", B)
    arrs = [I("x", x), O("vox", (res, res, res, B))]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointcloud_to_voxel")(p.x, N, B, res, p.vox, ws, n, None), arrs, nb)
    assert _bits_equal(r["vox"], oracle.pointcloud_to_voxel(x, res))


def uv_sphere(rings, segs, seed=0, drop=0):
    """A closed latitude / longitude sphere, V = 2 + rings segs and F = 2 rings segs (so E = 3 rings segs), its vertices moved a
    little by `seed` so that no two meshes of a batch are alike; `drop` faces taken off the end (an open mesh, any face count).
    (3, V) Float32 and (3, F) 1-based Int64."""
    rng = np.random.default_rng(1000 + seed)
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segs) / segs
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(segs))]).reshape(3, -1)
    v = np.concatenate([[[0.0], [0.0], [1.0]], ring, [[0.0], [0.0], [-1.0]]], axis=1)
    v = (v * (1.0 + 0.05 * rng.random((1, v.shape[1])))).astype(np.float32)
    at = lambda r, c: 1 + r * segs + c % segs  # noqa: E731
    f = [(0, at(0, c), at(0, c + 1)) for c in range(segs)]
    for r in range(rings - 1):
        for c in range(segs):
            f += [(at(r, c), at(r + 1, c), at(r + 1, c + 1)), (at(r, c), at(r + 1, c + 1), at(r, c + 1))]
    last = 1 + rings * segs
    f += [(last, at(rings - 1, c + 1), at(rings - 1, c)) for c in range(segs)]
    f = np.asarray(f, np.int64).T + 1
    assert v.shape[1] == 2 + rings * segs and f.shape[1] == 2 * rings * segs
    return np.asfortranarray(v), np.asfortranarray(f[:, :f.shape[1] - drop])


# kind: the meshes of the batch as (rings, segs, faces dropped)
MESHES = {
    "sphere_v1502": [(30, 50, 0)],                          # V = 1502, E = 4500, F = 3000: more than one block partial
    "sphere_v50": [(6, 8, 0)],                              # V = 50, F = 96
    "sphere_v102": [(10, 10, 0)],                           # V = 102, F = 200
    "ragged3": [(4, 5, 3), (3, 4, 0), (3, 5, 1)],           # Fmax = 37, B = 3: F = 37, 24, 29 and V = 22, 14, 17
    "sphere_f7688": [(62, 62, 0)],                          # F = 7688: the CDF's working copy no longer fits LDS, it is built in the workspace
    "equalv3_v1502": [(30, 50, 3), (30, 50, 0), (30, 50, 7)],   # the same at V = 1502 each: 4506 vertices, more than one block partial
    "equalv3": [(4, 5, 3), (4, 5, 0), (4, 5, 7)],           # ragged faces, F = 37, 40, 33, on equal vertex counts (padded == packed)
}


def _mesh(fx, kind="teapot_sphere", seed=0):
    """A mesh batch in every form the mesh entry points take (host arrays; int32 0-based indices): the teapot + sphere batch, or
    one of MESHES."""
    cache = _mesh.__dict__.setdefault("cache", {})
    if (kind, seed) not in cache:
        if kind == "teapot_sphere":
            m = _teapot_sphere(fx)
        else:
            parts = [uv_sphere(r, c, seed=17 * seed + i, drop=dr) for i, (r, c, dr) in enumerate(MESHES[kind])]
            m = fx.TriMesh([p[0] for p in parts], [p[1] for p in parts])
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
        cache[(kind, seed)] = d
    return cache[(kind, seed)]


def trimesh_to_voxel(fx, hold, res, kind="teapot_sphere"):
    import trimesh_voxel_ref
    d = _mesh(fx, kind)
    nb = _ws(fx, "fx3d_trimesh_voxel_workspace_bytes", d.Vmax, d.Fmax, d.B, res)
    arrs = [I("verts", d.vp), I("vlen", d.vlen), I("faces", d.fp), I("flen", d.flen), O("vox", (res, res, res, d.B)),
            O("bad", (1,), np.uint32)]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_trimesh_to_voxel")(p.verts, d.Vmax, p.vlen, p.faces, d.Fmax, p.flen, d.B, res, p.vox, p.bad,
                                                                     ws, n, None), arrs, nb)
    assert r["bad"][0] == 0
    assert _bits_equal(r["vox"], trimesh_voxel_ref.trimesh_to_voxel(d.m.get_verts_list(), d.m.get_faces_list(), res))


def voxel_to_trimesh_exact(fx, hold, extra, fill=0.4):
    """fx3d_voxel_mesh_count + _emit with the caller's verts and faces outputs: vm_emit_kernel stores a cube's 24 floats as six
    float4 at verts + 24 s0 and, when Fmax % 4 == 0 (extra = 0), its 36 face ids as nine int4 -- at whatever address."""
    import voxel_mesh_ref
    res, B = 8, 2
    rng = np.random.default_rng(70 + extra)
    vox = np.asfortranarray((rng.random((res, res, res, B)) < fill).astype(np.float32))
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
def mesh_faces_through_index_convert_and_upload(fx, hold, index_type, count=None):
    """The reference's 1-based UInt32 / Int64 face arrays to the library's int32 0-based form on the device, source and
    destination offset (fx3d_index_convert), and from the host through the staging workspace (fx3d_index_upload)."""
    d = _mesh(fx)
    dt = np.dtype(index_type.replace("upload_", ""))
    code = {"int32": 0, "uint32": 1, "int64": 2}[dt.name]
    src = np.asfortranarray(d.m.get_faces_padded().astype(dt))
    want = d.fp
    if count is not None:   # the first `count` indices of the same array: a staging buffer with a ragged tail
        src, want = np.ascontiguousarray(src.ravel(order="F")[:count]), d.fp.ravel(order="F")[:count]
    cnt = src.size
    if index_type.startswith("upload"):
        nb = _ws(fx, "fx3d_index_upload_workspace_bytes", code, cnt)
        arrs = [O("dst", src.shape, np.int32), O("bad", (1,), np.uint32)]
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_index_upload")(src.ctypes.data, code, 1, cnt, 1, d.Vmax, p.dst, p.bad, ws, n, None), arrs, nb)
    else:
        arrs = [I("src", src), O("dst", src.shape, np.int32), O("bad", (1,), np.uint32)]
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_index_convert")(p.src, code, 1, cnt, 1, d.Vmax, p.dst, p.bad, None), arrs)
    assert r["bad"][0] == 0 and np.array_equal(r["dst"], want)


def mesh_face_areas(fx, oracle, hold):
    d = _mesh(fx)
    arrs = [I("verts", d.v), I("faces", d.f), O("areas", (d.F,))]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_faces_areas_packed")(p.verts, d.V, p.faces, d.F, p.areas, None), arrs)
    assert _bits_equal(r["areas"], oracle.faces_areas_packed(d.v, d.f))
    arrs = [I("verts", d.vp), I("faces", d.fp), I("flen", d.flen), O("areas", (1, d.Fmax, d.B))]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_faces_areas_padded")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, p.areas, None), arrs)
    assert _bits_equal(r["areas"], oracle.faces_areas_padded(d.vp, d.fp, d.flen))


def mesh_losses_and_adjoints(fx, oracle, hold, kind="teapot_sphere", only_ws=False, reuse=((1, True),)):
    """laplacian_loss, edge_loss, the fused pair; their adjoints in the gather forms (bit for bit the oracle) and in the scatter
    forms, whose float atomics add in arrival order: no placement of those is bit-equal to another RUN of itself, so each is
    held to the family's bound against the oracle (test_gpu_parity / test_gpu_hardening: rtol 1e-4, atol 1e-9).
    `only_ws`: the entry points that take a workspace alone (edge_loss, laplacian_loss, mesh_losses + _bwd with both values of
    `fresh`)."""
    d = _mesh(fx, kind)
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
    if not only_ws:
        _mesh_adjoints_without_workspace(fx, hold, d, csr, gout, target, glap, gedge)
    # both losses in one launch, both adjoints in one gather launch, on top of a base gradient
    nb2 = _ws(fx, "fx3d_mesh_losses_workspace_bytes", d.V, d.E)
    base = _randn((3, d.V), 3)
    arrs = [I("verts", d.v)] + csr + [I("edges", d.e), O("lap", (1,)), O("edge", (1,)), O("total", (1,)), O("g", (3, d.V), init=base)]
    gl2 = oracle.laplacian_loss_bwd(d.v, r64, c64, d.vals, 0.1 * gout)
    # `reuse`: (reuse_forward, a forward runs first).  1: the adjoint reuses the unit rows the forward left in the workspace; 0: it
    # rebuilds them itself, with or without a forward before it
    for fresh, forward in reuse:
        def call(p, ws, n):
            if forward:
                _abi(fx, "fx3d_mesh_losses")(p.verts, d.V, p.rowptr, p.colind, p.vals, p.edges, d.E, target, 0.1, 1.0, None, p.lap, p.edge, p.total,
                                              ws, n, None)
            _abi(fx, "fx3d_mesh_losses_bwd")(p.verts, d.V, p.rowptr, p.colind, p.vals, d.E, target, 0.1 * gout, gout, fresh, p.g, 1, ws, n, None)
        r = hold(fx, call, arrs, nb2)
        if forward:
            assert np.isclose(r["lap"][0], ol, rtol=LOSS_RTOL, atol=0) and np.isclose(r["edge"][0], oe, rtol=LOSS_RTOL, atol=0)
            assert r["total"][0] == np.float32(np.float32(np.float32(0.1) * r["lap"][0]) + r["edge"][0])
        assert _bits_equal(r["g"], ((base + gl2).astype(np.float32) + gedge).astype(np.float32)), (fresh, forward)


def _mesh_adjoints_without_workspace(fx, hold, d, csr, gout, target, glap, gedge):
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


def mesh_sampling_and_ordered_adjoint(fx, oracle, hold, kind="teapot_sphere", n=500, only_ws=False):
    """fx3d_sample_points; the same draws from fx3d_sample_points_cdf -> _draw and, two meshes at a time, _cdf_pair -> _draw_pair
    (the CDF is what the pair carries in its workspace); the explicit form and the ordered adjoint (no workspace)."""
    from test_gpu_topology import host_vertex_faces
    d = _mesh(fx, kind)
    seed = 11
    out, fi, r1, r2 = oracle.sample_points_seeded(d.vp, d.fp, d.flen, n, seed, return_draws=True)
    nb = _ws(fx, "fx3d_sample_points_workspace_bytes", d.Fmax, d.B)
    mesh = [I("verts", d.vp), I("faces", d.fp), I("flen", d.flen)]
    arrs = mesh + [O("out", (3, n, d.B)), O("fi", (n, d.B), np.int32), O("r1", (n, d.B)), O("r2", (n, d.B))]
    r = hold(fx, lambda p, ws, nn: _abi(fx, "fx3d_sample_points")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, n, 1e-6, seed, p.out, p.fi, p.r1,
                                                                   p.r2, ws, nn, None), arrs, nb)
    assert _bits_equal(r["out"], out) and np.array_equal(r["fi"], fi) and _bits_equal(r["r1"], r1) and _bits_equal(r["r2"], r2)

    def cdf_draw(p, ws, nn):
        _abi(fx, "fx3d_sample_points_cdf")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, 1e-6, ws, nn, None)
        _abi(fx, "fx3d_sample_points_draw")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, n, seed, None, ws, nn, p.out, p.fi, p.r1, p.r2, None)
    r = hold(fx, cdf_draw, arrs, nb)
    assert _bits_equal(r["out"], out) and np.array_equal(r["fi"], fi) and _bits_equal(r["r1"], r1) and _bits_equal(r["r2"], r2)
    # the pair forms: this batch and the same batch scaled, seeds `seed` and `seed` + 1, each side with a workspace of its own
    vp2 = np.asfortranarray(d.vp * np.float32(1.5))
    out2 = oracle.sample_points_seeded(vp2, d.fp, d.flen, n, seed + 1)
    arrs = mesh + [I("verts2", vp2), O("out", (3, n, d.B)), O("fi", (n, d.B), np.int32), O("r1", (n, d.B)), O("r2", (n, d.B)), O("out2", (3, n, d.B))]
    for dirty_side in (0, 1):   # the driver's workspace is one side's, the other side's is a plain zeroed allocation
        other = fx.DeviceArray.zeros((max(nb, 256),), np.uint8)

        def pair(p, ws, nn):
            w0, w1 = (ws, other.ptr) if dirty_side == 0 else (other.ptr, ws)
            _abi(fx, "fx3d_sample_points_cdf_pair")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, w0, nn,
                                                     p.verts2, d.Vmax, p.faces, d.Fmax, p.flen, d.B, w1, nn, 1e-6, None)
            _abi(fx, "fx3d_sample_points_draw_pair")(p.verts, d.Vmax, p.faces, d.Fmax, p.flen, d.B, n, seed, w0, nn, p.out, p.fi, p.r1, p.r2,
                                                      p.verts2, d.Vmax, p.faces, d.Fmax, p.flen, d.B, n, seed + 1, w1, nn, p.out2, None, None, None,
                                                      None, None)
        r = hold(fx, pair, arrs, nb)
        assert _bits_equal(r["out"], out) and np.array_equal(r["fi"], fi) and _bits_equal(r["r1"], r1) and _bits_equal(r["r2"], r2)
        assert _bits_equal(r["out2"], out2), dirty_side
    if only_ws:
        return
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


def mesh_normals_and_adjoints(fx, hold, kind="teapot_sphere"):
    import normals_ref
    from test_gpu_topology import host_vertex_faces
    d = _mesh(fx, kind)
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


def mesh_topology_tables(fx, hold, kind="teapot_sphere"):
    """csrc/topology_dev.hip against the host builders of csrc/topology.cpp, as tests/test_gpu_topology.py holds them."""
    from test_gpu_topology import host_edges, host_laplacian, host_vertex_faces
    d = _mesh(fx, kind)
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


def _pointnet_case(fx, N=64):
    cache = _pointnet_case.__dict__.setdefault("c", {})
    if N not in cache:
        import pointnet_ref
        B, nc = 2, 10
        P = pointnet_ref.random_params(nc, seed=10)
        m = fx.PointNet(nc).load(P)
        c = SimpleNamespace(N=N, B=B, nc=nc, P=P, params=m.flat_params(), X=_randn((3, N, B), 500 + N), glogits=_randn((nc, B), 600 + N),
                            dropout=np.asfortranarray(m.dropout_mask(B, 3), dtype=np.float32))
        n = C.c_int64(0)
        fx._lib.call("fx3d_pointnet_stat_count", C.byref(n))
        c.nstat = n.value
        cache[N] = c
    return cache[N]


def _but(arrs, without, inputs=False):
    """`arrs` less the optional outputs (`inputs`: optional inputs) named in `without`: the drivers' pointer namespace (Ptrs)
    gives NULL for those."""
    assert set(without) <= {a.name for a in arrs if a.out != inputs}, without
    NULLABLE.update(without)
    return [a for a in arrs if a.name not in without]


def _same_if(r, k, want, what=None):
    """r[k] against `want`; an output may be absent only where a family left it out on purpose."""
    assert k in r or k in NULLABLE, k
    if k in r:
        _flat_same(r[k], want, what or k)


def pointnet(fx, hold, entry, N=64, without=()):
    """PointNet at 2 x N: X, params_dev, glogits, the dropout multipliers, the batch statistics and every output offset.
    `without`: optional outputs passed as NULL (the header: those then live in the workspace, or are not formed)."""
    import pointnet_grad_ref
    import pointnet_grad_train_ref
    import pointnet_ref
    import pointnet_train_ref
    c = _pointnet_case(fx, N)
    B, nc = c.B, c.nc
    fwd_outs = [O("probs", (nc, B)), O("logits", (nc, B)), O("stn", (3, 3, B)), O("fstn", (64, 64, B)), O("pooled", (1024, B))]
    grad_outs = [O("gparams", (c.params.size,)), O("gx", (3, N, B)), O("gstn", (3, 3, B)), O("gfstn", (64, 64, B)), O("gh", (64, N, B)),
                 O("gxt", (3, N, B))]
    if entry == "forward":
        nb = _ws(fx, "fx3d_pointnet_workspace_bytes", N, B, nc)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointnet_forward")(p.params, nc, p.x, N, B, p.probs, p.logits, p.stn, p.fstn, p.pooled, ws, n, None),
                 [I("params", c.params), I("x", c.X)] + _but(fwd_outs, without), nb)
        want = pointnet_ref.forward(c.X, c.P)
    elif entry == "forward_train":
        nb = _ws(fx, "fx3d_pointnet_train_workspace_bytes", N, B, nc)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointnet_forward_train")(p.params, nc, p.x, N, B, p.dropout, 0.1, p.probs, p.logits, p.stn, p.fstn,
                                                                              p.pooled, p.stats, p.running, ws, n, None),
                 [I("params", c.params), I("x", c.X), I("dropout", c.dropout)] + _but(fwd_outs + [O("stats", (c.nstat,)), O("running", (c.nstat,))], without), nb)
        want = pointnet_train_ref.forward_train(c.X, c.P, c.dropout, 0.1)
        _flat_same(r["stats"], pointnet_train_ref.flat_stats(want["batch_stats"]), "batch_stats")
        _same_if(r, "running", pointnet_train_ref.flat_stats(want["running"]))
    if entry.startswith("forward"):
        for k in ("logits", "stn", "fstn", "pooled"):
            _same_if(r, k, want[k])
        if without:   # probs has no restatement of its own: with the optional outputs left out it is the full call's bits
            return r
        return
    if entry == "grad":
        nb = _ws(fx, "fx3d_pointnet_grad_workspace_bytes", N, B, nc)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointnet_grad")(p.params, nc, p.x, N, B, p.glogits, p.gparams, p.gx, p.gstn, p.gfstn, p.gh, p.gxt,
                                                                     ws, n, None),
                 [I("params", c.params), I("x", c.X), I("glogits", c.glogits)] + _but(grad_outs, without), nb)
        grads, gx, mid = pointnet_grad_ref.grad(c.X, c.P, c.glogits)
        flat = pointnet_grad_ref.flat(grads)
    else:
        stats = pointnet_train_ref.flat_stats(pointnet_train_ref.forward_train(c.X, c.P, c.dropout, 0.1)["batch_stats"])
        nb = _ws(fx, "fx3d_pointnet_grad_train_workspace_bytes", N, B, nc)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_pointnet_grad_train")(p.params, nc, p.x, N, B, p.dropout, p.stats, p.glogits, p.gparams, p.gx,
                                                                           p.gstn, p.gfstn, p.gh, p.gxt, ws, n, None),
                 [I("params", c.params), I("x", c.X), I("dropout", c.dropout), I("stats", stats), I("glogits", c.glogits)] + _but(grad_outs, without), nb)
        grads, gx, mid = pointnet_grad_train_ref.grad_train(c.X, c.P, c.glogits, c.dropout)
        flat = pointnet_grad_ref.flat(grads)
    _flat_same(r["gparams"], flat, "gparams")
    _same_if(r, "gx", gx)
    for k in ("gstn", "gfstn", "gh", "gxt"):
        _same_if(r, k, mid[k])


EDGECONV_LAYERS = {"3_32_64_64": [3, 32, 64, 64], "64_128_256": [64, 128, 256]}


def _edgeconv_case(fx, name, N=64, K=4):
    cache = _edgeconv_case.__dict__.setdefault("c", {})
    if (name, N, K) not in cache:
        import dgcnn_train_ref
        import edgeconv_ref
        layers, B = EDGECONV_LAYERS[name], 2
        P = edgeconv_ref.random_params(layers, 5)
        c = SimpleNamespace(layers=layers, K=K, N=N, B=B, P=P, params=fx.EdgeConv(layers, K).load(P).flat_params(),
                            X=_randn((layers[0], N, B), 77 + layers[0]), gout=_randn((layers[-1], N, B), 78 + layers[0]))
        c.lc = (C.c_int32 * len(layers))(*layers)
        c.idx, c.out = edgeconv_ref.forward(c.X, P, layers, K)
        c.train = dgcnn_train_ref.edgeconv_forward_train(c.X, P, layers, K, idx=c.idx, momentum=0.1)
        c.order = [f"bn{i}" for i in range(1, len(layers))]
        c.stats = dgcnn_train_ref.flat_stats(c.train["batch_stats"], c.order)
        cache[(name, N, K)] = c
    return cache[(name, N, K)]


def edgeconv(fx, hold, name, entry, N=64, K=4, without=(), null_inputs=()):
    """EdgeConv [3, 32, 64, 64] and [64, 128, 256] at N = 64, B = 2, K = 4 (or the N and K given): X, params_dev, a given idx,
    out, gout, the batch statistics and every output offset.  `without`: optional outputs passed as NULL.  `null_inputs`: of
    "idx" and "out", the adjoints' optional inputs passed as NULL (the search runs again; the forward runs first, into the
    workspace)."""
    import dgcnn_train_ref
    import edgeconv_bwd_ref
    import edgeconv_grad_train_ref
    import edgeconv_pgrad_ref
    c = _edgeconv_case(fx, name, N, K)
    L, nl, B = c.lc, len(c.layers), c.B
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
                 [I("params", c.params), I("x", c.X), I("idx", c.idx), O("out", (cL, N, B)), O("stats", (ns.value,))] + _but([O("running", (ns.value,))], without), nb)
        _flat_same(r["out"], c.train["out"], "out")
        _flat_same(r["stats"], c.stats, "batch_stats")
        _same_if(r, "running", dgcnn_train_ref.flat_stats(c.train["running"], c.order))
    elif entry == "bwd":
        nb = _ws(fx, "fx3d_edgeconv_bwd_workspace_bytes", L, nl, K, N, B)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edgeconv_bwd")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, p.gout, p.gx, ws, n, None),
                 _but([I("params", c.params), I("x", c.X), I("idx", c.idx), I("out", c.out), I("gout", c.gout)], null_inputs, True) + [O("gx", (F, N, B))], nb)
        _flat_same(r["gx"], edgeconv_bwd_ref.input_grad(c.X, c.P, c.layers, K, c.gout, c.idx, c.out), "gx")
    elif entry == "grad":
        nb = _ws(fx, "fx3d_edgeconv_grad_workspace_bytes", L, nl, K, N, B)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edgeconv_grad")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, p.gout, p.gparams, p.gx, ws, n, None),
                 _but([I("params", c.params), I("x", c.X), I("idx", c.idx), I("out", c.out), I("gout", c.gout)], null_inputs, True) + [O("gparams", (np_,))]
                 + _but([O("gx", (F, N, B))], without), nb)
        G, gx = edgeconv_pgrad_ref.grad(c.X, c.P, c.layers, K, c.gout, c.idx, c.out)
        _flat_same(r["gparams"], edgeconv_pgrad_ref.flat(G, c.layers), "gparams")
        _same_if(r, "gx", gx)
    else:
        out = np.asfortranarray(c.train["out"], dtype=np.float32)
        nb = _ws(fx, "fx3d_edgeconv_grad_train_workspace_bytes", L, nl, K, N, B)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_edgeconv_grad_train")(p.params, L, nl, K, p.x, N, B, p.idx, p.out, p.stats, p.gout, p.gparams, p.gx,
                                                                           ws, n, None),
                 _but([I("params", c.params), I("x", c.X), I("idx", c.idx), I("out", out), I("stats", c.stats), I("gout", c.gout)], null_inputs, True)
                 + [O("gparams", (np_,))] + _but([O("gx", (F, N, B))], without), nb)
        G, gx = edgeconv_grad_train_ref.grad(c.X, c.P, c.layers, K, c.gout, c.train["batch_stats"], c.idx, out)
        _flat_same(r["gparams"], edgeconv_pgrad_ref.flat(G, c.layers), "gparams")
        _same_if(r, "gx", gx)


def _dgcnn_case(fx, N=64, K=10):
    cache = _dgcnn_case.__dict__.setdefault("c", {})
    if (N, K) not in cache:
        import dgcnn_ref
        B, nc = 2, 10
        P = dgcnn_ref.random_params(nc, seed=3)
        m = fx.DGCNN(nc, K, npoints=N).load(P)
        d4, d5 = m.dropout_masks(B, 7)
        c = SimpleNamespace(N=N, B=B, K=K, nc=nc, P=P, params=m.flat_params(), X=_randn((3, N, B), 27 + N), glogits=_randn((nc, B), 28 + N),
                            d4=np.asfortranarray(d4, dtype=np.float32), d5=np.asfortranarray(d5, dtype=np.float32))
        n = C.c_int64(0)
        fx._lib.call("fx3d_dgcnn_stat_count", C.byref(n))
        c.nstat = n.value
        c.fwd = dgcnn_ref.forward(c.X, P, K)
        cache[(N, K)] = c
    return cache[(N, K)]


def dgcnn(fx, hold, entry, N=64, K=10, without=(), null_inputs=()):
    """DGCNN at 2 x 64, K = 10 (or the N and K given).  x1 is the one array argument the header asks 16-byte alignment for (the
    forward entry points write it with 16-byte stores): it stays aligned, and a misaligned x1 is refused before any launch.
    `without`: optional outputs passed as NULL."""
    import dgcnn_grad_ref
    import dgcnn_grad_train_ref
    import dgcnn_train_ref
    c = _dgcnn_case(fx, N, K)
    B, nc = c.B, c.nc
    outs = [O("probs", (nc, B)), O("logits", (nc, B)), O("idx1", (K, N, B), np.int32), O("x1", (64, N, B)), O("idx2", (K, N, B), np.int32),
            O("x2", (256, N, B)), O("pooled", (1024, B))]
    bitwise = ("logits", "x1", "x2", "pooled")
    if entry == "forward":
        nb = _ws(fx, "fx3d_dgcnn_workspace_bytes", N, B, K, nc)
        call = lambda p, ws, n: _abi(fx, "fx3d_dgcnn_forward")(p.params, nc, K, p.x, N, B, p.probs, p.logits, p.idx1, p.x1, p.idx2, p.x2, p.pooled,  # noqa: E731
                                                               ws, n, None)
        r = hold(fx, call, [I("params", c.params), I("x", c.X)] + _but(outs, without), nb, skip=("x1",))
        want = c.fwd
        pd, xd, probs, x1 = fx.gpu(c.params), fx.gpu(c.X), fx.DeviceArray.empty((nc, B)), fx.DeviceArray.empty((64 * N * B + 4,))
        ws = fx.DeviceArray.empty((nb,), np.uint8)
        rc = fx._lib.load().fx3d_dgcnn_forward(pd.ptr, nc, K, xd.ptr, N, B, probs.ptr, None, None, x1.ptr + 4, None, None, None, ws.ptr, nb, None)
        assert rc == -1 and "x1" in fx._lib.last_error()
    elif entry == "forward_train":
        nb = _ws(fx, "fx3d_dgcnn_train_workspace_bytes", N, B, K, nc)
        call = lambda p, ws, n: _abi(fx, "fx3d_dgcnn_forward_train")(p.params, nc, K, p.x, N, B, p.d4, p.d5, 0.1, p.probs, p.logits, p.idx1, p.x1,  # noqa: E731
                                                                     p.idx2, p.x2, p.pooled, p.stats, p.running, ws, n, None)
        r = hold(fx, call, [I("params", c.params), I("x", c.X), I("d4", c.d4), I("d5", c.d5)] + _but(outs + [O("stats", (c.nstat,)), O("running", (c.nstat,))], without),
                 nb, skip=("x1",))
        want = dgcnn_train_ref.forward_train(c.X, c.P, K, dropout=(c.d4, c.d5), momentum=0.1)
        _flat_same(r["stats"], dgcnn_train_ref.flat_stats(want["batch_stats"]), "batch_stats")
        _same_if(r, "running", dgcnn_train_ref.flat_stats(want["running"]))
    if entry.startswith("forward"):
        for k in ("idx1", "idx2"):
            assert (k in r or k in NULLABLE) and (k not in r or np.array_equal(r[k], want[k])), k
        for k in bitwise:
            _same_if(r, k, want[k])
        if without:   # probs has no restatement of its own: with the optional outputs left out it is the full call's bits
            return r
        return
    if entry == "grad_train":
        f = dgcnn_train_ref.forward_train(c.X, c.P, K, dropout=(c.d4, c.d5), momentum=0.1)
        stats = dgcnn_train_ref.flat_stats(f["batch_stats"])
        nb = _ws(fx, "fx3d_dgcnn_grad_train_workspace_bytes", N, B, K, nc)
        arrs = [I("params", c.params), I("x", c.X), I("d4", c.d4), I("d5", c.d5), I("idx1", f["idx1"], np.int32), I("x1", f["x1"], np.float32),
                I("idx2", f["idx2"], np.int32), I("x2", f["x2"], np.float32), I("pooled", f["pooled"], np.float32), I("stats", stats),
                I("glogits", c.glogits), O("gparams", (c.params.size,))] + _but([O("gx", (3, N, B)), O("gx2", (256, N, B)), O("gx1", (64, N, B))], without)
        r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_dgcnn_grad_train")(p.params, nc, K, p.x, N, B, p.d4, p.d5, p.idx1, p.x1, p.idx2, p.x2, p.pooled,
                                                                        p.stats, p.glogits, p.gparams, p.gx, p.gx2, p.gx1, ws, n, None), arrs, nb)
        grads, gx, gx2, gx1 = dgcnn_grad_train_ref.grad_train(c.X, c.P, K, c.glogits, f, (c.d4, c.d5))
        _flat_same(r["gparams"], dgcnn_grad_ref.flat(grads), "gparams")
        for k, w in (("gx", gx), ("gx2", gx2), ("gx1", gx1)):
            _same_if(r, k, w)
        return
    f = c.fwd
    nb = _ws(fx, "fx3d_dgcnn_grad_workspace_bytes", N, B, K, nc)
    arrs = [I("params", c.params), I("x", c.X), I("idx1", f["idx1"], np.int32), I("x1", f["x1"], np.float32), I("idx2", f["idx2"], np.int32),
            I("x2", f["x2"], np.float32), I("pooled", f["pooled"], np.float32), I("glogits", c.glogits)]
    # (`null_inputs`: idx1, x1, idx2, x2, pooled all five -- fx3d_dgcnn_grad then runs the forward first, into the workspace)
    arrs = _but(arrs, null_inputs, True) + [O("gparams", (c.params.size,))]
    arrs += _but([O("gx", (3, N, B)), O("gx2", (256, N, B)), O("gx1", (64, N, B))], without)
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_dgcnn_grad")(p.params, nc, K, p.x, N, B, p.idx1, p.x1, p.idx2, p.x2, p.pooled, p.glogits, p.gparams, p.gx,
                                                              p.gx2, p.gx1, ws, n, None), arrs, nb)
    grads, gx, gx2, gx1 = dgcnn_grad_ref.grad(c.X, c.P, K, c.glogits, f)
    _flat_same(r["gparams"], dgcnn_grad_ref.flat(grads), "gparams")
    for k, w in (("gx", gx), ("gx2", gx2), ("gx1", gx1)):
        _same_if(r, k, w)


# ------------------------------------------------------- chamfer: sums -> finalize(_many), pairwise loss, the sharded entry points
def chamfer_sums_and_finalize(fx, oracle, fx_option, hold, shape):
    """fx3d_chamfer_sums, then fx3d_chamfer_finalize of its sums and fx3d_chamfer_finalize_many of two evaluations' sums."""
    N, M, B, D, opts, _, _ = {**NN_SHAPES, **NN_RAGGED}[shape]
    for k, v in opts.items():
        fx_option(k, v)
    x, y = _rand((D, N, B), 11 * N + B + D), _rand((D, M, B), 13 * M + B + D)
    ox, oy = _nn_reference(oracle, shape, x, y, {**NN_SHAPES, **NN_RAGGED}[shape][6])[:2]
    w1, w2 = 0.7, 1.3
    oloss, _, _, osums = oracle.chamfer_distance(x, y, w1, w2, return_all=True)
    nb = _ws(fx, "fx3d_chamfer_workspace_bytes", N, M, B, D)
    arrs = [I("x", x), I("y", y), O("sums", (2, 2), np.float64), O("idx_x", (N, B), np.int32), O("idx_y", (M, B), np.int32), O("loss", (1,)),
            O("losses", (2,))]

    def call(p, ws, n):
        _abi(fx, "fx3d_chamfer_sums")(p.x, N, p.y, M, B, D, p.sums, p.idx_x, p.idx_y, ws, n, None)
        _abi(fx, "fx3d_chamfer_sums")(p.x, N, p.y, M, B, D, p.sums + 16, None, None, ws, n, None)
        _abi(fx, "fx3d_chamfer_finalize")(p.sums, N, M, B, D, w1, w2, p.loss, None)
        _abi(fx, "fx3d_chamfer_finalize_many")(p.sums, 2, N, M, B, D, w1, w2, p.losses, None)
    r = hold(fx, call, arrs, nb)
    assert np.array_equal(r["idx_x"], ox) and np.array_equal(r["idx_y"], oy)
    # (device: the Float64 sum of the Float32 distances; oracle: of the squares -- test_gpu_hardening's bound)
    assert np.allclose(r["sums"][:, 0], osums, rtol=1e-7, atol=0) and _bits_equal(r["sums"][:, 0], r["sums"][:, 1])
    assert np.isclose(r["loss"][0], oloss, rtol=LOSS_RTOL, atol=0)
    assert r["losses"][0] == r["loss"][0] and r["losses"][1] == r["loss"][0]


def chamfer_pairwise(fx, oracle, hold, N=1024, M=1024, B=2, D=3):
    """fx3d_chamfer_loss_pairwise_f32: the reference's Float32 pairwise mean, bit for bit the oracle's."""
    x, y = _rand((D, N, B), 3 * N + 1), _rand((D, M, B), 3 * M + 2)
    ox, oy = oracle.nn1(x, y)
    want = oracle.chamfer_loss_pairwise(x, y, ox, oy, 0.7, 1.3)
    nb = _ws(fx, "fx3d_chamfer_pairwise_workspace_bytes", N, M, B, D)
    arrs = [I("x", x), I("y", y), I("idx_x", ox), I("idx_y", oy), O("loss", (1,))]
    r = hold(fx, lambda p, ws, n: _abi(fx, "fx3d_chamfer_loss_pairwise_f32")(p.x, N, p.y, M, B, D, p.idx_x, p.idx_y, 0.7, 1.3, p.loss, None, ws, n, None),
             arrs, nb)
    assert r["loss"][0] == np.float32(want), (r["loss"][0], want)


_COMM = []


def _comm(fx):
    """A communicator of world size 1 (fx3d_comm_bootstrap: no rendezvous traffic), one per process."""
    if not _COMM:
        from flux3d_jl_amd.distributed import NativeComm
        _COMM.append(NativeComm(0, 1))
    return _COMM[0]


def chamfer_sharded(fx, oracle, hold, entry, N=1024, M=1024, B=2, D=3):
    """fx3d_chamfer_fwd_sharded / _sharded_async at world size 1: the all-reduce of one rank's sums is those sums."""
    comm = _comm(fx)
    x, y = _rand((D, N, B), 5 * N + 1), _rand((D, M, B), 5 * M + 2)
    w1, w2 = 0.7, 1.3
    oloss, _, _, osums = oracle.chamfer_distance(x, y, w1, w2, return_all=True)
    nb = _ws(fx, "fx3d_chamfer_workspace_bytes", N, M, B, D)
    arrs = [I("x", x), I("y", y), O("sums", (2,), np.float64), O("loss", (1,))]
    if entry == "fx3d_chamfer_fwd_sharded":
        def call(p, ws, n):
            _abi(fx, entry)(comm.handle, p.x, N, p.y, M, B, D, B, w1, w2, p.sums, p.loss, None, ws, n, None)
    else:
        keep = _COMM[1:] or [fx.Stream.create(), fx.Stream.create(), fx.Event(), fx.Event()]
        _COMM[1:] = keep
        s, cs, ready, done = keep

        def call(p, ws, n):
            _abi(fx, entry)(comm.handle, p.x, N, p.y, M, B, D, B, w1, w2, p.sums, p.loss, ws, n, s.handle, cs.handle, ready.handle, done.handle)
            s.synchronize()
            cs.synchronize()
    r = hold(fx, call, arrs, nb)
    assert np.allclose(r["sums"], osums, rtol=1e-7, atol=0)
    assert np.isclose(r["loss"][0], oloss, rtol=LOSS_RTOL, atol=0)


# ------------------------------------------------ the fit iteration's adjoint: fx3d_chamfer_sampled_bwd, _step, _step_reg, draw_pair_reg
def _fit_case(fx, oracle, n, kind="equalv3"):
    """Source batch (three meshes of equal vertex counts, ragged faces), target batch (three ragged meshes), n draws of each by the
    oracle, the oracle's neighbours and chamfer adjoint rows, the vertex -> face tables."""
    cache = _fit_case.__dict__.setdefault("c", {})
    if (n, kind) not in cache:
        from test_gpu_topology import host_vertex_faces
        a, t = _mesh(fx, kind), _mesh(fx, "ragged3")
        c = SimpleNamespace(a=a, t=t, n=n, B=a.B, w1=0.9, w2=1.1, gout=1.5)
        assert a.B == t.B and a.m.verts_aliased and not t.m.verts_aliased
        for side, d, seed in (("sa", a, 21), ("st", t, 22)):
            out, fi, r1, r2 = oracle.sample_points_seeded(d.vp, d.fp, d.flen, n, seed, return_draws=True)
            vfr, vfe = host_vertex_faces(fx._lib, d.fp, d.flen, d.Vmax)
            setattr(c, side, SimpleNamespace(out=out, fi=fi, r1=r1, r2=r2, vfr=vfr, vfe=vfe, seed=seed))
            flag = C.c_int32(0)
            fx._lib.call("fx3d_sample_points_bwd_ordered", d.Fmax, n, C.byref(flag))
            assert flag.value == 1, "the shape no longer takes the ordered (atomic-free) adjoint"
        c.ix, c.iy = oracle.nn1(c.sa.out, c.st.out)
        c.gA, c.gB = oracle.chamfer_bwd(c.sa.out, c.st.out, c.ix, c.iy, c.w1, c.w2, c.gout)
        cache[(n, kind)] = c
    return cache[(n, kind)]


def _side_inputs(tag, d, s):
    return [I("faces" + tag, d.fp), I("fi" + tag, s.fi), I("r1" + tag, s.r1), I("r2" + tag, s.r2), I("vfr" + tag, s.vfr), I("vfe" + tag, s.vfe)]


def chamfer_sampled_bwd(fx, oracle, hold, n=100):
    """fx3d_chamfer_sampled_bwd in the ordered form, both meshes, on top of base gradients: the oracle's chamfer_bwd followed by
    its sample_points_bwd, bit for bit."""
    c = _fit_case(fx, oracle, n)
    a, t, sa, st, B = c.a, c.t, c.sa, c.st, c.B
    base_a, base_t = _randn((3, a.Vmax, B), 41), _randn((3, t.Vmax, B), 42)
    nb = _ws(fx, "fx3d_chamfer_sampled_bwd_workspace_bytes", n, n, B)
    for acc in (0, 1):
        arrs = ([I("x", sa.out), I("y", st.out), I("ix", c.ix), I("iy", c.iy)] + _side_inputs("_a", a, sa) + _side_inputs("_t", t, st)
                + [O("g_a", (3, a.Vmax, B), init=base_a), O("g_t", (3, t.Vmax, B), init=base_t)])
        r = hold(fx, lambda p, ws, nn: _abi(fx, "fx3d_chamfer_sampled_bwd")(
            p.x, n, p.y, n, B, p.ix, p.iy, c.w1, c.w2, c.gout, B, p.faces_a, a.Vmax, a.Fmax, p.fi_a, p.r1_a, p.r2_a, p.g_a,
            p.faces_t, t.Vmax, t.Fmax, p.fi_t, p.r1_t, p.r2_t, p.g_t, acc, p.vfr_a, p.vfe_a, p.vfr_t, p.vfe_t, ws, nn, None), arrs, nb)
        assert _bits_equal(r["g_a"], oracle.sample_points_bwd(a.fp, a.flen, a.Vmax, sa.fi, sa.r1, sa.r2, c.gA, base=base_a if acc else None)), acc
        assert _bits_equal(r["g_t"], oracle.sample_points_bwd(t.fp, t.flen, t.Vmax, st.fi, st.r1, st.r2, c.gB, base=base_t if acc else None)), acc


def _step_state(a, B):
    V = a.Vmax * B
    return (np.asfortranarray(_randn((3, V), 43) * np.float32(1e-3)), np.asfortranarray(_randn((3, V), 44) * np.float32(1e-2)))


def chamfer_sampled_bwd_step(fx, oracle, hold, n=100):
    """fx3d_chamfer_sampled_bwd_step: the ordered adjoint on top of a base gradient, then Momentum and the offset (tests/
    fit_chain_ref.py: momentum_step) and the seed counter, in the gather's launch."""
    import fit_chain_ref as fc
    c = _fit_case(fx, oracle, n)
    a, sa, st, B = c.a, c.sa, c.st, c.B
    rho, eta, inc = 0.9, 0.7, 2
    base_g = _randn((3, a.Vmax, B), 41)
    vel0, x0 = _step_state(a, B)
    nb = _ws(fx, "fx3d_chamfer_sampled_bwd_workspace_bytes", n, n, B)
    arrs = ([I("x", sa.out), I("y", st.out), I("ix", c.ix), I("iy", c.iy), I("verts", a.v)] + _side_inputs("_a", a, sa)
            + [O("g", (3, a.Vmax, B), init=base_g), O("vel", vel0.shape, init=vel0), O("params", x0.shape, init=x0), O("out", x0.shape),
               O("ctr", (1,), np.uint64, init=[5])])
    r = hold(fx, lambda p, ws, nn: _abi(fx, "fx3d_chamfer_sampled_bwd_step")(
        p.x, n, p.y, n, B, p.ix, p.iy, c.w1, c.w2, c.gout, p.faces_a, a.Vmax, a.Fmax, p.fi_a, p.r1_a, p.r2_a, p.g, 1, p.vfr_a, p.vfe_a,
        rho, eta, p.vel, p.params, p.verts, p.out, p.ctr, inc, ws, nn, None), arrs, nb)
    g = oracle.sample_points_bwd(a.fp, a.flen, a.Vmax, sa.fi, sa.r1, sa.r2, c.gA, base=base_g)
    v1, x1, o1 = fc.momentum_step(rho, eta, g.reshape(3, -1, order="F"), vel0, x0, a.v)
    assert _bits_equal(r["g"], g) and _bits_equal(r["vel"], v1) and _bits_equal(r["params"], x1) and _bits_equal(r["out"], o1)
    assert int(r["ctr"][0]) == 5 + inc


def fit_regularisers_as_passengers(fx, oracle, hold, dirty, n=100, kind="equalv3", w_lap=0.1):
    """fx3d_sample_points_cdf_pair -> fx3d_sample_points_draw_pair_reg -> fx3d_chamfer_sampled_bwd_step_reg: the regularisers'
    forward in the draw launch, their adjoint in the launch of the chamfer adjoint's rows.  Four workspaces take part -- the two
    CDFs, the adjoint's, fx3d_mesh_reg.ws (unit rows carried from the draw to the adjoint); `dirty` names the one the driver
    owns ("cdf_a", "cdf_t", "adjoint", "reg"), the others are plain zeroed allocations."""
    import fit_chain_ref as fc
    c = _fit_case(fx, oracle, n, kind)
    a, t, sa, st, B = c.a, c.t, c.sa, c.st, c.B
    rho, eta, inc, target, w_edge = 0.9, 0.7, 2, 0.05, 1.0
    vel0, x0 = _step_state(a, B)
    size = {"cdf_a": _ws(fx, "fx3d_sample_points_workspace_bytes", a.Fmax, B), "cdf_t": _ws(fx, "fx3d_sample_points_workspace_bytes", t.Fmax, B),
            "adjoint": _ws(fx, "fx3d_chamfer_sampled_bwd_workspace_bytes", n, n, B), "reg": _ws(fx, "fx3d_mesh_losses_workspace_bytes", a.V, a.E)}
    plain = {k: fx.DeviceArray.zeros((max(v, 256),), np.uint8) for k, v in size.items() if k != dirty}
    arrs = ([I("verts", a.v), I("faces_a", a.fp), I("flen_a", a.flen), I("verts_t", t.vp), I("faces_t", t.fp), I("flen_t", t.flen),
             I("rowptr", a.rowptr), I("colind", a.colind), I("vals", a.vals), I("edges", a.e), I("ix", c.ix), I("iy", c.iy), I("vfr", sa.vfr),
             I("vfe", sa.vfe), I("chamfer", np.array([0.25], np.float32))]
            + [O("x", (3, n, B)), O("fi", (n, B), np.int32), O("r1", (n, B)), O("r2", (n, B)), O("y", (3, n, B)), O("lap", (1,)), O("edge", (1,)),
               O("total", (1,)), O("g", (3, a.Vmax, B), init=_randn((3, a.Vmax, B), 45)), O("vel", vel0.shape, init=vel0),
               O("params", x0.shape, init=x0), O("out", x0.shape), O("ctr", (1,), np.uint64, init=[5])])

    def call(p, ws, nn):
        w = {k: (ws if k == dirty else plain[k].ptr) for k in size}
        reg = fx._lib.MeshRegStruct(p.verts, a.V, p.rowptr, p.colind, p.vals, p.edges, a.E, target, w_lap, w_edge, p.chamfer, p.lap, p.edge, p.total,
                                    w["reg"], nn if dirty == "reg" else size["reg"])
        nbytes = lambda k: nn if k == dirty else size[k]  # noqa: E731
        _abi(fx, "fx3d_sample_points_cdf_pair")(p.verts, a.Vmax, p.faces_a, a.Fmax, p.flen_a, B, w["cdf_a"], nbytes("cdf_a"),
                                                 p.verts_t, t.Vmax, p.faces_t, t.Fmax, p.flen_t, B, w["cdf_t"], nbytes("cdf_t"), 1e-6, None)
        _abi(fx, "fx3d_sample_points_draw_pair_reg")(p.verts, a.Vmax, p.faces_a, a.Fmax, p.flen_a, B, n, sa.seed, w["cdf_a"], nbytes("cdf_a"), p.x,
                                                      p.fi, p.r1, p.r2, p.verts_t, t.Vmax, p.faces_t, t.Fmax, p.flen_t, B, n, st.seed, w["cdf_t"],
                                                      nbytes("cdf_t"), p.y, None, None, None, None, C.byref(reg), None)
        _abi(fx, "fx3d_chamfer_sampled_bwd_step_reg")(p.x, n, p.y, n, B, p.ix, p.iy, c.w1, c.w2, c.gout, p.faces_a, a.Vmax, a.Fmax, p.fi, p.r1, p.r2,
                                                       p.g, 0, p.vfr, p.vfe, rho, eta, p.vel, p.params, p.verts, p.out, p.ctr, inc, w["adjoint"],
                                                       nbytes("adjoint"), C.byref(reg), None)
    r = hold(fx, call, arrs, size[dirty])
    assert _bits_equal(r["x"], sa.out) and np.array_equal(r["fi"], sa.fi) and _bits_equal(r["r1"], sa.r1) and _bits_equal(r["r2"], sa.r2)
    assert _bits_equal(r["y"], st.out)
    r64, c64, e64 = a.rowptr.astype(np.int64), a.colind.astype(np.int64), a.e.astype(np.int64)
    assert np.isclose(r["lap"][0], oracle.laplacian_loss(a.v, r64, c64, a.vals), rtol=LOSS_RTOL, atol=0)
    assert np.isclose(r["edge"][0], oracle.edge_loss(a.v, e64, target), rtol=LOSS_RTOL, atol=0)
    assert r["total"][0] == np.float32(np.float32(np.float32(0.25) + np.float32(np.float32(w_lap) * r["lap"][0])) + np.float32(np.float32(w_edge) * r["edge"][0]))
    g_reg = (oracle.laplacian_loss_bwd(a.v, r64, c64, a.vals, w_lap * c.gout) + oracle.edge_loss_bwd(a.v, e64, target, w_edge * c.gout)).astype(np.float32)
    g = oracle.sample_points_bwd(a.fp, a.flen, a.Vmax, sa.fi, sa.r1, sa.r2, c.gA, base=np.asfortranarray(g_reg.reshape(3, a.Vmax, B, order="F")))
    v1, x1, o1 = fc.momentum_step(rho, eta, g.reshape(3, -1, order="F"), vel0, x0, a.v)
    assert _bits_equal(r["g"], g) and _bits_equal(r["vel"], v1) and _bits_equal(r["params"], x1) and _bits_equal(r["out"], o1)
    assert int(r["ctr"][0]) == 5 + inc
