"""The fit_mesh loop on the device (flux3d_jl_amd/fit.py: loss_dolphin, Momentum, FitStepGraph) held to the host chain of
tests/fit_chain_ref.py -- the oracle's pieces composed into iterations with the state carried --, bit for bit:

(a) the element-wise kernels (fx3d_momentum_step, fx3d_momentum_step_offset, fx3d_lincomb, fx3d_counter_add) against numpy Float32;
(b) one eager iteration in every form (sync, async, the optimiser step in the adjoint's launch, with the folded regularisers);
(c) trajectories of FitStepGraph in every setting and of the plain eager loop, one mesh to ragged batches and eight meshes;
(d) FitStepGraph.resync;  (e) the float-atomic form;  (f) the comparison itself fails on perturbed host chains.

NaN: IEEE 754 leaves the sign and payload of a NaN result open (x86 SSE produces 0xFFC00000 for inf - inf, the GPU 0x7FC00000), so
the uint32 comparisons of (a) map every NaN to one pattern on both sides first; every other value is compared bit for bit."""
import numpy as np
import pytest

import fit_chain_ref as fc
from conftest import GOLDEN
from test_gpu_hardening import LOSS_RTOL

pytestmark = pytest.mark.gpu

F32 = np.float32


# ============================================================================================ (a) element-wise kernels
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, np.inf, -np.inf, np.nan], np.float32)
SIZES = [(1, 0), (255, 0), (256, 0), (257, 0), (257, 1), (257, 2), (1000, 1), (1000, 2), (1048577, 0)]  # (n, mesh_max_blocks)
RHOS, ETAS = (0.0, 0.9, 1.0), (0.0, 0.7, 1.0)


def _bits(a):
    a = np.ascontiguousarray(np.asarray(a, F32).reshape(-1, order="F"))
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def _assert_bits(got, exp, what):
    g, e = _bits(got), _bits(exp)
    assert g.size == e.size, what
    bad = np.flatnonzero(g != e)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} differ, first at {bad[0]}: device 0x{g[bad[0]]:08x} host 0x{e[bad[0]]:08x}"


def _arrays(n, seed, count=4):
    """``count`` Float32 arrays of n normal draws over the decades 1e-30 .. 1e30, with +-0, subnormals, +-inf and NaN in each array at
    places of its own (the other arrays hold ordinary values there) and, from 40 elements on, at common places."""
    rng = np.random.default_rng(seed)
    out = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(F32) for _ in range(count)]
    if n >= 8 * count:
        for j, a in enumerate(out):
            a[8 * j:8 * j + 8] = SPECIALS
    if n >= 8 * count + 8:
        for j, a in enumerate(out):
            a[8 * count:8 * count + 8] = np.roll(SPECIALS, j)
    if n > 300:  # ... and in the last block / beyond the first grid stride
        for j, a in enumerate(out):
            a[n - 8 - 8 * j:n - 8 * j] = SPECIALS
    return out


def _stream():
    from flux3d_jl_amd.device import current_stream
    return current_stream().handle


def _check_momentum(fx, rho, eta, g, v, x, base, what):
    """fx3d_momentum_step and fx3d_momentum_step_offset (counter None / inc 2 twice / inc 0), two steps each so that the velocity
    written by the first is the one the second reads; g and base unchanged."""
    from flux3d_jl_amd import _lib
    n = g.size
    hv1, hx1, hm1 = fc.momentum_step(rho, eta, g, v, x, base)
    hv2, hx2, hm2 = fc.momentum_step(rho, eta, g, hv1, hx1, base)
    dg, dbase = fx.gpu(g), fx.gpu(base)
    dv, dx = fx.gpu(v), fx.gpu(x)
    for k, (hv, hx) in enumerate(((hv1, hx1), (hv2, hx2))):
        _lib.call("fx3d_momentum_step", n, float(rho), float(eta), dg.ptr, dv.ptr, dx.ptr, _stream())
        _assert_bits(dv.to_host(), hv, f"{what} momentum_step v step {k}")
        _assert_bits(dx.to_host(), hx, f"{what} momentum_step x step {k}")
    start = (1 << 32) - 1  # the counter is 64 bits wide: + 2 + 2 carries into the high word
    for ctr0, inc in ((None, 0), (start, 2), (start, 0)):
        dv, dx, dout = fx.gpu(v), fx.gpu(x), fx.gpu(np.full(n, 7.0, F32))
        ctr = None if ctr0 is None else fx.gpu(np.array([ctr0], np.uint64))
        for k, (hv, hx, hm) in enumerate(((hv1, hx1, hm1), (hv2, hx2, hm2))):
            _lib.call("fx3d_momentum_step_offset", n, float(rho), float(eta), dg.ptr, dv.ptr, dx.ptr, dbase.ptr, dout.ptr,
                      ctr.ptr if ctr is not None else None, inc, _stream())
            tag = f"{what} momentum_step_offset(counter {ctr0}, inc {inc}) step {k}"
            _assert_bits(dv.to_host(), hv, tag + " v")
            _assert_bits(dx.to_host(), hx, tag + " x")
            _assert_bits(dout.to_host(), hm, tag + " out")
            if ctr is not None:
                assert int(ctr.to_host()[0]) == ctr0 + inc * (k + 1), tag
    _assert_bits(dg.to_host(), g, what + " g unchanged")
    _assert_bits(dbase.to_host(), base, what + " base unchanged")


@pytest.mark.parametrize("n,cap", SIZES)
def test_momentum_kernels_are_numpy_float32_bit_for_bit(gpu_fx, fx_option, n, cap):
    """v' = fl(fl(rho v) + fl(-eta g)), x' = fl(x + v'), out = fl(base + x'), counter += inc: one element, one 256-thread block and
    either side, the grid-stride loop run more than once (mesh_max_blocks 1 and 2) and one element past the default cap of 4096
    blocks; rho in {0, 0.9, 1} x eta in {0, 0.7, 1} (a kernel that ignored rho, or applied it to g, fails here)."""
    if cap:
        fx_option("mesh_max_blocks", cap)
    g, v, x, base = _arrays(n, 100 + n + cap)
    for rho in RHOS:
        for eta in ETAS:
            _check_momentum(gpu_fx, rho, eta, g, v, x, base, f"n={n} cap={cap} rho={rho} eta={eta}")


def test_momentum_kernels_special_values_one_element(gpu_fx):
    """n = 1: +-0, subnormals, +-inf and NaN in each of g, v, x, base in turn."""
    rng = np.random.default_rng(9)
    for j in range(4):
        for s in SPECIALS:
            arrs = [rng.standard_normal(1).astype(F32) for _ in range(4)]
            arrs[j][0] = s
            for rho, eta in ((0.9, 0.7), (0.0, 1.0), (1.0, 0.0)):
                _check_momentum(gpu_fx, rho, eta, *arrs, f"array {j} special {s!r} rho={rho} eta={eta}")


@pytest.mark.parametrize("n,cap", SIZES)
def test_lincomb_is_numpy_float32_bit_for_bit(gpu_fx, fx_option, n, cap):
    """fx3d_lincomb: fl(fl(a x) + fl(b y)) and its three-term form + fl(c z); a fresh output and ``out`` aliasing ``x``."""
    fx = gpu_fx
    if cap:
        fx_option("mesh_max_blocks", cap)
    x, y, z = _arrays(n, 200 + n + cap, count=3)
    dx, dy, dz = fx.gpu(x), fx.gpu(y), fx.gpu(z)
    for a, b, c in ((1.0, 1.0, 1.0), (0.5, -2.0, 0.3), (0.0, 1.0, 0.0), (0.9, -0.7, -1.0)):
        _assert_bits(fx.lincomb(a, dx, b, dy).to_host(), fc.lincomb(a, x, b, y), f"n={n} cap={cap} {a} x + {b} y")
        _assert_bits(fx.lincomb(a, dx, b, dy, c, dz).to_host(), fc.lincomb(a, x, b, y, c, z), f"n={n} cap={cap} {a} x + {b} y + {c} z")
        al = fx.gpu(x)
        assert fx.lincomb(a, al, b, dy, out=al) is al
        _assert_bits(al.to_host(), fc.lincomb(a, x, b, y), f"n={n} cap={cap} out = x: {a} x + {b} y")
        al = fx.gpu(x)
        fx.lincomb(a, al, b, dy, c, dz, out=al)
        _assert_bits(al.to_host(), fc.lincomb(a, x, b, y, c, z), f"n={n} cap={cap} out = x: {a} x + {b} y + {c} z")
    for d, h, name in ((dx, x, "x"), (dy, y, "y"), (dz, z, "z")):
        _assert_bits(d.to_host(), h, name + " unchanged")


def test_counter_add_values(gpu_fx):
    """fx3d_counter_add: inc in {0, 2} applied twice, across the 32-bit boundary."""
    from flux3d_jl_amd import _lib
    fx = gpu_fx
    for start in (0, (1 << 32) - 1, (1 << 63) + 5):
        for inc in (0, 2):
            ctr = fx.gpu(np.array([start], np.uint64))
            for k in range(2):
                _lib.call("fx3d_counter_add", ctr.ptr, inc, _stream())
                assert int(ctr.to_host()[0]) == start + inc * (k + 1)


def test_momentum_update_carries_the_velocity(gpu_fx):
    """Momentum.update / update_offset / step_args from v = None: the velocity starts at zero and the second update reads the first's."""
    fx = gpu_fx
    g, x, base = _arrays(777, 5, count=3)
    z = np.zeros_like(x)
    hv1, hx1, hm1 = fc.momentum_step(0.9, 0.7, g, z, x, base)
    hv2, hx2, hm2 = fc.momentum_step(0.9, 0.7, g, hv1, hx1, base)
    opt, dx, dg = fx.Momentum(0.7, 0.9), fx.gpu(x), fx.gpu(g)
    assert opt.v is None
    assert opt.update(dx, dg) is dx
    _assert_bits(opt.v.to_host(), hv1, "update 1 v")
    _assert_bits(dx.to_host(), hx1, "update 1 x")
    opt.update(dx, dg)
    _assert_bits(opt.v.to_host(), hv2, "update 2 v")
    _assert_bits(dx.to_host(), hx2, "update 2 x")
    opt, dx, dbase, dout = fx.Momentum(0.7, 0.9), fx.gpu(x), fx.gpu(base), fx.DeviceArray.zeros(x.shape, F32)
    ctr = fx.DeviceArray.zeros((1,), np.uint64)
    opt.update_offset(dx, dg, dbase, dout, ctr, 2)
    opt.update_offset(dx, dg, dbase, dout, ctr, 2)
    for got, exp, what in ((opt.v, hv2, "v"), (dx, hx2, "x"), (dout, hm2, "out")):
        _assert_bits(got.to_host(), exp, "update_offset 2 " + what)
    assert int(ctr.to_host()[0]) == 4
    opt = fx.Momentum(0.7, 0.9)
    st = opt.step_args(dx, dbase, dout, ctr, 2)
    assert st[:2] == (0.9, 0.7) and st[2] is opt.v and np.array_equal(opt.v.to_host(), z)


# ================================================================================================= the cases, shared state
_CASE, _HOST, _DEV = {}, {}, {}


def _case(fx, name):
    if name not in _CASE:
        _CASE[name] = fc.build_case(fx, GOLDEN, name)
    return _CASE[name]


def _host(fx, oracle, name):
    """The host chain's trajectory of a case: computed once per module, shared by every test, never written to."""
    if name not in _HOST:
        ms, mt, x0 = _case(fx, name)
        _, _, n, T, eta, rho, seed = fc.CASES[name]
        _HOST[name] = fc.FitChain(oracle, fc.mesh_host(ms), fc.mesh_host(mt), n, seed, rho=rho, eta=eta, x0=x0).run(T)
    return _HOST[name]


def _device(fx, name):
    """Fresh device meshes, offsets and optimiser of a case; the ordered sampling adjoint must take it (a plan change fails loudly
    here instead of switching the tests below to the atomic form)."""
    ms, mt, x0 = _case(fx, name)
    _, _, n, T, eta, rho, seed = fc.CASES[name]
    src, tgt = fx.gpu(ms), fx.gpu(mt)
    assert fx.sampling_adjoint_is_ordered(src, n), (name, src.F, n)
    assert src.verts_aliased == (name != "ragged2")
    return src, tgt, fx.gpu(x0.copy(order="F")), fx.Momentum(eta, rho), n, T, seed


def _device_stages(fx, src, tgt, x, n, seed_a, seed_b):
    """The stages of an iteration the loop does not hand out, from the same calls loss_dolphin makes."""
    from flux3d_jl_amd.metrics import _chamfer_points
    m = fx.offset(src, x)
    A, Bp, fa, r1, r2 = fx.sample_points_pair(m, tgt, n, seed_a=seed_a, seed_b=seed_b, return_draws_a=True)
    _, ix, iy = _chamfer_points(A, Bp, 1.0, 1.0, return_indices=True)
    gA, _ = fx.chamfer_distance_grad(A, Bp, ix, iy)
    return {k: a.to_host() for k, a in dict(fa=fa, r1=r1, r2=r2, A=A, Bp=Bp, ix=ix, iy=iy, gA=gA).items()}


def _locate(fx, name, host, it):
    """After a trajectory mismatch at iteration ``it``: the eager stages on the device from the HOST chain's state at the start of
    that iteration, compared stage by stage -- names the first stage (draws, clouds, indices, gA, g) that differs, if one does."""
    src, tgt, _, _, n, _, seed = _device(fx, name)
    x0 = _case(fx, name)[2] if it == 1 else host[it - 2]["x"]
    x = fx.gpu(np.asfortranarray(x0))
    d = _device_stages(fx, src, tgt, x, n, seed + 2 * (it - 1), seed + 1 + 2 * (it - 1))
    _, g = fx.loss_dolphin(x, src, tgt, n, seed=seed + 2 * (it - 1), with_grad=True)
    d["g"] = g.to_host()
    bad = fc.first_mismatch([d], [host[it - 1]])
    return "the eager stages from the host state of that iteration agree" if bad is None else f"eager stages from the host state: first differing stage {bad[1]} ({bad[2]})"


def _assert_trajectory(fx, name, device, host, what):
    assert len(device) <= len(host)
    bad = fc.first_mismatch(device, host, loss_rtol=LOSS_RTOL)
    if bad is not None:
        it, stage, detail = bad
        pytest.fail(f"{name} {what}: first mismatch at iteration {it}, stage {stage}: {detail}; {_locate(fx, name, host, it)}")
    dev = fc.max_loss_deviation(device, host)
    equal = all(F32(d["loss"]) == h["loss"] for d, h in zip(device, host))
    print(f"{name} {what}: {len(device)} iterations bit-equal; largest relative loss deviation {dev:.3e} (LOSS_RTOL {LOSS_RTOL}); losses equal: {equal}")


# ================================================================================== (b) one eager iteration in every form
FORMS = [(name, form) for name in fc.CASES for form in ("sync", "async", "step", "step_fold") if name != "ragged2" or form in ("sync", "async")]


@pytest.mark.parametrize("name,form", FORMS)
def test_eager_iteration_is_the_host_chains(gpu_fx, oracle, name, form):
    """loss_dolphin(with_grad=True) at iteration 0 and the optimiser step after it (or in its last launch): draws, clouds, indices, the
    chamfer adjoint's rows, the gradient, v, x, the next offset mesh and the seed counter array_equal to the host chain's first
    step; the loss within LOSS_RTOL (its chamfer term is a Float64 sum in another order).  ragged2 takes fit.py's last branch
    (chamfer_distance_grad -> sample_points_grad -> padded_to_packed_dev -> mesh_losses_grad(out=))."""
    fx = gpu_fx
    host = _host(fx, oracle, name)[:1]
    src, tgt, x, opt, n, _, seed = _device(fx, name)
    base = src.dev("verts_packed")
    rec = {}
    if form == "sync":
        rec.update(_device_stages(fx, src, tgt, x, n, seed, seed + 1))
        loss, g = fx.loss_dolphin(x, src, tgt, n, seed=seed, with_grad=True)
        assert isinstance(loss, np.float32)
        rec.update(g=g.to_host(), loss=loss)
        opt.update(x, g)
    elif form == "async":
        loss, g = fx.loss_dolphin(x, src, tgt, n, seed=seed, with_grad=True, sync=False)
        out, ctr = fx.DeviceArray.zeros(x.shape, F32), fx.DeviceArray.zeros((1,), np.uint64)
        rec.update(g=g.to_host(), loss=F32(loss.item()))
        opt.update_offset(x, g, base, out, ctr, 2)
        rec.update(mverts=out.to_host(), counter=int(ctr.to_host()[0]))
    else:
        out, ctr = fx.DeviceArray.zeros(x.shape, F32), fx.DeviceArray.zeros((1,), np.uint64)
        loss, g = fx.loss_dolphin(x, src, tgt, n, seed=seed, with_grad=True, sync=False,
                                  step=opt.step_args(x, base, out, ctr, 2), fold=(form == "step_fold"))
        rec.update(g=g.to_host(), loss=F32(loss.item()), mverts=out.to_host(), counter=int(ctr.to_host()[0]))
    rec.update(v=opt.v.to_host(), x=x.to_host())
    assert rec["g"].size == 3 * int(src._verts_len.sum())
    assert np.array_equal(base.to_host(), _case(fx, name)[0].get_verts_packed_host())  # the source's own vertices are never written
    _assert_trajectory(fx, name, [rec], host, f"eager {form}")


# ================================================================================================== (c) trajectories
SETTINGS = {"fold": dict(fold=True), "nofold": dict(fold=False), "separate": dict(step_in_launch=False), "default": {}}


def _graph_trajectory(fx, name, setting, ordered=True, iterations=None):
    key = (name, setting, ordered)
    if key not in _DEV:
        src, tgt, x, opt, n, T, seed = _device(fx, name)
        step = fx.FitStepGraph(x, src, tgt, opt, n, seed=seed, ordered=ordered, **SETTINGS[setting])
        recs = []

        def record(loss):
            step.synchronize()
            assert step.iterations == len(recs) + 1
            d = dict(x=x.to_host(), v=opt.v.to_host(), counter=int(step.counter.to_host()[0]), loss=F32(loss.item()))
            if step.mverts is not None:
                d["mverts"] = step.mverts.to_host()
            assert d["counter"] == 2 * step.iterations
            recs.append(d)
        record(step.first_loss)
        for _ in range((iterations or T) - 1):
            record(step.step())
        _DEV[key] = (recs, step.mverts is not None, src.verts_aliased)
    return _DEV[key]


def _eager_trajectory(fx, name):
    key = (name, "eager")
    if key not in _DEV:
        src, tgt, x, opt, n, T, seed = _device(fx, name)
        recs = []
        for it in range(T):
            loss, g = fx.loss_dolphin(x, src, tgt, n, seed=seed + 2 * it, with_grad=True)
            opt.update(x, g)
            recs.append(dict(g=g.to_host(), x=x.to_host(), v=opt.v.to_host(), loss=loss))
        _DEV[key] = recs
    return _DEV[key]


GRAPHS = [(name, s) for name in fc.CASES for s in (("default",) if name == "ragged2" else ("fold", "nofold", "separate"))]


@pytest.mark.parametrize("name,setting", GRAPHS)
def test_fit_step_graph_walks_the_host_chains_trajectory(gpu_fx, oracle, name, setting):
    """FitStepGraph(ordered=True): after the constructor's eager iteration and after every replay x, the velocity, the offset-mesh
    buffer mverts (where the graph keeps one) and the seed counter (2 per iteration) are array_equal to the host chain's step and
    the loss is within LOSS_RTOL: 6 iterations (3 at eight meshes).  ragged2 takes the unfused body (opt.update + fx3d_counter_add,
    mverts is None); the aliased cases run folded (five launches), unfolded (seven) and with the optimiser in a launch of its own."""
    fx = gpu_fx
    host = _host(fx, oracle, name)
    recs, has_mverts, aliased = _graph_trajectory(fx, name, setting)
    assert len(recs) == fc.CASES[name][3]
    assert has_mverts == aliased == (name != "ragged2")
    assert recs[-1]["counter"] == 2 * len(recs)
    _assert_trajectory(fx, name, recs, host, f"FitStepGraph {setting}")


@pytest.mark.parametrize("name", list(fc.CASES))
def test_plain_eager_loop_walks_the_host_chains_trajectory(gpu_fx, oracle, name):
    """loss_dolphin(seed = seed + 2 it) + opt.update: the gradient, x and the velocity of every iteration array_equal to the host
    chain's, hence to FitStepGraph's."""
    fx = gpu_fx
    recs = _eager_trajectory(fx, name)
    assert len(recs) == fc.CASES[name][3]
    _assert_trajectory(fx, name, recs, _host(fx, oracle, name), "eager loop")


# ======================================================================================================= (d) resync
def test_resync_after_an_external_write_to_x(gpu_fx, oracle):
    """Case one: three iterations, a new x written from the host, resync(), two replays = the host chain continued from the new x
    with the velocity and the seed counter kept.  Without resync() the replays still optimise from the old offset mesh (the
    documented contract) and the comparison says so at the first replay after the write."""
    fx = gpu_fx
    name = "one"
    ms, mt, x0 = _case(fx, name)
    _, _, n, _, eta, rho, seed = fc.CASES[name]
    chain = fc.FitChain(oracle, fc.mesh_host(ms), fc.mesh_host(mt), n, seed, rho=rho, eta=eta, x0=x0)
    before = chain.run(3)
    assert fc.first_mismatch(before, _host(fx, oracle, name)) is None
    new_x = fc.f32(np.random.default_rng(4).standard_normal(x0.shape) * 2e-2)
    chain.x = new_x.copy(order="F")
    after = chain.run(2)
    for resync in (True, False):
        src, tgt, x, opt, _, _, _ = _device(fx, name)
        step = fx.FitStepGraph(x, src, tgt, opt, n, seed=seed)
        step.step()
        step.step()
        step.synchronize()
        assert np.array_equal(x.to_host(), before[2]["x"]) and np.array_equal(opt.v.to_host(), before[2]["v"])
        x.copy_(new_x)
        fx.synchronize()
        if resync:
            step.resync()
        recs = []
        for _ in range(2):
            loss = step.step()
            step.synchronize()
            recs.append(dict(v=opt.v.to_host(), x=x.to_host(), mverts=step.mverts.to_host(), counter=int(step.counter.to_host()[0]),
                             loss=F32(loss.item())))
        bad = fc.first_mismatch(recs, after, loss_rtol=LOSS_RTOL)
        if resync:
            assert bad is None, bad
            assert recs[-1]["counter"] == 10
        else:
            assert bad is not None and bad[:2] == (1, "v"), bad


# ================================================================================================ (e) the atomic form
@pytest.mark.parametrize("name", ["one", "equal8"])
def test_fit_step_graph_atomic_form_follows_the_host_chain(gpu_fx, oracle, name):
    """FitStepGraph(ordered=False): sums in arrival order, three iterations within the tolerances
    test_fit_step_graph_matches_eager_loop uses for this form (x: rtol 1e-3, atol 1e-5; losses: 2e-4)."""
    fx = gpu_fx
    host = _host(fx, oracle, name)[:3]
    recs, _, _ = _graph_trajectory(fx, name, "default", ordered=False, iterations=3)
    assert len(recs) == 3
    for it, (d, h) in enumerate(zip(recs, host), start=1):
        assert d["counter"] == h["counter"]
        assert np.allclose(d["x"], h["x"], rtol=1e-3, atol=1e-5), it
        assert np.isclose(d["loss"], h["loss"], rtol=2e-4, atol=0), (it, d["loss"], h["loss"])


# ==================================================================================== (f) the comparison has teeth
@pytest.mark.parametrize("perturb,graph_first,eager_first", [
    ("swap_seeds", (1, "v"), (1, "g")),          # other draws from the first iteration on
    ("counter_by_one", (1, "counter"), (2, "g")),  # the counter itself at once, the draws it seeds one iteration later
    ("drop_velocity", (2, "v"), (2, "v")),       # v0 = 0: the first iteration cannot show it
    ("pack_vmax", (1, "v"), (1, "g")),           # the shorter mesh's padding packed as if it were vertices
])
def test_perturbed_host_chains_fail_the_comparison(gpu_fx, oracle, perturb, graph_first, eager_first):
    """The device trajectories of ragged2 that (c) ran (cached: nothing runs on the device here unless this test runs alone) against
    host chains that are wrong in one way each: the comparison fails at the first iteration the perturbation can show itself in."""
    fx = gpu_fx
    ms, mt, x0 = _case(fx, "ragged2")
    _, _, n, _, eta, rho, seed = fc.CASES["ragged2"]
    bad = fc.FitChain(oracle, fc.mesh_host(ms), fc.mesh_host(mt), n, seed, rho=rho, eta=eta, x0=x0, perturb=perturb).run(2)
    graph, _, _ = _graph_trajectory(fx, "ragged2", "default")
    eager = _eager_trajectory(fx, "ragged2")
    good = _host(fx, oracle, "ragged2")
    assert fc.first_mismatch(graph, good, loss_rtol=LOSS_RTOL) is None and fc.first_mismatch(eager, good, loss_rtol=LOSS_RTOL) is None
    assert fc.first_mismatch(graph, bad, loss_rtol=LOSS_RTOL)[:2] == graph_first
    assert fc.first_mismatch(eager, bad, loss_rtol=LOSS_RTOL)[:2] == eager_first
    if perturb == "counter_by_one":
        assert fc.first_mismatch(graph, bad, loss_rtol=LOSS_RTOL, skip=("counter",))[:2] == (2, "v")
