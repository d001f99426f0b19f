"""The training step on the device (include/flux3d_hip.h "Training step": fx3d_adam_step, fx3d_crossentropy, fx3d_dropout_mask through
fx.ADAM, fx.PointNet / fx.DGCNN ``train_step`` and ``evaluate``, fx.TrainStepGraph) against the host restatement
tests/train_step_ref.py and the models' restatements, bit for bit (integer views, no element left out) -- all but the loss, whose
log is the device's.  One step is checked stage by stage, every stage on the device's own upstream output."""
import numpy as np
import pytest

import dgcnn_grad_train_ref as dgref
import dgcnn_ref
import dgcnn_train_ref as dtref
import misaligned
import pointnet_grad_train_ref as pgref
import pointnet_ref
import pointnet_train_ref as ptref
import train_step_ref as tsr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
INVALID = -1   # FX3D_ERR_INVALID_ARG (include/flux3d_hip.h)
BLOCK_SPAN = 256 * 4           # elements one block of the float4 form takes per pass
GRID_SPAN = 2048 * BLOCK_SPAN  # ... and the whole grid: one element more and the kernel strides
SPECIAL = np.array([0.0, -0.0, 1e-42, 1e30, -1e30, np.nan], F32)   # (1e-42: a denormal)
HYPER = dict(eta=1e-3, beta=(0.9, 0.999), eps=1e-8)


def _host(v):
    return v.to_host() if hasattr(v, "to_host") else np.asarray(v)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what, any_nan=False):
    """Equal bits, element by element.  ``any_nan`` (the ADAM tests, whose gradients hold a NaN): where the restatement has a NaN
    the device must have a NaN, whichever -- sign and payload of the NaN an operation returns are the machine's choice (IEEE 754
    section 6.2), and the host and the device choose differently."""
    got, want = _host(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    differ = _bits(got).ravel() != _bits(want).ravel()
    if any_nan:
        both = np.isnan(got).ravel() & np.isnan(want).ravel()
        print(f"{what}: {np.count_nonzero(differ & both)} NaNs of other bits")
        differ &= ~both
    bad = np.flatnonzero(differ)
    print(f"{what}: {bad.size} of {got.size} elements differ")
    assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


def _abi():
    from flux3d_jl_amd import _lib
    return _lib


# ---------------------------------------------------------------- ADAM
def _gradient(rng, n, step):
    """Normal draws at scales 1e-6 .. 10 with +0, -0, a denormal, 1e30, -1e30 and a NaN among them (their places move with the step,
    so that a buffer of one element meets most of them)."""
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(F32)
    sp = np.roll(SPECIAL, step)
    at = np.arange(min(n, sp.size)) * max(1, n // 7)
    g[at] = sp[:at.size]
    return g


def _adam_call(n, g, m, v, bp, x, running=None, smap=None):
    return _abi().load().fx3d_adam_step(n, HYPER["eta"], *HYPER["beta"], HYPER["eps"], g.ptr, m.ptr, v.ptr, bp.ptr, x.ptr,
                                        running.ptr if running is not None else None, smap.ptr if smap is not None else None,
                                        0 if running is None else running.size, None)


@pytest.mark.parametrize("n", [1, 3, BLOCK_SPAN - 1, BLOCK_SPAN, BLOCK_SPAN + 1, GRID_SPAN + 1])
def test_adam_five_steps(gpu_fx, n):
    """x, m, v and betap after each of five steps; from three elements on the statistics map hits the first and the last one."""
    fx = gpu_fx
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(F32)
    m, v, bp = np.zeros(n, F32), np.zeros(n, F32), np.array(HYPER["beta"], F64)
    xd, md, vd, bd = fx.gpu(x), fx.gpu(m), fx.gpu(v), fx.gpu(bp)
    smap = np.array([n - 1, 0], np.int32) if n > 1 else None
    sd = None if smap is None else fx.gpu(smap)
    for step in range(5):
        g = _gradient(rng, n, step)
        running = None
        if smap is not None:
            g[smap] = 0  # (a mapped slot has gradient +0)
            running = rng.standard_normal(smap.size).astype(F32)
        assert _adam_call(n, fx.gpu(g), md, vd, bd, xd, None if running is None else fx.gpu(running), sd) == 0
        x, m, v, bp = tsr.adam_step(x, g, m, v, bp, **HYPER, running=running, stat_map=smap)
        for got, want, name in ((xd, x, "x"), (md, m, "m"), (vd, v, "v"), (bd, bp, "betap")):
            _same(got, want, f"n = {n}, step {step + 1}: {name}", any_nan=True)
    assert n < 7 or (np.isnan(x).any() and np.isinf(v).any())   # (the special values took part)


@pytest.mark.parametrize("case", misaligned.cases(["x", "g", "m", "v"]), ids=misaligned.case_id)
def test_adam_on_pointers_aligned_to_four_bytes(gpu_fx, case):
    fx = gpu_fx
    n = BLOCK_SPAN + 5   # a head, whole float4 groups and a tail
    rng = np.random.default_rng(7)
    x, m, v, bp = rng.standard_normal(n).astype(F32), np.zeros(n, F32), np.zeros(n, F32), np.array(HYPER["beta"], F64)
    bd = fx.gpu(bp)
    smap = np.array([n - 1, 0], np.int32)
    for step in range(2):
        g = _gradient(rng, n, step)
        g[smap] = 0
        running = rng.standard_normal(2).astype(F32)
        px, pm, pv = (misaligned.place(fx, a, case[k], output=True) for a, k in ((x, "x"), (m, "m"), (v, "v")))
        pg, pr, ps = misaligned.place(fx, g, case["g"]), misaligned.place(fx, running, 4), misaligned.place(fx, smap, 4)
        assert _adam_call(n, pg.arr, pm.arr, pv.arr, bd, px.arr, pr.arr, ps.arr) == 0
        x, m, v, bp = tsr.adam_step(x, g, m, v, bp, **HYPER, running=running, stat_map=smap)
        for p, want, name in ((px, x, "x"), (pm, m, "m"), (pv, v, "v")):
            _same(p.arr, want, f"{misaligned.case_id(case)}, step {step + 1}: {name}", any_nan=True)
            p.check_pads(name)
        _same(bd, bp, "betap")


def test_adam_through_the_optimiser(gpu_fx):
    fx = gpu_fx
    n = 777
    rng = np.random.default_rng(3)
    x, g = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    opt = fx.ADAM(eta=0.01, beta=(0.8, 0.99), eps=1e-6)
    assert opt.state() == (None, None, None)
    xd = fx.gpu(x)
    assert opt.update(xd, fx.gpu(g)) is xd
    opt.update(xd, fx.gpu(g))
    want = (x, np.zeros(n, F32), np.zeros(n, F32), np.array([0.8, 0.99]))
    for _ in range(2):
        want = tsr.adam_step(want[0], g, *want[1:], eta=0.01, beta=(0.8, 0.99), eps=1e-6)
    for got, w, name in zip((xd,) + opt.state(), want, ("x", "m", "v", "betap")):
        _same(got, w, f"ADAM.update twice: {name}")
    with pytest.raises(ValueError, match="size of x"):
        opt.update(xd, fx.gpu(g[:5]))
    with pytest.raises(ValueError, match="state is for"):
        opt.update(fx.gpu(x[:5]), fx.gpu(g[:5]))
    with pytest.raises(ValueError, match="go together"):
        opt.update(xd, fx.gpu(g), running=fx.gpu(g[:2]))


def test_adam_status_codes(gpu_fx):
    fx = gpu_fx
    n = 8
    x, g, m, v = (fx.gpu(np.zeros(n, F32)) for _ in range(4))
    buf = fx.gpu(np.array([0.9, 0.999, 0.9, 0.999], F64))
    lib = _abi().load()
    off = fx.DeviceArray(buf.ptr + 4, (2,), F64, owned=False, keep=buf)
    assert _adam_call(n, g, m, v, off, x) == INVALID and "8-byte" in _abi().last_error()
    assert _adam_call(-1, g, m, v, buf, x) == INVALID
    for k in range(5):
        ptrs = [a.ptr for a in (g, m, v, buf, x)]
        ptrs[k] = None
        assert lib.fx3d_adam_step(n, 1e-3, 0.9, 0.999, 1e-8, *ptrs, None, None, 0, None) == INVALID, k
    assert lib.fx3d_adam_step(n, 1e-3, 0.9, 0.999, 1e-8, g.ptr, m.ptr, v.ptr, buf.ptr, x.ptr, None, None, 1, None) == INVALID
    assert lib.fx3d_adam_step(n, 1e-3, 0.9, 0.999, 1e-8, g.ptr, m.ptr, v.ptr, buf.ptr, x.ptr, None, None, -1, None) == INVALID
    fx.synchronize()
    _same(buf, np.array([0.9, 0.999, 0.9, 0.999], F64), "betap after the refusals")
    assert _adam_call(0, g, m, v, buf, x) == 0   # no element: betap alone advances
    _same(buf, np.array([0.9 * 0.9, 0.999 * 0.999, 0.9, 0.999], F64), "betap after a step of no element")


# ---------------------------------------------------------------- cross-entropy
def _probs(rng, nc, B):
    z = (3 * rng.standard_normal((nc, B))).astype(F64)
    e = np.exp(z - z.max(axis=0))
    return np.asfortranarray((e / e.sum(axis=0)).astype(F32))


def _crossentropy(fx, probs, labels, offset=4):
    """fx3d_crossentropy on probs between NaN pads and labels between index pads, both at ``offset``: (loss, glogits, counts) on
    the host after the pad checks."""
    nc, B = probs.shape
    pp, pl = misaligned.place(fx, probs, offset), misaligned.place(fx, np.asarray(labels, np.int32), offset)
    pg = misaligned.place(fx, np.zeros((nc, B), F32, order="F"), offset, output=True)
    pc = misaligned.place(fx, np.zeros(2, np.int32), offset, output=True)
    loss = fx.gpu(np.array([-7.0, -7.0], F64))
    rc = _abi().load().fx3d_crossentropy(pp.ptr, pl.ptr, nc, B, pg.ptr, loss.ptr, pc.ptr, None)
    assert rc == 0, _abi().last_error()
    pg.check_pads("glogits")
    pc.check_pads("counts")
    lh = loss.to_host()
    assert lh[1] == -7.0
    return lh[0], pg.to_host(), pc.to_host()


def _check_crossentropy(fx, probs, labels, what):
    probs = np.asfortranarray(probs)
    loss, g, counts = _crossentropy(fx, probs, labels)
    wl, wg, wc = tsr.crossentropy(probs, labels)
    _same(g, wg, f"{what}: glogits")
    assert counts.dtype == np.int32 and list(counts) == list(wc), (what, counts, wc)
    nc, B = probs.shape
    y = np.asarray(labels)
    ok = (y >= 0) & (y < nc)
    with np.errstate(divide="ignore"):
        logp = np.log(probs[y[ok], np.flatnonzero(ok)].astype(F64))
    finite = logp[np.isfinite(logp)]
    bound = (B + 4) * 2.0 ** -53 * (np.abs(finite).max() if finite.size else 0.0)
    print(f"{what}: loss {loss!r}, restatement {wl!r}, difference {abs(loss - wl) if np.isfinite(wl) else 0.0:.3g}, bound {bound:.3g}")
    if np.isfinite(wl):
        assert abs(loss - wl) <= bound, (what, loss, wl, bound)
    else:
        assert (np.isnan(loss) and np.isnan(wl)) or loss == wl, (what, loss, wl)
    return loss, counts


@pytest.mark.parametrize("nc,B", [(1, 2), (10, 2), (40, 3), (10, 300)], ids=str)   # (300: more clouds than the block has threads)
def test_crossentropy_shapes(gpu_fx, nc, B):
    rng = np.random.default_rng(nc * 1000 + B)
    probs = _probs(rng, nc, B)
    _, counts = _check_crossentropy(gpu_fx, probs, rng.integers(0, nc, B), f"{(nc, B)}")
    if B == 300:
        assert 0 < counts[0] < B


def test_crossentropy_special_columns(gpu_fx):
    fx = gpu_fx
    probs = np.array([[0.5, 0.0, 0.25, 0.2, 0.1], [0.5, 1.0, 0.25, 0.3, 0.2], [0.0, 0.0, 0.5, 0.5, 0.7]], F32)
    loss, counts = _check_crossentropy(fx, probs[:, [0, 2, 3, 4]], [1, 2, 2, 2], "a tie for the maximum")
    assert list(counts) == [3, 0] and np.isfinite(loss)   # the tie's first maximum, class 0, is not the label
    loss, counts = _check_crossentropy(fx, probs[:, [0, 2, 3, 4]], [0, 2, 2, 2], "a tie, the label first")
    assert list(counts) == [4, 0]
    loss, counts = _check_crossentropy(fx, probs, [0, 0, 2, 2, 2], "a zero probability at the label")
    assert loss == np.inf and list(counts) == [4, 0]
    loss, counts = _check_crossentropy(fx, probs, [0, -1, 3, 2, 2], "labels -1 and num_classes")
    assert np.isnan(loss) and list(counts) == [3, 2]


def test_crossentropy_status_codes(gpu_fx):
    fx = gpu_fx
    lib = _abi().load()
    probs, labels = fx.gpu(_probs(np.random.default_rng(0), 4, 2)), fx.gpu(np.array([0, 1], np.int32))
    g, loss, counts = fx.DeviceArray.empty((4, 2), F32), fx.gpu(np.zeros(2, F64)), fx.gpu(np.zeros(2, np.int32))
    args = [probs.ptr, labels.ptr, 4, 2, g.ptr, loss.ptr, counts.ptr, None]
    assert lib.fx3d_crossentropy(*args) == 0
    for k in (0, 1, 4, 5, 6):
        bad = list(args)
        bad[k] = None
        assert lib.fx3d_crossentropy(*bad) == INVALID, k
    assert lib.fx3d_crossentropy(probs.ptr, labels.ptr, 4, 0, g.ptr, loss.ptr, counts.ptr, None) == INVALID
    assert lib.fx3d_crossentropy(probs.ptr, labels.ptr, 0, 2, g.ptr, loss.ptr, counts.ptr, None) == INVALID
    assert lib.fx3d_crossentropy(probs.ptr, labels.ptr, 4, 2, g.ptr, loss.ptr + 4, counts.ptr, None) == INVALID
    fx.synchronize()


# ---------------------------------------------------------------- dropout
def _mask(fx, n, p, seed, counter=None, stream_id=0, offset=4):
    out = misaligned.place(fx, np.full(n, 3.0, F32), offset, output=True)
    cd = None if counter is None else fx.gpu(np.array([counter], np.uint64))
    rc = _abi().load().fx3d_dropout_mask(n, p, seed, cd.ptr if cd is not None else None, stream_id, out.ptr, None)
    assert rc == 0, _abi().last_error()
    out.check_pads("dropout mask")
    return out.to_host()


@pytest.mark.parametrize("n", [5, 512, 768])
@pytest.mark.parametrize("p", [0.0, 0.4, 0.5])
def test_dropout_mask(gpu_fx, n, p):
    fx = gpu_fx
    seed = 0x1234_5678_9ABC_DEF0
    one = _mask(fx, n, p, seed, counter=2, stream_id=1)
    _same(one, tsr.dropout_mask(n, p, seed, 2, 1), f"n = {n}, p = {p}")
    _same(_mask(fx, n, p, seed, counter=2, stream_id=1, offset=0), one, "the same (seed, counter) on a 16-byte aligned pointer")
    _same(_mask(fx, n, p, seed + 2, counter=None, stream_id=1), one, "the counter is added to the seed")
    other = _mask(fx, n, p, seed, counter=3, stream_id=1)
    _same(other, tsr.dropout_mask(n, p, seed, 3, 1), "another counter")
    if p == 0:
        assert np.all(one == 1)
    elif n >= 512:
        assert not np.array_equal(one, other) and not np.array_equal(one, _mask(fx, n, p, seed, counter=2, stream_id=0))
        assert np.any(one == 0) and np.any(one == F32(1.0 / (1.0 - p)))


def test_dropout_status_codes(gpu_fx):
    fx = gpu_fx
    lib = _abi().load()
    out = fx.gpu(np.full(8, 3.0, F32))
    assert lib.fx3d_dropout_mask(8, 0.5, 1, None, 0, None, None) == INVALID
    assert lib.fx3d_dropout_mask(-1, 0.5, 1, None, 0, out.ptr, None) == INVALID
    for p in (-0.1, 1.0, float("nan")):
        assert lib.fx3d_dropout_mask(8, p, 1, None, 0, out.ptr, None) == INVALID and "[0, 1)" in _abi().last_error()
    assert lib.fx3d_dropout_mask(8, 0.5, 1, None, -1, out.ptr, None) == INVALID
    assert lib.fx3d_dropout_mask(0, 0.5, 1, None, 0, out.ptr, None) == 0
    fx.synchronize()
    assert np.all(out.to_host() == 3.0)


# ---------------------------------------------------------------- one step, chained
def _flat(model, named):
    return np.concatenate([np.asarray(named[n], F32).ravel(order="F") for n in model._shapes()])


def _models(fx, kind, N, B, K, nc):
    """The model under test and what restates it: (model, forward(X, P, masks), gradient(X, P, glogits, fwd, masks) flat);
    masks: None or the list of the multipliers, one array per Dropout layer."""
    if kind == "pointnet":
        m = fx.PointNet(nc).load(pointnet_ref.random_params(nc, seed=10))

        def forward(X, P, masks):
            r = ptref.forward_train(X, P, None if masks is None else masks[0])
            return r, ptref.flat_stats(r["batch_stats"]), ptref.flat_stats(r["running"])

        def gradient(X, P, glogits, r, masks):
            return _flat(m, pgref.grad_train(X, P, glogits, None if masks is None else masks[0])[0])
    else:
        m = fx.DGCNN(nc, K, N).load(dgcnn_ref.random_params(nc, seed=3))

        def forward(X, P, masks):
            r = dtref.forward_train(X, P, K, masks)
            return r, dtref.flat_stats(r["batch_stats"]), dtref.flat_stats(r["running"])

        def gradient(X, P, glogits, r, masks):
            return _flat(m, dgref.grad_train(X, P, K, glogits, r, masks)[0])
    return m, forward, gradient


# PointNet (N, B, nc); DGCNN: the two smallest rows of tests/test_gpu_dgcnn_grad_train.py's CASES, (N, B, K, nc)
STEP_CASES = [("pointnet", 33, 2, 0, 3), ("pointnet", 65, 3, 0, 10), ("dgcnn", 33, 2, 1, 1), ("dgcnn", 64, 2, 3, 10)]


@pytest.mark.parametrize("kind,N,B,K,nc", STEP_CASES, ids=str)
def test_three_steps_stage_by_stage(gpu_fx, kind, N, B, K, nc):
    """Step 1 without dropout, step 2 under host masks that hold both values, step 3 under masks drawn on the device."""
    fx = gpu_fx
    m, forward, gradient = _models(fx, kind, N, B, K, nc)
    rng = np.random.default_rng(N + B)
    X = np.asfortranarray(rng.standard_normal((3, N, B)).astype(F32))
    labels = rng.integers(0, nc, B)
    xd, opt, smap = fx.gpu(X), fx.ADAM(**HYPER), tsr.stat_map(m)
    rows, p = m._DROPOUT
    host_masks = [np.asfortranarray(tsr.dropout_mask(r * B, p, 99, 0, i).reshape(r, B, order="F")) for i, r in enumerate(rows)]
    assert all(np.any(mk == 0) and np.any(mk != 0) for mk in host_masks)
    counter = fx.gpu(np.array([5], np.uint64))
    state = (np.zeros(m.param_count, F32), np.zeros(m.param_count, F32), np.array(HYPER["beta"], F64))
    for step, dropout in enumerate((None, host_masks if kind == "dgcnn" else host_masks[0], ("device", 4242, counter)), 1):
        P = {k: v.copy() for k, v in m.pull_params().items()}
        out = m.train_step(xd, labels, opt, dropout=dropout, intermediates=True)
        what = f"{kind} {(N, B, K, nc)} step {step}"
        used = None if dropout is None else [_host(mk) for mk in out.dropout]
        if step == 3:
            for i, r in enumerate(rows):
                _same(used[i].ravel(order="F"), tsr.dropout_mask(r * B, p, 4242, 5, i), f"{what}: mask {i} drawn on the device")
        r, bstats, running = forward(X, P, used)
        _same(out.logits, r["logits"], f"{what}: logits")
        _same(out.batch_stats, bstats, f"{what}: batch_stats")
        _same(out.running, running, f"{what}: running")
        probs, glogits = _host(out.probs), _host(out.glogits)
        wl, wg, wc = tsr.crossentropy(probs, labels)
        _same(glogits, wg, f"{what}: glogits")
        bound = (B + 4) * 2.0 ** -53 * np.abs(np.log(probs[labels, np.arange(B)].astype(F64))).max()
        print(f"{what}: loss {float(out)!r}, restatement {wl!r}, bound {bound:.3g}, correct {out.correct}")
        assert out.correct == wc[0] and abs(float(out) - wl) <= bound and float(out.loss) == float(out)
        grad = _host(out.grad)
        _same(grad, gradient(X, P, glogits, r, used), f"{what}: the flat gradient")
        assert not _bits(grad[smap]).any()
        x, mm, vv, bp = tsr.adam_step(_flat(m, P), grad, *state, **HYPER, running=_host(out.running), stat_map=smap)
        state = (mm, vv, bp)
        _same(m._params_dev(), x, f"{what}: the parameters")
        for got, want, name in zip(opt.state(), state, ("m", "v", "betap")):
            _same(got, want, f"{what}: {name}")
        assert m._stale
        _same(m.flat_params(), x, f"{what}: flat_params pulls")
        assert not m._stale
    fresh = type(m)(*((nc,) if kind == "pointnet" else (nc, K, N))).load(m.pull_params())
    _same(m.forward(xd), _host(fresh.forward(xd)), "forward after the steps against a fresh model with the pulled parameters")
    ev = m.evaluate(xd, labels)
    wl, _, wc = tsr.crossentropy(_host(m.forward(xd)), labels)
    assert ev.correct == wc[0] and abs(float(ev) - wl) <= 1e-12 * max(1.0, abs(wl))
    bad = m.evaluate(xd, fx.gpu(np.array([0] * (B - 1) + [nc], np.int32)))
    with pytest.raises(ValueError, match="outside"):
        bad.correct
    assert np.isnan(float(bad))


# ---------------------------------------------------------------- captured graph
@pytest.mark.parametrize("kind,N,B,K,nc", [STEP_CASES[0], STEP_CASES[3]], ids=str)
def test_graph_replays_equal_eager_steps(gpu_fx, kind, N, B, K, nc):
    """The eager first step and three replays against four eager steps of an identical model: parameters, m, v, betap, the dropout
    counter.  That the capture succeeds is the check that a step makes no host round trip."""
    fx = gpu_fx
    rng = np.random.default_rng(17)
    X = np.asfortranarray(rng.standard_normal((3, N, B)).astype(F32))
    labels = rng.integers(0, nc, B)
    a, b = _models(fx, kind, N, B, K, nc)[0], _models(fx, kind, N, B, K, nc)[0]
    start = _flat(a, a.params)
    oa, ob = fx.ADAM(**HYPER), fx.ADAM(**HYPER)
    g = fx.TrainStepGraph(a, oa, X, labels, seed=77)
    for _ in range(3):
        out = g.step()
    g.synchronize()
    xd, counter = fx.gpu(X), fx.gpu(np.zeros(1, np.uint64))
    for _ in range(4):
        eager = b.train_step(xd, labels, ob, dropout=("device", 77, counter))
        _abi().call("fx3d_counter_add", counter.ptr, 1, None)
    assert g.steps == 4
    _same(a._params_dev(), _host(b._params_dev()), "graph against eager: the parameters")
    for got, want, name in zip(oa.state(), ob.state(), ("m", "v", "betap")):
        _same(got, _host(want), f"graph against eager: {name}")
    _same(g.counter, _host(counter), "the dropout counter")
    assert _host(counter)[0] == 4
    assert float(out) == float(eager) and out.correct == eager.correct
    moved = np.count_nonzero(_bits(_host(a._params_dev())) != _bits(start))
    print(f"{moved} of {start.size} parameters moved in four steps")
    assert 2 * moved > start.size


# ---------------------------------------------------------------- learning
def learning_batch():
    """Four clouds of 64 points, two classes: points on the unit sphere, and points on a flat disc."""
    rng = np.random.default_rng(2024)
    X = np.zeros((3, 64, 4), F32, order="F")
    for b in range(4):
        pts = rng.standard_normal((3, 64))
        if b % 2 == 0:
            pts /= np.linalg.norm(pts, axis=0)
        else:
            pts[2] *= 0.02
        X[:, :, b] = pts
    return X, np.array([0, 1, 0, 1])


LEARNING_STEPS = 4   # the smallest S at which the torch float64 loop below has a quarter of its first loss


def test_the_loss_falls(gpu_fx):
    """PointNet(2, seed=0), one fixed batch, no dropout, eta = 1e-3: the loss of step S = 4 is below half the first step's.
    The same loop in torch float64 on the CPU (the network of tests/pointnet_train_torch_eval.py with autograd, torch.optim.Adam,
    the same initial parameters and batch) gives, per step,
        0.7101 0.6779 0.7064 0.1417 0.1385 0.0627 0.0344 0.0940 0.0081 0.0305 0.0084 0.0015 0.0058 0.0024 0.0073 0.0006
    so it is below a quarter of 0.7101 from step 4 on: a factor two of margin."""
    fx = gpu_fx
    X, y = learning_batch()
    m, opt, xd = fx.PointNet(2, seed=0), fx.ADAM(eta=1e-3), fx.gpu(X)
    losses = [float(m.train_step(xd, y, opt)) for _ in range(LEARNING_STEPS)]
    print("losses:", " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < 0.5 * losses[0], losses
