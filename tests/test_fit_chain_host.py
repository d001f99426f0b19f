"""tests/fit_chain_ref.py (the fit_mesh iteration composed from the oracle's pieces, the reference of tests/test_gpu_fit_chain.py)
checked on the host, no device: its gradient is the gradient of the objective it reports, its Momentum restatement is Float32
arithmetic with one rounding per operation, and it carries its state deterministically."""
import numpy as np
import pytest

import fit_chain_ref as fc
from conftest import GOLDEN

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------- the chain's gradient against a float64 objective
def _objective64(chain, rec):
    """x (3, sumV) float64 -> the objective at FIXED draws and FIXED neighbour indices in numpy float64: barycentric points from
    sqrt(r1) and r2, the mean of squared nearest distances both ways over the batch, + w_lap * laplacian + w_edge * edge."""
    s, t = chain.src, chain.tgt
    base = s["base"].astype(np.float64)
    lens, B, n = s["verts_len"], s["N"], chain.n
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    u = np.sqrt(rec.r1.astype(np.float32)).astype(np.float64)
    v = rec.r2.astype(np.float64)
    w = [1 - u, u * (1 - v), u * v]                                           # (n, B) each
    corner = [np.stack([s["faces_padded0"][c, rec.fa[:, b], b] + offs[b] for b in range(B)], axis=1) for c in range(3)]
    Bp = rec.Bp.astype(np.float64)
    rows = np.repeat(np.arange(len(s["rowptr"]) - 1), np.diff(s["rowptr"]))
    vals = s["vals"].astype(np.float64)
    e0 = s["edges0"]

    def f(x):
        p = base + x
        cham = 0.0
        for b in range(B):
            A = sum(w[c][None, :, b] * p[:, corner[c][:, b]] for c in range(3))  # (3, n)
            cham += ((A - Bp[:, rec.ix[:, b], b]) ** 2).sum() / (n * B) + ((Bp[:, :, b] - A[:, rec.iy[:, b]]) ** 2).sum() / (n * B)
        lv = np.zeros_like(p)
        np.add.at(lv.T, rows, (vals[None, :] * p[:, s["colind"]]).T)
        lap = np.sqrt((lv ** 2).sum(0)).mean()
        edge = ((p[:, e0[:, 0]] - p[:, e0[:, 1]]) ** 2).sum(0).mean()
        return cham + float(F32(chain.w_lap)) * lap + float(F32(chain.w_edge)) * edge
    return f


# |<g, d> - fd(h)| <= K * |fd(h) - fd(h/2)| + R:  a central difference of step h is off the derivative by c h^2 + O(h^4) and the one at
# h/2 by c h^2 / 4, so the first term with K = 4/3 is the discretisation error alone; K = 2 leaves room for the O(h^4) terms.  R is
# the Float32 rounding of the chain: every entry of g is an ordered Float32 sum of at most ~64 terms (a vertex's (face, corner) pairs
# times the draws of a face, plus its Laplacian row and its edges), each formed with a few roundings: 64 eps32 relative to the sum
# of magnitudes, taken here as sum |g_k d_k| (no cancellation inside an entry is assumed beyond what the factor 64 carries).
FD_K = 2.0
FD_R = 64.0


@pytest.mark.parametrize("name", ["one", "ragged2"])
def test_the_host_chain_is_the_gradient_of_the_objective_it_reports(fx, oracle, name):
    """Central differences of the float64 objective along random unit directions against <g, d> of the host chain, for an aliased
    source (sphere -> teapot) and a ragged one (teapot, sphere -> sphere, teapot), 300 draws per mesh, h = 2e-2.
    Measured (h = 2e-2, four directions each): |<g,d> - fd(h)| / |fd(h) - fd(h/2)| = 1.327, 1.337, 1.331, 1.339 (one) and 1.104, 1.332,
    1.336, 1.291 (ragged2) -- the 4/3 of a central difference's discretisation error, so the chain's own Float32 rounding is well
    below it --, with deviations of 4e-9 .. 4.5e-7 on derivatives of 2e-4 .. 1.6e-3; the Float32 allowance R came to 1.0e-7 .. 1.5e-7.
    The float64 objective at x0 equals the chain's Float32 loss to 1e-7 relative (0.40178585 / 0.40178588, 0.36188976 / 0.36188975)."""
    chain = fc.host_chain(oracle, fx, GOLDEN, name, n=300)
    rec = chain.gradient(chain.x)
    f = _objective64(chain, rec)
    x = chain.x.astype(np.float64)
    f0 = f(x)
    print(f"{name}: objective float64 {f0!r} chain loss {rec.loss!r}")
    assert np.isclose(f0, float(rec.loss), rtol=1e-5, atol=0)
    g = rec.g.astype(np.float64)
    assert g.shape == x.shape
    rng = np.random.default_rng(17)
    h = 2e-2
    for k in range(4):
        d = rng.standard_normal(x.shape)
        if k == 3 and name == "ragged2":  # a direction that moves the shorter mesh only: its columns are the first verts_len[0]
            d[:, int(chain.src["verts_len"][0]):] = 0.0
        d /= np.sqrt((d ** 2).sum())
        fd = [(f(x + s * d) - f(x - s * d)) / (2 * s) for s in (h, h / 2)]
        gd = float((g * d).sum())
        dev, disc = abs(gd - fd[0]), abs(fd[0] - fd[1])
        rnd = FD_R * EPS32 * float(np.abs(g * d).sum())
        print(f"{name} dir {k}: <g,d> {gd!r} fd(h) {fd[0]!r} fd(h/2) {fd[1]!r} deviation {dev:.3e} discretisation {disc:.3e} "
              f"ratio {dev / disc:.3f} float32 allowance {rnd:.3e}")
        assert abs(gd) > 1e-4  # a direction the objective does depend on
        assert dev <= FD_K * disc + rnd, (k, dev, disc, rnd)


# ------------------------------------------------------------------------------------------- the Momentum restatement
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, np.inf, -np.inf, np.nan], np.float32)


def _mul1(a, b32):
    """fl(a * b) of a Float32 scalar and a Float32 array with ONE rounding: the product of two Float32 is exact in float64."""
    return (float(F32(a)) * b32.astype(np.float64)).astype(F32)


def _add1(a32, b32):
    """fl(a + b) of two Float32 arrays with ONE rounding.  The float64 sum is exact unless the exponents are more than 29 bits apart
    (TwoSum's error term says which); there the smaller operand is far below half a Float32 ulp of the larger, which is the result."""
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    return np.where(err == 0, s.astype(F32), np.where(np.abs(a) >= np.abs(b), a32, b32)).astype(F32)


def test_momentum_restatement_is_float32_with_one_rounding_per_operation():
    """fc.momentum_step / fc.lincomb on random values over 30 decades: bit-equal to the same expressions evaluated in float64 and
    rounded to Float32 once per operation."""
    rng = np.random.default_rng(3)
    n = 20000

    def draw():
        return (rng.standard_normal(n) * 10.0 ** rng.uniform(-15, 15, n)).astype(F32)
    g, v, x, base = draw(), draw(), draw(), draw()
    for rho in (0.0, 0.9, 1.0):
        for eta in (0.0, 0.7, 1.0):
            vn, xn, mv = fc.momentum_step(rho, eta, g, v, x, base)
            ev = _add1(_mul1(rho, v), _mul1(-F32(eta), g))
            ex = _add1(x, ev)
            em = _add1(base, ex)
            for got, exp in ((vn, ev), (xn, ex), (mv, em)):
                assert got.dtype == F32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (rho, eta)
    out = fc.lincomb(0.5, x, -2.0, g, 0.3, v)
    exp = _add1(_add1(_mul1(0.5, x), _mul1(-2.0, g)), _mul1(0.3, v))
    assert np.array_equal(out.view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(fc.lincomb(0.5, x, -2.0, g).view(np.uint32), _add1(_mul1(0.5, x), _mul1(-2.0, g)).view(np.uint32))


def test_momentum_restatement_special_values():
    """+-0, subnormals, +-inf and NaN in each of g, v, x, base: IEEE results (rho = 0 times inf is NaN, not 0; a subnormal survives
    rho = 1, eta = 0; -0 + 0 = +0), checked against the definition spelled with Python floats."""
    one = np.ones(len(SPECIALS), F32)
    z = np.zeros(len(SPECIALS), F32)
    # g special, eta = 1, rho = 0, v = 0: v' = 0*0 + (-1)*g = -g (0 + -0 = +0 ... ) ; x' = x + v'
    vn, xn, mv = fc.momentum_step(0.0, 1.0, SPECIALS, z, one, one)
    with np.errstate(all="ignore"):
        exp_v = z * F32(0) + (-SPECIALS)
    assert np.array_equal(vn.view(np.uint32)[~np.isnan(vn)], exp_v.view(np.uint32)[~np.isnan(exp_v)]) and np.isnan(vn[-1])
    assert vn[5] == -np.inf and vn[6] == np.inf and xn[5] == -np.inf and mv[6] == np.inf
    assert vn[2] == F32(-1e-45) and vn[2] != 0  # the subnormal is not flushed
    assert xn[0] == 1 and xn[2] == 1            # 1 + tiny
    # v special, rho = 0: 0 * inf = NaN, 0 * NaN = NaN, 0 * subnormal = +-0
    vn, xn = fc.momentum_step(0.0, 0.0, z, SPECIALS, one)
    assert np.isnan(vn[5]) and np.isnan(vn[6]) and np.isnan(vn[7]) and np.isnan(xn[5])
    assert np.all(vn[:5] == 0) and np.all(xn[:5] == 1)
    # rho = 1, eta = 0 keeps v bit for bit (x + (-0 * g): the zero's sign cannot show) where v is not NaN
    vn, xn = fc.momentum_step(1.0, 0.0, one, SPECIALS, z)
    keep = ~np.isnan(SPECIALS)
    assert np.array_equal(vn.view(np.uint32)[keep][2:], SPECIALS.view(np.uint32)[keep][2:])   # (+-0 + -0: +0 / -0)
    assert vn.view(np.uint32)[0] == 0 and vn.view(np.uint32)[1] == 0x80000000                 # 0 + -0 = +0 ; -0 + -0 = -0
    assert np.array_equal(xn[keep], vn[keep])
    # x and base special
    vn, xn, mv = fc.momentum_step(0.9, 0.7, one, one, SPECIALS, SPECIALS)
    step = F32(F32(0.9) * F32(1)) + F32(-F32(0.7) * F32(1))
    assert np.all(vn == step)
    assert xn[5] == np.inf and xn[6] == -np.inf and np.isnan(xn[7]) and np.all(xn[:5] == step)
    assert mv[5] == np.inf and mv[6] == -np.inf and np.isnan(mv[7])
    with np.errstate(all="ignore"):
        vn, xn, mv = fc.momentum_step(0.9, 0.7, z, z, F32([np.inf]), F32([-np.inf]))
    assert xn[0] == np.inf and np.isnan(mv[0])   # inf + -inf


# -------------------------------------------------------------------------------------------------------- three steps
@pytest.mark.parametrize("name", ["one", "ragged2"])
def test_three_steps_of_the_host_chain(fx, oracle, name):
    """Deterministic (two chains walk the same bits), the seed counter is 2 (i + 1), the draws of iteration i are those of seeds
    seed + 2 i / seed + 1 + 2 i, the velocity is carried, and on the ragged case the packed gradient has sum(verts_len) columns."""
    a = fc.host_chain(oracle, fx, GOLDEN, name, n=300)
    b = fc.host_chain(oracle, fx, GOLDEN, name, n=300)
    ra, rb = a.run(3), b.run(3)
    assert fc.first_mismatch(ra, rb, loss_rtol=0.0) is None
    sum_v = int(a.src["verts_len"].sum())
    seed = fc.CASES[name][6]
    for i, r in enumerate(ra):
        assert r.counter == 2 * (i + 1) and r.iteration == i + 1
        assert (r.seed_a, r.seed_b) == (seed + 2 * i, seed + 1 + 2 * i)
        assert r.g.shape == r.x.shape == r.v.shape == r.mverts.shape == (3, sum_v)
        assert r.g.dtype == r.x.dtype == r.v.dtype == r.mverts.dtype == F32 and r.loss.dtype == F32
        assert np.isfinite(r.g).all() and np.isfinite(r.loss)
        assert np.array_equal(r.mverts, a.src["base"] + r.x)
    assert not np.array_equal(ra[0].fa, ra[1].fa) and not np.array_equal(ra[0].Bp, ra[1].Bp)   # fresh draws every iteration
    # iteration 2's velocity is rho * v1 - eta * g2, not -eta * g2
    _, _, _, _, eta, rho, _ = fc.CASES[name]
    assert np.array_equal(ra[1].v, F32(rho) * ra[0].v + (-F32(eta)) * ra[1].g)
    assert not np.array_equal(ra[1].v, (-F32(eta)) * ra[1].g)
    if name == "ragged2":
        assert not a.aliased and ra[0].g0 is None and sum_v < a.src["V"] * a.src["N"]
        # the perturbed packings the device tests use: same shape, different values from the first iteration on
        p = fc.host_chain(oracle, fx, GOLDEN, name, n=300, perturb="pack_vmax").run(1)
        assert p[0].g.shape == (3, sum_v) and fc.first_mismatch(p, ra, loss_rtol=0.0)[:2] == (1, "g")
    else:
        assert a.aliased and ra[0].g0 is not None


@pytest.mark.parametrize("perturb,where", [("swap_seeds", (1, "draws")), ("counter_by_one", (1, "counter")), ("drop_velocity", (2, "v"))])
def test_first_mismatch_names_the_iteration_and_the_stage(fx, oracle, perturb, where):
    good = fc.host_chain(oracle, fx, GOLDEN, "ragged2", n=300).run(2)
    bad = fc.host_chain(oracle, fx, GOLDEN, "ragged2", n=300, perturb=perturb).run(2)
    assert fc.first_mismatch(good, bad, loss_rtol=1e-5)[:2] == where
    if perturb == "counter_by_one":  # without the counter itself: the second iteration's draws
        assert fc.first_mismatch(good, bad, loss_rtol=1e-5, skip=("counter",))[:2] == (2, "draws")
