"""The fit_mesh iteration (flux3d_jl_amd/fit.py: loss_dolphin + Momentum, examples/fit_mesh.jl:78-110) composed on the HOST from the
oracle's pieces, with the state carried from one iteration to the next.  TEST INFRASTRUCTURE ONLY, no device.

One iteration i (from 0), state x, v (Float32, (3, sumV)), seed counter c = inc * i (inc = 2):

    mverts = fl(base + x)                                                       the offset mesh (fx3d_lincomb, 1*a + 1*b)
    A  = sample_points_seeded(mverts padded, seed + c)      with its draws      (source)
    Bp = sample_points_seeded(target,        seed + 1 + c)                      (target)
    ix, iy = nn1_allcores(A, Bp)   brute force                                  gA = chamfer_bwd(A, Bp, ix, iy)  (unit weights)
    aliased source (one mesh / equal vertex counts):
        g0 = fl(lap_bwd(w_lap) + edge_bwd(w_edge));  g = sample_points_bwd(draws, gA, base = g0 as (3, V, B))
    ragged source:
        gpad = sample_points_bwd(draws, gA);  g = fl(fl(pack(gpad, verts_len) + lap_bwd) + edge_bwd)
    loss = fl(fl(l1 + fl(w_lap * l2)) + fl(w_edge * l3))                        (l1: the Float64-sum chamfer term of the oracle)
    v' = fl(fl(rho * v) + fl(-eta * g)) ;  x' = fl(x + v') ;  mverts' = fl(base + x') ;  counter' = inc * (i + 1)

The library is built with -ffp-contract=off and the kernels spell every product and sum out, so numpy Float32 array arithmetic
(one rounding per operation) restates the element-wise steps exactly.

``perturb`` (tests of the comparison itself): "swap_seeds", "counter_by_one", "drop_velocity", "pack_vmax"."""
import numpy as np

F32 = np.float32
NN1_THREADS = 16

# the order a mismatch is searched in: the first differing stage of an iteration is the one to look at
STAGES = (("draws", ("fa", "r1", "r2")), ("clouds", ("A", "Bp")), ("indices", ("ix", "iy")), ("gA", ("gA",)), ("g0", ("g0",)),
          ("g", ("g",)), ("v", ("v",)), ("x", ("x",)), ("mverts", ("mverts",)), ("counter", ("counter",)))


def f32(a):
    return np.asfortranarray(np.asarray(a, dtype=F32))


def packed_to_padded(packed, lens, vmax):
    """_packed_to_padded (src/rep/utils.jl:119-139), pad value 0: (3, sumV) -> (3, Vmax, B)."""
    out = np.zeros((3, int(vmax), len(lens)), F32, order="F")
    cur = 0
    for b, n in enumerate(lens):
        out[:, :n, b] = packed[:, cur:cur + n]
        cur += int(n)
    return out


def padded_to_packed(padded, lens):
    """_padded_to_packed (src/rep/utils.jl:159-181): (3, Vmax, B) -> (3, sum(lens)); the columns beyond a mesh's length are dropped."""
    return np.asfortranarray(np.concatenate([padded[:, :int(n), b] for b, n in enumerate(lens)], axis=1))


def mesh_host(m):
    """Everything the chain reads of a TriMesh, through its host accessors (0-based indices, int64 where the oracle wants them)."""
    rp, ci, va = m.get_laplacian_packed()
    return dict(faces_padded0=np.asfortranarray(m.get_faces_padded().astype(np.int64) - 1),
                faces_len=np.asarray(m._faces_len, np.int64).copy(), verts_len=np.asarray(m._verts_len, np.int64).copy(),
                V=int(m.V), N=int(m.N), base=f32(m.get_verts_packed_host()).copy(order="F"),
                verts_padded=f32(m.get_verts_padded_host()).copy(order="F"),
                edges0=np.ascontiguousarray(m.get_edges_packed().astype(np.int64) - 1),
                rowptr=rp.astype(np.int64), colind=ci.astype(np.int64), vals=np.asarray(va, F32))


def momentum_step(rho, eta, g, v, x, base=None):
    """Flux.Optimise.Momentum, unfused Float32 (csrc/mesh_update.hip): returns (v', x') or (v', x', fl(base + x'))."""
    with np.errstate(all="ignore"):
        vn = (F32(rho) * v) + ((-F32(eta)) * g)
        xn = x + vn
        assert vn.dtype == F32 and xn.dtype == F32
        return (vn, xn) if base is None else (vn, xn, base + xn)


def lincomb(a, x, b, y, c=0.0, z=None):
    """fx3d_lincomb: fl(fl(a*x) + fl(b*y)) (+ fl(c*z))."""
    with np.errstate(all="ignore"):
        out = (F32(a) * x) + (F32(b) * y)
        if z is not None:
            out = out + (F32(c) * z)
        assert out.dtype == F32
        return out


def chamfer_term(A, Bp, ix, iy):
    """The chamfer loss from given indices as the oracle's forward defines it (Float32 squares, Float64 sums, one rounding per
    direction, unit weights): fl(fl(1 * dA) + fl(1 * dB))."""
    out = []
    for p, q, idx in ((A, Bp, ix), (Bp, A, iy)):
        D, R, B = p.shape
        s = 0.0
        for b in range(B):
            t = p[:, :, b] - q[:, idx[:, b], b]
            s += float(np.sum((t * t).astype(np.float64)))
        out.append(F32(F32(s / (float(D) * R * B)) * F32(3.0)))
    return F32(F32(F32(1.0) * out[0]) + F32(F32(1.0) * out[1]))


def total_loss(l1, l2, l3, w_lap, w_edge):
    return F32(F32(F32(l1) + F32(F32(w_lap) * F32(l2))) + F32(F32(w_edge) * F32(l3)))


class Step(dict):
    """One iteration's record: the stages as items and as attributes."""
    __getattr__ = dict.__getitem__


class FitChain:
    def __init__(self, oracle, src, tgt, n, seed, w_lap=0.1, w_edge=1.0, rho=0.9, eta=1.0, x0=None, v0=None, perturb=None):
        """``src`` / ``tgt``: :func:`mesh_host` dicts."""
        assert perturb in (None, "swap_seeds", "counter_by_one", "drop_velocity", "pack_vmax")
        self.o, self.src, self.tgt, self.n, self.seed = oracle, src, tgt, int(n), int(seed)
        self.w_lap, self.w_edge, self.rho, self.eta, self.perturb = w_lap, w_edge, rho, eta, perturb
        self.aliased = bool(np.all(src["verts_len"] == src["V"]))
        shape = src["base"].shape
        self.x = np.zeros(shape, F32, order="F") if x0 is None else f32(x0).copy(order="F")
        self.v = np.zeros(shape, F32, order="F") if v0 is None else f32(v0).copy(order="F")
        assert self.x.shape == shape and self.v.shape == shape
        self.i = 0
        self.counter = 0
        self.inc = 1 if perturb == "counter_by_one" else 2

    def gradient(self, x):
        """Loss, gradient and every stage of the iteration at offsets ``x`` with the current seed counter (no state change)."""
        o, s, t, n = self.o, self.src, self.tgt, self.n
        mverts = np.asfortranarray(s["base"] + f32(x))
        sa, sb = self.seed + self.counter, self.seed + 1 + self.counter
        if self.perturb == "swap_seeds":
            sa, sb = sb, sa
        vp = packed_to_padded(mverts, s["verts_len"], s["V"])
        A, fa, r1, r2 = o.sample_points_seeded(vp, s["faces_padded0"], s["faces_len"], n, sa, return_draws=True)
        Bp = o.sample_points_seeded(t["verts_padded"], t["faces_padded0"], t["faces_len"], n, sb)
        ix, iy, _ = o.nn1_allcores(A, Bp, threads=NN1_THREADS)
        gA, _ = o.chamfer_bwd(A, Bp, ix, iy)
        glap = o.laplacian_loss_bwd(mverts, s["rowptr"], s["colind"], s["vals"], self.w_lap)
        gedge = o.edge_loss_bwd(mverts, s["edges0"], 0.0, self.w_edge)
        if self.aliased:
            g0 = np.asfortranarray(glap + gedge)
            assert g0.dtype == F32
            g = o.sample_points_bwd(s["faces_padded0"], s["faces_len"], s["V"], fa, r1, r2, gA,
                                    base=g0.reshape((3, s["V"], s["N"]), order="F"))
            g = np.asfortranarray(g.reshape((3, s["V"] * s["N"]), order="F"))
        else:
            g0 = None
            gpad = o.sample_points_bwd(s["faces_padded0"], s["faces_len"], s["V"], fa, r1, r2, gA)
            lens = s["verts_len"]
            if self.perturb == "pack_vmax":  # Vmax columns per mesh (padding included), cut to the packed buffer's size
                gp = padded_to_packed(gpad, [s["V"]] * s["N"])[:, :int(lens.sum())]
            else:
                gp = padded_to_packed(gpad, lens)
            g = np.asfortranarray((gp + glap) + gedge)
            assert g.dtype == F32
        l1 = chamfer_term(A, Bp, ix, iy)
        l2 = o.laplacian_loss(mverts, s["rowptr"], s["colind"], s["vals"])
        l3 = o.edge_loss(mverts, s["edges0"], 0.0)
        return Step(seed_a=sa, seed_b=sb, mverts_in=mverts, fa=fa, r1=r1, r2=r2, A=A, Bp=Bp, ix=ix, iy=iy, gA=gA, g0=g0, g=g,
                    l1=l1, l2=l2, l3=l3, loss=total_loss(l1, l2, l3, self.w_lap, self.w_edge))

    def step(self):
        """One iteration: the record of :meth:`gradient` plus the new x, v, mverts and the seed counter inc * (i + 1)."""
        r = self.gradient(self.x)
        v = np.zeros_like(self.v) if self.perturb == "drop_velocity" else self.v
        vn, xn, mv = momentum_step(self.rho, self.eta, r.g, v, self.x, self.src["base"])
        self.v, self.x = np.asfortranarray(vn), np.asfortranarray(xn)
        self.i += 1
        self.counter = self.inc * self.i
        r.update(v=self.v.copy(order="F"), x=self.x.copy(order="F"), mverts=np.asfortranarray(mv), counter=self.counter, iteration=self.i)
        return r

    def run(self, iterations):
        return [self.step() for _ in range(iterations)]


# ---------------------------------------------------------------------------------------------------------------- the cases
CASES = {  # name: (sources, targets, n, iterations compared, eta, rho, seed)
    "one": (1, 1, 5000, 6, 1.0, 0.9, 4242),       # the tutorial's: sphere -> teapot, 5000 draws (the split nn1 plan)
    "equal3": (3, 3, 1500, 6, 0.7, 0.9, 77),      # aliased sources (equal vertex counts), ragged targets
    "ragged2": (2, 2, 1500, 6, 0.7, 0.9, 1001),   # ragged sources: fit.py's last branch, the unfused FitStepGraph body
    "equal8": (8, 8, 5000, 3, 1.0, 0.9, 0x5EED0C3),  # BASELINE configs[2]: eight teapots, 5000 draws
}


def build_case(fx, golden, name):
    """Host meshes and the start offsets of a case: (src TriMesh, tgt TriMesh, x0 (3, sumV) Float32).  Targets are normalised as the
    fit tests do ((v - mean) / std, the tutorial's); both committed meshes, teapot (2256 faces) and sphere (2562 vertices, 5120 faces)."""
    import os
    sv, sf = fx.load_obj(os.path.join(golden, "sphere.obj"))
    tv, tf = fx.load_obj(os.path.join(golden, "teapot.obj"))
    tv = (tv - tv.mean(1, keepdims=True)) / tv.std()
    sv, tv = f32(sv), f32(tv)
    rng = np.random.default_rng(sum(map(ord, name)))

    def scaled(v, s):
        return f32(v * F32(s))
    if name == "one":
        src, tgt, x0 = ([sv], [sf]), ([tv], [tf]), None
    elif name == "equal3":
        src, tgt = ([sv] * 3, [sf] * 3), ([tv, scaled(sv, 1.3), scaled(tv, 0.5)], [tf, sf, tf])
        x0 = rng.standard_normal((3, 3 * sv.shape[1])) * 5e-3
    elif name == "ragged2":
        src, tgt = ([tv, sv], [tf, sf]), ([sv, tv], [sf, tf])
        x0 = rng.standard_normal((3, tv.shape[1] + sv.shape[1])) * 5e-3
    elif name == "equal8":
        src = ([tv] * 8, [tf] * 8)
        tgt = ([scaled(tv, 0.8 + 0.05 * b) for b in range(8)], [tf] * 8)
        x0 = rng.standard_normal((3, 8 * tv.shape[1])) * 1e-2
    else:
        raise KeyError(name)
    ms, mt = fx.TriMesh(*src), fx.TriMesh(*tgt)
    x0 = np.zeros((3, int(ms._verts_len.sum())), F32, order="F") if x0 is None else f32(x0)
    assert ms.N == CASES[name][0] and mt.N == CASES[name][1]
    return ms, mt, x0


def host_chain(oracle, fx, golden, name, n=None, perturb=None):
    ms, mt, x0 = build_case(fx, golden, name)
    _, _, n0, _, eta, rho, seed = CASES[name]
    return FitChain(oracle, mesh_host(ms), mesh_host(mt), n or n0, seed, rho=rho, eta=eta, x0=x0, perturb=perturb)


def _same(a, b):
    if a is None or b is None:
        return True  # a stage the device run does not expose (or the host chain does not have: g0 of a ragged source)
    if np.isscalar(a) or np.isscalar(b) or np.ndim(a) == 0:
        return int(a) == int(b)
    a, b = np.asarray(a), np.asarray(b)
    return a.size == b.size and np.array_equal(a.reshape(-1, order="F"), b.reshape(-1, order="F"))


def first_mismatch(device, host, loss_rtol=None, skip=()):
    """``device`` / ``host``: lists of per-iteration records (dicts holding any of the STAGES' items, 'loss').  Returns None when every
    stage the device records hold is array_equal to the host chain's (and every loss within ``loss_rtol``), else
    (iteration counted from 1, stage name, detail)."""
    for it, (d, h) in enumerate(zip(device, host), start=1):
        for stage, keys in STAGES:
            if stage in skip:
                continue
            for k in keys:
                if not _same(d.get(k), h.get(k)):
                    a, b = d[k], h[k]
                    if np.ndim(a) == 0:
                        return it, stage, f"{k}: device {a} != host {b}"
                    a, b = np.asarray(a).reshape(-1, order="F"), np.asarray(b).reshape(-1, order="F")
                    if a.size != b.size:
                        return it, stage, f"{k}: sizes {a.size} != {b.size}"
                    bad = np.flatnonzero(~((a == b) | ((a != a) & (b != b))))
                    j = int(bad[0])
                    return it, stage, f"{k}: {bad.size} of {a.size} elements differ, first at flat index {j}: device {a[j]!r} host {b[j]!r}"
        if loss_rtol is not None and d.get("loss") is not None:
            if not np.isclose(F32(d["loss"]), h["loss"], rtol=loss_rtol, atol=0):
                return it, "loss", f"device {F32(d['loss'])!r} host {h['loss']!r}"
    return None


def max_loss_deviation(device, host):
    return max(abs(float(d["loss"]) - float(h["loss"])) / abs(float(h["loss"])) for d, h in zip(device, host) if d.get("loss") is not None)
