"""The restatement tests/train_step_ref.py of include/flux3d_hip.h "Training step" against independent references, and the Python
argument checks of the training step that raise before any device call.  No GPU: the device side is held to the restatement bit for
bit in tests/test_gpu_train_step.py."""
import numpy as np
import pytest
import torch

import train_step_ref as tsr

F32, F64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


# ---------------------------------------------------------------- ADAM
def test_adam_float64_against_torch():
    """Every array Float64: five steps agree with torch.optim.Adam in float64 within 1e-11 eta per element (the two differ in where
    the bias corrections are divided in; measured 3.7e-13 eta)."""
    rng = np.random.default_rng(1)
    n, eta = 4096, 1e-3
    x0 = rng.standard_normal(n)
    p = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=eta, betas=(0.9, 0.999), eps=1e-8)
    x, m, v, bp = x0.copy(), np.zeros(n), np.zeros(n), np.array([0.9, 0.999])
    worst = 0.0
    for step in range(5):
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n)  # gradients spanning 1e-6 .. 10
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        x, m, v, bp = tsr.adam_step(x, g, m, v, bp, eta=eta, dtype=F64)
        worst = max(worst, float(np.abs(x - p.detach().numpy()).max()))
        print(f"step {step + 1}: max |x - torch| = {worst / eta:.3g} eta")
        assert worst <= 1e-11 * eta
    assert np.abs(x - x0).max() > eta  # (the steps moved x)


def test_adam_special_values():
    """The mixed-precision form: g = +0 on zero state keeps every bit of x (-0.0 too); g = 1e30 gives v = +Inf and delta = 0; NaN
    propagates; betap after k steps is the running product."""
    x0 = np.array([1.5, -0.0, 0.0, 3e-41, -2.25], F32)  # (3e-41: a denormal)
    z = np.zeros(5, F32)
    x, m, v, bp = tsr.adam_step(x0, z, z, z, [0.9, 0.999])
    assert np.array_equal(_bits(x), _bits(x0)) and not _bits(m).any() and not _bits(v).any()
    g = np.array([1e30, -1e30, np.nan, 1.0, -1e-6], F32)
    x, m, v, _ = tsr.adam_step(x0, g, z, z, [0.9, 0.999])
    assert np.isinf(v[0]) and np.isinf(v[1]) and np.isfinite(m[0]) and m[0] > 9e28 and m[1] < -9e28
    assert _bits(x[0]) == _bits(x0[0]) and _bits(x[1]) == 0  # delta = +0 and -0: (-0.0) - (-0.0) is +0.0
    assert np.isnan(x[2]) and np.isnan(m[2]) and np.isnan(v[2])
    assert x[3] < x0[3] and x[4] > x0[4] and abs(float(x[3]) - float(x0[3]) + 1e-3) < 1e-9  # the first step moves by eta
    bp, want = np.array([0.9, 0.999]), np.array([0.9, 0.999])
    for k in range(7):
        _, _, _, bp = tsr.adam_step(x0, g, z, z, bp)
        want = want * np.array([0.9, 0.999])
        assert np.array_equal(bp, want) and bp.dtype == F64
    assert bp[0] != 0.9 ** 8 or bp[1] != 0.999 ** 8  # (a running product, not a power: they differ in the last bits)
    x, *_ = tsr.adam_step(x0, g, z, z, [0.9, 0.999], running=np.array([7.0, 9.0], F32), stat_map=np.array([4, 0]))
    assert x[4] == 7.0 and x[0] == 9.0


# ---------------------------------------------------------------- cross-entropy
@pytest.mark.parametrize("nc,B", [(1, 2), (10, 2), (40, 3), (10, 300)], ids=str)
def test_crossentropy_against_the_wrapper_and_torch(fx, nc, B):
    rng = np.random.default_rng(nc + B)
    logits = (3 * rng.standard_normal((nc, B))).astype(F32)
    e = np.exp(logits.astype(F64) - logits.astype(F64).max(axis=0))  # (probs: the Float64 softmax rounded to Float32 once)
    probs = np.asfortranarray((e / e.sum(axis=0)).astype(F32))
    y = rng.integers(0, nc, B)
    loss, glogits, counts = tsr.crossentropy(probs, y)
    wloss, wg = fx.PointNet(nc)._crossentropy(probs, y, B)
    assert np.array_equal(_bits(glogits), _bits(wg)) and glogits.dtype == F32
    logp = np.log(probs[y, np.arange(B)].astype(F64))
    bound = (B + 4) * 2.0 ** -53 * np.abs(logp).max()  # one rounding per term and per addition: the two sums differ in order only
    print(f"loss {loss!r} against the wrapper's {wloss!r}: {abs(loss - wloss):.3g}, bound {bound:.3g}")
    assert isinstance(loss, F64) and abs(loss - wloss) <= bound
    assert counts.dtype == np.int32 and counts[0] == np.count_nonzero(np.argmax(probs, axis=0) == y) and counts[1] == 0
    # torch float64 autograd of -mean log softmax at the same logits: glogits within the Float32 rounding of probs (the
    # restatement's input), of the subtraction and of the division
    t = torch.tensor(logits.astype(F64), requires_grad=True)
    tl = -torch.log_softmax(t, dim=0)[torch.tensor(y), torch.arange(B)].mean()
    tl.backward()
    tol = (2.0 ** -24 * 3) * np.maximum(np.abs(probs.astype(F64) - (np.arange(nc)[:, None] == y[None, :])), probs) / B + 2.0 ** -149
    assert np.all(np.abs(glogits.astype(F64) - t.grad.numpy()) <= tol)
    assert abs(loss - float(tl.detach())) <= 2.0 ** -23 + bound # (log of a Float32-rounded probability: relative 2^-24 in p)


def test_crossentropy_edges():
    probs = np.asfortranarray(np.array([[0.5, 0.0, 0.25, 0.2], [0.5, 1.0, 0.25, 0.3], [0.0, 0.0, 0.5, 0.5]], F32))
    loss, g, counts = tsr.crossentropy(probs, [1, 0, 2, 2])  # column 0: a tie, the first maximum (0) is not the label
    assert loss == np.inf and list(counts) == [2, 0]         # column 1: probability 0 at the label
    loss, g, counts = tsr.crossentropy(probs, [0, -1, 3, 2])
    assert np.isnan(loss) and list(counts) == [2, 2]
    assert np.array_equal(_bits(g[:, 1]), _bits(probs[:, 1] / F32(4))) and np.array_equal(_bits(g[:, 2]), _bits(probs[:, 2] / F32(4)))


# ---------------------------------------------------------------- the dropout generator
def test_philox_known_answers():
    """The two vectors of tests/test_oracle_golden.py::test_philox_known_answer (Random123 kat_vectors)."""
    assert [int(w[0]) for w in tsr.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = tsr.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(w[0]) for w in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    both = tsr.philox4x32_10(np.array([0, 0x243F6A88]), np.array([0, 0x85A308D3]), np.array([0, 0x13198A2E]), np.array([0, 0x03707344]), 0, 0)
    assert [int(w[0]) for w in both] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]  # (arrays of counters)


@pytest.mark.parametrize("p", [0.4, 0.5])
def test_dropout_keeps_its_share(p):
    n = 1 << 16
    mask = tsr.dropout_mask(n, p, seed=12345, counter=3, stream_id=1)
    keep = F32(1.0 / (1.0 - p))
    assert mask.dtype == F32 and mask.shape == (n,) and set(np.unique(mask)) == {F32(0), keep}
    share, sd = np.count_nonzero(mask) / n, np.sqrt(p * (1 - p) / n)
    print(f"p = {p}: kept {share:.5f}, {abs(share - (1 - p)) / sd:.2f} standard deviations from {1 - p}")
    assert abs(share - (1 - p)) <= 6 * sd
    assert np.array_equal(mask[:777], tsr.dropout_mask(777, p, seed=12345, counter=3, stream_id=1))  # a prefix, whatever n
    assert not np.array_equal(mask, tsr.dropout_mask(n, p, seed=12345, counter=4, stream_id=1))
    assert not np.array_equal(mask, tsr.dropout_mask(n, p, seed=12345, counter=3, stream_id=0))
    assert np.array_equal(tsr.dropout_mask(n, p, seed=12348, counter=0, stream_id=1), mask)  # the key is seed + counter
    assert np.all(tsr.dropout_mask(64, 0.0, seed=1) == 1)  # p = 0 keeps everything but a draw of exactly 0 (none among these)


def test_the_stat_map_names_only_statistics(fx):
    for m in (fx.PointNet(10), fx.DGCNN(10, 3, 16)):
        smap, names, at = tsr.stat_map(m), {}, 0
        for name, shape in m._shapes().items():
            for i in range(int(np.prod(shape))):
                names[at + i] = name
            at += int(np.prod(shape))
        assert at == m.param_count and len(set(smap)) == len(smap)
        assert all(names[i].endswith((".mu", ".sigma2")) for i in smap)
        assert len(smap) == sum(1 for n in names.values() if n.endswith((".mu", ".sigma2")))


# ---------------------------------------------------------------- argument checks before any device call
def test_argument_checks(fx):
    X = np.zeros((3, 16, 2), F32)
    for m in (fx.PointNet(10), fx.DGCNN(10, 3, 16)):
        opt = fx.ADAM()
        with pytest.raises(ValueError, match="two clouds"):
            m.train_step(X[:, :, :1], [0], opt)
        with pytest.raises(TypeError, match="update"):
            m.train_step(X, [0, 1], object())
        with pytest.raises(ValueError, match="labels must be in"):
            m.train_step(X, [0, 10], opt)
        with pytest.raises(ValueError, match="labels must be"):
            m.train_step(X, [0, 1, 2], opt)
        with pytest.raises(TypeError, match="integers"):
            m.train_step(X, [0.5, 1.0], opt)
        with pytest.raises(ValueError, match="momentum"):
            m.train_step(X, [0, 1], opt, momentum=1.5)
        with pytest.raises(ValueError, match='"device", seed, counter'):
            m.train_step(X, [0, 1], opt, dropout=("host", 1, None))
        with pytest.raises(ValueError, match='"device", seed, counter'):
            m.train_step(X, [0, 1], opt, dropout=("device", 1.5, None))
        with pytest.raises(TypeError, match="UInt64"):
            m.train_step(X, [0, 1], opt, dropout=("device", 1, np.zeros(1, np.uint64)))
        with pytest.raises(ValueError, match="labels must be in"):
            m.evaluate(X, [0, -1])
        with pytest.raises(ValueError):
            m.train_step(np.zeros((2, 16, 2), F32), [0, 1], opt)
        assert opt.state() == (None, None, None) and not m._stale
    with pytest.raises(ValueError, match="dropout must be"):
        fx.PointNet(10).train_step(X, [0, 1], fx.ADAM(), dropout=np.ones((255, 2), F32))
    with pytest.raises(ValueError, match="beta1 and beta2"):
        fx.ADAM(beta=(0.9, 1.0))
    with pytest.raises(TypeError, match="pair"):
        fx.ADAM(beta=0.9)
    with pytest.raises(ValueError, match="eta"):
        fx.ADAM(eta=float("nan"))
    with pytest.raises(ValueError, match="eps"):
        fx.ADAM(eps=-1.0)
    with pytest.raises(TypeError, match="Float32 device array"):
        fx.ADAM().update(np.zeros(4, F32), np.zeros(4, F32))
    a = fx.ADAM(eta=0.01, beta=(0.8, 0.99), eps=1e-6)
    assert (a.eta, a.beta, a.eps) == (0.01, (0.8, 0.99), 1e-6)
