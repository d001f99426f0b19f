"""Host restatement of PointNet inference (include/flux3d_hip.h "PointNet inference"; src/models/pointnet.jl:3-20,41-85,
src/models/utils.jl:1-3) in numpy: the definition the device kernels are held to, bit for bit, up to the logits.

Float32 throughout.  A contraction is ``acc = +0; for c ascending: acc = fma32(x[c], W[c, o], acc)``; everything else is
numpy's own Float32 arithmetic (IEEE: one rounding per operation, division and square root correctly rounded).

numpy has no fmaf, so :func:`fma32` builds one: the Float64 product of two Float32 is exact, the one Float64 addition is
repaired to round-to-odd (TwoSum residual), and the cast to Float32 then rounds once.  ``contract`` runs the chain with it;
because that costs seconds per thousand points, the same chain is also compiled from tests/pointnet_ref_fma.c (libm's
fmaf) when a C compiler is there, checked against :func:`fma32` at load, and used instead -- same bits, much faster."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

F32 = np.float32
BN_EPS = F32(1e-5)


def fma32(a, b, c):
    """fmaf(a, b, c) elementwise: a * b + c with ONE rounding to Float32."""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)  # exact: 24 + 24 bits, exponents far inside Float64's range
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)                # TwoSum: s + err == p + c64 exactly (finite operands)
        # round to odd: an inexact sum whose Float64 mantissa is even moves one ulp towards the exact value, so that
        # the second rounding (53 -> 24 bits) sees on which side of every Float32 tie the exact value lies
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def contract_numpy(x, W):
    """x (..., Cin), W (Cin, Cout) -> (..., Cout): the fma32 chain over c, ascending, from +0.0."""
    x, W = np.asarray(x, F32), np.asarray(W, F32)
    acc = np.zeros(x.shape[:-1] + (W.shape[1],), F32)
    for c in range(W.shape[0]):
        acc = fma32(x[..., c:c + 1], W[c], acc)
    return acc


_HERE = os.path.dirname(os.path.abspath(__file__))
_clib = [None, False]  # (library or None, tried)


def _c_contract():
    """The chain of tests/pointnet_ref_fma.c, or None without a C compiler; checked against contract_numpy once."""
    if _clib[1]:
        return _clib[0]
    _clib[1] = True
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        return None
    out = os.path.join(tempfile.mkdtemp(prefix="pointnet_ref_"), "libpointnet_ref_fma.so")
    try:
        subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fopenmp",
                               "-o", out, os.path.join(_HERE, "pointnet_ref_fma.c"), "-lm"])
        lib = ctypes.CDLL(out)
    except (subprocess.CalledProcessError, OSError):
        return None
    lib.pointnet_ref_contract.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.c_void_p]
    lib.pointnet_ref_contract.restype = None
    _clib[0] = lib
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((37, 21)) * 10.0 ** rng.integers(-3, 4, (37, 21))).astype(F32)
    W = rng.standard_normal((21, 13)).astype(F32)
    assert np.array_equal(contract(x, W).view(np.uint32), contract_numpy(x, W).view(np.uint32)), \
        "the compiled fmaf chain disagrees with fma32"
    return lib


def contract(x, W):
    """contract_numpy's result by the compiled chain when there is one."""
    lib = _c_contract()
    if lib is None:
        return contract_numpy(x, W)
    x = np.ascontiguousarray(x, F32)
    W = np.ascontiguousarray(W, F32)
    out = np.empty(x.shape[:-1] + (W.shape[1],), F32)
    lib.pointnet_ref_contract(x.ctypes.data, x.size // x.shape[-1], W.shape[0], W.ctypes.data, W.shape[1], out.ctypes.data)
    return out


def relu(v):
    """Julia's max(0, v): NaN stays NaN, relu(-0.0) = +0.0."""
    return np.where(v > 0, v, np.where(np.isnan(v), v, F32(0.0))).astype(F32)


def batchnorm(v, P, name):
    """(gamma * ((v - mu) / sqrt(sigma2 + eps))) + beta over the last axis, each operation rounded to Float32."""
    g, be, mu, var = (np.asarray(P[f"{name}.{f}"], F32) for f in ("gamma", "beta", "mu", "sigma2"))
    with np.errstate(all="ignore"):
        return ((g * ((v - mu) / np.sqrt(var + BN_EPS))) + be).astype(F32)


def jmax(v, axis):
    """Julia's maximum along `axis`: NaN wins, max(-0.0, +0.0) = +0.0."""
    m = np.max(v, axis=axis)  # propagates NaN; the sign of a zero result is settled below
    pos_zero = np.any((v == 0) & ~np.signbit(v), axis=axis)
    return np.where(m == 0, np.where(pos_zero, F32(0.0), F32(-0.0)), m).astype(F32)


def conv(x, P, name):
    """1x1 convolution over the points, before its activation: x (B, N, Cin) -> (B, N, Cout).  Flux's weight (1, Cin, Cout)."""
    with np.errstate(all="ignore"):
        return (contract(x, np.asarray(P[name + ".weight"], F32)[0]) + np.asarray(P[name + ".bias"], F32)).astype(F32)


def dense(x, P, name):
    """Dense before its activation: x (B, in) -> (B, out).  Flux's weight (out, in)."""
    with np.errstate(all="ignore"):
        return (contract(x, np.asarray(P[name + ".weight"], F32).T) + np.asarray(P[name + ".bias"], F32)).astype(F32)


def apply_transform(x, T):
    """x (B, N, K), T (K, K, B): x'[j] = sum_i x[i] T[i, j, b] per point (batched_mul, no bias)."""
    return np.stack([contract(x[b], T[:, :, b]) for b in range(x.shape[0])])


def stn_stage(x, P, name, K):
    """stnKD(K) (src/models/pointnet.jl:3-20): x (B, N, K) -> T (K, K, B) with T[i, j, b] = d[j + K i]."""
    r = {}
    r["a1"] = batchnorm(relu(conv(x, P, f"{name}.conv1")), P, f"{name}.bn1")
    r["a2"] = batchnorm(relu(conv(r["a1"], P, f"{name}.conv2")), P, f"{name}.bn2")
    r["relu3"] = relu(conv(r["a2"], P, f"{name}.conv3"))
    r["a3"] = batchnorm(r["relu3"], P, f"{name}.bn3")
    r["max"] = jmax(r["a3"], axis=1)
    r["d1"] = relu(dense(r["max"], P, f"{name}.dense1"))
    r["d2"] = batchnorm(relu(dense(r["d1"], P, f"{name}.dense2")), P, f"{name}.bn4")
    r["d3"] = dense(r["d2"], P, f"{name}.dense3")  # (B, K K)
    # reshape(d, K, K, B) is column-major: M[p, q, b] = d[p + K q]; then PermutedDimsArray (2, 1, 3): T[i, j] = M[j, i]
    B = x.shape[0]
    r["T"] = np.ascontiguousarray(np.transpose(r["d3"].reshape(B, K, K), (1, 2, 0)))  # [i, j, b] = d[b][K i + j]
    return r


def forward(X, P):
    """X (3, N, B) or (3, N), P: name -> array in Flux's shapes.  Returns every intermediate; ``logits`` (num_classes, B),
    ``stn`` (3, 3, B), ``fstn`` (64, 64, B), ``pooled`` (1024, B) and ``probs`` are laid out as the library returns them."""
    X = np.asarray(X, F32)
    if X.ndim == 2:
        X = X[:, :, None]
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, 3)
    r = {}
    r["stn_stage"] = stn_stage(x, P, "stn", 3)
    r["stn"] = r["stn_stage"]["T"]
    r["x_t"] = apply_transform(x, r["stn"])
    r["block1_bn"] = batchnorm(conv(r["x_t"], P, "conv_block1.conv"), P, "conv_block1.bn")
    r["h"] = relu(r["block1_bn"])
    r["fstn_stage"] = stn_stage(r["h"], P, "fstn", 64)
    r["fstn"] = r["fstn_stage"]["T"]
    r["h_t"] = apply_transform(r["h"], r["fstn"])
    r["feat_relu1"] = relu(conv(r["h_t"], P, "feat.conv1"))
    r["feat_a1"] = batchnorm(r["feat_relu1"], P, "feat.bn1")
    r["feat_a2"] = batchnorm(conv(r["feat_a1"], P, "feat.conv2"), P, "feat.bn2")
    pooled = jmax(r["feat_a2"], axis=1)  # (B, 1024)
    r["feat_d1"] = batchnorm(relu(dense(pooled, P, "feat.dense1")), P, "feat.bn3")
    r["feat_d2"] = batchnorm(relu(dense(r["feat_d1"], P, "feat.dense2")), P, "feat.bn4")
    logits = relu(dense(r["feat_d2"], P, "cls"))
    r["pooled"] = np.asfortranarray(pooled.T)
    r["logits"] = np.asfortranarray(logits.T)
    r["probs"] = softmax32(r["logits"])
    return r


def softmax32(z):
    """softmax over the classes (axis 0) in Float32: e = exp(z - max z), e / sum e with the sum in class order."""
    z = np.asarray(z, F32)
    with np.errstate(all="ignore"):
        e = np.exp(z - jmax(z, axis=0)).astype(F32)
        s = np.zeros(z.shape[1:], F32)
        for i in range(z.shape[0]):
            s = (s + e[i]).astype(F32)
        return (e / s).astype(F32)


def softmax64(z):
    """The same in Float64: what the device's probabilities are compared with, from the device's own logits."""
    z = np.asarray(z, np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(z - np.max(z, axis=0))
        return e / np.sum(e, axis=0)


def param_shapes(num_classes):
    """name -> shape in Flux's shapes, in forward order, derived here from the layer table (not from the package)."""
    def stn(p, K):
        return [(f"{p}.conv1", (K, 64)), (f"{p}.bn1", 64), (f"{p}.conv2", (64, 128)), (f"{p}.bn2", 128),
                (f"{p}.conv3", (128, 1024)), (f"{p}.bn3", 1024), (f"{p}.dense1", [1024, 512]), (f"{p}.dense2", [512, 256]),
                (f"{p}.bn4", 256), (f"{p}.dense3", [256, K * K])]
    layers = stn("stn", 3) + [("conv_block1.conv", (3, 64)), ("conv_block1.bn", 64)] + stn("fstn", 64) + [
        ("feat.conv1", (64, 128)), ("feat.bn1", 128), ("feat.conv2", (128, 1024)), ("feat.bn2", 1024),
        ("feat.dense1", [1024, 512]), ("feat.bn3", 512), ("feat.dense2", [512, 256]), ("feat.bn4", 256),
        ("cls", [256, num_classes])]
    shapes = {}
    for name, ch in layers:
        if isinstance(ch, tuple):    # conv Cin => Cout
            shapes[name + ".weight"], shapes[name + ".bias"] = (1, ch[0], ch[1]), (ch[1],)
        elif isinstance(ch, list):   # dense in => out
            shapes[name + ".weight"], shapes[name + ".bias"] = (ch[1], ch[0]), (ch[1],)
        else:
            for f in ("gamma", "beta", "mu", "sigma2"):
                shapes[f"{name}.{f}"] = (ch,)
    return shapes


# The reference adds no identity to its transforms (src/models/pointnet.jl:18), so with He-scaled heads a random (K, K)
# matrix has entries of order 10 and multiplies the activations by about 10 sqrt(K); the logits then lie thousands apart
# and every probability is 0 or 1.  These factors keep the transforms near unit gain and the logits within a few units of
# each other, so that the softmax under test has something to compute.
WEIGHT_SCALE = {"stn.dense3.weight": 0.1, "fstn.dense3.weight": 0.02, "cls.weight": 0.25}


def random_params(num_classes, seed):
    """Random weights AND random running statistics (mu = 0, sigma2 = 1 would hide BatchNorm): He-scaled weights (times
    WEIGHT_SCALE), small biases, gamma in [0.5, 1.5], beta and mu of order 0.1, sigma2 in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    P = {}
    for name, shape in param_shapes(num_classes).items():
        field = name.rsplit(".", 1)[1]
        if field == "weight":
            fan_in = shape[1]
            P[name] = (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in) * WEIGHT_SCALE.get(name, 1.0)).astype(F32)
        elif field == "gamma":
            P[name] = rng.uniform(0.5, 1.5, shape).astype(F32)
        elif field == "sigma2":
            P[name] = rng.uniform(0.5, 2.0, shape).astype(F32)
        else:
            P[name] = (0.1 * rng.standard_normal(shape)).astype(F32)
    return P
