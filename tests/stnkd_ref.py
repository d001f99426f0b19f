"""Host restatement of stnKD(K) (include/flux3d_hip_layers.h "stnKD(K)"; src/models/pointnet.jl:3-20) in numpy, test mode and
training mode: the definition the device kernels are held to, bit for bit.

Nothing is restated twice: the layer chain and its Float32 arithmetic are ``pointnet_ref.stn_stage`` (``contract``: the fmaf
chain over ALL K channels, ascending, from +0.0), the training-mode chain and the Float64 statistics are
``pointnet_train_ref``'s (``_stn_stage``, ``point_sums``, ``dense_sums``, ``mean_var``, ``running_update`` through ``_Train``).
What is here is the layer's own interface: parameters under the names ``conv1.weight`` ... ``dense3.bias``, the input as
(K, N, B), the outputs laid out as the library returns them.  tests/stnkd_torch_eval.py holds it against torch float64."""
import numpy as np

import pointnet_ref as ref
import pointnet_train_ref as tref

F32 = np.float32
BN_ORDER = ("bn1", "bn2", "bn3", "bn4")
BN_WIDTH = {"bn1": 64, "bn2": 128, "bn3": 1024, "bn4": 256}
_PREFIX = "s"  # stn_stage takes its parameters under a layer name


def param_shapes(K):
    """name -> shape in Flux's shapes, in forward order: the ``stn.`` entries of pointnet_ref's table for this K, prefix dropped."""
    K = int(K)
    layers = [("conv1", (K, 64)), ("bn1", 64), ("conv2", (64, 128)), ("bn2", 128), ("conv3", (128, 1024)), ("bn3", 1024),
              ("dense1", [1024, 512]), ("dense2", [512, 256]), ("bn4", 256), ("dense3", [256, K * K])]
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


def random_params(K, seed, dense3_scale=0.1):
    """As pointnet_ref.random_params: He-scaled weights (dense3 times ``dense3_scale``, which keeps the transform's entries
    of order one), small biases, random BatchNorm parameters AND random running statistics."""
    rng = np.random.default_rng(seed)
    P = {}
    for name, shape in param_shapes(K).items():
        field = name.rsplit(".", 1)[1]
        if field == "weight":
            P[name] = (rng.standard_normal(shape) * np.sqrt(2.0 / shape[1]) * (dense3_scale if name == "dense3.weight" else 1.0)).astype(F32)
        elif field == "gamma":
            P[name] = rng.uniform(0.5, 1.5, shape).astype(F32)
        elif field == "sigma2":
            P[name] = rng.uniform(0.5, 2.0, shape).astype(F32)
        else:
            P[name] = (0.1 * rng.standard_normal(shape)).astype(F32)
    return P


def _prefixed(P):
    return {f"{_PREFIX}.{k}": v for k, v in P.items()}


def _points(X, K):
    X = np.asarray(X, F32)
    if X.ndim == 2:
        X = X[:, :, None]
    assert X.ndim == 3 and X.shape[0] == K, (X.shape, K)
    return np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, K)


def _laid_out(r):
    r["out"] = r["T"]                                   # (K, K, B), out[i, j, b] = d[j + K i]
    r["pooled"] = np.asfortranarray(r["max"].T)         # (1024, B)
    return r


def forward(X, P, K):
    """X (K, N, B) or (K, N), P: name -> array in Flux's shapes.  Every intermediate of ``pointnet_ref.stn_stage``, with ``out``
    (K, K, B) and ``pooled`` (1024, B) laid out as the library returns them."""
    return _laid_out(ref.stn_stage(_points(X, K), _prefixed(P), _PREFIX, int(K)))


def forward_train(X, P, K, momentum=0.1):
    """X (K, N, B) with B >= 2; the mu / sigma2 of P are the running statistics.  ``out`` and ``pooled`` as :func:`forward`;
    ``batch_stats`` and ``running``: name -> (C,) under ``bn1.mu`` ... ``bn4.sigma2``, in forward order."""
    x = _points(X, K)
    assert x.shape[0] >= 2
    t = tref._Train(_prefixed(P), momentum)
    r = _laid_out(tref._stn_stage(x, t, _PREFIX, int(K)))
    cut = len(_PREFIX) + 1
    r["batch_stats"] = {k[cut:]: v for k, v in t.batch_stats.items()}
    r["running"] = {k[cut:]: v for k, v in t.running.items()}
    r["bn_inputs"] = {k[cut:]: v for k, v in t.bn_inputs.items()}
    assert list(r["batch_stats"]) == [f"{bn}.{f}" for bn in BN_ORDER for f in ("mu", "sigma2")]
    return r


def flat_stats(named):
    """name -> (C,) as the library's flat statistics buffer: bn1 .. bn4, each mu (C) then sigma2 (C)."""
    return np.concatenate([np.asarray(named[f"{bn}.{f}"], F32) for bn in BN_ORDER for f in ("mu", "sigma2")])
