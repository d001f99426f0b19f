"""Host restatement of EdgeConv(layers, K) inference (include/flux3d_hip.h "EdgeConv inference"; src/models/dgcnn.jl:11-71,
src/models/utils.jl:1-3) in numpy, for any layer widths: the definition fx3d_edgeconv_forward is held to, bit for bit.

Written from tests/dgcnn_ref.py's pieces -- the edge rows, the oracle's neighbour search, the fma32 chain, Float32 BatchNorm and
Julia's max of tests/pointnet_ref.py -- with the layer names of a standalone layer (``conv{i}``, ``bn{i}``) and, unlike
dgcnn_ref.edgeconv, neighbour lists that may be given."""
import numpy as np

from dgcnn_ref import BETA_MEAN, F32, batchnorm, conv, edge_rows, jmax, relu, self_knn


def param_shapes(layers):
    """name -> shape in Flux's shapes, in forward order: conv_bn_blocks 2 layers[0] => layers[1], layers[1] => layers[2], ..."""
    shapes = {}
    for i in range(1, len(layers)):
        cin, cout = (2 * layers[0] if i == 1 else layers[i - 1]), layers[i]
        shapes[f"conv{i}.weight"], shapes[f"conv{i}.bias"] = (1, cin, cout), (cout,)
        for f in ("gamma", "beta", "mu", "sigma2"):
            shapes[f"bn{i}.{f}"] = (cout,)
    return shapes


def random_params(layers, seed):
    """dgcnn_ref.random_params' distribution: He-scaled weights, small biases, gamma in [0.5, 1.5], mu of order 0.1, beta of
    order 0.1 about BETA_MEAN = 0.2, sigma2 in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    P = {}
    for name, shape in param_shapes(layers).items():
        field = name.rsplit(".", 1)[1]
        if field == "weight":
            P[name] = (rng.standard_normal(shape) * np.sqrt(2.0 / shape[1])).astype(F32)
        elif field == "gamma":
            P[name] = rng.uniform(0.5, 1.5, shape).astype(F32)
        elif field == "sigma2":
            P[name] = rng.uniform(0.5, 2.0, shape).astype(F32)
        else:
            P[name] = ((BETA_MEAN if field == "beta" else 0.0) + 0.1 * rng.standard_normal(shape)).astype(F32)
    return P


def forward(X, P, layers, K, idx=None):
    """X (F, N, B) or (F, N); P: name -> array in Flux's shapes; idx: (K, N, B) 0-based lists to use instead of the search.
    Returns (idx (K, N, B) int32, out (cL, N, B)) laid out as the library returns them."""
    X = np.asarray(X, F32)
    if X.ndim == 2:
        X = X[:, :, None]
    assert X.shape[0] == layers[0], (X.shape, layers)
    x = np.ascontiguousarray(np.transpose(X, (2, 1, 0)))  # (B, N, F)
    idx = self_knn(x, K) if idx is None else np.asarray(idx).reshape((K,) + x.shape[1::-1], order="F")
    out = []
    for b in range(x.shape[0]):
        a = edge_rows(x[b], idx[:, :, b])  # (K, N, 2F)
        for i in range(1, len(layers)):
            a = relu(batchnorm(conv(a, P, f"conv{i}"), P, f"bn{i}"))  # conv_bn_block: Conv, BatchNorm, relu
        out.append(jmax(a, axis=0))  # (N, cL)
    return np.asfortranarray(idx.astype(np.int32)), np.asfortranarray(np.transpose(np.stack(out), (2, 1, 0)))


def check_draw(out):
    """The condition a draw of inputs must meet for a comparison to mean something, asserted on the restatement's own output:
    it is finite and the relu has left at least half of it alive."""
    assert np.all(np.isfinite(out)), "the restatement's output is not finite"
    nz = np.count_nonzero(out)
    assert 2 * nz >= out.size, f"only {nz} of {out.size} elements are non-zero"
