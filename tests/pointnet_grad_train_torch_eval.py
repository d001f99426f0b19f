"""An independent evaluation of the PointNet training-mode adjoint by torch autograd on the CPU: what
tests/test_pointnet_grad_train_host.py holds the restatement tests/pointnet_grad_train_ref.py against.  The whole network is
evaluated from X as tests/pointnet_train_torch_eval.py evaluates it -- conv1d, batch_norm(training=True), relu, amax over the
points, bmm with the two transforms, the dropout multipliers as a given mask --, and sum(glogits * logits), with the logits after
cls's relu, is differentiated with respect to every conv and dense weight and bias, every BatchNorm gamma and beta, and X: autograd
goes through the batch mean and variance.  As a script, in float64 and float32,

    python tests/pointnet_grad_train_torch_eval.py in.npz out.npz

in: ``X`` (3, N, B), ``glogits`` (num_classes, B), optionally ``dropout`` (256, B), and the parameters under their names in Flux's
shapes; out: ``{g64,g32}.X`` (3, N, B) and ``{g64,g32}.{name}`` in Flux's shapes.  A test process that has loaded the HIP library
never imports torch."""
import sys

import numpy as np


def evaluate(X, glogits, P, dtype, dropout=None):
    """X (3, N, B), glogits (nc, B), dropout (256, B) or None, numpy; P: name -> array.  Returns name -> gradient as numpy."""
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)

    T = {k: t(v[0].T[:, :, None] if v.ndim == 3 else v) for k, v in P.items()}  # conv: (Cout, Cin, 1); dense: (out, in)
    leaves = {k: v.requires_grad_(True) for k, v in T.items() if k.rsplit(".", 1)[1] in ("weight", "bias", "gamma", "beta")}
    mask = None if dropout is None else t(np.asarray(dropout).T)  # (B, 256)

    def conv(x, name):
        return Fn.conv1d(x, T[name + ".weight"], T[name + ".bias"])

    def bn(x, name):  # the running statistics are not read in training mode
        return Fn.batch_norm(x, None, None, weight=T[name + ".gamma"], bias=T[name + ".beta"], training=True, eps=1e-5)

    def lin(x, name):
        return Fn.linear(x, T[name + ".weight"], T[name + ".bias"])

    def stn(x, name, K):
        a = bn(torch.relu(conv(x, name + ".conv1")), name + ".bn1")
        a = bn(torch.relu(conv(a, name + ".conv2")), name + ".bn2")
        a = bn(torch.relu(conv(a, name + ".conv3")), name + ".bn3")
        d = torch.relu(lin(a.amax(dim=2), name + ".dense1"))
        d = bn(torch.relu(lin(d, name + ".dense2")), name + ".bn4")
        return lin(d, name + ".dense3").reshape(-1, K, K)  # [b, i, j] = d[j + K i]

    def transform(x, M):  # x (B, K, N): x'[j] = sum_i x[i] M[i, j]
        return torch.bmm(x.transpose(1, 2), M).transpose(1, 2)

    x0 = t(np.transpose(np.asarray(X), (2, 0, 1))).requires_grad_(True)  # (B, 3, N)
    x = transform(x0, stn(x0, "stn", 3))
    h = torch.relu(bn(conv(x, "conv_block1.conv"), "conv_block1.bn"))
    h = transform(h, stn(h, "fstn", 64))
    a = bn(torch.relu(conv(h, "feat.conv1")), "feat.bn1")
    a = bn(conv(a, "feat.conv2"), "feat.bn2")
    d = bn(torch.relu(lin(a.amax(dim=2), "feat.dense1")), "feat.bn3")
    d = torch.relu(lin(d, "feat.dense2"))
    if mask is not None:
        d = d * mask
    d = bn(d, "feat.bn4")
    logits = torch.relu(lin(d, "cls"))  # (B, nc)
    (logits * t(np.asarray(glogits).T)).sum().backward()
    res = {"X": np.transpose(x0.grad.numpy(), (1, 2, 0))}
    for k, v in leaves.items():
        g = v.grad.numpy()
        res[k] = np.ascontiguousarray(g[:, :, 0].T)[None] if g.ndim == 3 else g  # conv: back to (1, Cin, Cout)
    return res


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    X, glogits, dropout = case.pop("X"), case.pop("glogits"), case.pop("dropout", None)
    out = {}
    for tag, dtype in (("g64", torch.float64), ("g32", torch.float32)):
        out.update({f"{tag}.{k}": v for k, v in evaluate(X, glogits, case, dtype, dropout).items()})
    np.savez(sys.argv[2], **out)
