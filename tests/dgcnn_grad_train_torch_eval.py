"""An independent evaluation of the DGCNN training-mode adjoint by torch autograd on the CPU: what
tests/test_dgcnn_grad_train_host.py holds the restatement tests/dgcnn_grad_train_ref.py against.  The whole network is evaluated as
tests/dgcnn_train_torch_eval.py evaluates it -- every BatchNorm batch_norm(training=True), the dropout multipliers applied as the
given masks, both neighbour lists GIVEN and constant -- and sum(glogits * logits) is differentiated with respect to every conv and
dense weight and bias, every BatchNorm gamma and beta, and to X.  As a script, in float64 and float32,

    python tests/dgcnn_grad_train_torch_eval.py in.npz out.npz

in: X (3, N, B), glogits (nc, B), idx1, idx2 (K, N, B), optionally dropout4 (512, B) and dropout5 (256, B), and the parameters by
name (their mu / sigma2 are not read).  out: ``g64.<name>`` / ``g32.<name>`` in Flux's shapes, and ``g64.X`` / ``g32.X`` (3, N, B).
A test process that has loaded the HIP library never imports torch."""
import sys

import numpy as np


def evaluate(X, glogits, P, idx, dropout, dtype):
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)

    T = {k: t(v[0].T[:, :, None] if k.endswith(".weight") and v.ndim == 3 else v) for k, v in P.items()}  # conv: (Cout, Cin, 1)
    leaves = {k: v.requires_grad_(True) for k, v in T.items() if k.rsplit(".", 1)[1] in ("weight", "bias", "gamma", "beta")}
    x = t(np.transpose(np.asarray(X), (2, 0, 1))).requires_grad_(True)  # (B, 3, N)
    nbrs = [torch.from_numpy(np.ascontiguousarray(np.transpose(i, (2, 0, 1))).astype(np.int64)) for i in idx]  # (B, K, N)
    masks = [None if m is None else t(np.asarray(m).T) for m in dropout]

    def bn(v, name):
        return Fn.batch_norm(v, None, None, weight=T[name + ".gamma"], bias=T[name + ".beta"], training=True, eps=1e-5)

    def edgeconv(y, prefix, nblocks, nbr):
        B, F, N = y.shape
        K = nbr.shape[1]
        xj = torch.gather(y.detach(), 2, nbr.reshape(B, 1, K * N).expand(B, F, K * N))  # the neighbours are constants
        xi = y.repeat(1, 1, K)
        a = torch.cat([xi, xj - xi], dim=1)
        for i in range(1, nblocks + 1):
            a = torch.relu(bn(Fn.conv1d(a, T[f"{prefix}conv{i}.weight"], T[f"{prefix}conv{i}.bias"]), f"{prefix}bn{i}"))
        return a.reshape(B, -1, K, N).amax(dim=2)

    def fc(v, dense, name, mask):
        v = torch.relu(bn(Fn.linear(v, T[dense + ".weight"], T[dense + ".bias"]), name))
        return v if mask is None else v * mask

    x1 = edgeconv(x, "ec1.", 3, nbrs[0])
    x2 = edgeconv(x1, "ec2.", 2, nbrs[1])
    a = torch.relu(bn(Fn.conv1d(x2, T["conv3.conv.weight"], T["conv3.conv.bias"]), "conv3.bn")).amax(dim=2)
    d = fc(fc(a, "fc4.dense", "fc4.bn", masks[0]), "fc5.dense", "fc5.bn", masks[1])
    logits = Fn.linear(d, T["fc6.weight"], T["fc6.bias"])  # (B, nc)
    (logits * t(np.asarray(glogits).T)).sum().backward()
    res = {"X": np.transpose(x.grad.numpy(), (1, 2, 0))}
    for k, v in leaves.items():
        g = v.grad.numpy()
        res[k] = np.ascontiguousarray(g[:, :, 0].T)[None] if g.ndim == 3 else g  # a conv's back to (1, Cin, Cout)
    return res


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    X, glogits = case.pop("X"), case.pop("glogits")
    idx = [case.pop("idx1"), case.pop("idx2")]
    dropout = (case.pop("dropout4", None), case.pop("dropout5", None))
    out = {}
    for tag, dtype in (("g64", torch.float64), ("g32", torch.float32)):
        out.update({f"{tag}.{k}": v for k, v in evaluate(X, glogits, case, idx, dropout, dtype).items()})
    np.savez(sys.argv[2], **out)
