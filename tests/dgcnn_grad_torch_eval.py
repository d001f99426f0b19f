"""An independent evaluation of the DGCNN adjoint by torch autograd on the CPU: what tests/test_dgcnn_grad_host.py holds the
restatement tests/dgcnn_grad_ref.py against.  The whole network is evaluated from X as tests/edgeconv_pgrad_torch_eval.py
evaluates an EdgeConv -- conv1d, batch_norm(training=False), relu, amax over k, the neighbours GIVEN and constant --, then conv_3,
amax over the points, linear, batch_norm, relu twice and a last linear; sum(glogits * logits) is differentiated with respect to
every conv and dense weight and bias, every BatchNorm gamma and beta, and X.  As a script, in float64 and float32,

    python tests/dgcnn_grad_torch_eval.py in.npz out.npz

in: ``X`` (3, N, B), ``glogits`` (num_classes, B), ``idx1`` and ``idx2`` (K, N, B), and the parameters under their names in Flux's
shapes; out: ``{g64,g32}.X`` (3, N, B) and ``{g64,g32}.{name}`` in Flux's shapes.  A test process that has loaded the HIP library
never imports torch."""
import sys

import numpy as np

STAGES = (("ec1", 3), ("ec2", 2))


def evaluate(X, glogits, P, idx, dtype):
    """X (3, N, B), glogits (nc, B) numpy; P: name -> array; idx: the two stages' lists.  Returns name -> gradient as numpy."""
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)

    T = {k: t(v[0].T[:, :, None] if v.ndim == 3 else v) for k, v in P.items()}  # conv: (Cout, Cin, 1); dense: (out, in)
    leaves = {k: v.requires_grad_(True) for k, v in T.items() if k.rsplit(".", 1)[1] in ("weight", "bias", "gamma", "beta")}

    def bn(a, name):
        return Fn.batch_norm(a, T[name + ".mu"], T[name + ".sigma2"], weight=T[name + ".gamma"], bias=T[name + ".beta"],
                             training=False, eps=1e-5)

    x = t(np.transpose(X, (2, 0, 1))).requires_grad_(True)
    y = x
    for (name, nblocks), lists in zip(STAGES, idx):
        nbr = torch.from_numpy(np.ascontiguousarray(np.transpose(lists, (2, 0, 1))).astype(np.int64))  # (B, K, N)
        B, F, N = y.shape
        K = nbr.shape[1]
        xj = torch.gather(y.detach(), 2, nbr.reshape(B, 1, K * N).expand(B, F, K * N))  # the neighbours are constants
        xi = y.repeat(1, 1, K)
        a = torch.cat([xi, xj - xi], dim=1)
        for i in range(1, nblocks + 1):
            a = torch.relu(bn(Fn.conv1d(a, T[f"{name}.conv{i}.weight"], T[f"{name}.conv{i}.bias"]), f"{name}.bn{i}"))
        y = a.reshape(B, -1, K, N).amax(dim=2)
    a = torch.relu(bn(Fn.conv1d(y, T["conv3.conv.weight"], T["conv3.conv.bias"]), "conv3.bn")).amax(dim=2)  # (B, 1024)
    a = torch.relu(bn(Fn.linear(a, T["fc4.dense.weight"], T["fc4.dense.bias"]), "fc4.bn"))
    a = torch.relu(bn(Fn.linear(a, T["fc5.dense.weight"], T["fc5.dense.bias"]), "fc5.bn"))
    logits = Fn.linear(a, T["fc6.weight"], T["fc6.bias"])  # (B, nc)
    (logits * t(np.asarray(glogits).T)).sum().backward()
    res = {"X": np.transpose(x.grad.numpy(), (1, 2, 0))}
    for k, v in leaves.items():
        g = v.grad.numpy()
        res[k] = np.ascontiguousarray(g[:, :, 0].T)[None] if g.ndim == 3 else g  # conv: back to (1, Cin, Cout)
    return res


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    X, glogits, idx = case.pop("X"), case.pop("glogits"), (case.pop("idx1"), case.pop("idx2"))
    out = {}
    for tag, dtype in (("g64", torch.float64), ("g32", torch.float32)):
        out.update({f"{tag}.{k}": v for k, v in evaluate(X, glogits, case, idx, dtype).items()})
    np.savez(sys.argv[2], **out)
