"""An independent evaluation of the EdgeConv training-mode adjoint by torch autograd on the CPU: what
tests/test_edgeconv_grad_train_host.py holds the restatement tests/edgeconv_grad_train_ref.py against.  A chain of EdgeConv stages
(one, or DGCNN's two) is evaluated as tests/edgeconv_pgrad_torch_eval.py evaluates it, but with batch_norm(training=True): every
BatchNorm normalises by the mean and uncorrected variance of its input over all K N B edge rows, and autograd differentiates
through them.  The neighbours are GIVEN and constant.  sum(gout * last stage's output) is differentiated with respect to every conv
weight and bias and every BatchNorm gamma and beta, and to X.  As a script, in float64 and float32,

    python tests/edgeconv_grad_train_torch_eval.py in.npz out.npz

in and out: as tests/edgeconv_pgrad_torch_eval.py (mu / sigma2 of the parameters are not read).  A test process that has loaded the
HIP library never imports torch."""
import sys

import numpy as np


def evaluate(X, gout, stages, dtype):
    """X (F, N, B), gout (cL, N, B) numpy; stages: a list of (P, layers, idx).  Returns name -> gradient as numpy."""
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)

    x = t(np.transpose(X, (2, 0, 1))).requires_grad_(True)
    leaves, y = {}, x
    for s, (P, layers, idx) in enumerate(stages):
        T = {k: t(v[0].T[:, :, None] if k.endswith(".weight") else v) for k, v in P.items()}  # conv: (Cout, Cin, 1)
        for k, v in T.items():
            if k.rsplit(".", 1)[1] in ("weight", "bias", "gamma", "beta"):
                leaves[f"s{s}.{k}"] = v.requires_grad_(True)
        nbr = torch.from_numpy(np.ascontiguousarray(np.transpose(idx, (2, 0, 1))).astype(np.int64))  # (B, K, N)
        B, F, N = y.shape
        K = nbr.shape[1]
        xj = torch.gather(y.detach(), 2, nbr.reshape(B, 1, K * N).expand(B, F, K * N))  # the neighbours are constants
        xi = y.repeat(1, 1, K)
        a = torch.cat([xi, xj - xi], dim=1)
        for i in range(1, len(layers)):
            a = Fn.conv1d(a, T[f"conv{i}.weight"], T[f"conv{i}.bias"])
            a = Fn.batch_norm(a, None, None, weight=T[f"bn{i}.gamma"], bias=T[f"bn{i}.beta"], training=True, eps=1e-5)
            a = torch.relu(a)
        y = a.reshape(B, -1, K, N).amax(dim=2)
    (y * t(np.transpose(gout, (2, 0, 1)))).sum().backward()
    res = {"X": np.transpose(x.grad.numpy(), (1, 2, 0))}
    for k, v in leaves.items():
        g = v.grad.numpy()
        res[k] = np.ascontiguousarray(g[:, :, 0].T)[None] if k.endswith(".weight") else g  # back to (1, Cin, Cout)
    return res


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    stages = []
    for s in range(int(case["nstages"])):
        pre = f"s{s}."
        own = {k[len(pre):]: v for k, v in case.items() if k.startswith(pre)}
        layers, idx = [int(c) for c in own.pop("layers")], own.pop("idx")
        stages.append((own, layers, idx))
    out = {}
    for tag, dtype in (("g64", torch.float64), ("g32", torch.float32)):
        out.update({f"{tag}.{k}": v for k, v in evaluate(case["X"], case["gout"], stages, dtype).items()})
    np.savez(sys.argv[2], **out)
