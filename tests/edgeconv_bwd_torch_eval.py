"""An independent evaluation of the EdgeConv input adjoint by torch autograd on the CPU: what tests/test_edgeconv_bwd_host.py
holds the restatement tests/edgeconv_bwd_ref.py against.  A chain of EdgeConv stages (one, or DGCNN's two) is evaluated with
conv1d, batch_norm(training=False), relu and amax over k, the neighbours GIVEN and constant (indices carry no gradient), and
sum(gout * last stage's output) is differentiated with respect to X.  As a script, in float64 and float32,

    python tests/edgeconv_bwd_torch_eval.py in.npz out.npz

in: X (F, N, B), gout (cL, N, B), nstages, and per stage s = 0, 1, ...: ``s{s}.layers``, ``s{s}.idx`` (K, N, B) 0-based and
the parameters by name, ``s{s}.conv1.weight`` ...; out: g64, g32 (F, N, B).  A test process that has loaded the HIP library
never imports torch."""
import sys

import numpy as np


def stage(x, P, layers, idx, dtype):
    """x (B, F, N) torch, P: name -> numpy array in Flux's shapes, idx (K, N, B) -> (B, cL, N)."""
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)

    T = {k: t(v[0].T[:, :, None] if k.endswith(".weight") else v) for k, v in P.items()}  # conv: (Cout, Cin, 1)
    nbr = torch.from_numpy(np.ascontiguousarray(np.transpose(idx, (2, 0, 1))).astype(np.int64))  # (B, K, N)
    B, F, N = x.shape
    K = nbr.shape[1]
    xj = torch.gather(x.detach(), 2, nbr.reshape(B, 1, K * N).expand(B, F, K * N))  # the neighbours are constants
    xi = x.repeat(1, 1, K)
    a = torch.cat([xi, xj - xi], dim=1)
    for i in range(1, len(layers)):
        a = Fn.conv1d(a, T[f"conv{i}.weight"], T[f"conv{i}.bias"])
        a = Fn.batch_norm(a, T[f"bn{i}.mu"], T[f"bn{i}.sigma2"], weight=T[f"bn{i}.gamma"], bias=T[f"bn{i}.beta"],
                          training=False, eps=1e-5)
        a = torch.relu(a)
    return a.reshape(B, -1, K, N).amax(dim=2)


def input_grad(X, gout, stages, dtype):
    """X (F, N, B), gout (cL, N, B) numpy; stages: a list of (P, layers, idx).  Returns the gradient (F, N, B) as numpy."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(X, np.float64), (2, 0, 1)))).to(dtype).requires_grad_(True)
    y = x
    for P, layers, idx in stages:
        y = stage(y, P, layers, idx, dtype)
    g = torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(gout, np.float64), (2, 0, 1)))).to(dtype)
    (y * g).sum().backward()
    return np.transpose(x.grad.numpy(), (1, 2, 0))


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    stages = []
    for s in range(int(case["nstages"])):
        pre = f"s{s}."
        own = {k[len(pre):]: v for k, v in case.items() if k.startswith(pre)}
        layers, idx = [int(c) for c in own.pop("layers")], own.pop("idx")
        stages.append((own, layers, idx))
    np.savez(sys.argv[2], g64=input_grad(case["X"], case["gout"], stages, torch.float64),
             g32=input_grad(case["X"], case["gout"], stages, torch.float32))
