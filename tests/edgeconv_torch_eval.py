"""An independent evaluation of EdgeConv(layers, K) inference (src/models/dgcnn.jl:11-71, test mode) by torch.nn.functional
on (B, C, K N) tensors: what tests/test_edgeconv_host.py holds the restatement tests/edgeconv_ref.py against.  As a script it
evaluates one saved case in float64 and float32 on the CPU,

    python tests/edgeconv_torch_eval.py in.npz out.npz     (in: X, idx, layers and the parameters by name; out: out64, out32)

with the neighbours GIVEN (idx (K, N, B), 0-based), as tests/dgcnn_torch_eval.py does and for its reason: a float64 search could
break a near-tie of the Float32 distances the other way.  A test process that has loaded the HIP library never imports torch."""
import sys

import numpy as np


def forward(X, P, layers, idx, dtype):
    """X (F, N, B) numpy, P: name -> array in Flux's shapes, idx (K, N, B).  Returns out (cL, N, B) as a numpy array."""
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)

    T = {k: t(v[0].T[:, :, None] if k.endswith(".weight") else v) for k, v in P.items()}  # conv: (Cout, Cin, 1)
    x = t(np.transpose(np.asarray(X), (2, 0, 1)))  # (B, F, N)
    nbr = torch.from_numpy(np.ascontiguousarray(np.transpose(idx, (2, 0, 1))).astype(np.int64))  # (B, K, N)
    B, F, N = x.shape
    K = nbr.shape[1]
    with torch.no_grad():
        xj = torch.gather(x, 2, nbr.reshape(B, 1, K * N).expand(B, F, K * N))  # column k N + n is neighbour k of point n
        xi = x.repeat(1, 1, K)
        a = torch.cat([xi, xj - xi], dim=1)
        for i in range(1, len(layers)):
            a = Fn.conv1d(a, T[f"conv{i}.weight"], T[f"conv{i}.bias"])
            a = Fn.batch_norm(a, T[f"bn{i}.mu"], T[f"bn{i}.sigma2"], weight=T[f"bn{i}.gamma"], bias=T[f"bn{i}.beta"],
                              training=False, eps=1e-5)
            a = torch.relu(a)
        out = a.reshape(B, -1, K, N).amax(dim=2)  # (B, cL, N)
    return np.transpose(out.numpy(), (1, 2, 0))


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    X, idx, layers = case.pop("X"), case.pop("idx"), [int(c) for c in case.pop("layers")]
    np.savez(sys.argv[2], out64=forward(X, case, layers, idx, torch.float64), out32=forward(X, case, layers, idx, torch.float32))
