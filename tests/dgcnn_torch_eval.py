"""An independent evaluation of DGCNN inference (src/models/dgcnn.jl:32-71,113-147, test mode) by torch.nn.functional on
(B, C, K N) tensors: what tests/test_dgcnn_host.py holds the restatement tests/dgcnn_ref.py against, and the torch figure of
tools/dgcnn_time.py.  As a script it evaluates one saved case in float64 and float32 on the CPU,

    python tests/dgcnn_torch_eval.py in.npz out.npz     (in: X, idx1, idx2 and the parameters by name; out: logits64, logits32)

with the neighbours GIVEN (idx1, idx2 (K, N, B), 0-based): a float64 search could break a near-tie of the Float32 distances
the other way, and the two evaluations would then run different networks.  forward(..., idx=None) searches itself (cdist +
topk): the timing tool's use.  A test process that has loaded the HIP library never has to import torch itself."""
import sys

import numpy as np


def forward(X, P, K, dtype, device="cpu", softmax=False, idx=None):
    """X (3, N, B) numpy, P: name -> array in Flux's shapes.  Returns the logits (num_classes, B) as a tensor on `device`
    (the probabilities with softmax=True) and the closure that computes them."""
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype).to(device)

    T = {k: t(v[0].T[:, :, None] if k.endswith(".weight") and v.ndim == 3 else v) for k, v in P.items()}  # conv: (Cout, Cin, 1)
    x0 = t(np.transpose(np.asarray(X), (2, 0, 1)))  # (B, 3, N)
    given = None if idx is None else [torch.from_numpy(np.ascontiguousarray(np.transpose(i, (2, 0, 1))).astype(np.int64)).to(device)
                                      for i in idx]  # (B, K, N)

    def block(x, conv, bn):
        x = Fn.conv1d(x, T[conv + ".weight"], T[conv + ".bias"])
        x = Fn.batch_norm(x, T[bn + ".mu"], T[bn + ".sigma2"], weight=T[bn + ".gamma"], bias=T[bn + ".beta"], training=False, eps=1e-5)
        return torch.relu(x)

    def fc(x, dense, bn):
        x = Fn.linear(x, T[dense + ".weight"], T[dense + ".bias"])
        x = Fn.batch_norm(x, T[bn + ".mu"], T[bn + ".sigma2"], weight=T[bn + ".gamma"], bias=T[bn + ".beta"], training=False, eps=1e-5)
        return torch.relu(x)

    def edgeconv(x, name, nlayers, nbr):
        B, F, N = x.shape
        if nbr is None:  # the K nearest besides the point itself
            pts = x.transpose(1, 2)
            nbr = torch.cdist(pts, pts).topk(K + 1, dim=2, largest=False).indices[:, :, 1:].transpose(1, 2)  # (B, K, N)
        flat = nbr.reshape(B, 1, K * N).expand(B, F, K * N)
        xj = torch.gather(x, 2, flat)                     # (B, F, K N): column k N + n is neighbour k of point n
        xi = x.repeat(1, 1, K)                            # the same columns: point n
        a = torch.cat([xi, xj - xi], dim=1)
        for i in range(1, nlayers + 1):
            a = block(a, f"{name}.conv{i}", f"{name}.bn{i}")
        return a.reshape(B, -1, K, N).amax(dim=2)

    def run():
        x1 = edgeconv(x0, "ec1", 3, None if given is None else given[0])
        x2 = edgeconv(x1, "ec2", 2, None if given is None else given[1])
        a = block(x2, "conv3.conv", "conv3.bn").amax(dim=2)
        z = Fn.linear(fc(fc(a, "fc4.dense", "fc4.bn"), "fc5.dense", "fc5.bn"), T["fc6.weight"], T["fc6.bias"])
        return (torch.softmax(z, dim=1) if softmax else z).T

    with torch.no_grad():
        out = run()
    return out, run


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    X, idx = case.pop("X"), (case.pop("idx1"), case.pop("idx2"))
    K = idx[0].shape[0]
    np.savez(sys.argv[2], logits64=forward(X, case, K, torch.float64, idx=idx)[0].numpy(),
             logits32=forward(X, case, K, torch.float32, idx=idx)[0].numpy())
