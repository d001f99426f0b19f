"""An independent evaluation of PointNet inference (src/models/pointnet.jl:62-85, test mode) by torch.nn.functional on
(B, C, N) tensors: what tests/test_pointnet_host.py holds the restatement tests/pointnet_ref.py against, and the torch
figure of tools/pointnet_time.py.  As a script it evaluates one saved case in float64 and float32 on the CPU,

    python tests/pointnet_torch_eval.py in.npz out.npz      (in: X and the parameters by name; out: logits64, logits32)

so that a test process that has loaded the HIP library never has to import torch itself."""
import sys

import numpy as np


def forward(X, P, dtype, device="cpu", softmax=False):
    """X (3, N, B) numpy, P: name -> array in Flux's shapes.  Returns the logits (num_classes, B) as a tensor on `device`
    (the probabilities with softmax=True)."""
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype).to(device)

    T = {k: t(v[0].T[:, :, None] if k.endswith(".weight") and v.ndim == 3 else v) for k, v in P.items()}  # conv: (Cout, Cin, 1)
    x0 = t(np.transpose(np.asarray(X), (2, 0, 1)))  # (B, 3, N)

    def conv(x, name):
        return Fn.conv1d(x, T[name + ".weight"], T[name + ".bias"])

    def bn(x, name):
        return Fn.batch_norm(x, T[name + ".mu"], T[name + ".sigma2"], weight=T[name + ".gamma"], bias=T[name + ".beta"],
                             training=False, eps=1e-5)

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

    def run():
        x = transform(x0, stn(x0, "stn", 3))
        h = torch.relu(bn(conv(x, "conv_block1.conv"), "conv_block1.bn"))
        h = transform(h, stn(h, "fstn", 64))
        a = bn(torch.relu(conv(h, "feat.conv1")), "feat.bn1")
        a = bn(conv(a, "feat.conv2"), "feat.bn2")
        d = bn(torch.relu(lin(a.amax(dim=2), "feat.dense1")), "feat.bn3")
        d = bn(torch.relu(lin(d, "feat.dense2")), "feat.bn4")
        z = torch.relu(lin(d, "cls"))
        return (torch.softmax(z, dim=1) if softmax else z).T

    with torch.no_grad():
        out = run()
    return out, run


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    X = case.pop("X")
    np.savez(sys.argv[2], logits64=forward(X, case, torch.float64)[0].numpy(), logits32=forward(X, case, torch.float32)[0].numpy())
