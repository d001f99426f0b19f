"""An independent evaluation of the PointNet training-mode forward by torch.nn.functional on (B, C, N) tensors, BatchNorm with
``training=True``: what tests/test_pointnet_train_host.py holds the restatement tests/pointnet_train_ref.py against.  The
dropout multipliers are applied as the given mask; torch's own Dropout is not used.  As a script it evaluates one saved case in
float64 and float32 on the CPU,

    python tests/pointnet_train_torch_eval.py in.npz out.npz

in: X, momentum, optionally dropout (256, B), and the parameters by name (their mu / sigma2 are the running statistics).
out, for T in 64, 32: logitsT (num_classes, B); statsT: every BatchNorm's batch mean and biased variance of what it is given,
in the library's statistics layout (per BatchNorm in forward order mean (C), variance (C)); runningT: running_mean /
running_var after the step in the same layout -- so that a test process that has loaded the HIP library never imports torch."""
import sys

import numpy as np


def forward_train(X, P, dtype, dropout=None, momentum=0.1):
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)

    T = {k: t(v[0].T[:, :, None] if k.endswith(".weight") and v.ndim == 3 else v) for k, v in P.items()}  # conv: (Cout, Cin, 1)
    x0 = t(np.transpose(np.asarray(X), (2, 0, 1)))  # (B, 3, N)
    mask = None if dropout is None else t(np.asarray(dropout).T)  # (B, 256)
    stats, running = [], []

    def conv(x, name):
        return Fn.conv1d(x, T[name + ".weight"], T[name + ".bias"])

    def bn(x, name):
        dims = (0, 2) if x.dim() == 3 else (0,)
        stats.extend([x.mean(dim=dims), x.var(dim=dims, unbiased=False)])
        rm, rv = T[name + ".mu"].clone(), T[name + ".sigma2"].clone()
        y = Fn.batch_norm(x, rm, rv, weight=T[name + ".gamma"], bias=T[name + ".beta"], training=True, momentum=momentum, eps=1e-5)
        running.extend([rm, rv])  # updated in place: (1 - momentum) running + momentum (batch mean, unbiased batch variance)
        return y

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

    with torch.no_grad():
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
        z = torch.relu(lin(d, "cls")).T
    return z.numpy(), torch.cat(stats).numpy(), torch.cat(running).numpy()


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    X, momentum, dropout = case.pop("X"), float(case.pop("momentum")), case.pop("dropout", None)
    out = {}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        out["logits" + tag], out["stats" + tag], out["running" + tag] = forward_train(X, case, dtype, dropout, momentum)
    np.savez(sys.argv[2], **out)
