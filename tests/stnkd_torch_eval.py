"""An independent evaluation of stnKD(K) by torch.nn.functional on (B, C, N) tensors, in eval mode and with
``batch_norm(training=True)``: what tests/test_stnkd_host.py holds the restatement tests/stnkd_ref.py against (the bound is
recorded there, as tests/test_pointnet_train_host.py records it for PointNet).  As a script it evaluates one saved case in
float64 and float32 on the CPU,

    python tests/stnkd_torch_eval.py in.npz out.npz

in: X (K, N, B), momentum, and the parameters by name (their mu / sigma2 are the running statistics).
out, for T in 64, 32: evalT (K, K, B), the test-mode transform; trainT (K, K, B), the training-mode one; statsT: every
BatchNorm's batch mean and biased variance of what it is given, in the library's statistics layout (bn1 .. bn4, each mean (C)
then variance (C)); runningT: running_mean / running_var after the step in the same layout -- so that a test process that has
loaded the HIP library never imports torch."""
import sys

import numpy as np


def forward(X, P, dtype, training, momentum=0.1):
    """(out (K, K, B), stats, running); stats and running are empty in eval mode."""
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)

    T = {k: t(v[0].T[:, :, None] if k.endswith(".weight") and v.ndim == 3 else v) for k, v in P.items()}  # conv: (Cout, Cin, 1)
    x = t(np.transpose(np.asarray(X), (2, 0, 1)))  # (B, K, N)
    K = x.shape[1]
    stats, running = [], []

    def conv(x, name):
        return Fn.conv1d(x, T[name + ".weight"], T[name + ".bias"])

    def bn(x, name):
        rm, rv = T[name + ".mu"].clone(), T[name + ".sigma2"].clone()
        if training:
            dims = (0, 2) if x.dim() == 3 else (0,)
            stats.extend([x.mean(dim=dims), x.var(dim=dims, unbiased=False)])
        y = Fn.batch_norm(x, rm, rv, weight=T[name + ".gamma"], bias=T[name + ".beta"], training=training, momentum=momentum, eps=1e-5)
        if training:
            running.extend([rm, rv])  # updated in place: (1 - momentum) running + momentum (batch mean, unbiased batch variance)
        return y

    def lin(x, name):
        return Fn.linear(x, T[name + ".weight"], T[name + ".bias"])

    with torch.no_grad():
        a = bn(torch.relu(conv(x, "conv1")), "bn1")
        a = bn(torch.relu(conv(a, "conv2")), "bn2")
        a = bn(torch.relu(conv(a, "conv3")), "bn3")
        d = torch.relu(lin(a.amax(dim=2), "dense1"))
        d = bn(torch.relu(lin(d, "dense2")), "bn4")
        out = lin(d, "dense3").reshape(-1, K, K).permute(1, 2, 0)  # [i, j, b] = d[b][j + K i]
    empty = np.zeros(0)
    return (out.numpy(), torch.cat(stats).numpy() if training else empty, torch.cat(running).numpy() if training else empty)


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    X, momentum = case.pop("X"), float(case.pop("momentum"))
    res = {}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        res["eval" + tag] = forward(X, case, dtype, False)[0]
        res["train" + tag], res["stats" + tag], res["running" + tag] = forward(X, case, dtype, True, momentum)
    np.savez(sys.argv[2], **res)
