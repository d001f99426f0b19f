"""An independent evaluation of the DGCNN / EdgeConv training-mode forward by torch.nn.functional on (B, C, K N) tensors, BatchNorm
with ``training=True``: what tests/test_dgcnn_train_host.py holds the restatement tests/dgcnn_train_ref.py against.  The dropout
multipliers are applied as the given masks; torch's own Dropout is not used.  The neighbours are GIVEN, from the restatement
(tests/dgcnn_torch_eval.py explains why: a float64 search could break a near-tie of the Float32 distances the other way).  As a
script it evaluates one saved case in float64 and float32 on the CPU,

    python tests/dgcnn_train_torch_eval.py in.npz out.npz

in: X, momentum, the parameters by name (their mu / sigma2 are the running statistics) and either
  ``layers`` and ``idx``: a generic EdgeConv with edgeconv_ref's names; its result is the layer's output (cL, N, B); or
  ``idx1``, ``idx2`` and optionally ``dropout4`` (512, B), ``dropout5`` (256, B): DGCNN; its result is the logits.
out, for T in 64, 32: resultT; statsT: every BatchNorm's batch mean and biased variance of what it is given, in the library's
statistics layout (per BatchNorm in forward order mean (C), variance (C)); runningT: running_mean / running_var after the step in
the same layout -- so that a test process that has loaded the HIP library never imports torch."""
import sys

import numpy as np


def forward_train(X, P, dtype, momentum, layers=None, idx=None, dropout=(None, None)):
    import torch
    import torch.nn.functional as Fn

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)

    T = {k: t(v[0].T[:, :, None] if k.endswith(".weight") and v.ndim == 3 else v) for k, v in P.items()}  # conv: (Cout, Cin, 1)
    x0 = t(np.transpose(np.asarray(X), (2, 0, 1)))  # (B, F, N)
    nbrs = [torch.from_numpy(np.ascontiguousarray(np.transpose(i, (2, 0, 1))).astype(np.int64)) for i in idx]  # (B, K, N)
    masks = [None if m is None else t(np.asarray(m).T) for m in dropout]
    stats, running = [], []

    def bn(x, name):
        dims = (0, 2) if x.dim() == 3 else (0,)
        stats.extend([x.mean(dim=dims), x.var(dim=dims, unbiased=False)])
        rm, rv = T[name + ".mu"].clone(), T[name + ".sigma2"].clone()
        y = Fn.batch_norm(x, rm, rv, weight=T[name + ".gamma"], bias=T[name + ".beta"], training=True, momentum=momentum, eps=1e-5)
        running.extend([rm, rv])  # updated in place: (1 - momentum) running + momentum (batch mean, unbiased batch variance)
        return y

    def block(x, conv, name):
        return torch.relu(bn(Fn.conv1d(x, T[conv + ".weight"], T[conv + ".bias"]), name))

    def fc(x, dense, name, mask):
        x = torch.relu(bn(Fn.linear(x, T[dense + ".weight"], T[dense + ".bias"]), name))
        return x if mask is None else x * mask

    def edgeconv(x, prefix, nblocks, nbr):
        B, F, N = x.shape
        K = nbr.shape[1]
        flat = nbr.reshape(B, 1, K * N).expand(B, F, K * N)
        xj = torch.gather(x, 2, flat)                     # (B, F, K N): column k N + n is neighbour k of point n
        xi = x.repeat(1, 1, K)                            # the same columns: point n
        a = torch.cat([xi, xj - xi], dim=1)
        for i in range(1, nblocks + 1):
            a = block(a, f"{prefix}conv{i}", f"{prefix}bn{i}")  # the statistics run over all B K N columns
        return a.reshape(B, -1, K, N).amax(dim=2)

    with torch.no_grad():
        if layers is not None:
            out = edgeconv(x0, "", len(layers) - 1, nbrs[0]).permute(1, 2, 0)  # (cL, N, B)
        else:
            x1 = edgeconv(x0, "ec1.", 3, nbrs[0])
            x2 = edgeconv(x1, "ec2.", 2, nbrs[1])
            a = block(x2, "conv3.conv", "conv3.bn").amax(dim=2)
            d = fc(fc(a, "fc4.dense", "fc4.bn", masks[0]), "fc5.dense", "fc5.bn", masks[1])
            out = Fn.linear(d, T["fc6.weight"], T["fc6.bias"]).T
    return out.contiguous().numpy(), torch.cat(stats).numpy(), torch.cat(running).numpy()


if __name__ == "__main__":
    import torch
    case = dict(np.load(sys.argv[1]))
    X, momentum = case.pop("X"), float(case.pop("momentum"))
    if "layers" in case:
        kw = dict(layers=[int(c) for c in case.pop("layers")], idx=[case.pop("idx")])
    else:
        kw = dict(idx=[case.pop("idx1"), case.pop("idx2")], dropout=(case.pop("dropout4", None), case.pop("dropout5", None)))
    out = {}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        out["result" + tag], out["stats" + tag], out["running" + tag] = forward_train(X, case, dtype, momentum, **kw)
    np.savez(sys.argv[2], **out)
