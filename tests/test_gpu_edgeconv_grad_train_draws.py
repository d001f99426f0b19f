"""The EdgeConv training-mode adjoint on the device beyond unit scale: fx.EdgeConv.grad_train against the host restatement
tests/edgeconv_grad_train_ref.py on training-mode families of tests/model_draws.py -- weights and inputs spread over decades, negative
gamma, subnormal inputs, a constant cloud (channels of zero variance, sd = sqrt(eps)) and a variance beyond Float32 (sd = +Inf)
-- at [5, 33, 70], 65 x 2, K = 6.

tests/test_gpu_model_draws_train.py's rule: every array is compared as uint32, no element left out; where the restatement has a
NaN the device must have one (payload not compared), +-Inf and both zeros bit for bit.  Every draw is first held to its family's
condition on the restatement's own forward (model_draws.check_train).  The upstream gradient is the draw's own ``g``
(model_draws.upstream serves PointNet's logits only).  idx, out and batch_stats are the device's own forward_train's."""
import numpy as np
import pytest

import edgeconv_grad_train_ref as gref
import model_draws as md
from test_gpu_model_draws import _host, _same, _same_grads, _same_run

pytestmark = pytest.mark.gpu

LAYERS, N, B, K = md.EDGECONV[0]
FAMILIES = ("decades", "negative_gamma", "subnormal_input", "constant_cloud", "variance_overflow")


@pytest.mark.parametrize("family", FAMILIES)
def test_grad_train(gpu_fx, family):
    fx = gpu_fx
    assert (LAYERS, N, B, K) == ([5, 33, 70], 65, 2, 6)
    net = ("edgeconv", LAYERS)
    d = md.draw_train(family, net, N, B)
    want_fwd = md.restate_forward_train(net, d, K)
    md.check_train(family, net, d, want_fwd)
    m = fx.EdgeConv(LAYERS, K).load(d["P"])
    xd, gd = fx.gpu(d["X"]), fx.gpu(d["g"])
    fwd = m.forward_train(xd, intermediates=True)
    hf = {k: ({n: _host(v) for n, v in w.items()} if isinstance(w, dict) else _host(w)) for k, w in fwd.items()}
    _same(hf["idx"], want_fwd["idx"], f"{family}: idx against the oracle's search")
    _same(hf["out"], want_fwd["out"], f"{family}: out")
    want, wx = gref.grad(d["X"], d["P"], LAYERS, K, d["g"], hf["batch_stats"], hf["idx"], hf["out"])
    assert all(np.all(np.isfinite(v)) for v in want.values()) and np.all(np.isfinite(wx)), family
    assert np.count_nonzero(gref.family(want, LAYERS, "dW")) > 0
    assert (family == "variance_overflow") == (not wx.any()), family   # sd_1 = +Inf: nothing reaches X
    got, gx = m.grad_train(xd, gd, fwd=fwd)
    _same_grads({n: _host(v) for n, v in got.items()}, want, f"{family} grad_train")
    _same(gx, wx, f"{family} grad_train: gx")
    again, gx2 = m.grad_train(xd, gd)   # its own forward, a second run: NaN payloads included
    for n in got:
        _same_run(again[n], got[n], f"{family} grad_train, two runs: {n}")
    _same_run(gx2, gx, f"{family} grad_train, two runs: gx")
