"""The DGCNN training-mode adjoint on the device beyond unit scale: fx.DGCNN.grad_train against the host restatement
tests/dgcnn_grad_train_ref.py on training-mode families of tests/model_draws.py -- weights and inputs spread over decades, negative
gamma, subnormal inputs, values of 1e20, a variance beyond Float32 (sd = +Inf) and a cloud that is one point (channels of zero
variance, sd = sqrt(eps)) -- at md.DGCNN: 65 x 2, K = 3, 10 classes.

tests/test_gpu_model_draws_train.py's rule: every array is compared as uint32, no element left out; where the restatement has a
NaN the device must have one (payload not compared), +-Inf and both zeros bit for bit.  Every draw is first held to its family's
condition on the restatement's own forward (model_draws.check_train).  The upstream gradient is the draw's own ``g``.  idx1, x1,
idx2, x2, pooled and batch_stats are the device's own forward_train's."""
import numpy as np
import pytest

import dgcnn_grad_train_ref as gref
import model_draws as md
from test_gpu_model_draws import _host, _same, _same_grads, _same_run

pytestmark = pytest.mark.gpu

N, B, K, NC = md.DGCNN
FAMILIES = ("decades", "negative_gamma", "subnormal_input", "large", "variance_overflow", "one_point")


@pytest.mark.parametrize("family", FAMILIES)
def test_grad_train(gpu_fx, family):
    fx = gpu_fx
    assert (N, B, K, NC) == (65, 2, 3, 10)
    net = ("dgcnn", NC)
    d = md.draw_train(family, net, N, B)
    md.check_train(family, net, d, md.restate_forward_train(net, d, K))
    m = fx.DGCNN(NC, K, N).load(d["P"])
    xd, gd = fx.gpu(d["X"]), fx.gpu(d["g"])
    fwd = m.forward_train(xd, intermediates=True)
    hf = {k: ({n: _host(v) for n, v in w.items()} if isinstance(w, dict) else _host(w)) for k, w in fwd.items()}
    want, wx, wx2, wx1 = gref.grad_train(d["X"], d["P"], K, d["g"], hf)
    assert np.count_nonzero(gref.family(want, "dW")) > 0
    got, gx, mid = m.grad_train(xd, gd, fwd=fwd, intermediates=True)
    _same_grads({n: _host(v) for n, v in got.items()}, want, f"{family} grad_train")
    for name, g, w in (("gx", gx, wx), ("gx2", mid["gx2"], wx2), ("gx1", mid["gx1"], wx1)):
        _same(g, w, f"{family} grad_train: {name}")
    again, gx_again = m.grad_train(xd, gd)   # its own forward, a second run: NaN payloads included
    for n in got:
        _same_run(again[n], got[n], f"{family} grad_train, two runs: {n}")
    _same_run(gx_again, gx, f"{family} grad_train, two runs: gx")
