"""The optimiser of the reference's classification tutorials (examples/pointnet_classification.jl, dgcnn_classification.jl:
``opt = Flux.ADAM(lr)``, ``Flux.update!(opt, ps, gs)``) over a model's flat device parameters, and one training step captured as a
graph.  include/flux3d_hip.h "Training step" states the arithmetic; :meth:`PointNet.train_step` / :meth:`DGCNN.train_step` is the
step."""
import numpy as np

from . import _lib
from .device import DeviceArray, Graph, Stream, current_stream, is_device, stream


class ADAM:
    """``Flux.Optimise.ADAM(eta, (beta1, beta2))`` with Flux's ``eps = 1e-8`` over one flat Float32 device buffer: fx3d_adam_step.
    The state -- ``m``, ``v`` (Float32, zero) and ``betap`` (two Float64, ``beta``) -- is created on the device at the first
    :meth:`update`; it mirrors :class:`fit.Momentum`."""

    def __init__(self, eta=0.001, beta=(0.9, 0.999), eps=1e-8):
        try:
            b1, b2 = beta
        except (TypeError, ValueError):
            raise TypeError(f"beta must be the pair (beta1, beta2), got {beta!r}") from None
        self.eta, self.beta, self.eps = float(eta), (float(b1), float(b2)), float(eps)
        if not np.isfinite(self.eta):
            raise ValueError(f"eta must be finite, got {eta}")
        if not all(0.0 <= b < 1.0 for b in self.beta):
            raise ValueError(f"beta1 and beta2 must be in [0, 1), got {beta}")
        if not self.eps >= 0.0:
            raise ValueError(f"eps must not be negative, got {eps}")
        self.m = self.v = self.betap = None

    def update(self, x, g, running=None, stat_map=None):
        """One ADAM step of the device buffer ``x`` along the gradient ``g`` (Float32, the same size), in place, in one library
        call.  ``running`` with ``stat_map`` (device Float32 and int32 of one size): ``x[stat_map[i]] = running[i]`` in the same
        call -- a model's running statistics into their slots, whose gradient is +0 (:meth:`train_step` passes them)."""
        for name, a in (("x", x), ("g", g)):
            if not is_device(a) or a.dtype != np.float32:
                raise TypeError(f"{name} must be a Float32 device array")
        if g.size != x.size:
            raise ValueError(f"g must have the size of x ({x.size}), got {g.size}")
        if (running is None) != (stat_map is None):
            raise ValueError("running and stat_map go together")
        nstat = 0
        if running is not None:
            if not (is_device(running) and running.dtype == np.float32 and is_device(stat_map) and stat_map.dtype == np.int32):
                raise TypeError("running must be a Float32 and stat_map an int32 device array")
            if running.size != stat_map.size:
                raise ValueError(f"running and stat_map must have one size, got {running.size} and {stat_map.size}")
            nstat = running.size
        if self.m is None:
            self.m, self.v = DeviceArray.zeros((x.size,), np.float32), DeviceArray.zeros((x.size,), np.float32)
            self.betap = DeviceArray.from_host(np.array(self.beta, np.float64))
        elif self.m.size != x.size:
            raise ValueError(f"this optimiser's state is for {self.m.size} parameters, got {x.size}")
        _lib.call("fx3d_adam_step", x.size, self.eta, self.beta[0], self.beta[1], self.eps, g.ptr, self.m.ptr, self.v.ptr,
                  self.betap.ptr, x.ptr, running.ptr if nstat else None, stat_map.ptr if nstat else None, nstat,
                  current_stream().handle)
        return x

    def state(self):
        """``(m, v, betap)``: the device arrays of the state (``None`` before the first update), for tests and checkpoints."""
        return self.m, self.v, self.betap


class TrainStepGraph:
    """One :meth:`train_step` of a classifier -- forward, loss, gradient, ADAM update, running statistics, the dropout draw and
    the advance of its counter -- captured as a graph and replayed with one launch per step, as :class:`fit.FitStepGraph` does
    for the mesh fit.

    ``x`` (3, N, B) Float32 and ``labels`` (B,) int32 are the graph's device buffers, filled from ``X`` and ``labels``: refill
    them between replays (:meth:`refill`, or ``copy_`` under the graph's stream).  ``seed``: of the dropout masks, drawn on the
    device under ``seed`` plus the device ``counter`` the graph advances by one per step; ``dropout=False``: no dropout.  The
    constructor runs step 1 eagerly on the graph's own stream (``first``: its :class:`StepResult`; workspaces, the device
    parameters and the optimiser's state exist afterwards) and records step 2; :meth:`step` replays it and returns ``out``, the
    :class:`StepResult` every replay writes.  The recording is one stream, one chain of launches."""

    def __init__(self, model, opt, X, labels, seed=0x5EED0C3, dropout=True, momentum=0.1):
        self.model, self.opt = model, opt
        pts, N, B, on_dev = model._clouds(X, model._WHY)
        y = model._step_labels(labels, B)
        self.stream = Stream.create()
        current_stream().synchronize()  # X / the parameters may still be in flight on the caller's stream
        with stream(self.stream):
            self.x = model._on_device(pts, N, B, on_dev)
            self.labels = y if is_device(y) else DeviceArray.from_host(y)
            self.counter = DeviceArray.zeros((1,), np.uint64)

        def body():
            out = model.train_step(self.x, self.labels, opt, dropout=("device", int(seed), self.counter) if dropout else None,
                                   momentum=momentum)
            _lib.call("fx3d_counter_add", self.counter.ptr, 1, current_stream().handle)
            return out

        with stream(self.stream):
            self.first = body()  # eager once on the capture stream: a real step
            self.stream.synchronize()
        self.steps = 1
        self.graph = Graph()
        with self.graph.capture(self.stream):
            self.out = body()

    def step(self):
        self.graph.launch(self.stream)
        self.steps += 1
        return self.out

    def refill(self, X, labels):
        """The next batch into the graph's buffers: host arrays (3, N, B) and (B,) of the shapes the graph was built with."""
        with stream(self.stream):
            self.x.copy_(np.asarray(X, np.float32).reshape(self.x.shape, order="F"))
            self.labels.copy_(self.model._labels(labels, self.labels.size).astype(np.int32))

    def synchronize(self):
        self.stream.synchronize()
