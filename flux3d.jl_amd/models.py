"""PointNet inference on the device (src/models/pointnet.jl): ``PointNet(num_classes, 64)(X)`` in test mode.

include/flux3d_hip.h states the network and its arithmetic ("PointNet inference"); this module owns the parameters (a name ->
numpy array mapping in Flux's shapes), flattens them into the one device buffer fx3d_pointnet_forward reads, and checks
every argument on the host before any launch.  Forward only: no training, no gradients."""
import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, current_stream, is_device, workspace
from .rep import PointCloud


def _stn_spec(prefix, K):
    """stnKD(K) (src/models/pointnet.jl:3-20)."""
    return [(f"{prefix}.conv1", "conv", (K, 64)), (f"{prefix}.bn1", "bn", 64),
            (f"{prefix}.conv2", "conv", (64, 128)), (f"{prefix}.bn2", "bn", 128),
            (f"{prefix}.conv3", "conv", (128, 1024)), (f"{prefix}.bn3", "bn", 1024),
            (f"{prefix}.dense1", "dense", (1024, 512)), (f"{prefix}.dense2", "dense", (512, 256)),
            (f"{prefix}.bn4", "bn", 256), (f"{prefix}.dense3", "dense", (256, K * K))]


def layer_spec(num_classes):
    """The layers that carry parameters, in forward order: (name, kind, channels) with channels = (in, out) or C."""
    return (_stn_spec("stn", 3) + [("conv_block1.conv", "conv", (3, 64)), ("conv_block1.bn", "bn", 64)] + _stn_spec("fstn", 64)
            + [("feat.conv1", "conv", (64, 128)), ("feat.bn1", "bn", 128), ("feat.conv2", "conv", (128, 1024)),
               ("feat.bn2", "bn", 1024), ("feat.dense1", "dense", (1024, 512)), ("feat.bn3", "bn", 512),
               ("feat.dense2", "dense", (512, 256)), ("feat.bn4", "bn", 256), ("cls", "dense", (256, int(num_classes)))])


def param_shapes(num_classes):
    """name -> shape of every parameter array, in the order of the flat buffer.  Flux's shapes: Conv((1,), Cin => Cout) has
    weight (1, Cin, Cout) and bias (Cout,); BatchNorm(C) has gamma, beta, mu, sigma2 (C,); Dense(in, out) has weight
    (out, in) and bias (out,)."""
    shapes = {}
    for name, kind, ch in layer_spec(num_classes):
        if kind == "conv":
            shapes[name + ".weight"], shapes[name + ".bias"] = (1, ch[0], ch[1]), (ch[1],)
        elif kind == "dense":
            shapes[name + ".weight"], shapes[name + ".bias"] = (ch[1], ch[0]), (ch[1],)
        else:
            for f in ("gamma", "beta", "mu", "sigma2"):
                shapes[f"{name}.{f}"] = (ch,)
    return shapes


class PointNet:
    """``PointNet(num_classes=10, K=64)`` (src/models/pointnet.jl:41-60).

    ``params``: name -> Float32 numpy array in Flux's shapes (:func:`param_shapes`).  A new model is filled the way Flux
    fills one -- Glorot-uniform weights, zero biases, BatchNorm gamma = 1, beta = 0, mu = 0, sigma2 = 1 -- from a numpy
    generator seeded with ``seed``: the reference's draws come from Julia's global RNG and cannot be reproduced here.
    ``load(params)`` replaces them (a trained model's arrays) after shape checks.  They are uploaded once, at the first
    forward after construction or ``load``, and the device copy is kept."""

    def __init__(self, num_classes=10, K=64, seed=0):
        if int(K) != 64:
            raise ValueError(f"PointNet(num_classes, K) needs K = 64, got {K}: the reference's conv_block1 has 64 output "
                             "channels whatever K is, so its batched_mul with the (K, K) feature transform throws for any other K")
        if int(num_classes) < 1:
            raise ValueError(f"num_classes must be positive, got {num_classes}")
        self.num_classes, self.K = int(num_classes), 64
        rng = np.random.default_rng(seed)
        self.params = {}
        for name, shape in param_shapes(self.num_classes).items():
            field = name.rsplit(".", 1)[1]
            if field == "weight":
                fan_in, fan_out = (shape[1], shape[2]) if len(shape) == 3 else (shape[1], shape[0])
                lim = np.sqrt(6.0 / (fan_in + fan_out))
                self.params[name] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
            else:
                self.params[name] = np.full(shape, 1.0 if field in ("gamma", "sigma2") else 0.0, np.float32)
        self._dev = None
        count = C.c_int64(0)
        _lib.call("fx3d_pointnet_param_count", self.num_classes, C.byref(count))
        self.param_count = count.value

    def load(self, params):
        """Replace the parameters: a mapping with exactly the names and shapes of :func:`param_shapes`."""
        shapes = param_shapes(self.num_classes)
        missing, extra = sorted(set(shapes) - set(params)), sorted(set(params) - set(shapes))
        if missing or extra:
            raise ValueError(f"parameter names do not match: missing {missing[:4]}, unknown {extra[:4]}")
        new = {}
        for name, shape in shapes.items():
            a = np.asarray(params[name])
            if a.shape != shape:
                raise ValueError(f"{name} must be {shape}, got {a.shape}")
            new[name] = np.array(a, dtype=np.float32)
        self.params, self._dev = new, None
        return self

    def flat_params(self):
        """The flat Float32 buffer of fx3d_pointnet_forward: every array column-major, in forward order."""
        flat = np.concatenate([self.params[n].ravel(order="F") for n in param_shapes(self.num_classes)]).astype(np.float32)
        assert flat.size == self.param_count, (flat.size, self.param_count)
        return flat

    def _params_dev(self):
        if self._dev is None:
            self._dev = DeviceArray.from_host(self.flat_params())
        return self._dev

    def forward(self, X, intermediates=False):
        """Class probabilities ``(num_classes, B)`` of the clouds ``X``: a PointCloud, a device array or a numpy array,
        ``(3, N, B)`` or ``(3, N)`` (one cloud).  The result lives where the input lives.  ``intermediates=True``: a dict
        with ``probs``, ``logits`` (num_classes, B), ``stn`` (3, 3, B), ``fstn`` (64, 64, B) and ``pooled`` (1024, B)."""
        pts = X.points if isinstance(X, PointCloud) else X
        on_dev = is_device(pts)
        if on_dev:
            if pts.dtype != np.float32:
                raise TypeError("device point arrays must be Float32")
            shape = pts.shape
        else:
            pts = np.asarray(pts, dtype=np.float32)
            shape = pts.shape
        if len(shape) == 2:
            shape = shape + (1,)
        if len(shape) != 3:
            raise ValueError(f"points must be (3, N) or (3, N, B), got {tuple(shape)}")
        if shape[0] != 3:
            raise ValueError(f"PointNet takes 3 channels per point (stnKD(3)), got {shape[0]}")
        N, B = int(shape[1]), int(shape[2])
        if N < 1 or B < 1:
            raise ValueError(f"PointNet needs at least one point and one cloud, got N={N}, B={B}")
        x = pts.reshape(3, N, B) if on_dev else DeviceArray.from_host(np.asfortranarray(pts.reshape(3, N, B, order="F")))
        nc = self.num_classes
        out = {"probs": DeviceArray.empty((nc, B), np.float32)}
        if intermediates:
            out.update(logits=DeviceArray.empty((nc, B), np.float32), stn=DeviceArray.empty((3, 3, B), np.float32),
                       fstn=DeviceArray.empty((64, 64, B), np.float32), pooled=DeviceArray.empty((1024, B), np.float32))
        nb = C.c_size_t(0)
        _lib.call("fx3d_pointnet_workspace_bytes", N, B, nc, C.byref(nb))
        ws = workspace(nb.value, tag="pointnet")
        opt = [out[k].ptr if intermediates else None for k in ("logits", "stn", "fstn", "pooled")]
        _lib.call("fx3d_pointnet_forward", self._params_dev().ptr, nc, x.ptr, N, B, out["probs"].ptr, *opt, ws.ptr, ws.nbytes,
                  current_stream().handle)
        if not on_dev:
            out = {k: v.to_host() for k, v in out.items()}
        return out if intermediates else out["probs"]

    __call__ = forward
