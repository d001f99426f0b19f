"""PointNet, DGCNN and EdgeConv inference on the device (src/models/pointnet.jl, src/models/dgcnn.jl):
``PointNet(num_classes, 64)(X)``, ``DGCNN(num_classes, K, npoints)(X)`` and the layer ``EdgeConv(layers, K)(X)`` in test mode.

include/flux3d_hip.h states the networks and their arithmetic ("PointNet inference", "DGCNN inference", "EdgeConv inference");
this module owns the parameters (a name -> numpy array mapping in Flux's shapes), flattens them into the one device buffer
fx3d_pointnet_forward / fx3d_dgcnn_forward / fx3d_edgeconv_forward reads, and checks every argument on the host before any
launch.  EdgeConv has its input gradient and its parameter gradients, and DGCNN and PointNet the gradients of the
whole network with respect to every parameter and to the input points (``DGCNN.grad`` over fx3d_dgcnn_grad, "DGCNN adjoint";
``PointNet.grad`` over fx3d_pointnet_grad, "PointNet adjoint"), all with BatchNorm in test mode.  PointNet also has its
training-mode forward (``PointNet.forward_train`` over fx3d_pointnet_forward_train, "PointNet training-mode forward") and that
forward's gradients (``PointNet.grad_train`` over fx3d_pointnet_grad_train, "PointNet training-mode adjoint"); DGCNN and EdgeConv have their training-mode forwards (``DGCNN.forward_train`` over
fx3d_dgcnn_forward_train, ``EdgeConv.forward_train`` over fx3d_edgeconv_forward_train, "DGCNN / EdgeConv training-mode forward") and those
forwards' gradients (``EdgeConv.grad_train`` over fx3d_edgeconv_grad_train, "EdgeConv training-mode adjoint"; ``DGCNN.grad_train`` over
fx3d_dgcnn_grad_train, "DGCNN training-mode adjoint").  ``stnKD(K)`` (src/models/pointnet.jl:3-20) is a layer of its own as well,
forward and training-mode forward (:class:`stnKD` over fx3d_stnkd_forward / fx3d_stnkd_forward_train, include/flux3d_hip_layers.h)."""
import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray, current_stream, is_device, workspace
from .device import stream as stream_scope
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


def _shapes(spec):
    """name -> shape of every parameter array of a layer table, in the order of the flat buffer.  Flux's shapes:
    Conv((1,), Cin => Cout) has weight (1, Cin, Cout) and bias (Cout,); BatchNorm(C) has gamma, beta, mu, sigma2 (C,);
    Dense(in, out) has weight (out, in) and bias (out,)."""
    shapes = {}
    for name, kind, ch in spec:
        if kind == "conv":
            shapes[name + ".weight"], shapes[name + ".bias"] = (1, ch[0], ch[1]), (ch[1],)
        elif kind == "dense":
            shapes[name + ".weight"], shapes[name + ".bias"] = (ch[1], ch[0]), (ch[1],)
        else:
            for f in ("gamma", "beta", "mu", "sigma2"):
                shapes[f"{name}.{f}"] = (ch,)
    return shapes


def param_shapes(num_classes):
    """PointNet: name -> shape of every parameter array, in the order of the flat buffer (Flux's shapes, :func:`_shapes`)."""
    return _shapes(layer_spec(num_classes))


def dgcnn_layer_spec(num_classes):
    """DGCNN's layers that carry parameters, in forward order (src/models/dgcnn.jl:18-30,99-111): EdgeConv([3, 32, 64, 64], K)
    has conv_bn_blocks 6 => 32, 32 => 64, 64 => 64; EdgeConv([64, 128, 256], K) has 128 => 128, 128 => 256."""
    return [("ec1.conv1", "conv", (6, 32)), ("ec1.bn1", "bn", 32), ("ec1.conv2", "conv", (32, 64)), ("ec1.bn2", "bn", 64),
            ("ec1.conv3", "conv", (64, 64)), ("ec1.bn3", "bn", 64),
            ("ec2.conv1", "conv", (128, 128)), ("ec2.bn1", "bn", 128), ("ec2.conv2", "conv", (128, 256)), ("ec2.bn2", "bn", 256),
            ("conv3.conv", "conv", (256, 1024)), ("conv3.bn", "bn", 1024),
            ("fc4.dense", "dense", (1024, 512)), ("fc4.bn", "bn", 512), ("fc5.dense", "dense", (512, 256)), ("fc5.bn", "bn", 256),
            ("fc6", "dense", (256, int(num_classes)))]


def dgcnn_param_shapes(num_classes):
    """DGCNN: name -> shape of every parameter array, in the order of the flat buffer (Flux's shapes, :func:`_shapes`)."""
    return _shapes(dgcnn_layer_spec(num_classes))


def edgeconv_layer_spec(layers):
    """EdgeConv(layers, K)'s layers that carry parameters, in forward order (src/models/dgcnn.jl:18-30): conv_bn_blocks
    2 layers[0] => layers[1], layers[1] => layers[2], ..."""
    spec = []
    for i in range(1, len(layers)):
        spec += [(f"conv{i}", "conv", (2 * layers[0] if i == 1 else layers[i - 1], layers[i])), (f"bn{i}", "bn", layers[i])]
    return spec


def edgeconv_param_shapes(layers):
    """EdgeConv: name -> shape of every parameter array, in the order of the flat buffer (Flux's shapes, :func:`_shapes`)."""
    return _shapes(edgeconv_layer_spec([int(c) for c in layers]))


class _Model:
    """What the models share: the parameters (name -> Float32 numpy array in Flux's shapes), their flat device copy, the
    check of the input clouds and the classifiers' forward.  A subclass sets ``_NAME``, ``_COUNT_FN`` and ``_shapes()``, ``_count_args()`` where
    the count is not a function of ``num_classes``, and a classifier ``_WHY`` (the layer that fixes its 3 input channels) and the
    data of its entry points (below: "the classifiers' training-mode path") for the shared ``forward_train``, ``grad`` /
    ``flat_grad`` / ``crossentropy_grad`` bodies, their ``_train`` forms and ``train_step``."""

    def _count_args(self):
        return (self.num_classes,)

    def _init_params(self, seed):
        """Filled the way Flux fills a new model -- Glorot-uniform weights, zero biases, BatchNorm gamma = 1, beta = 0, mu = 0,
        sigma2 = 1 -- from a numpy generator seeded with ``seed``."""
        rng = np.random.default_rng(seed)
        self.params = {}
        for name, shape in self._shapes().items():
            field = name.rsplit(".", 1)[1]
            if field == "weight":
                fan_in, fan_out = (shape[1], shape[2]) if len(shape) == 3 else (shape[1], shape[0])
                lim = np.sqrt(6.0 / (fan_in + fan_out))
                self.params[name] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
            else:
                self.params[name] = np.full(shape, 1.0 if field in ("gamma", "sigma2") else 0.0, np.float32)
        self._dev, self._stale, self._smap = None, False, None
        count = C.c_int64(0)
        _lib.call(self._COUNT_FN, *self._count_args(), C.byref(count))
        self.param_count = count.value

    def load(self, params):
        """Replace the parameters: a mapping with exactly the names and shapes of the model's ``param_shapes``."""
        shapes = self._shapes()
        missing, extra = sorted(set(shapes) - set(params)), sorted(set(params) - set(shapes))
        if missing or extra:
            raise ValueError(f"parameter names do not match: missing {missing[:4]}, unknown {extra[:4]}")
        new = {}
        for name, shape in shapes.items():
            a = np.asarray(params[name])
            if a.shape != shape:
                raise ValueError(f"{name} must be {shape}, got {a.shape}")
            new[name] = np.array(a, dtype=np.float32)
        self.params, self._dev, self._stale = new, None, False
        return self

    def flat_params(self):
        """The flat Float32 buffer the forward entry point reads: every array column-major, in forward order.  After a
        :meth:`train_step` the device copy is the authority: it is pulled into ``params`` first (:meth:`pull_params`)."""
        if self._stale:
            self.pull_params()
        flat = np.concatenate([self.params[n].ravel(order="F") for n in self._shapes()]).astype(np.float32)
        assert flat.size == self.param_count, (flat.size, self.param_count)
        return flat

    def _params_dev(self):
        if self._dev is None:
            self._dev = DeviceArray.from_host(self.flat_params())
        return self._dev

    def pull_params(self):
        """Read the kept device copy of the parameters back into ``params`` (which :meth:`train_step` leaves stale: it updates the
        device copy only) and return ``params``.  Synchronises the current stream."""
        if self._dev is not None:
            flat, at = self._dev.to_host(), 0
            for name, shape in self._shapes().items():
                n = int(np.prod(shape))
                self.params[name] = flat[at:at + n].reshape(shape, order="F").copy(order="F")
                at += n
        self._stale = False
        return self.params

    def _clouds(self, X, why, F=3):
        """(the points, N, B, whether they are on the device) after the shape checks; nothing is uploaded yet.  F: the
        channels per point the model takes, `why` the layer that fixes them."""
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
            raise ValueError(f"points must be ({F}, N) or ({F}, N, B), got {tuple(shape)}")
        if shape[0] != F:
            raise ValueError(f"{self._NAME} takes {F} channels per point ({why}), got {shape[0]}")
        N, B = int(shape[1]), int(shape[2])
        if N < 1 or B < 1:
            raise ValueError(f"{self._NAME} needs at least one point and one cloud, got N={N}, B={B}")
        return pts, N, B, on_dev

    @staticmethod
    def _on_device(pts, N, B, on_dev, F=3):
        return pts.reshape(F, N, B) if on_dev else DeviceArray.from_host(np.asfortranarray(pts.reshape(F, N, B, order="F")))

    def _classify(self, clouds, entry, lead, size_args, optional, intermediates):
        """The forward of a classifier on the checked ``clouds`` (:meth:`_clouds`) through ``fx3d_{entry}_forward``, whose
        arguments are the parameters, ``lead``, x, N, B, probs, the optional outputs in the order of the table ``optional``
        (name -> (shape, dtype); allocated and passed with ``intermediates`` only) and the workspace of
        ``fx3d_{entry}_workspace_bytes(*size_args)``.  Probabilities, or the dict of all outputs, where the input lives."""
        pts, N, B, on_dev = clouds
        x = self._on_device(pts, N, B, on_dev)
        out = self._outputs(B, optional, intermediates)
        ws = workspace(_lib.query_bytes(f"fx3d_{entry}_workspace_bytes", *size_args), tag=entry)
        opt = [out[k].ptr if intermediates else None for k in optional]
        _lib.call(f"fx3d_{entry}_forward", self._params_dev().ptr, *lead, x.ptr, N, B, out["probs"].ptr, *opt, ws.ptr, ws.nbytes,
                  current_stream().handle)
        if not on_dev:
            out = {k: v.to_host() for k, v in out.items()}
        return out if intermediates else out["probs"]

    def _outputs(self, B, optional, intermediates):
        """``probs`` and, with ``intermediates``, the optional outputs of the table ``optional``, new on the device."""
        out = {"probs": DeviceArray.empty((self.num_classes, B), np.float32)}
        if intermediates:
            out.update({k: DeviceArray.empty(shape, dtype) for k, (shape, dtype) in optional.items()})
        return out

    @staticmethod
    def _like(a, name, shape, dtype, on_dev):
        """An argument of a model's ``grad`` after its checks, with exactly ``shape`` (a trailing batch axis of 1 may be left out): a
        device array, or a host array of ``dtype`` still to be uploaded.  It must live where ``X`` lives."""
        ok = (shape,) + ((shape[:-1],) if shape[-1] == 1 else ())
        what = "Float32" if dtype == np.float32 else "int32"
        if is_device(a) != on_dev:
            raise TypeError(f"{name} must live where X lives ({'the device' if on_dev else 'the host'})")
        if on_dev:
            if a.dtype != dtype:
                raise TypeError(f"device {name} must be {what}, got {a.dtype}")
            if tuple(a.shape) not in ok:
                raise ValueError(f"{name} must be {shape}, got {tuple(a.shape)}")
            return a.reshape(*shape)
        a = np.asarray(a)
        if dtype == np.int32:
            if not np.issubdtype(a.dtype, np.integer):
                raise TypeError(f"{name} must hold integers, got {a.dtype}")
        elif not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise TypeError(f"{name} must hold real numbers, got {a.dtype}")
        if a.shape not in ok:
            raise ValueError(f"{name} must be {shape}, got {a.shape}")
        return np.asfortranarray(a.reshape(shape, order="F").astype(dtype))

    def _grad_views(self, gp, on_dev):
        """The flat gradient ``gp`` (on the device) as a dict with the names and Flux shapes of the model's parameters, where
        ``X`` lives: views of the flat buffer on the device, of its host copy otherwise."""
        flat = None if on_dev else gp.to_host()
        grads, at = {}, 0
        for name, shape in self._shapes().items():
            n = int(np.prod(shape))
            if on_dev:  # a view of the flat buffer, which it keeps alive
                grads[name] = DeviceArray(gp.ptr + 4 * at, shape, np.float32, owned=False, keep=gp)
            else:
                grads[name] = flat[at:at + n].reshape(shape, order="F")
            at += n
        return grads

    def _stat_slots(self):
        """(BatchNorm name, C, offset in the statistics layout, offset of its ``mu`` in the flat parameter buffer) for the
        model's BatchNorms in forward order; in both buffers ``sigma2`` (C) follows ``mu`` (C) directly."""
        slots, at, flat = [], 0, 0
        for name, shape in self._shapes().items():
            if name.endswith(".mu"):
                slots.append((name[:-3], shape[0], at, flat))
                at += 2 * shape[0]
            flat += int(np.prod(shape))
        return slots

    @staticmethod
    def _momentum(momentum):
        """``momentum`` of the training-mode forwards after its check, a float."""
        momentum = float(momentum)
        if not (np.isfinite(momentum) and 0.0 <= momentum <= 1.0):
            raise ValueError(f"momentum must be finite and in [0, 1], got {momentum}")
        return momentum

    def _adopt_running(self, run, slots, stream):
        """``update=True`` of the training-mode forwards: the flat ``running`` buffer into the model's parameters, on the host
        (which reads it back: not inside a graph capture) and in the kept device copy."""
        host, params = run.to_host(), self._params_dev()
        for name, C, at, flat in slots:  # mu then sigma2, adjacent in both layouts
            self.params[name + ".mu"], self.params[name + ".sigma2"] = host[at:at + C].copy(), host[at + C:at + 2 * C].copy()
            _lib.call("fx3d_memcpy_d2d", params.ptr + 4 * flat, run.ptr + 4 * at, 8 * C, stream)

    @staticmethod
    def _named_stats(buf, slots, on_dev):
        """A flat statistics buffer on the device as name -> array under the ``...bnK.mu`` / ``.sigma2`` names: views of the
        buffer on the device, of its host copy otherwise."""
        named, host = {}, (None if on_dev else buf.to_host())
        for name, C, at, _ in slots:
            for f, o in ((".mu", at), (".sigma2", at + C)):
                named[name + f] = (DeviceArray(buf.ptr + 4 * o, (C,), np.float32, owned=False, keep=buf) if on_dev else host[o:o + C])
        return named

    def _labels(self, labels, B):
        """``labels`` of ``crossentropy_grad`` after their checks: B integers in [0, num_classes)."""
        y = np.asarray(labels)
        if not np.issubdtype(y.dtype, np.integer):
            raise TypeError(f"labels must hold integers, got {y.dtype}")
        if y.shape != (B,):
            raise ValueError(f"labels must be ({B},), got {y.shape}")
        if y.size and (y.min() < 0 or y.max() >= self.num_classes):
            raise ValueError(f"labels must be in [0, {self.num_classes}), got values from {y.min()} to {y.max()}")
        return y

    def _crossentropy(self, probs, y, B):
        """``(loss, glogits)`` of ``Flux.crossentropy(probs, onehot(y))`` from the host copy of ``probs``: the loss
        ``-mean_b log(probs[y_b, b])`` in float64 (a Python float), ``glogits[o, b] = (probs[o, b] - [o == y_b]) / Float32(B)``
        with one Float32 subtraction and one Float32 division."""
        cols = np.arange(B)
        with np.errstate(divide="ignore"):
            loss = float(-np.mean(np.log(probs[y, cols].astype(np.float64))))
        onehot = np.zeros((self.num_classes, B), np.float32)
        onehot[y, cols] = 1
        return loss, np.asfortranarray(((probs - onehot).astype(np.float32) / np.float32(B)).astype(np.float32))

    def _grads(self, named, X, glogits, input_grad, intermediates, **fwd):
        """What a classifier's ``grad`` (``named``) and ``flat_grad`` return, from its ``_grad_call(X, glogits, input_grad,
        intermediates, **fwd)``: the parameter gradients as named views or as the flat buffer, ``gx`` and, with
        ``intermediates``, ``mid``, all where ``X`` lives."""
        gp, gx, mid, on_dev = self._grad_call(X, glogits, input_grad, intermediates, **fwd)
        if not on_dev:
            gx = None if gx is None else gx.to_host()
            mid = None if mid is None else {k: v.to_host() for k, v in mid.items()}
        g = self._grad_views(gp, on_dev) if named else (gp if on_dev else gp.to_host())
        return (g, gx, mid) if intermediates else (g, gx)

    def _crossentropy_grad(self, X, labels, with_fwd):
        """A classifier's ``crossentropy_grad``: one forward (``with_fwd``: with its intermediates, which :meth:`grad` is then
        given as ``fwd``), the loss and ``glogits`` on the host (:meth:`_crossentropy`), then :meth:`grad`."""
        _, N, B, on_dev = self._clouds(X, self._WHY)
        y = self._labels(labels, B)
        fwd = self.forward(X, intermediates=with_fwd)
        probs = fwd["probs"] if with_fwd else fwd
        loss, glogits = self._crossentropy(probs.to_host() if on_dev else probs, y, B)
        grads, gx = self.grad(X, DeviceArray.from_host(glogits) if on_dev else glogits, **({"fwd": fwd} if with_fwd else {}))
        return loss, grads, gx

    # ---- the classifiers' training-mode path and adjoint calls.  A classifier sets _ENTRY (the stem of its fx3d_{entry}_* entry
    #      points), _FWD_KEYS (the forward's intermediates its adjoints take, in argument order) and _MID (the adjoints' optional
    #      outputs: name -> (rows, columns or None for N)), and has _lead() (the entries' arguments between the parameters and x),
    #      _sizes(N, B) (the workspace queries' arguments), _optional(N, B) and _masks_of(dropout, B, on_dev) (``dropout`` after its
    #      checks: one entry per Dropout layer, each None, a device array, or a host array still to be uploaded)
    def _train_bytes(self, N, B):
        return _lib.query_bytes(f"fx3d_{self._ENTRY}_train_workspace_bytes", *self._sizes(N, B))

    def _as_dropout(self, masks):
        """Checked masks in the form the public ``dropout`` argument takes them: the array where the model has one Dropout layer."""
        return masks[0] if len(self._DROPOUT[0]) == 1 else tuple(masks)

    def _forward_train(self, X, dropout, momentum, update, intermediates):
        """A classifier's :meth:`forward_train`."""
        pts, N, B, on_dev = self._clouds(X, self._WHY)
        if B < 2:
            raise ValueError(f"training-mode BatchNorm needs at least two clouds (a Dense BatchNorm's running variance divides by "
                             f"B - 1), got B={B}")
        momentum = self._momentum(momentum)
        masks = self._masks_of(dropout, B, on_dev)
        nb = self._train_bytes(N, B)  # (the library's own size limits)
        masks = [m if m is None or is_device(m) else DeviceArray.from_host(m) for m in masks]
        x = self._on_device(pts, N, B, on_dev)
        slots = self._stat_slots()
        out, stats = self._forward_train_call(x, N, B, masks, momentum, nb, intermediates, intermediates or update)
        if update:
            self._adopt_running(stats["running"], slots, current_stream().handle)
        if not intermediates:
            return out["probs"] if on_dev else out["probs"].to_host()
        for key, buf in stats.items():
            out[key] = self._named_stats(buf, slots, on_dev)
        if not on_dev:
            out = {k: (v if isinstance(v, dict) else v.to_host()) for k, v in out.items()}
        return out

    def _forward_train_call(self, x, N, B, masks, momentum, nb, intermediates, running):
        """fx3d_{entry}_forward_train on the device arrays ``x`` and ``masks`` (each possibly ``None``) with a workspace of ``nb``
        bytes: ``(out, stats)`` -- ``probs`` and, with ``intermediates``, the optional outputs; the flat ``batch_stats`` and, with
        ``running``, the flat ``running``."""
        f32 = np.float32
        slots = self._stat_slots()
        nstat = slots[-1][2] + 2 * slots[-1][1]
        optional = self._optional(N, B)
        out = self._outputs(B, optional, intermediates)
        stats = {"batch_stats": DeviceArray.empty((nstat,), f32)}
        if running:
            stats["running"] = DeviceArray.empty((nstat,), f32)
        ws = workspace(nb, tag=f"{self._ENTRY}_train")
        _lib.call(f"fx3d_{self._ENTRY}_forward_train", self._params_dev().ptr, *self._lead(), x.ptr, N, B,
                  *(m.ptr if m is not None else None for m in masks), momentum, out["probs"].ptr,
                  *(out[k].ptr if intermediates else None for k in optional), stats["batch_stats"].ptr,
                  stats["running"].ptr if running else None, ws.ptr, ws.nbytes, current_stream().handle)
        return out, stats

    def _grad_train_call(self, x, N, B, masks, out, batch_stats, glogits):
        """fx3d_{entry}_grad_train on device arrays, the forward's intermediates ``out`` and its flat ``batch_stats`` as it wrote
        them: the flat gradient."""
        entry = f"{self._ENTRY}_grad_train"
        ws = workspace(_lib.query_bytes(f"fx3d_{entry}_workspace_bytes", *self._sizes(N, B)), tag=entry)
        gp = DeviceArray.empty((self.param_count,), np.float32)
        _lib.call(f"fx3d_{entry}", self._params_dev().ptr, *self._lead(), x.ptr, N, B, *(m.ptr if m is not None else None for m in masks),
                  *(out[k].ptr for k in self._FWD_KEYS), batch_stats.ptr, glogits.ptr, gp.ptr, *([None] * (1 + len(self._MID))),
                  ws.ptr, ws.nbytes, current_stream().handle)
        return gp

    def _grad_call(self, X, glogits, input_grad, intermediates, fwd=None, train=False, dropout=None):
        """fx3d_{entry}_grad (``train``: fx3d_{entry}_grad_train, with the dropout multipliers and with the intermediates and batch
        statistics of ``fwd``, or of a :meth:`forward_train` run here) after the argument checks: (the flat gradient, gx or None,
        the intermediates or None) on the device, and whether ``X`` lives there.  Every refusal comes before any device work."""
        pts, N, B, on_dev = self._clouds(X, self._WHY)
        nc, f32 = self.num_classes, np.float32
        entry = f"fx3d_{self._ENTRY}_grad" + ("_train" if train else "")
        if train:
            if B < 2:
                raise ValueError(f"training-mode BatchNorm needs at least two clouds, got B={B}")
            masks = self._masks_of(dropout, B, on_dev)
            slots = self._stat_slots()
            nstat = slots[-1][2] + 2 * slots[-1][1]
            names = [bn + f for bn, *_ in slots for f in (".mu", ".sigma2")]
            if fwd is not None:
                if not isinstance(fwd, dict) or "batch_stats" not in fwd:
                    raise TypeError("fwd must be the dict of forward_train(..., intermediates=True)")
                named = fwd["batch_stats"]
                if not isinstance(named, dict) or [k for k in named] != names:
                    raise ValueError(f"fwd['batch_stats'] must hold mu and sigma2 of the {len(slots)} BatchNorms in forward order")
                for (bn, C_, _, _) in slots:
                    for f in (".mu", ".sigma2"):
                        v = named[bn + f]
                        if is_device(v) != on_dev:
                            raise TypeError("fwd must live where X lives")
                        if tuple(v.shape) != (C_,) or v.dtype != f32:
                            raise ValueError(f"fwd['batch_stats'][{bn + f!r}] must be Float32 ({C_},), got {v.dtype} {tuple(v.shape)}")
        nb = _lib.query_bytes(entry + "_workspace_bytes", *self._sizes(N, B))  # (the library's own size limits)
        g = self._like(glogits, "glogits", (nc, B), f32, on_dev)
        given = [None] * len(self._FWD_KEYS)
        if fwd is not None:
            missing = [k for k in self._FWD_KEYS if k not in fwd]
            if missing:
                raise ValueError(f"fwd must be the dict of forward{'_train' if train else ''}(X, intermediates=True): it has no {missing}")
            shapes = self._optional(N, B)
            given = [self._like(fwd[k], f"fwd['{k}']", *shapes[k], on_dev) for k in self._FWD_KEYS]
            for k, a in zip(self._FWD_KEYS, given):
                if not on_dev and a.dtype == np.int32 and a.size and (a.min() < 0 or a.max() >= N):
                    raise ValueError(f"fwd['{k}'] must hold 0-based indices in [0, {N}), got values from {a.min()} to {a.max()}")
        if not on_dev:
            g = DeviceArray.from_host(g)
            given = [None if a is None else DeviceArray.from_host(a) for a in given]
        x = self._on_device(pts, N, B, on_dev)
        stream = current_stream().handle
        lead = ()
        if train:
            masks = [m if m is None or is_device(m) else DeviceArray.from_host(m) for m in masks]
            if fwd is None:
                fwd_made = self.forward_train(x, dropout=None if dropout is None else self._as_dropout(masks), intermediates=True)
                given, named = [fwd_made[k] for k in self._FWD_KEYS], fwd_made["batch_stats"]
            # the BatchNorms' statistics (views of forward_train's buffer, or the caller's arrays) as one buffer in the layout's order
            if on_dev or fwd is None:
                stats = DeviceArray.empty((nstat,), f32)
                for bn, C_, at, _ in slots:
                    for fld, off in ((".mu", at), (".sigma2", at + C_)):
                        _lib.call("fx3d_memcpy_d2d", stats.ptr + 4 * off, named[bn + fld].ptr, 4 * C_, stream)
            else:
                stats = DeviceArray.from_host(np.concatenate([np.asarray(named[k], f32) for k in names]))
            lead = tuple(m.ptr if m is not None else None for m in masks)
        gp = DeviceArray.empty((self.param_count,), f32)
        gx = DeviceArray.empty((3, N, B), f32) if input_grad else None
        mid = {k: DeviceArray.empty((r, N if c is None else c, B), f32) for k, (r, c) in self._MID.items()} if intermediates else None
        ws = workspace(nb, tag=entry[5:])
        _lib.call(entry, self._params_dev().ptr, *self._lead(), x.ptr, N, B, *lead, *(None if a is None else a.ptr for a in given),
                  *((stats.ptr,) if train else ()), g.ptr, gp.ptr, gx.ptr if gx is not None else None,
                  *(mid[k].ptr if mid else None for k in self._MID), ws.ptr, ws.nbytes, stream)
        return gp, gx, mid, on_dev

    def _crossentropy_grad_train(self, X, labels, dropout):
        """A classifier's :meth:`crossentropy_grad_train`."""
        _, N, B, on_dev = self._clouds(X, self._WHY)
        y = self._labels(labels, B)
        if isinstance(dropout, (int, np.integer)):  # drawn once, for the forward and the adjoint
            masks = self._masks_of(int(dropout), B, on_dev)
            dropout = self._as_dropout([DeviceArray.from_host(m) for m in masks] if on_dev else masks)
        fwd = self.forward_train(X, dropout=dropout, intermediates=True)
        probs = fwd["probs"]
        loss, glogits = self._crossentropy(probs.to_host() if on_dev else probs, y, B)
        grads, gx = self.grad_train(X, DeviceArray.from_host(glogits) if on_dev else glogits, dropout=dropout, fwd=fwd)
        return loss, grads, gx

    # ---- the training step (include/flux3d_hip.h "Training step"): a classifier sets _STAT_FN, _DROPOUT (rows of each mask, p)
    #      and _GRAD_NEEDS_FWD
    def _stat_map(self):
        """The device int32 map of fx3d_adam_step: for every element of the flat statistics buffer its index in the flat parameter
        buffer.  Built from the names: only ``mu`` / ``sigma2`` slots, the only ones whose gradient is always +0."""
        if self._smap is None:
            idx, at = [], 0
            for name, shape in self._shapes().items():
                n = int(np.prod(shape))
                if name.endswith((".mu", ".sigma2")):
                    idx.extend(range(at, at + n))
                at += n
            count = C.c_int64(0)
            _lib.call(self._STAT_FN, C.byref(count))
            slots = self._stat_slots()
            if len(idx) != count.value or any(idx[s] != f or idx[s + 2 * c - 1] != f + 2 * c - 1 for _, c, s, f in slots):
                raise AssertionError("the mu / sigma2 slots of the parameters do not match the statistics layout")
            self._smap = DeviceArray.from_host(np.array(idx, np.int32))
        return self._smap

    def _step_labels(self, labels, B):
        """``labels`` of :meth:`train_step` / :meth:`evaluate` after their checks: a device int32 ``(B,)`` array as it is (its values
        are checked on the device: ``counts[1]``), or host integers in [0, num_classes) as int32, still to be uploaded."""
        if is_device(labels):
            if labels.dtype != np.int32 or tuple(labels.shape) != (B,):
                raise TypeError(f"device labels must be int32 ({B},), got {labels.dtype} {tuple(labels.shape)}")
            return labels
        return self._labels(labels, B).astype(np.int32)

    def _step_masks(self, dropout, B, on_dev):
        """``dropout`` of :meth:`train_step` after its checks: ``("device", seed, counter or None)``, or one entry per Dropout
        layer as :meth:`forward_train` takes them (``None``, a device array, or a host array still to be uploaded)."""
        if isinstance(dropout, tuple) and len(dropout) == 3 and isinstance(dropout[0], str):
            kind, seed, counter = dropout
            if kind != "device" or not isinstance(seed, (int, np.integer)):
                raise ValueError('dropout drawn on the device is ("device", seed, counter) with an int seed')
            if counter is not None and not (is_device(counter) and counter.dtype == np.uint64 and counter.size == 1):
                raise TypeError("the dropout counter must be a device UInt64 array of one element, or None")
            return ("device", int(seed) & 0xFFFFFFFFFFFFFFFF, counter)
        return list(self._masks_of(dropout, B, on_dev))

    def _crossentropy_dev(self, probs, y, B):
        """fx3d_crossentropy on device ``probs`` and labels: (loss (1,) Float64, glogits, counts (2,) int32), all on the device."""
        loss, counts = DeviceArray.empty((1,), np.float64), DeviceArray.empty((2,), np.int32)
        glogits = DeviceArray.empty((self.num_classes, B), np.float32)
        _lib.call("fx3d_crossentropy", probs.ptr, y.ptr, self.num_classes, B, glogits.ptr, loss.ptr, counts.ptr, current_stream().handle)
        return loss, glogits, counts

    def train_step(self, X, labels, opt, dropout=None, momentum=0.1, intermediates=False):
        """One step of the reference's training loop (examples/pointnet_classification.jl, dgcnn_classification.jl) on the device:
        :meth:`forward_train` with its running statistics, ``Flux.crossentropy`` (fx3d_crossentropy), :meth:`grad_train` given that
        forward, then ``opt.update`` (:class:`ADAM`: fx3d_adam_step) on the kept device parameters, the running statistics
        written into their ``mu`` / ``sigma2`` slots by the same call.  ``X`` as in :meth:`forward_train`; ``labels``: B host
        integers in [0, num_classes) or a device int32 array; ``dropout``: ``None``, multipliers as in :meth:`forward_train`, or
        ``("device", seed, counter)`` for masks drawn by fx3d_dropout_mask under ``seed`` plus the device UInt64 ``counter``
        (``None``: 0), one stream id per Dropout layer in forward order.  Returns a :class:`StepResult`: ``loss`` (1,) Float64 and
        ``counts`` (2,) int32 stay on the device until they are read.  ``intermediates=True`` adds, as device arrays, ``probs``,
        ``logits``, ``glogits``, ``grad`` (the flat gradient), ``batch_stats`` and ``running`` (the flat buffers) and ``dropout``
        (the list of masks used).  Nothing is read back, uploaded or waited for unless ``X``, ``labels`` or the masks are host
        arrays, so the step can be captured (:class:`TrainStepGraph`).  Afterwards the device copy of the parameters is the
        authority: :meth:`pull_params` brings ``params`` up to date (``flat_params`` does so itself)."""
        pts, N, B, on_dev = self._clouds(X, self._WHY)
        if B < 2:
            raise ValueError(f"training-mode BatchNorm needs at least two clouds, got B={B}")
        if not callable(getattr(opt, "update", None)):
            raise TypeError("opt must be an optimiser with update(x, g, running, stat_map), such as ADAM")
        momentum = self._momentum(momentum)
        y = self._step_labels(labels, B)
        masks = self._step_masks(dropout, B, on_dev)
        nb = self._train_bytes(N, B)  # (the library's own size limits)
        smap, params = self._stat_map(), self._params_dev()
        x = self._on_device(pts, N, B, on_dev)
        if not is_device(y):
            y = DeviceArray.from_host(y)
        stream = current_stream().handle
        if isinstance(masks, tuple):  # drawn here, stream id = the Dropout layer's position
            _, seed, counter = masks
            masks = [DeviceArray.empty((rows, B), np.float32) for rows in self._DROPOUT[0]]
            for sid, mk in enumerate(masks):
                _lib.call("fx3d_dropout_mask", mk.size, self._DROPOUT[1], seed, counter.ptr if counter is not None else None, sid,
                          mk.ptr, stream)
        else:
            masks = [mk if mk is None or is_device(mk) else DeviceArray.from_host(mk) for mk in masks]
        out, stats = self._forward_train_call(x, N, B, masks, momentum, nb, intermediates or self._GRAD_NEEDS_FWD, True)
        loss, glogits, counts = self._crossentropy_dev(out["probs"], y, B)
        gp = self._grad_train_call(x, N, B, masks, out, stats["batch_stats"], glogits)
        opt.update(params, gp, running=stats["running"], stat_map=smap)
        self._stale = True
        extra = None
        if intermediates:
            extra = dict(probs=out["probs"], logits=out["logits"], glogits=glogits, grad=gp, batch_stats=stats["batch_stats"],
                         running=stats["running"], dropout=masks)
        return StepResult(loss, counts, current_stream(), extra)

    def evaluate(self, X, labels):
        """The tutorial's ``accuracy`` and loss on one batch: the test-mode :meth:`forward`, then fx3d_crossentropy.  The
        :class:`StepResult` of :meth:`train_step` (``loss``, ``correct``), read lazily."""
        pts, N, B, on_dev = self._clouds(X, self._WHY)
        y = self._step_labels(labels, B)
        probs = self.forward(self._on_device(pts, N, B, on_dev))
        if not is_device(y):
            y = DeviceArray.from_host(y)
        loss, _, counts = self._crossentropy_dev(probs, y, B)
        return StepResult(loss, counts, current_stream())


class StepResult:
    """What :meth:`train_step` and :meth:`evaluate` return.  ``loss`` (1,) Float64 and ``counts`` (2,) int32 -- the clouds
    classified correctly, the labels out of range -- are device arrays; ``float(result)`` / ``float(result.loss)`` and
    ``result.correct`` copy them to the host, which waits for the step, and nothing else does.  With ``intermediates`` the
    further device arrays are attributes too."""

    def __init__(self, loss, counts, on, extra=None):
        self.loss, self.counts, self._on = loss, counts, on
        self.__dict__.update(extra or {})

    def _read(self, a):
        with stream_scope(self._on):  # the copy is ordered behind the step on the stream the step ran on
            return a.to_host()

    def __float__(self):
        return float(self._read(self.loss)[0])

    @property
    def correct(self):
        """The number of clouds whose most probable class is their label; raises if a label was outside [0, num_classes)."""
        counts = self._read(self.counts)
        if counts[1]:
            raise ValueError(f"{int(counts[1])} labels are outside [0, num_classes): the loss is NaN")
        return int(counts[0])


class PointNet(_Model):
    """``PointNet(num_classes=10, K=64)`` (src/models/pointnet.jl:41-60).

    ``params``: name -> Float32 numpy array in Flux's shapes (:func:`param_shapes`).  A new model is filled the way Flux
    fills one -- Glorot-uniform weights, zero biases, BatchNorm gamma = 1, beta = 0, mu = 0, sigma2 = 1 -- from a numpy
    generator seeded with ``seed``: the reference's draws come from Julia's global RNG and cannot be reproduced here.
    ``load(params)`` replaces them (a trained model's arrays) after shape checks.  They are uploaded once, at the first
    forward after construction or ``load``, and the device copy is kept.

    The network has its gradients, in test mode (BatchNorm's running statistics are constants, Dropout is the identity):
    :meth:`grad` gives the gradient of ``sum(glogits * logits)`` with respect to every parameter and to the input points from
    one library call (include/flux3d_hip.h "PointNet adjoint"), :meth:`flat_grad` the same as one flat buffer,
    :meth:`crossentropy_grad` the loss ``Flux.crossentropy(m(X), onehot(labels))`` with its gradients.  The training-mode
    forward -- BatchNorm at the batch statistics, Dropout as a given mask, the updated running statistics -- is
    :meth:`forward_train` (include/flux3d_hip.h "PointNet training-mode forward"), and its gradients -- mu and sigma2 functions of
    the batch -- are :meth:`grad_train`, :meth:`flat_grad_train` and :meth:`crossentropy_grad_train` (include/flux3d_hip.h
    "PointNet training-mode adjoint")."""

    _NAME, _COUNT_FN, _WHY, _ENTRY = "PointNet", "fx3d_pointnet_param_count", "stnKD(3)", "pointnet"

    def __init__(self, num_classes=10, K=64, seed=0):
        if int(K) != 64:
            raise ValueError(f"PointNet(num_classes, K) needs K = 64, got {K}: the reference's conv_block1 has 64 output "
                             "channels whatever K is, so its batched_mul with the (K, K) feature transform throws for any other K")
        if int(num_classes) < 1:
            raise ValueError(f"num_classes must be positive, got {num_classes}")
        self.num_classes, self.K = int(num_classes), 64
        self._init_params(seed)

    def _shapes(self):
        return param_shapes(self.num_classes)

    def forward(self, X, intermediates=False):
        """Class probabilities ``(num_classes, B)`` of the clouds ``X``: a PointCloud, a device array or a numpy array,
        ``(3, N, B)`` or ``(3, N)`` (one cloud).  The result lives where the input lives.  ``intermediates=True``: a dict
        with ``probs``, ``logits`` (num_classes, B), ``stn`` (3, 3, B), ``fstn`` (64, 64, B) and ``pooled`` (1024, B)."""
        _, N, B, _ = clouds = self._clouds(X, self._WHY)
        return self._classify(clouds, self._ENTRY, self._lead(), self._sizes(N, B), self._optional(N, B), intermediates)

    __call__ = forward

    def _lead(self):
        return (self.num_classes,)

    def _sizes(self, N, B):
        return (N, B, self.num_classes)

    def _optional(self, N, B):
        """The forward entries' optional outputs in their argument order: name -> (shape, dtype)."""
        f32 = np.float32
        return {"logits": ((self.num_classes, B), f32), "stn": ((3, 3, B), f32), "fstn": ((64, 64, B), f32), "pooled": ((1024, B), f32)}

    @staticmethod
    def dropout_mask(B, seed, p=0.4):
        """The multipliers ``(256, B)`` Float32 of ``Dropout(p)`` in training mode for :meth:`forward_train`, from a numpy
        generator seeded with ``seed``: Flux's ``rand > p ? T(1 / (1 - p)) : 0`` per entry, so every entry is 0 or
        ``np.float32(1.0 / (1.0 - p))`` (bits 0x3FD55555 for p = 0.4).  The draws are numpy's, not Julia's."""
        if not 0.0 <= float(p) < 1.0:
            raise ValueError(f"p must be in [0, 1), got {p}")
        if int(B) < 1:
            raise ValueError(f"B must be positive, got {B}")
        u = np.random.default_rng(seed).random((256, int(B)))
        return np.asfortranarray(np.where(u > p, np.float32(1.0 / (1.0 - float(p))), np.float32(0.0)).astype(np.float32))

    def forward_train(self, X, dropout=None, momentum=0.1, update=False, intermediates=False):
        """Class probabilities ``(num_classes, B)`` of the clouds ``X`` (as in :meth:`forward`, at least two clouds) with the
        network in TRAINING mode: include/flux3d_hip.h "PointNet training-mode forward".  Every BatchNorm normalises by the
        mean and uncorrected variance of the current batch; ``dropout`` is ``None`` (the identity), a ``(256, B)`` array of
        multipliers for the output of ``feat``'s ``Dense(512, 256, relu)`` (numpy, or a device array beside a device ``X``), or an ``int`` seed for
        :meth:`dropout_mask`.  ``intermediates=True``: a dict with ``probs``, ``logits``, ``stn``, ``fstn``, ``pooled`` as
        :meth:`forward` gives them, ``batch_stats`` and ``running``: dicts name -> array with the ``...bnK.mu`` / ``.sigma2``
        names of :func:`param_shapes`, the batch statistics and the running statistics Flux's BatchNorm would hold after this
        step (``momentum``; computed from the model's ``mu`` / ``sigma2``).  Everything lives where ``X`` lives.
        ``update=True`` writes ``running`` into the model's parameters, on the host (which reads them back: not inside a graph
        capture) and in the kept device copy: the next :meth:`forward` is the test-mode network after one training step's worth
        of statistics.  The gradient of this forward is :meth:`grad_train`."""
        return self._forward_train(X, dropout, momentum, update, intermediates)

    _MID = {"gstn": (3, 3), "gfstn": (64, 64), "gh": (64, None), "gxt": (3, None)}  # fx3d_pointnet_grad's optional outputs, in order
    _FWD_KEYS, _STAT_FN, _DROPOUT, _GRAD_NEEDS_FWD = (), "fx3d_pointnet_stat_count", ((256,), 0.4), False  # (train_step)

    def _masks_of(self, dropout, B, on_dev):
        """``dropout`` of the training-mode methods after its checks, as a 1-tuple: ``None``, or the ``(256, B)`` multipliers (an
        ``int``: the seed of :meth:`dropout_mask`) as a device array, or as a host array still to be uploaded."""
        if dropout is None:
            return (None,)
        if isinstance(dropout, (int, np.integer)):
            return (self.dropout_mask(B, int(dropout)),)
        if is_device(dropout) and not on_dev:
            raise TypeError("a device dropout mask needs X on the device")
        return (self._like(dropout, "dropout", (256, B), np.float32, is_device(dropout)),)

    def flat_grad(self, X, glogits, input_grad=True, intermediates=False):
        """``(gflat, gx)``: the gradient of ``sum(glogits * logits)`` with respect to the parameters as ONE flat Float32 buffer
        with the layout of :meth:`flat_params` (the ``mu`` / ``sigma2`` slots are zero), and the gradient with respect to ``X``
        (``None`` with ``input_grad=False``).  Arguments, ``intermediates`` and placement as :meth:`grad`."""
        return self._grads(False, X, glogits, input_grad, intermediates)

    def grad(self, X, glogits, input_grad=True, intermediates=False):
        """``(grads, gx)``: the gradients of ``sum(glogits * logits)`` with respect to every parameter of the network and to
        the points ``X``, test mode: include/flux3d_hip.h "PointNet adjoint".  ``X`` as in :meth:`forward`; ``glogits``
        ``(num_classes, B)`` is the gradient with respect to the logits as :meth:`forward` returns them, after ``cls``'s relu
        (the softmax stays with the caller, see :meth:`crossentropy_grad`).  The forward runs again inside the call.  ``grads``
        has the names and Flux shapes of :func:`param_shapes` (on the device: views of one flat buffer); its ``mu`` /
        ``sigma2`` entries are zero.  ``gx`` is ``(3, N, B)``, or ``None`` with ``input_grad=False``.  ``intermediates=True``:
        ``(grads, gx, mid)`` with ``mid`` a dict of ``gstn`` (3, 3, B) and ``gfstn`` (64, 64, B), the gradients at the two
        transforms, ``gh`` (64, N, B), the gradient at conv_block1's output, and ``gxt`` (3, N, B), the gradient at the
        transformed points.  Everything lives where ``X`` lives."""
        return self._grads(True, X, glogits, input_grad, intermediates)

    def grad_train(self, X, glogits, dropout=None, fwd=None, input_grad=True, intermediates=False):
        """:meth:`grad` for the TRAINING-mode network: the gradients of ``sum(glogits * logits)`` for the logits of
        :meth:`forward_train` ``(X, dropout)``, with every BatchNorm's mean and variance functions of the batch and the dropout
        multipliers constants: include/flux3d_hip.h "PointNet training-mode adjoint".  ``dropout`` as in :meth:`forward_train`.
        ``fwd``: the dict of ``forward_train(X, dropout, intermediates=True)`` for the same ``X`` and ``dropout``, whose batch
        statistics are then used; without it :meth:`forward_train` runs first.  Returns what :meth:`grad` returns (the ``mu`` /
        ``sigma2`` entries are zero: the running statistics do not enter this forward).  At least two clouds."""
        return self._grads(True, X, glogits, input_grad, intermediates, train=True, dropout=dropout, fwd=fwd)

    def flat_grad_train(self, X, glogits, dropout=None, fwd=None, input_grad=True, intermediates=False):
        """:meth:`grad_train` with the parameter gradients as one flat buffer, as :meth:`flat_grad`."""
        return self._grads(False, X, glogits, input_grad, intermediates, train=True, dropout=dropout, fwd=fwd)

    def crossentropy_grad(self, X, labels):
        """``(loss, grads, gx)`` for ``Flux.crossentropy(m(X), onehot(labels))``, the mean over the batch: ``labels`` are B
        integers in [0, num_classes), 0-based.  One :meth:`forward` for ``probs``, which are read back to the host; ``loss =
        -mean_b log(probs[y_b, b])`` in float64 (a Python float), ``glogits[o, b] = (probs[o, b] - [o == y_b]) / Float32(B)``
        with one Float32 subtraction and one Float32 division, then :meth:`grad`, inside which the forward runs again."""
        return self._crossentropy_grad(X, labels, with_fwd=False)

    def crossentropy_grad_train(self, X, labels, dropout=None):
        """:meth:`crossentropy_grad` on :meth:`forward_train`'s probabilities: ``(loss, grads, gx)`` of
        ``Flux.crossentropy(m(X), onehot(labels))`` with the network in training mode under the multipliers ``dropout`` (as in
        :meth:`forward_train`; an ``int`` seed is drawn once).  One :meth:`forward_train` with its intermediates, the loss and
        ``glogits`` on the host as in :meth:`crossentropy_grad`, then :meth:`grad_train` with that forward's statistics."""
        return self._crossentropy_grad_train(X, labels, dropout)


class DGCNN(_Model):
    """``DGCNN(num_classes=10, K=10, npoints=1024)`` (src/models/dgcnn.jl:99-111) in test mode: include/flux3d_hip.h
    "DGCNN inference" states the network and its arithmetic.

    ``params`` (:func:`dgcnn_param_shapes`), ``load``, ``flat_params`` and the seeded initialisation are PointNet's.
    ``npoints`` is the window of the reference's ``MaxPool((npoints,))`` over the (N, 1024, B) output of conv_3: only with
    N == npoints is that the one maximum per cloud and channel whose reshape gives the (1024, B) the classifier takes -- a
    multiple of npoints leaves several windows per cloud, which the reshape folds into the batch, anything else drops
    points.  ``forward`` therefore raises ``ValueError`` for clouds of any other size.

    The network has its gradients, in test mode (BatchNorm's running statistics are constants, Dropout is the identity, the
    neighbour lists are constants): :meth:`grad` gives the gradient of ``sum(glogits * logits)`` with respect to every parameter
    and to the input points from one library call (include/flux3d_hip.h "DGCNN adjoint"), :meth:`flat_grad` the same as one
    flat buffer, :meth:`crossentropy_grad` the loss ``Flux.crossentropy(m(X), onehot(labels))`` with its gradients.  The two
    EdgeConv stages inside are :meth:`EdgeConv.grad`'s kernel on the ``ec2.`` and ``ec1.`` parameters, bit for bit.  The
    training-mode forward -- BatchNorm at the batch statistics, the two Dropouts as given masks, the updated running statistics --
    is :meth:`forward_train` (include/flux3d_hip.h "DGCNN / EdgeConv training-mode forward"), and its gradients -- mu and sigma2
    functions of the batch -- are :meth:`grad_train`, :meth:`flat_grad_train` and :meth:`crossentropy_grad_train`
    (include/flux3d_hip.h "DGCNN training-mode adjoint")."""

    _NAME, _COUNT_FN, _WHY, _ENTRY = "DGCNN", "fx3d_dgcnn_param_count", "EdgeConv([3, 32, 64, 64], K)", "dgcnn"

    def __init__(self, num_classes=10, K=10, npoints=1024, seed=0):
        if int(num_classes) < 1:
            raise ValueError(f"num_classes must be positive, got {num_classes}")
        if int(K) < 1 or int(K) + 1 > int(npoints):
            raise ValueError(f"DGCNN needs 1 <= K <= npoints - 1 (K neighbours besides the point itself), got K={K}, npoints={npoints}")
        self.num_classes, self.K, self.npoints = int(num_classes), int(K), int(npoints)
        self._init_params(seed)

    def _shapes(self):
        return dgcnn_param_shapes(self.num_classes)

    def _clouds(self, X, why, F=3):
        """:meth:`_Model._clouds` for clouds of ``npoints`` points."""
        clouds = super()._clouds(X, why, F)
        if clouds[1] != self.npoints:
            raise ValueError(f"DGCNN(num_classes, K, npoints={self.npoints}) takes clouds of npoints points, got N={clouds[1]}: "
                             "MaxPool((npoints,)) is the maximum over a whole cloud only then")
        return clouds

    def forward(self, X, intermediates=False):
        """Class probabilities ``(num_classes, B)`` of the clouds ``X``: a PointCloud, a device array or a numpy array,
        ``(3, npoints, B)`` or ``(3, npoints)`` (one cloud).  The result lives where the input lives.
        ``intermediates=True``: a dict with ``probs``, ``logits`` (num_classes, B), ``idx1`` and ``idx2`` (K, N, B) int32,
        0-based, ``x1`` (64, N, B), ``x2`` (256, N, B) and ``pooled`` (1024, B)."""
        _, N, B, _ = clouds = self._clouds(X, self._WHY)
        return self._classify(clouds, self._ENTRY, self._lead(), self._sizes(N, B), self._optional(N, B), intermediates)

    __call__ = forward

    def _lead(self):
        return (self.num_classes, self.K)

    def _sizes(self, N, B):
        return (N, B, self.K, self.num_classes)

    def _optional(self, N, B):
        """The forward entries' optional outputs in their argument order: name -> (shape, dtype)."""
        nc, K, f32, i32 = self.num_classes, self.K, np.float32, np.int32
        return {"logits": ((nc, B), f32), "idx1": ((K, N, B), i32), "x1": ((64, N, B), f32), "idx2": ((K, N, B), i32),
                "x2": ((256, N, B), f32), "pooled": ((1024, B), f32)}

    @staticmethod
    def dropout_masks(B, seed, p=0.5):
        """The two arrays of multipliers, ``(512, B)`` and ``(256, B)`` Float32, of the ``Dropout(p)`` after ``fc_4`` and after
        ``fc_5`` in training mode for :meth:`forward_train`, from one numpy generator seeded with ``seed`` (the first mask is
        drawn first): Flux's ``rand > p ? T(1 / (1 - p)) : 0`` per entry, so every entry is 0 or ``np.float32(1.0 / (1.0 - p))``
        (``np.float32(2.0)`` for p = 0.5).  The draws are numpy's, not Julia's."""
        if not 0.0 <= float(p) < 1.0:
            raise ValueError(f"p must be in [0, 1), got {p}")
        if int(B) < 1:
            raise ValueError(f"B must be positive, got {B}")
        rng = np.random.default_rng(seed)
        keep = np.float32(1.0 / (1.0 - float(p)))
        return tuple(np.asfortranarray(np.where(rng.random((C_, int(B))) > p, keep, np.float32(0.0)).astype(np.float32))
                     for C_ in (512, 256))

    def _masks_of(self, dropout, B, on_dev):
        """``dropout`` of :meth:`forward_train` after its checks: ``(None, None)``, or the ``(512, B)`` and ``(256, B)``
        multipliers (an ``int``: the seed of :meth:`dropout_masks`), each a device array or a host array still to be uploaded."""
        if dropout is None:
            return None, None
        if isinstance(dropout, (int, np.integer)):
            return self.dropout_masks(B, int(dropout))
        if isinstance(dropout, (str, bytes)) or is_device(dropout) or isinstance(dropout, np.ndarray):
            raise TypeError("dropout must be None, an int seed or a pair of arrays (512, B) and (256, B)")
        try:
            m4, m5 = dropout
        except (TypeError, ValueError):
            raise TypeError("dropout must be None, an int seed or a pair of arrays (512, B) and (256, B)") from None
        masks = []
        for m, C_, name in ((m4, 512, "dropout[0]"), (m5, 256, "dropout[1]")):
            if is_device(m) and not on_dev:
                raise TypeError("a device dropout mask needs X on the device")
            masks.append(self._like(m, name, (C_, B), np.float32, is_device(m)))
        return tuple(masks)

    def forward_train(self, X, dropout=None, momentum=0.1, update=False, intermediates=False):
        """Class probabilities ``(num_classes, B)`` of the clouds ``X`` (as in :meth:`forward`, at least two clouds) with the
        network in TRAINING mode: include/flux3d_hip.h "DGCNN / EdgeConv training-mode forward".  All 8 BatchNorms normalise by
        the mean and uncorrected variance of the current batch (over the K N B edge rows in the EdgeConvs, the N B points at
        conv_3, the B clouds in the head); EdgeConv2's neighbours are searched on the training-mode ``x1``.  ``dropout`` is
        ``None`` (the identity), a pair of arrays of multipliers ``(512, B)`` and ``(256, B)`` for the outputs of ``fc_4`` and
        ``fc_5`` (numpy, or device arrays beside a device ``X``), or an ``int`` seed for :meth:`dropout_masks`.
        ``intermediates=True``: a dict with ``probs``, ``logits``, ``idx1``, ``x1``, ``idx2``, ``x2``, ``pooled`` as
        :meth:`forward` gives them, ``batch_stats`` and ``running``: dicts name -> array with the ``...bn.mu`` / ``.sigma2`` names
        of :func:`dgcnn_param_shapes`, the batch statistics and the running statistics Flux's BatchNorm would hold after this
        step (``momentum``; computed from the model's ``mu`` / ``sigma2``).  Everything lives where ``X`` lives.
        ``update=True`` writes ``running`` into the model's parameters, on the host (which reads them back: not inside a graph
        capture) and in the kept device copy: the next :meth:`forward` is the test-mode network after one training step's worth
        of statistics."""
        return self._forward_train(X, dropout, momentum, update, intermediates)

    _FWD_KEYS = ("idx1", "x1", "idx2", "x2", "pooled")
    _MID = {"gx2": (256, None), "gx1": (64, None)}  # fx3d_dgcnn_grad's optional outputs, in order
    _STAT_FN, _DROPOUT, _GRAD_NEEDS_FWD = "fx3d_dgcnn_stat_count", ((512, 256), 0.5), True  # (train_step)

    def flat_grad(self, X, glogits, fwd=None, input_grad=True, intermediates=False):
        """``(gflat, gx)``: the gradient of ``sum(glogits * logits)`` with respect to the parameters as ONE flat Float32 buffer
        with the layout of :meth:`flat_params` (the ``mu`` / ``sigma2`` slots are zero), and the gradient with respect to ``X``
        (``None`` with ``input_grad=False``).  Arguments, ``intermediates`` and placement as :meth:`grad`."""
        return self._grads(False, X, glogits, input_grad, intermediates, fwd=fwd)

    def grad(self, X, glogits, fwd=None, input_grad=True, intermediates=False):
        """``(grads, gx)``: the gradients of ``sum(glogits * logits)`` with respect to every parameter of the network and to
        the points ``X``, test mode: include/flux3d_hip.h "DGCNN adjoint".  ``X`` as in :meth:`forward`; ``glogits``
        ``(num_classes, B)`` is the gradient with respect to the logits (the softmax stays with the caller, see
        :meth:`crossentropy_grad`).  ``fwd``: the dict of ``forward(X, intermediates=True)``, whose ``idx1``, ``x1``, ``idx2``,
        ``x2`` and ``pooled`` are used; without it the forward runs again inside the call.  ``grads`` has the names and Flux
        shapes of :func:`dgcnn_param_shapes` (on the device: views of one flat buffer); its ``mu`` / ``sigma2`` entries are zero.
        ``gx`` is ``(3, N, B)``, or ``None`` with ``input_grad=False``.  ``intermediates=True``: ``(grads, gx, mid)`` with
        ``mid`` a dict of ``gx2`` (256, N, B) and ``gx1`` (64, N, B), the gradients at ``x2`` and ``x1``.  Everything lives where
        ``X`` lives."""
        return self._grads(True, X, glogits, input_grad, intermediates, fwd=fwd)

    def crossentropy_grad(self, X, labels):
        """``(loss, grads, gx)`` for ``Flux.crossentropy(m(X), onehot(labels))``, the mean over the batch: ``labels`` are B
        integers in [0, num_classes), 0-based.  One ``forward(X, intermediates=True)``; its ``probs`` are read back to the host,
        ``loss = -mean_b log(probs[y_b, b])`` in float64 (a Python float), ``glogits[o, b] = (probs[o, b] - [o == y_b]) /
        Float32(B)`` with one Float32 subtraction and one Float32 division, then :meth:`grad` with that forward."""
        return self._crossentropy_grad(X, labels, with_fwd=True)

    def grad_train(self, X, glogits, dropout=None, fwd=None, input_grad=True, intermediates=False):
        """:meth:`grad` for the TRAINING-mode network: the gradients of ``sum(glogits * logits)`` for the logits of
        :meth:`forward_train` ``(X, dropout)``, with every BatchNorm's mean and variance functions of the batch and the dropout
        multipliers and both neighbour lists constants: include/flux3d_hip.h "DGCNN training-mode adjoint".  ``dropout`` as in
        :meth:`forward_train`.  ``fwd``: the dict of ``forward_train(X, dropout, intermediates=True)`` for the same ``X`` and
        ``dropout``, whose ``idx1``, ``x1``, ``idx2``, ``x2``, ``pooled`` and ``batch_stats`` are then used; without it
        :meth:`forward_train` runs first.  Returns what :meth:`grad` returns (the ``mu`` / ``sigma2`` entries are zero: the
        running statistics do not enter this forward); ``intermediates=True`` adds ``mid`` with ``gx2`` and ``gx1``.  The two
        EdgeConv stages inside are :meth:`EdgeConv.grad_train`'s kernels, bit for bit.  At least two clouds."""
        return self._grads(True, X, glogits, input_grad, intermediates, fwd=fwd, train=True, dropout=dropout)

    def flat_grad_train(self, X, glogits, dropout=None, fwd=None, input_grad=True, intermediates=False):
        """:meth:`grad_train` with the parameter gradients as one flat buffer, as :meth:`flat_grad`."""
        return self._grads(False, X, glogits, input_grad, intermediates, fwd=fwd, train=True, dropout=dropout)

    def crossentropy_grad_train(self, X, labels, dropout=None):
        """:meth:`crossentropy_grad` on :meth:`forward_train`'s probabilities: ``(loss, grads, gx)`` of
        ``Flux.crossentropy(m(X), onehot(labels))`` with the network in training mode under the multipliers ``dropout`` (as in
        :meth:`forward_train`; an ``int`` seed is drawn once).  One :meth:`forward_train` with its intermediates, the loss and
        ``glogits`` on the host as in :meth:`crossentropy_grad`, then :meth:`grad_train` with that forward."""
        return self._crossentropy_grad_train(X, labels, dropout)


class EdgeConv(_Model):
    """``EdgeConv(layers, K)`` (src/models/dgcnn.jl:11-71) in test mode, as a layer in its own right: include/flux3d_hip.h
    "EdgeConv inference" states the layer, its arithmetic and the envelope.  ``layers = [F, c1, ..., cL]`` is the reference
    constructor's argument: L conv_bn_blocks 2F => c1, c1 => c2, ... on the edge rows [x_n, x_idx(k,n) - x_n] of the K nearest
    neighbours of every point, then the maximum over k.  1 <= L <= 4, 1 <= F <= 128, every width in [1, 256].

    ``params`` (:func:`edgeconv_param_shapes`: ``conv{i}.weight``, ``conv{i}.bias``, ``bn{i}.gamma`` / ``beta`` / ``mu`` /
    ``sigma2``), ``load``, ``flat_params`` and the seeded initialisation are the classifiers'.  The ``ec1.`` / ``ec2.`` arrays
    of a DGCNN, with that prefix dropped, are the parameters of ``EdgeConv([3, 32, 64, 64], K)`` / ``EdgeConv([64, 128, 256], K)``."""

    _NAME, _COUNT_FN = "EdgeConv", "fx3d_edgeconv_param_count"
    MAX_BLOCKS, MAX_F, MAX_WIDTH = 4, 128, 256

    def __init__(self, layers, K, seed=0):
        try:
            widths = [int(c) for c in layers]
            exact = all(c == w for c, w in zip(layers, widths))
        except (TypeError, ValueError):
            raise TypeError(f"layers must be a sequence of integers [F, c1, ..., cL], got {layers!r}") from None
        if not exact:
            raise TypeError(f"layers must be integers, got {list(layers)!r}")
        if not 2 <= len(widths) <= self.MAX_BLOCKS + 1:
            raise ValueError(f"EdgeConv takes F and 1 to {self.MAX_BLOCKS} widths, got {len(widths)} entries")
        if not 1 <= widths[0] <= self.MAX_F:
            raise ValueError(f"layers[0] = F must be in [1, {self.MAX_F}], got {widths[0]}")
        for i, c in enumerate(widths[1:], 1):
            if not 1 <= c <= self.MAX_WIDTH:
                raise ValueError(f"layers[{i}] must be in [1, {self.MAX_WIDTH}], got {c}")
        if int(K) < 1:
            raise ValueError(f"EdgeConv needs K >= 1 neighbours besides the point itself, got K={K}")
        self.layers, self.K = widths, int(K)
        self._init_params(seed)

    def _layers_c(self):
        return (C.c_int32 * len(self.layers))(*self.layers), len(self.layers)

    def _count_args(self):
        return self._layers_c()

    def _shapes(self):
        return edgeconv_param_shapes(self.layers)

    def _neighbours(self, idx, N, B):
        """The caller's lists as a (K, N, B) int32 device array.  Host lists are range-checked here; lists that are on the
        device already are used as they are (an index outside [0, N) reads the point itself, flux3d_hip.h)."""
        K = self.K
        if is_device(idx):
            if idx.dtype != np.int32:
                raise TypeError(f"device neighbour lists must be int32, got {idx.dtype}")
            if tuple(idx.shape) not in ((K, N, B),) + (((K, N),) if B == 1 else ()):
                raise ValueError(f"idx must be ({K}, {N}, {B}), got {tuple(idx.shape)}")
            return idx.reshape(K, N, B)
        a = np.asarray(idx)
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"idx must hold integers, got {a.dtype}")
        if a.shape not in ((K, N, B),) + (((K, N),) if B == 1 else ()):
            raise ValueError(f"idx must be ({K}, {N}, {B}), got {a.shape}")
        if a.size and (a.min() < 0 or a.max() >= N):
            raise ValueError(f"idx must hold 0-based indices in [0, {N}), got values from {a.min()} to {a.max()}")
        return DeviceArray.from_host(np.asfortranarray(a.reshape(K, N, B, order="F").astype(np.int32)))

    def _head(self, X):
        """The checks every call begins with, in their order: a PointCloud only for F = 3, the clouds (:meth:`_clouds`), K against
        N.  ``(pts, N, B, on_dev, layers, nl)`` with the widths as the C array the library takes."""
        F, K = self.layers[0], self.K
        if isinstance(X, PointCloud) and F != 3:
            raise ValueError(f"a PointCloud has 3 channels per point, EdgeConv({self.layers}, {K}) takes {F}")
        pts, N, B, on_dev = self._clouds(X, f"EdgeConv({self.layers}, {K})", F)
        if K + 1 > N:
            raise ValueError(f"EdgeConv needs 1 <= K <= N - 1 (K neighbours besides the point itself), got K={K}, N={N}")
        return (pts, N, B, on_dev) + self._layers_c()

    def forward(self, X, idx=None, return_idx=False):
        """``(cL, N, B)`` for the clouds ``X``: a device array or a numpy array, ``(F, N, B)`` or ``(F, N)`` (one cloud); a
        PointCloud when F = 3.  The result lives where the input lives.  ``idx``: neighbour lists ``(K, N, B)``, 0-based,
        to use instead of the search (numpy integers, checked against [0, N) here, or an int32 device array).
        ``return_idx=True``: ``(out, idx)`` with the lists that were used, int32."""
        F, K = self.layers[0], self.K
        pts, N, B, on_dev, layers, nl = self._head(X)
        nb = _lib.query_bytes("fx3d_edgeconv_workspace_bytes", layers, nl, K, N, B)  # (the library's own size limits)
        given = None if idx is None else self._neighbours(idx, N, B)
        x = self._on_device(pts, N, B, on_dev, F)
        out = DeviceArray.empty((self.layers[-1], N, B), np.float32)
        found = DeviceArray.empty((K, N, B), np.int32) if return_idx and given is None else None
        ws = workspace(nb, tag="edgeconv")
        _lib.call("fx3d_edgeconv_forward", self._params_dev().ptr, layers, nl, K, x.ptr, N, B, given.ptr if given else None,
                  out.ptr, found.ptr if found else None, ws.ptr, ws.nbytes, current_stream().handle)
        used = given if given is not None else found
        if not on_dev:
            out, used = out.to_host(), (used.to_host() if used is not None else None)
        return (out, used) if return_idx else out

    __call__ = forward

    def forward_train(self, X, idx=None, momentum=0.1, update=False, return_idx=False, intermediates=False):
        """:meth:`forward` with the layer in TRAINING mode: include/flux3d_hip.h "DGCNN / EdgeConv training-mode forward".  Every
        BatchNorm normalises by the mean and uncorrected variance of what it is given over the K N B edge rows of the batch (one
        cloud is enough).  ``X``, ``idx``, ``return_idx`` and the placement of the results as in :meth:`forward`.
        ``intermediates=True``: a dict with ``out``, ``idx`` (the lists that were used), ``batch_stats`` and ``running``: dicts
        name -> array with the ``bnK.mu`` / ``.sigma2`` names of :func:`edgeconv_param_shapes`, the batch statistics and the
        running statistics Flux's BatchNorm would hold after this step (``momentum``; computed from the layer's ``mu`` /
        ``sigma2``).  ``update=True`` writes ``running`` into the layer's parameters, on the host (which reads them back: not
        inside a graph capture) and in the kept device copy."""
        F, K, f32 = self.layers[0], self.K, np.float32
        pts, N, B, on_dev, layers, nl = self._head(X)
        momentum = self._momentum(momentum)
        nb = _lib.query_bytes("fx3d_edgeconv_train_workspace_bytes", layers, nl, K, N, B)  # (the library's own size limits)
        given = None if idx is None else self._neighbours(idx, N, B)
        x = self._on_device(pts, N, B, on_dev, F)
        slots = self._stat_slots()
        nstat = slots[-1][2] + 2 * slots[-1][1]
        out = DeviceArray.empty((self.layers[-1], N, B), f32)
        found = DeviceArray.empty((K, N, B), np.int32) if (return_idx or intermediates) and given is None else None
        stats = {"batch_stats": DeviceArray.empty((nstat,), f32)}
        if intermediates or update:
            stats["running"] = DeviceArray.empty((nstat,), f32)
        ws = workspace(nb, tag="edgeconv_train")
        stream = current_stream().handle
        _lib.call("fx3d_edgeconv_forward_train", self._params_dev().ptr, layers, nl, K, x.ptr, N, B, given.ptr if given else None,
                  momentum, out.ptr, found.ptr if found else None, stats["batch_stats"].ptr,
                  stats["running"].ptr if "running" in stats else None, ws.ptr, ws.nbytes, stream)
        if update:
            self._adopt_running(stats["running"], slots, stream)
        used = given if given is not None else found
        if not on_dev:
            out, used = out.to_host(), (used.to_host() if used is not None else None)
        if intermediates:
            res = {"out": out, "idx": used}
            res.update({key: self._named_stats(buf, slots, on_dev) for key, buf in stats.items()})
            return res
        return (out, used) if return_idx else out

    def _like_out(self, a, name, N, B, on_dev):
        """``gout`` / ``out`` after its checks (:meth:`_like`), as (cL, N, B)."""
        return self._like(a, name, (self.layers[-1], N, B), np.float32, on_dev)

    def _adjoint_call(self, entry, X, gout, idx, out, results):
        """``fx3d_{entry}`` on the checked ``(X, gout, idx, out)`` of :meth:`input_grad`, everything on the device, with the
        workspace of ``fx3d_{entry}_workspace_bytes``.  ``results(N, B)``: the entry's result arrays in its argument order (one
        may be None).  They come back on the device, with whether ``X`` lives there."""
        F, K = self.layers[0], self.K
        pts, N, B, on_dev, layers, nl = self._head(X)
        nb = _lib.query_bytes(f"fx3d_{entry}_workspace_bytes", layers, nl, K, N, B)
        g = self._like_out(gout, "gout", N, B, on_dev)
        o = None if out is None else self._like_out(out, "out", N, B, on_dev)
        given = None if idx is None else self._neighbours(idx, N, B)
        if not on_dev:
            g, o = DeviceArray.from_host(g), (None if o is None else DeviceArray.from_host(o))
        x = self._on_device(pts, N, B, on_dev, F)
        res = results(N, B)
        ws = workspace(nb, tag=entry)
        _lib.call(f"fx3d_{entry}", self._params_dev().ptr, layers, nl, K, x.ptr, N, B, given.ptr if given else None,
                  o.ptr if o is not None else None, g.ptr, *(r.ptr if r is not None else None for r in res), ws.ptr, ws.nbytes,
                  current_stream().handle)
        return res, on_dev

    def input_grad(self, X, gout, idx=None, out=None):
        """The gradient ``(F, N, B)`` of ``sum(gout * forward(X))`` with respect to ``X``, with the neighbours held constant
        as the reference holds them (CreateSingleKNNGraph is @nograd) and BatchNorm in test mode: include/flux3d_hip.h
        "EdgeConv input adjoint".  ``X`` as in :meth:`forward`; ``gout`` ``(cL, N, B)`` lives where ``X`` lives, and so does
        the result.  ``idx``: the forward's neighbour lists (``return_idx=True``), ``out``: the forward's result; either may
        be left out, and is then computed again (the search is deterministic).  An ``out`` that is not this forward's passes
        gradient only where some k reproduces it.  The weights are constants here; :meth:`grad` gives their gradients too."""
        (gx,), on_dev = self._adjoint_call("edgeconv_bwd", X, gout, idx, out,
                                           lambda N, B: (DeviceArray.empty((self.layers[0], N, B), np.float32),))
        return gx if on_dev else gx.to_host()

    def _grad_call(self, X, gout, idx, out, input_grad):
        """fx3d_edgeconv_grad after :meth:`input_grad`'s checks: (the flat gradient, gx or None) on the device, and whether
        ``X`` lives there."""
        (gp, gx), on_dev = self._adjoint_call(
            "edgeconv_grad", X, gout, idx, out,
            lambda N, B: (DeviceArray.empty((self.param_count,), np.float32),
                          DeviceArray.empty((self.layers[0], N, B), np.float32) if input_grad else None))
        return gp, gx, on_dev

    def flat_grad(self, X, gout, idx=None, out=None, input_grad=True):
        """``(gflat, gx)``: the gradient of ``sum(gout * forward(X))`` with respect to the parameters as ONE flat Float32
        buffer with the layout of :meth:`flat_params` (the ``mu`` / ``sigma2`` slots are zero), for callers that step the
        flat parameter buffer, and the gradient with respect to ``X`` (``None`` with ``input_grad=False``).  Arguments and
        placement as :meth:`grad`."""
        gp, gx, on_dev = self._grad_call(X, gout, idx, out, input_grad)
        if not on_dev:
            gp, gx = gp.to_host(), (None if gx is None else gx.to_host())
        return gp, gx

    def grad(self, X, gout, idx=None, out=None, input_grad=True):
        """``(grads, gx)``: the gradients of ``sum(gout * forward(X))`` with respect to the parameters and to ``X``, from one
        fused kernel: include/flux3d_hip.h "EdgeConv parameter adjoint".  BatchNorm in test mode: ``gamma`` and ``beta``
        are parameters, the running statistics constants.  ``grads`` has the names and Flux shapes of
        :func:`edgeconv_param_shapes`; its ``mu`` / ``sigma2`` entries are zero.  ``gx`` is :meth:`input_grad`'s result,
        bit for bit, or ``None`` with ``input_grad=False``.  ``X``, ``gout``, ``idx`` and ``out`` as in :meth:`input_grad`;
        everything lives where ``X`` lives."""
        gp, gx, on_dev = self._grad_call(X, gout, idx, out, input_grad)
        return self._grad_views(gp, on_dev), (gx if on_dev or gx is None else gx.to_host())

    def _train_grad_call(self, X, gout, idx, fwd, input_grad):
        """fx3d_edgeconv_grad_train after the checks of :meth:`input_grad` and of ``fwd``: (the flat gradient, gx or None) on the
        device, and whether ``X`` lives there.  Every refusal comes before any device work."""
        F, K, f32 = self.layers[0], self.K, np.float32
        pts, N, B, on_dev, layers, nl = self._head(X)
        nb = _lib.query_bytes("fx3d_edgeconv_grad_train_workspace_bytes", layers, nl, K, N, B)
        g = self._like_out(gout, "gout", N, B, on_dev)
        slots = self._stat_slots()
        nstat = slots[-1][2] + 2 * slots[-1][1]
        names = [bn + f for bn, *_ in slots for f in (".mu", ".sigma2")]
        if fwd is not None:
            if not isinstance(fwd, dict) or any(k not in fwd for k in ("out", "idx", "batch_stats")):
                raise TypeError("fwd must be the dict of forward_train(..., intermediates=True)")
            named = fwd["batch_stats"]
            if [k for k in named] != names:
                raise ValueError(f"fwd['batch_stats'] must hold mu and sigma2 of the {len(slots)} BatchNorms in forward order")
            for (bn, C, _, _) in slots:
                for f in (".mu", ".sigma2"):
                    v = named[bn + f]
                    if is_device(v) != on_dev:
                        raise TypeError("fwd must live where X lives")
                    if tuple(v.shape) != (C,) or v.dtype != f32:
                        raise ValueError(f"fwd['batch_stats'][{bn + f!r}] must be Float32 ({C},), got {v.dtype} {tuple(v.shape)}")
            o = self._like_out(fwd["out"], "fwd['out']", N, B, on_dev)
            given = self._neighbours(fwd["idx"] if idx is None else idx, N, B)
        else:
            given = None if idx is None else self._neighbours(idx, N, B)
        x = self._on_device(pts, N, B, on_dev, F)
        stream = current_stream().handle
        if fwd is None:
            made = self.forward_train(x, idx=given, intermediates=True)
            o, given, named = made["out"], made["idx"], made["batch_stats"]
        if not on_dev:
            g = DeviceArray.from_host(g)
            if fwd is not None:
                o = DeviceArray.from_host(o)
        # the BatchNorms' statistics (views of forward_train's buffer, or the caller's arrays) as one buffer in the layout's order
        if on_dev or fwd is None:
            stats = DeviceArray.empty((nstat,), f32)
            for bn, C, at, _ in slots:
                for fld, off in ((".mu", at), (".sigma2", at + C)):
                    _lib.call("fx3d_memcpy_d2d", stats.ptr + 4 * off, named[bn + fld].ptr, 4 * C, stream)
        else:
            stats = DeviceArray.from_host(np.concatenate([np.asarray(named[k], f32) for k in names]))
        gp = DeviceArray.empty((self.param_count,), f32)
        gx = DeviceArray.empty((F, N, B), f32) if input_grad else None
        ws = workspace(nb, tag="edgeconv_grad_train")
        _lib.call("fx3d_edgeconv_grad_train", self._params_dev().ptr, layers, nl, K, x.ptr, N, B, given.ptr, o.ptr, stats.ptr, g.ptr,
                  gp.ptr, gx.ptr if gx is not None else None, ws.ptr, ws.nbytes, stream)
        return gp, gx, on_dev

    def flat_grad_train(self, X, gout, idx=None, fwd=None, input_grad=True):
        """:meth:`grad_train` with the parameter gradients as one flat buffer, as :meth:`flat_grad`."""
        gp, gx, on_dev = self._train_grad_call(X, gout, idx, fwd, input_grad)
        if not on_dev:
            gp, gx = gp.to_host(), (None if gx is None else gx.to_host())
        return gp, gx

    def grad_train(self, X, gout, idx=None, fwd=None, input_grad=True):
        """:meth:`grad` for the layer in TRAINING mode: ``(grads, gx)``, the gradients of ``sum(gout * forward_train(X))`` with
        every BatchNorm's mean and variance functions of the batch: include/flux3d_hip.h "EdgeConv training-mode adjoint".  The
        neighbours are constants.  ``fwd``: the dict of ``forward_train(X, idx, intermediates=True)`` for the same ``X`` -- its
        ``out``, ``idx`` (unless ``idx`` is given here) and ``batch_stats`` are used; without it :meth:`forward_train` runs first,
        on ``idx`` if given.  ``grads`` and ``gx`` as :meth:`grad` returns them (the ``mu`` / ``sigma2`` entries are zero: the
        running statistics do not enter this forward); ``gx`` is ``None`` with ``input_grad=False``.  Everything lives where
        ``X`` lives."""
        gp, gx, on_dev = self._train_grad_call(X, gout, idx, fwd, input_grad)
        return self._grad_views(gp, on_dev), (gx if on_dev or gx is None else gx.to_host())


def stnkd_layer_spec(K):
    """stnKD(K)'s layers that carry parameters, in forward order: :func:`_stn_spec` without a prefix (``conv1`` ... ``dense3``)."""
    return [(name[1:], kind, ch) for name, kind, ch in _stn_spec("", int(K))]


def stnkd_param_shapes(K):
    """stnKD(K): name -> shape of every parameter array, in the order of the flat buffer (Flux's shapes, :func:`_shapes`)."""
    return _shapes(stnkd_layer_spec(K))


class stnKD(_Model):
    """``stnKD(K)`` (src/models/pointnet.jl:3-20), the spatial-transformer block as a layer in its own right, in test mode and in
    training mode: include/flux3d_hip_layers.h "stnKD(K)" states the layer, its arithmetic and the envelope.  Three 1x1
    convolutions K => 64 => 128 => 1024 (relu, BatchNorm), the maximum over the points, Dense 1024 => 512 => 256 (relu), BatchNorm,
    Dense 256 => K K, returned as the (K, K) matrix per cloud in the orientation of PointNet's ``stn`` / ``fstn``.  1 <= K <= 128.

    The input is ``(K, N, B)``, channels first like every model here; the reference's Chain takes the permuted ``(N, K, B)``.
    ``params`` (:func:`stnkd_param_shapes`: ``conv1.weight`` ... ``dense3.bias``), ``load``, ``flat_params`` and the seeded
    initialisation are the classifiers'.  The ``stn.`` / ``fstn.`` arrays of a PointNet, with that prefix dropped, are the
    parameters of ``stnKD(3)`` / ``stnKD(64)``: :meth:`from_pointnet`.  Gradients are not there yet."""

    _NAME, _COUNT_FN = "stnKD", "fx3d_stnkd_param_count"
    MAX_K = 128

    def __init__(self, K, seed=0):
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)):
            raise TypeError(f"K must be an integer, got {K!r}")
        if not 1 <= int(K) <= self.MAX_K:
            raise ValueError(f"stnKD(K) needs K in [1, {self.MAX_K}], got {K}")
        self.K = int(K)
        self._init_params(seed)

    @classmethod
    def from_pointnet(cls, model, which):
        """The ``stn`` (K = 3) or ``fstn`` (K = 64) block of the PointNet ``model`` as a layer of its own, its parameters copied."""
        if not isinstance(model, PointNet):
            raise TypeError(f"model must be a PointNet, got {type(model).__name__}")
        if which not in ("stn", "fstn"):
            raise ValueError(f"which must be 'stn' or 'fstn', got {which!r}")
        if model._stale:
            model.pull_params()
        layer = cls(3 if which == "stn" else 64)
        return layer.load({name: model.params[f"{which}.{name}"] for name in layer._shapes()})

    def _count_args(self):
        return (self.K,)

    def _shapes(self):
        return stnkd_param_shapes(self.K)

    def _head(self, X):
        """The checks every call begins with: a PointCloud only for K = 3, then the clouds (:meth:`_clouds`)."""
        if isinstance(X, PointCloud) and self.K != 3:
            raise ValueError(f"a PointCloud has 3 channels per point, stnKD({self.K}) takes {self.K}")
        return self._clouds(X, f"stnKD({self.K})", self.K)

    def forward(self, X, intermediates=False):
        """The transforms ``(K, K, B)`` of the clouds ``X``: a device array or a numpy array, ``(K, N, B)`` or ``(K, N)`` (one
        cloud); a PointCloud when K = 3.  The result lives where the input lives.  ``intermediates=True``: a dict with ``out``
        and ``pooled`` (1024, B), the maximum over the points."""
        K = self.K
        pts, N, B, on_dev = self._head(X)
        nb = _lib.query_bytes("fx3d_stnkd_workspace_bytes", N, B, K)  # (the library's own size limits)
        x = self._on_device(pts, N, B, on_dev, K)
        out = {"out": DeviceArray.empty((K, K, B), np.float32)}
        if intermediates:
            out["pooled"] = DeviceArray.empty((1024, B), np.float32)
        ws = workspace(nb, tag="stnkd")
        _lib.call("fx3d_stnkd_forward", self._params_dev().ptr, K, x.ptr, N, B, out["out"].ptr,
                  out["pooled"].ptr if intermediates else None, ws.ptr, ws.nbytes, current_stream().handle)
        if not on_dev:
            out = {k: v.to_host() for k, v in out.items()}
        return out if intermediates else out["out"]

    __call__ = forward

    def forward_train(self, X, momentum=0.1, update=False, intermediates=False):
        """:meth:`forward` with the layer in TRAINING mode (at least two clouds): include/flux3d_hip_layers.h "stnKD(K),
        training-mode forward".  Each of the four BatchNorms normalises by the mean and uncorrected variance of the current batch.
        ``intermediates=True``: a dict with ``out``, ``pooled``, ``batch_stats`` and ``running``: dicts name -> array with the
        ``bnK.mu`` / ``.sigma2`` names of :func:`stnkd_param_shapes`, the batch statistics and the running statistics Flux's
        BatchNorm would hold after this step (``momentum``; computed from the layer's ``mu`` / ``sigma2``).  Everything lives
        where ``X`` lives.  ``update=True`` writes ``running`` into the layer's parameters, on the host (which reads them back: not
        inside a graph capture) and in the kept device copy."""
        K, f32 = self.K, np.float32
        pts, N, B, on_dev = self._head(X)
        if B < 2:
            raise ValueError(f"training-mode BatchNorm needs at least two clouds (the dense BatchNorm's running variance divides by "
                             f"B - 1), got B={B}")
        momentum = self._momentum(momentum)
        nb = _lib.query_bytes("fx3d_stnkd_train_workspace_bytes", N, B, K)  # (the library's own size limits)
        x = self._on_device(pts, N, B, on_dev, K)
        slots = self._stat_slots()
        nstat = slots[-1][2] + 2 * slots[-1][1]
        out = {"out": DeviceArray.empty((K, K, B), f32)}
        if intermediates:
            out["pooled"] = DeviceArray.empty((1024, B), f32)
        stats = {"batch_stats": DeviceArray.empty((nstat,), f32)}
        if intermediates or update:
            stats["running"] = DeviceArray.empty((nstat,), f32)
        ws = workspace(nb, tag="stnkd_train")
        stream = current_stream().handle
        _lib.call("fx3d_stnkd_forward_train", self._params_dev().ptr, K, x.ptr, N, B, momentum, out["out"].ptr,
                  out["pooled"].ptr if intermediates else None, stats["batch_stats"].ptr,
                  stats["running"].ptr if "running" in stats else None, ws.ptr, ws.nbytes, stream)
        if update:
            self._adopt_running(stats["running"], slots, stream)
        if not on_dev:
            out = {k: v.to_host() for k, v in out.items()}
        if not intermediates:
            return out["out"]
        out.update({key: self._named_stats(buf, slots, on_dev) for key, buf in stats.items()})
        return out
