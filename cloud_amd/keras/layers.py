"""Keras layers (``tf.keras.layers`` names/arguments) on cloud_amd NHWC ops.

Used by the reference workloads: Dense, Conv2D, MaxPooling2D, GlobalMax/Avg
pooling, Flatten, Dropout, BatchNormalization, Activation, Rescaling and the
CIFAR augmentation layers (``keras_tuner_cifar_example.py:24-77``,
``mnist_example_using_fit.py:54-63``, README MLP).  Weight layouts are the
MI355X kernel layouts: Dense ``[units, in]``, Conv2D ``[filters, kh, kw, in]``.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .. import ops
from ..ops.dense import conv2d as conv_act_op
from ..ops.dense import dense as dense_op
from ..ops.dropout import dropout as dropout_op
from . import activations, initializers, regularizers
from .engine import Input, InputLayer, KerasTensor, Layer, global_policy  # noqa: F401


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


_ACT_NAMES = {activations.linear: None, activations.relu: "relu", activations.elu: "elu",
              activations.tanh: "tanh", activations.gelu: "gelu"}


def _fused_act(fn):
    """(epilogue activation name, remaining activation fn) for a Keras activation."""
    if fn in _ACT_NAMES:
        return _ACT_NAMES[fn], None
    return None, fn


def _bias_dtype(layer):
    """Biases are variables: fp32 under the mixed policy (the epilogue adds them in fp32)."""
    return layer._dtype_policy.variable_dtype if layer.compute_dtype == torch.bfloat16 else layer.compute_dtype


class _Regularized:
    """kernel/bias regularizers -> ``regularization_loss()`` (summed into the loss by Model)."""

    def _set_regularizers(self, kernel_regularizer, bias_regularizer):
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.bias_regularizer = regularizers.get(bias_regularizer)

    def regularization_loss(self):
        out = None
        for reg, w in ((self.kernel_regularizer, getattr(self, "kernel", None)),
                       (self.bias_regularizer, getattr(self, "bias", None))):
            if reg is not None and w is not None and self.trainable:
                p = reg(w)
                out = p if out is None else out + p
        return out if out is not None else 0.0


class Dense(_Regularized, Layer):
    def __init__(self, units, activation=None, use_bias=True, kernel_initializer="glorot_uniform",
                 bias_initializer="zeros", kernel_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(**kw)
        self.units = int(units)
        self.activation = activations.get(activation)
        self.use_bias = use_bias
        self.kernel_initializer, self.bias_initializer = kernel_initializer, bias_initializer
        self._set_regularizers(kernel_regularizer, bias_regularizer)

    def build(self, input_shape):
        fin = int(input_shape[-1])
        w = torch.empty(self.units, fin)
        initializers.get(self.kernel_initializer)(w)
        self.kernel = torch.nn.Parameter(w.to(self.compute_dtype))
        if self.use_bias:
            b = torch.empty(self.units)
            initializers.get(self.bias_initializer)(b)
            self.bias = torch.nn.Parameter(b.to(_bias_dtype(self)))
        else:
            self.bias = None

    def call(self, x, training=None):
        x = x.to(self.kernel.dtype)
        if getattr(self, "_emit_logits", False):  # fused softmax-xent training path (Model.fit)
            return dense_op(x, self.kernel, self.bias, None)
        act, rest = _fused_act(self.activation)
        y = dense_op(x, self.kernel, self.bias, act)
        return rest(y) if rest is not None else y

    def get_config(self):
        c = super().get_config()
        c.update(units=self.units, activation=activations.serialize(self.activation), use_bias=self.use_bias,
                 kernel_initializer=self.kernel_initializer if isinstance(self.kernel_initializer, str)
                 else "glorot_uniform")
        return c


class Conv2D(_Regularized, Layer):
    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", activation=None, use_bias=True,
                 kernel_initializer="glorot_uniform", data_format=None, kernel_regularizer=None,
                 bias_regularizer=None, **kw):
        super().__init__(**kw)
        self._set_regularizers(kernel_regularizer, bias_regularizer)
        if data_format not in (None, "channels_last"):
            raise ValueError("cloud_amd layers are channels_last (NHWC) only")
        self.filters = int(filters)
        self.kernel_size = _pair(kernel_size)
        self.strides = _pair(strides)
        self.padding = padding.lower()
        self.activation = activations.get(activation)
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer

    def build(self, input_shape):
        cin = int(input_shape[-1])
        kh, kw = self.kernel_size
        w = torch.empty(self.filters, kh, kw, cin)
        initializers.get(self.kernel_initializer)(w)
        self.kernel = torch.nn.Parameter(w.to(self.compute_dtype))
        self.bias = torch.nn.Parameter(torch.zeros(self.filters, dtype=_bias_dtype(self))) if self.use_bias else None

    def _same_pads(self, H, W):
        out = []
        for n, k, s in ((H, self.kernel_size[0], self.strides[0]), (W, self.kernel_size[1], self.strides[1])):
            o = math.ceil(n / s)
            tot = max((o - 1) * s + k - n, 0)
            out.append((tot // 2, tot - tot // 2))
        return out

    def call(self, x, training=None):
        x = x.to(self.kernel.dtype)
        pad = (0, 0)
        if self.padding == "same":
            (pt, pb), (pl, pr) = self._same_pads(x.shape[1], x.shape[2])
            if pt == pb and pl == pr:
                pad = (pt, pl)
            else:  # TF's asymmetric SAME split (extra row/column at the bottom/right)
                x = F.pad(x, (0, 0, pl, pr, pt, pb))
        act, rest = _fused_act(self.activation)
        y = conv_act_op(x.contiguous(), self.kernel, self.bias, tuple(self.strides), pad, act)
        return rest(y) if rest is not None else y

    def get_config(self):
        c = super().get_config()
        c.update(filters=self.filters, kernel_size=list(self.kernel_size), strides=list(self.strides),
                 padding=self.padding, activation=activations.serialize(self.activation), use_bias=self.use_bias)
        return c


def _same_pads(size, kernel, strides, dilation=(1, 1)):
    """TF's SAME split per axis ((top, bottom), (left, right)): ``Conv2D._same_pads``' formula on
    the dilated kernel extent; the odd row / column goes to the bottom / right."""
    out = []
    for n, k, s, d in zip(size, kernel, strides, dilation):
        k = (k - 1) * d + 1
        tot = max((math.ceil(n / s) - 1) * s + k - n, 0)
        out.append((tot // 2, tot - tot // 2))
    return out


def _init_name(init):
    return init if isinstance(init, str) else "glorot_uniform"


class DepthwiseConv2D(Layer):
    """``tf.keras.layers.DepthwiseConv2D``: ``depthwise_kernel [kh, kw, cin, dm]`` (the Keras
    layout; output channel ``c * dm + m`` reads input channel ``c``) and ``bias [cin * dm]``.
    Under the mixed policy it runs ``ops.depthwise_conv2d`` natively, with bias and a fusable
    activation in the kernel's epilogue and SAME padding passed as pads (no padded copy);
    ``dilation_rate != 1`` is the same expression in PyTorch."""

    def __init__(self, kernel_size, strides=(1, 1), padding="valid", depth_multiplier=1, data_format=None,
                 dilation_rate=(1, 1), activation=None, use_bias=True, depthwise_initializer="glorot_uniform",
                 bias_initializer="zeros", depthwise_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(**kw)
        if data_format not in (None, "channels_last"):
            raise ValueError("cloud_amd layers are channels_last (NHWC) only")
        self.kernel_size = _pair(kernel_size)
        self.strides = _pair(strides)
        self.padding = padding.lower()
        if self.padding not in ("valid", "same"):
            raise ValueError(f"padding must be 'valid' or 'same', got {padding!r}")
        self.depth_multiplier = int(depth_multiplier)
        self.dilation_rate = _pair(dilation_rate)
        self.activation = activations.get(activation)
        self.use_bias = use_bias
        self.depthwise_initializer, self.bias_initializer = depthwise_initializer, bias_initializer
        self.depthwise_regularizer = regularizers.get(depthwise_regularizer)
        self.bias_regularizer = regularizers.get(bias_regularizer)

    def _new_depthwise_kernel(self, cin):
        # drawn as [dm, kh, kw, cin], whose fans are Keras's for [kh, kw, cin, dm]:
        # fan_in = kh*kw*cin, fan_out = kh*kw*dm
        kh, kw = self.kernel_size
        w = torch.empty(self.depth_multiplier, kh, kw, cin)
        initializers.get(self.depthwise_initializer)(w)
        return torch.nn.Parameter(w.permute(1, 2, 3, 0).contiguous().to(self.compute_dtype))

    def build(self, input_shape):
        cin = int(input_shape[-1])
        self.depthwise_kernel = self._new_depthwise_kernel(cin)
        if self.use_bias:
            b = torch.empty(cin * self.depth_multiplier)
            initializers.get(self.bias_initializer)(b)
            self.bias = torch.nn.Parameter(b.to(_bias_dtype(self)))
        else:
            self.bias = None

    def _depthwise(self, x, bias, act):
        x = x.to(self.depthwise_kernel.dtype)
        pads = ((0, 0), (0, 0))
        if self.padding == "same":
            pads = _same_pads(x.shape[1:3], self.kernel_size, self.strides, self.dilation_rate)
        return ops.depthwise_conv2d(x.contiguous(), self.depthwise_kernel, bias, self.strides, pads, act,
                                    dilation=self.dilation_rate)

    def call(self, x, training=None):
        act, rest = _fused_act(self.activation)
        y = self._depthwise(x, self.bias, act)
        return rest(y) if rest is not None else y

    def _penalties(self):
        return ((self.depthwise_regularizer, self.depthwise_kernel), (self.bias_regularizer, self.bias))

    def regularization_loss(self):
        out = None
        for reg, w in self._penalties():
            if reg is not None and w is not None and self.trainable:
                p = reg(w)
                out = p if out is None else out + p
        return out if out is not None else 0.0

    def get_config(self):
        c = super().get_config()
        c.update(kernel_size=list(self.kernel_size), strides=list(self.strides), padding=self.padding,
                 depth_multiplier=self.depth_multiplier, dilation_rate=list(self.dilation_rate),
                 activation=activations.serialize(self.activation), use_bias=self.use_bias,
                 depthwise_initializer=_init_name(self.depthwise_initializer),
                 bias_initializer=_init_name(self.bias_initializer),
                 depthwise_regularizer=regularizers.serialize(self.depthwise_regularizer),
                 bias_regularizer=regularizers.serialize(self.bias_regularizer))
        return c


class SeparableConv2D(DepthwiseConv2D):
    """``tf.keras.layers.SeparableConv2D``: the depthwise convolution (no bias, no activation)
    followed by the 1x1 pointwise convolution ``pointwise_kernel [filters, 1, 1, cin * dm]`` on
    the in-tree GEMM, bias and activation in its epilogue.  Weight order: ``depthwise_kernel,
    pointwise_kernel, bias``."""

    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", data_format=None,
                 dilation_rate=(1, 1), depth_multiplier=1, activation=None, use_bias=True,
                 depthwise_initializer="glorot_uniform", pointwise_initializer="glorot_uniform",
                 bias_initializer="zeros", depthwise_regularizer=None, pointwise_regularizer=None,
                 bias_regularizer=None, **kw):
        super().__init__(kernel_size, strides=strides, padding=padding, depth_multiplier=depth_multiplier,
                         data_format=data_format, dilation_rate=dilation_rate, activation=activation,
                         use_bias=use_bias, depthwise_initializer=depthwise_initializer,
                         bias_initializer=bias_initializer, depthwise_regularizer=depthwise_regularizer,
                         bias_regularizer=bias_regularizer, **kw)
        self.filters = int(filters)
        self.pointwise_initializer = pointwise_initializer
        self.pointwise_regularizer = regularizers.get(pointwise_regularizer)

    def build(self, input_shape):
        cin = int(input_shape[-1])
        self.depthwise_kernel = self._new_depthwise_kernel(cin)
        w = torch.empty(self.filters, 1, 1, cin * self.depth_multiplier)
        initializers.get(self.pointwise_initializer)(w)
        self.pointwise_kernel = torch.nn.Parameter(w.to(self.compute_dtype))
        if self.use_bias:
            b = torch.empty(self.filters)
            initializers.get(self.bias_initializer)(b)
            self.bias = torch.nn.Parameter(b.to(_bias_dtype(self)))
        else:
            self.bias = None

    def call(self, x, training=None):
        act, rest = _fused_act(self.activation)
        y = conv_act_op(self._depthwise(x, None, None), self.pointwise_kernel, self.bias, 1, 0, act)
        return rest(y) if rest is not None else y

    def _penalties(self):
        return super()._penalties() + ((self.pointwise_regularizer, self.pointwise_kernel),)

    def get_config(self):
        c = super().get_config()
        c.update(filters=self.filters, pointwise_initializer=_init_name(self.pointwise_initializer),
                 pointwise_regularizer=regularizers.serialize(self.pointwise_regularizer))
        return c


def _pool_nhwc(op, x, pool_size, strides, padding):
    """``op`` (an ``ops.*_pool2d_nhwc``) under TF's "valid" / "same" geometry.  "same" goes to the op
    as its pad split plus the output size, so no padded copy is made; where it pads nothing it is
    "valid"."""
    x = x.contiguous()
    if padding == "same":
        pads = _same_pads(x.shape[1:3], pool_size, strides)
        if any(p for ax in pads for p in ax):
            out_hw = (math.ceil(x.shape[1] / strides[0]), math.ceil(x.shape[2] / strides[1]))
            return op(x, pool_size, strides, pads, out_hw)
    return op(x, pool_size, strides, 0)


def _check_padding(padding):
    padding = padding.lower()
    if padding not in ("valid", "same"):
        raise ValueError(f"padding must be 'valid' or 'same', got {padding!r}")
    return padding


class _Pool2D(Layer):
    """``pool_size`` and ``strides`` are ints or (h, w) pairs, ``padding`` "valid" or "same" (TF's
    split: the odd row / column goes to the bottom / right).  [N, H, W, C] -> [N, OH, OW, C]."""

    _op = None

    def __init__(self, pool_size=(2, 2), strides=None, padding="valid", **kw):
        super().__init__(**kw)
        self.pool_size = _pair(pool_size)
        self.strides = _pair(strides) if strides is not None else self.pool_size
        self.padding = _check_padding(padding)

    def call(self, x, training=None):
        return _pool_nhwc(type(self)._op, x, self.pool_size, self.strides, self.padding)

    def get_config(self):
        c = super().get_config()
        c.update(pool_size=list(self.pool_size), strides=list(self.strides), padding=self.padding)
        return c


class MaxPooling2D(_Pool2D):
    _op = staticmethod(ops.max_pool2d_nhwc)


class AveragePooling2D(_Pool2D):
    """The divisor is the number of in-image taps: "same" padding is not averaged in (TF)."""

    _op = staticmethod(ops.avg_pool2d_nhwc)


def _one(v):
    return int(v) if isinstance(v, int) else int(tuple(v)[0])


class _Pool1D(Layer):
    """``tf.keras.layers.{Max,Average}Pooling1D``: [B, T, C] -> [B, OT, C] over the steps, through
    the 2D ops on the [B, 1, T, C] view (no copy)."""

    _op = None

    def __init__(self, pool_size=2, strides=None, padding="valid", **kw):
        super().__init__(**kw)
        self.pool_size = _one(pool_size)
        self.strides = _one(strides) if strides is not None else self.pool_size
        self.padding = _check_padding(padding)

    def call(self, x, training=None):
        y = _pool_nhwc(type(self)._op, x.contiguous().unsqueeze(1), (1, self.pool_size), (1, self.strides),
                       self.padding)
        return y.squeeze(1)

    def get_config(self):
        c = super().get_config()
        c.update(pool_size=[self.pool_size], strides=[self.strides], padding=self.padding)
        return c


class MaxPooling1D(_Pool1D):
    _op = staticmethod(ops.max_pool2d_nhwc)


class AveragePooling1D(_Pool1D):
    _op = staticmethod(ops.avg_pool2d_nhwc)


class GlobalAveragePooling2D(Layer):
    def call(self, x, training=None):
        return ops.global_avg_pool_nhwc(x.contiguous())


class GlobalMaxPooling2D(Layer):
    def call(self, x, training=None):
        return ops.global_max_pool_nhwc(x.contiguous())


def _no_mask(layer, mask):
    if mask is not None:
        raise ValueError(f"{type(layer).__name__}: a mask is not supported")


class GlobalAveragePooling1D(Layer):
    """[B, T, C] -> [B, C], the mean over the steps (the [B, 1, T, C] view through the 2D op)."""

    def call(self, x, training=None, mask=None):
        _no_mask(self, mask)
        return ops.global_avg_pool_nhwc(x.contiguous().unsqueeze(1))


class GlobalMaxPooling1D(Layer):
    """[B, T, C] -> [B, C], the maximum over the steps."""

    def call(self, x, training=None, mask=None):
        _no_mask(self, mask)
        return ops.global_max_pool_nhwc(x.contiguous().unsqueeze(1))


class Flatten(Layer):
    def call(self, x, training=None):
        return x.reshape(x.shape[0], -1)


class Reshape(Layer):
    def __init__(self, target_shape, **kw):
        super().__init__(**kw)
        self.target_shape = tuple(target_shape)

    def call(self, x, training=None):
        return x.reshape((x.shape[0],) + self.target_shape)

    def get_config(self):
        c = super().get_config()
        c["target_shape"] = list(self.target_shape)
        return c


class Dropout(Layer):
    def __init__(self, rate, seed=None, **kw):
        super().__init__(**kw)
        self.rate = float(rate)

    def call(self, x, training=None):
        return dropout_op(x, self.rate, training=bool(training))

    def get_config(self):
        c = super().get_config()
        c["rate"] = self.rate
        return c


class Activation(Layer):
    def __init__(self, activation, **kw):
        super().__init__(**kw)
        self.activation = activations.get(activation)

    def call(self, x, training=None):
        if getattr(self, "_emit_logits", False):
            return x
        return self.activation(x)

    def get_config(self):
        c = super().get_config()
        c["activation"] = activations.serialize(self.activation)
        return c


class ReLU(Activation):
    def __init__(self, **kw):
        super().__init__("relu", **kw)

    def get_config(self):
        c = super().get_config()
        c.pop("activation")
        return c


class Softmax(Activation):
    def __init__(self, **kw):
        super().__init__("softmax", **kw)

    def get_config(self):
        c = super().get_config()
        c.pop("activation")
        return c


class BatchNormalization(Layer):
    """Keras semantics: moving = momentum * moving + (1 - momentum) * batch; epsilon 1e-3."""

    def __init__(self, axis=-1, momentum=0.99, epsilon=1e-3, center=True, scale=True, **kw):
        super().__init__(**kw)
        if axis not in (-1, 3):
            raise ValueError("BatchNormalization normalises the channel (last) axis in NHWC")
        self.momentum, self.epsilon, self.center, self.scale = float(momentum), float(epsilon), center, scale

    def build(self, input_shape):
        c = int(input_shape[-1])
        self.gamma = torch.nn.Parameter(torch.ones(c)) if self.scale else None
        self.beta = torch.nn.Parameter(torch.zeros(c)) if self.center else None
        self.register_buffer("moving_mean", torch.zeros(c))
        self.register_buffer("moving_variance", torch.ones(c))

    _frozen_runs_inference = True

    def call(self, x, training=None):
        # frozen (trainable = False) means inference mode, whatever `training` says
        return ops.bn_act(x.contiguous(), self.gamma, self.beta, self.moving_mean, self.moving_variance,
                          eps=self.epsilon, momentum=1.0 - self.momentum, relu=False,
                          training=bool(training) and self._trainable)

    def get_config(self):
        c = super().get_config()
        c.update(momentum=self.momentum, epsilon=self.epsilon, center=self.center, scale=self.scale)
        return c


class LayerNormalization(Layer):
    def __init__(self, axis=-1, epsilon=1e-3, center=True, scale=True, **kw):
        super().__init__(**kw)
        self.epsilon = float(epsilon)
        self.center, self.scale = bool(center), bool(scale)

    def build(self, input_shape):
        c = int(input_shape[-1])
        # a disabled scale / offset creates no parameter (ops.layer_norm takes None for it)
        self.gamma = torch.nn.Parameter(torch.ones(c)) if self.scale else None
        self.beta = torch.nn.Parameter(torch.zeros(c)) if self.center else None

    def call(self, x, training=None):
        return ops.layer_norm(x, self.gamma, self.beta, self.epsilon)

    def get_config(self):
        c = super().get_config()
        c.update(epsilon=self.epsilon, center=self.center, scale=self.scale)
        return c


class Embedding(Layer):
    def __init__(self, input_dim, output_dim, **kw):
        super().__init__(**kw)
        self.input_dim, self.output_dim = int(input_dim), int(output_dim)

    def build(self, input_shape):
        w = torch.empty(self.input_dim, self.output_dim)
        torch.nn.init.uniform_(w, -0.05, 0.05)
        self.embeddings = torch.nn.Parameter(w.to(self.compute_dtype))

    def call(self, x, training=None):
        return F.embedding(x.long(), self.embeddings)

    def get_config(self):
        c = super().get_config()
        c.update(input_dim=self.input_dim, output_dim=self.output_dim)
        return c


class Rescaling(Layer):
    def __init__(self, scale, offset=0.0, **kw):
        super().__init__(**kw)
        self.scale, self.offset = float(scale), float(offset)

    def call(self, x, training=None):
        return x.float() * self.scale + self.offset

    def get_config(self):
        c = super().get_config()
        c.update(scale=self.scale, offset=self.offset)
        return c


class Add(Layer):
    def call(self, xs, training=None):
        out = xs[0]
        for t in xs[1:]:
            out = out + t
        return out


class Concatenate(Layer):
    def __init__(self, axis=-1, **kw):
        super().__init__(**kw)
        self.axis = axis

    def call(self, xs, training=None):
        return torch.cat(list(xs), dim=self.axis)

    def get_config(self):
        c = super().get_config()
        c["axis"] = self.axis
        return c


class MultiHeadAttention(Layer):
    """``tf.keras.layers.MultiHeadAttention`` with ``value_dim == key_dim`` and the default
    output shape and attention axes.

    Weights are packed for the kernels, in the ``[units, fan_in]`` layout of ``Dense``:
    ``qkv_kernel [3*H*key_dim, dim]`` (Q | K | V, head ``h`` at rows ``h*key_dim`` of each third)
    with ``qkv_bias``, and ``out_kernel [dim, H*key_dim]`` with ``out_bias``.
    ``get_weights`` / ``set_weights`` present Keras's arrays in Keras's order and shapes (query,
    key, value kernels ``[dim, H, key_dim]`` with biases ``[H, key_dim]``, output kernel
    ``[H, key_dim, dim]`` with bias ``[dim]``), so weights copied from a Keras model give the
    same function.

    Self-attention (``query is value``, no ``key`` or the same tensor) without an
    ``attention_mask`` and without ``return_attention_scores`` is one packed projection,
    ``ops.attention`` and the output projection: under the mixed policy with ``key_dim`` in
    ``ops.raw.ATTN_HEAD_DIMS`` (32, 64 or 128) all three run on the in-tree kernels, forward and
    backward.  Cross-attention (``query`` is
    not ``value``) without a mask, returned scores or the causal flag is native under the same
    conditions: the Q projection from the first third of ``qkv_kernel``, the K | V projection
    from the other two as one GEMM (two and a concatenation when ``key`` is a tensor of its own),
    ``ops.cross_attention`` and the output projection.  An ``attention_mask`` (any shape Keras
    broadcasts to ``[B, T, S]``, or per head ``[B, H, T, S]``; torch or numpy; with or without the
    causal flag) and causal cross-attention (the top-left ``tril`` of ``[T, S]``) are native under
    the same conditions too, same projections, with the mask handed to ``ops.attention(mask=)`` /
    ``ops.cross_attention(mask=)``.  Everything else (float32 layers, CPU, another ``key_dim``,
    returned scores) is the same math in PyTorch.

    One difference between the two: a query row whose mask allows no key at all gets a zero
    context on the native route (the kernels define a softmax over nothing as zeros, and such a
    row sends no gradient), where the PyTorch branch, like Keras, fills with ``finfo.min`` and so
    returns the mean of the values.  Padded query rows are the usual case and are discarded
    downstream either way.

    Calls: Keras style ``layer(query, value, key=None, attention_mask=None,
    use_causal_mask=False, return_attention_scores=False, training=None)``, or the list form
    of ``Add`` / ``Concatenate``, ``layer([query, value])`` / ``layer([query, value, key])``.
    The functional graph replays ``layer(inputs, training=...)`` only, so causality also lives
    on the layer (``use_causal_mask`` constructor argument, kept by ``get_config``); a symbolic
    ``layer(x, x, use_causal_mask=True)`` records the flag on the layer.
    """

    def __init__(self, num_heads, key_dim, value_dim=None, dropout=0.0, use_bias=True, output_shape=None,
                 attention_axes=None, kernel_initializer="glorot_uniform", use_causal_mask=False, **kw):
        super().__init__(**kw)
        self.num_heads, self.key_dim = int(num_heads), int(key_dim)
        if value_dim is not None and int(value_dim) != self.key_dim:
            raise ValueError(f"MultiHeadAttention: value_dim must equal key_dim ({self.key_dim}), got {value_dim}")
        if output_shape is not None:
            raise ValueError("MultiHeadAttention: output_shape is not supported (the output has the query's width)")
        if attention_axes is not None:
            raise ValueError("MultiHeadAttention: attention_axes is not supported (attention runs over axis 1)")
        self.dropout = float(dropout)
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.use_causal_mask = bool(use_causal_mask)

    def build(self, input_shape):
        shapes = input_shape if isinstance(input_shape, list) else [input_shape]
        dim = int(shapes[0][-1])
        if any(int(s[-1]) != dim for s in shapes[1:]):
            raise ValueError("MultiHeadAttention: query, value and key must have the same width "
                             f"(the projections are packed), got {[tuple(s) for s in shapes]}")
        hd = self.num_heads * self.key_dim
        init = initializers.get(self.kernel_initializer)
        thirds = [torch.empty(hd, dim) for _ in range(3)]
        for t in thirds:
            init(t)
        self.qkv_kernel = torch.nn.Parameter(torch.cat(thirds, 0).to(self.compute_dtype))
        wo = torch.empty(dim, hd)
        init(wo)
        self.out_kernel = torch.nn.Parameter(wo.to(self.compute_dtype))
        if self.use_bias:
            self.qkv_bias = torch.nn.Parameter(torch.zeros(3 * hd, dtype=_bias_dtype(self)))
            self.out_bias = torch.nn.Parameter(torch.zeros(dim, dtype=_bias_dtype(self)))
        else:
            self.qkv_bias = self.out_bias = None

    def __call__(self, query, value=None, key=None, attention_mask=None, use_causal_mask=False,
                 return_attention_scores=False, training=None):
        if isinstance(query, (list, tuple)):
            if value is not None or key is not None:
                raise ValueError("MultiHeadAttention: pass either [query, value(, key)] or query, value(, key)")
            if len(query) not in (2, 3):
                raise ValueError("MultiHeadAttention: the list form is [query, value] or [query, value, key]")
            query, value, key = (*query, None)[:3]
        elif value is None:
            raise ValueError("MultiHeadAttention: value is required")
        ins, seen = [], {}
        for t in (query, value) + ((key,) if key is not None else ()):
            if id(t) not in seen:  # the same object stays the same object: that is what selects self-attention
                seen[id(t)] = self._convert_inputs(t)
            ins.append(seen[id(t)])
        if all(isinstance(t, KerasTensor) for t in ins):
            if attention_mask is not None or return_attention_scores:
                raise ValueError("MultiHeadAttention: attention_mask and return_attention_scores need an eager "
                                 "call (the functional graph replays layer(inputs, training=...) only)")
            if use_causal_mask:
                self.use_causal_mask = True
            return super().__call__(ins)
        return super().__call__(ins, attention_mask=attention_mask, use_causal_mask=use_causal_mask,
                                return_attention_scores=return_attention_scores, training=training)

    def call(self, inputs, training=None, attention_mask=None, use_causal_mask=False, return_attention_scores=False):
        query, value = inputs[0], inputs[1]
        key = inputs[2] if len(inputs) > 2 else value
        causal = self.use_causal_mask or bool(use_causal_mask)
        H, D = self.num_heads, self.key_dim
        hd = H * D
        p = self.dropout if training else 0.0
        dt = self.qkv_kernel.dtype
        if query is value and key is value and attention_mask is None and not return_attention_scores:
            qkv = dense_op(query.to(dt), self.qkv_kernel, self.qkv_bias, None)
            ctx = ops.attention(qkv, H, None, p, bool(training), causal=causal)
            return dense_op(ctx, self.out_kernel, self.out_bias, None)
        def cross_proj():  # Q from the first third of the packed kernel, K | V from the other two
            bias = self.qkv_bias
            q = dense_op(query.to(dt), self.qkv_kernel[:hd], None if bias is None else bias[:hd], None)
            if key is value:  # K | V are adjacent row blocks of the packed kernel: one GEMM
                kv = dense_op(value.to(dt), self.qkv_kernel[hd:], None if bias is None else bias[hd:], None)
            else:
                k = dense_op(key.to(dt), self.qkv_kernel[hd:2 * hd], None if bias is None else bias[hd:2 * hd], None)
                v = dense_op(value.to(dt), self.qkv_kernel[2 * hd:], None if bias is None else bias[2 * hd:], None)
                kv = torch.cat([k, v], dim=-1)
            return q, kv

        if attention_mask is None and not return_attention_scores and not causal:
            q, kv = cross_proj()
            ctx = ops.cross_attention(q, kv, H, None, p, bool(training))
            return dense_op(ctx, self.out_kernel, self.out_bias, None)
        if (not return_attention_scores and dt == torch.bfloat16 and D in ops.raw.ATTN_HEAD_DIMS
                and ops.use_native(query, value, key)):
            # masked attention (an attention_mask, or causal cross-attention) on the mask kernels
            allowed = None
            if attention_mask is not None:
                allowed = torch.as_tensor(attention_mask, device=query.device).bool()
                while allowed.dim() < 3:
                    allowed = allowed[None]
                if allowed.dim() == 3:
                    allowed = allowed[:, None]  # heads
            if query is value and key is value:
                qkv = dense_op(query.to(dt), self.qkv_kernel, self.qkv_bias, None)
                ctx = ops.attention(qkv, H, None, p, bool(training), causal=causal, mask=allowed)
            else:
                if causal:
                    tri = torch.ones(query.shape[1], key.shape[1], dtype=torch.bool, device=query.device).tril()
                    allowed = tri if allowed is None else allowed & tri
                q, kv = cross_proj()
                ctx = ops.cross_attention(q, kv, H, None, p, bool(training), mask=allowed)
            return dense_op(ctx, self.out_kernel, self.out_bias, None)

        def proj(x, i):
            b = None if self.qkv_bias is None else self.qkv_bias[i * hd:(i + 1) * hd]
            y = dense_op(x.to(dt), self.qkv_kernel[i * hd:(i + 1) * hd], b, None)
            return y.float().reshape(y.shape[0], y.shape[1], H, D).transpose(1, 2)  # [B, H, len, D]

        q, k, v = proj(query, 0), proj(key, 1), proj(value, 2)
        T, S = q.shape[2], k.shape[2]
        att = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
        allowed = None
        if attention_mask is not None:
            allowed = torch.as_tensor(attention_mask, device=att.device).bool()
            while allowed.dim() < 3:
                allowed = allowed[None]
            if allowed.dim() == 3:
                allowed = allowed[:, None]  # heads
        if causal:
            tri = torch.ones(T, S, dtype=torch.bool, device=att.device).tril()
            allowed = tri if allowed is None else allowed & tri
        if allowed is not None:
            att = att.masked_fill(~allowed, torch.finfo(att.dtype).min)
        scores = att.softmax(-1)
        pd = F.dropout(scores, p, training=True) if p > 0 else scores
        ctx = (pd @ v).transpose(1, 2).reshape(q.shape[0], T, hd).to(dt)
        out = dense_op(ctx, self.out_kernel, self.out_bias, None)
        return (out, scores) if return_attention_scores else out

    def compute_output_shape(self, input_shape):
        self._maybe_build(input_shape)
        return tuple(input_shape[0])

    def get_weights(self):
        H, D = self.num_heads, self.key_dim
        hd = H * D
        w = self.qkv_kernel.detach().float().cpu()
        dim = w.shape[1]
        out = []
        for i in range(3):
            out.append(w[i * hd:(i + 1) * hd].t().reshape(dim, H, D).contiguous().numpy())
            if self.use_bias:
                out.append(self.qkv_bias.detach().float().cpu()[i * hd:(i + 1) * hd].reshape(H, D).numpy())
        out.append(self.out_kernel.detach().float().cpu().t().reshape(H, D, dim).contiguous().numpy())
        if self.use_bias:
            out.append(self.out_bias.detach().float().cpu().numpy())
        return out

    def set_weights(self, weights):
        import numpy as np

        n = 8 if self.use_bias else 4
        if len(weights) != n:
            raise ValueError(f"expected {n} weight arrays, got {len(weights)}")
        hd = self.num_heads * self.key_dim
        ws = [torch.as_tensor(np.asarray(w)).float() for w in weights]
        step = 2 if self.use_bias else 1
        dim = self.qkv_kernel.shape[1]
        with torch.no_grad():
            for i in range(3):
                self.qkv_kernel[i * hd:(i + 1) * hd].copy_(ws[i * step].reshape(dim, hd).t())
                if self.use_bias:
                    self.qkv_bias[i * hd:(i + 1) * hd].copy_(ws[i * step + 1].reshape(hd))
            self.out_kernel.copy_(ws[3 * step].reshape(hd, dim).t())
            if self.use_bias:
                self.out_bias.copy_(ws[3 * step + 1].reshape(dim))

    def get_config(self):
        c = super().get_config()
        c.update(num_heads=self.num_heads, key_dim=self.key_dim, dropout=self.dropout, use_bias=self.use_bias,
                 kernel_initializer=self.kernel_initializer if isinstance(self.kernel_initializer, str)
                 else "glorot_uniform", use_causal_mask=self.use_causal_mask)
        return c


# ---- augmentation (K11): active only in training ------------------------------
class RandomFlip(Layer):
    def __init__(self, mode="horizontal", seed=None, **kw):
        super().__init__(**kw)
        self.mode = mode

    def call(self, x, training=None):
        if not training:
            return x
        B = x.shape[0]
        if "horizontal" in self.mode:
            m = torch.rand(B, device=x.device) < 0.5
            x = torch.where(m[:, None, None, None], x.flip(2), x)
        if "vertical" in self.mode:
            m = torch.rand(B, device=x.device) < 0.5
            x = torch.where(m[:, None, None, None], x.flip(1), x)
        return x

    def get_config(self):
        c = super().get_config()
        c["mode"] = self.mode
        return c


class _RandomAffine(Layer):
    def _affine(self, x, theta):
        grid = F.affine_grid(theta, (x.shape[0], x.shape[3], x.shape[1], x.shape[2]), align_corners=False)
        y = F.grid_sample(x.permute(0, 3, 1, 2).float(), grid, padding_mode="reflection", align_corners=False)
        return y.permute(0, 2, 3, 1).to(x.dtype).contiguous()


class RandomRotation(_RandomAffine):
    def __init__(self, factor, seed=None, **kw):
        super().__init__(**kw)
        self.factor = factor

    def call(self, x, training=None):
        if not training:
            return x
        lo, hi = (-self.factor, self.factor) if not isinstance(self.factor, (tuple, list)) else self.factor
        ang = (torch.rand(x.shape[0], device=x.device) * (hi - lo) + lo) * 2 * math.pi
        c, s = torch.cos(ang), torch.sin(ang)
        z = torch.zeros_like(c)
        theta = torch.stack([torch.stack([c, -s, z], 1), torch.stack([s, c, z], 1)], 1)
        return self._affine(x, theta)

    def get_config(self):
        c = super().get_config()
        c["factor"] = self.factor
        return c


class RandomTranslation(_RandomAffine):
    def __init__(self, height_factor, width_factor, seed=None, **kw):
        super().__init__(**kw)
        self.hf, self.wf = height_factor, width_factor

    def call(self, x, training=None):
        if not training:
            return x
        B = x.shape[0]
        ty = (torch.rand(B, device=x.device) * 2 - 1) * self.hf * 2
        tx = (torch.rand(B, device=x.device) * 2 - 1) * self.wf * 2
        o, z = torch.ones(B, device=x.device), torch.zeros(B, device=x.device)
        theta = torch.stack([torch.stack([o, z, tx], 1), torch.stack([z, o, ty], 1)], 1)
        return self._affine(x, theta)


class RandomZoom(_RandomAffine):
    def __init__(self, height_factor, width_factor=None, seed=None, **kw):
        super().__init__(**kw)
        self.hf = height_factor
        self.wf = width_factor if width_factor is not None else height_factor

    def call(self, x, training=None):
        if not training:
            return x
        B = x.shape[0]
        zy = 1 + (torch.rand(B, device=x.device) * 2 - 1) * abs(self.hf)
        zx = 1 + (torch.rand(B, device=x.device) * 2 - 1) * abs(self.wf)
        z = torch.zeros(B, device=x.device)
        theta = torch.stack([torch.stack([zx, z, z], 1), torch.stack([z, zy, z], 1)], 1)
        return self._affine(x, theta)


class _RandomResize(Layer):
    """Keras RandomHeight / RandomWidth: one factor per batch, the output size changes."""

    axis = 1

    def __init__(self, factor, interpolation="bilinear", seed=None, **kw):
        super().__init__(**kw)
        self.factor = factor
        self.interpolation = interpolation

    def call(self, x, training=None):
        if not training:
            return x
        lo, hi = (-self.factor, self.factor) if not isinstance(self.factor, (tuple, list)) else self.factor
        f = 1.0 + float(torch.empty(()).uniform_(lo, hi))
        size = [x.shape[1], x.shape[2]]
        size[self.axis - 1] = max(1, int(round(size[self.axis - 1] * f)))
        mode = "bilinear" if self.interpolation == "bilinear" else "nearest"
        y = F.interpolate(x.permute(0, 3, 1, 2).float(), size=size, mode=mode,
                          align_corners=False if mode == "bilinear" else None)
        return y.permute(0, 2, 3, 1).to(x.dtype).contiguous()

    def get_config(self):
        c = super().get_config()
        c["factor"] = self.factor
        return c


class RandomHeight(_RandomResize):
    axis = 1


class RandomWidth(_RandomResize):
    axis = 2


class RandomContrast(Layer):
    def __init__(self, factor, seed=None, **kw):
        super().__init__(**kw)
        self.factor = factor

    def call(self, x, training=None):
        if not training:
            return x
        f = 1 + (torch.rand(x.shape[0], 1, 1, 1, device=x.device) * 2 - 1) * self.factor
        m = x.mean(dim=(1, 2), keepdim=True)
        return (x - m) * f + m


class Lambda(Layer):
    def __init__(self, function, **kw):
        super().__init__(**kw)
        self.function = function

    def call(self, x, training=None):
        return self.function(x)


class TorchModule(Layer):
    """Wrap an arbitrary (already-built) ``nn.Module`` as a Keras layer."""

    def __init__(self, module, **kw):
        super().__init__(**kw)
        self.module = module
        self.built = True

    def call(self, x, training=None):
        return self.module(x)


LAYERS = {cls.__name__: cls for cls in [
    Dense, Conv2D, DepthwiseConv2D, SeparableConv2D, MaxPooling2D, AveragePooling2D, GlobalAveragePooling2D,
    GlobalMaxPooling2D, MaxPooling1D, AveragePooling1D, GlobalAveragePooling1D, GlobalMaxPooling1D, Flatten, Reshape,
    Dropout, Activation, ReLU, Softmax, BatchNormalization, LayerNormalization, Embedding, Rescaling, Add,
    Concatenate, MultiHeadAttention, RandomFlip, RandomRotation, RandomTranslation, RandomZoom, RandomContrast,
    InputLayer]}
MaxPool2D = MaxPooling2D
AvgPool2D = AveragePooling2D
GlobalAvgPool2D = GlobalAveragePooling2D
GlobalMaxPool2D = GlobalMaxPooling2D
MaxPool1D = MaxPooling1D
AvgPool1D = AveragePooling1D
GlobalAvgPool1D = GlobalAveragePooling1D
GlobalMaxPool1D = GlobalMaxPooling1D
Convolution2D = Conv2D
SeparableConvolution2D = SeparableConv2D


class experimental:  # namespace parity: tf.keras.layers.experimental.preprocessing (TF 2.3)
    class preprocessing:
        RandomFlip = RandomFlip
        RandomRotation = RandomRotation
        RandomTranslation = RandomTranslation
        RandomZoom = RandomZoom
        RandomContrast = RandomContrast
        RandomHeight = RandomHeight
        RandomWidth = RandomWidth
        Rescaling = Rescaling
