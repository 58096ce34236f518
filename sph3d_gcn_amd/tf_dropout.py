"""Keyed dropout — tf.layers.dropout with a counter-based mask (csrc/dropout.hip; harness/dropout.py states it in numpy).

``dropout_keyed(x, rate, key=(seed, step), layer, row0=0)`` is a pure function of its arguments: no generator, no saved mask.
The backward pass is the same kernel on grad_output with the same key.
"""
import math

import numpy as np
import torch

from . import _lib

MAX_LAYERS = 16          # csrc/feed_draws.hpp: kFeedDropoutLayers


def _threshold(rate):
    return min(2 ** 32 - 1, int(math.ceil(rate * 2.0 ** 32)))


def _dropout_keyed_impl(x, rate, seed, step, layer, row0):
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise ValueError("dropout_keyed: fp32 input expected, got %s" % x.dtype)
    if x.dim() < 2:
        raise ValueError("dropout_keyed: x [B, C] or [B, ..., C] expected")
    x = x.contiguous()
    B = x.shape[0]
    row_len = x.numel() // B if B else 0
    y = torch.empty_like(x)
    _lib.check(_lib.lib().sph3d_dropout_keyed(B, row_len, _lib.ptr(x), _lib.ptr(y), seed & 0xffffffffffffffff, step & 0xffffffffffffffff,
                                              row0, layer, _threshold(rate), float(np.float32(1.0 / (1.0 - rate))), _lib.stream_ptr()))
    return y


class _DropoutKeyedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rate, seed, step, layer, row0):
        ctx.args = (rate, seed, step, layer, row0)         # the key, not a mask
        return _dropout_keyed_impl(x, rate, seed, step, layer, row0)

    @staticmethod
    def backward(ctx, grad_output):
        return _dropout_keyed_impl(grad_output, *ctx.args), None, None, None, None, None


def dropout_keyed(x, rate, key, layer, row0=0):
    """x [B, C] or [B, ..., C] fp32 on the device -> x / (1 - rate) where element i of row row0 + b survives the draw of
    (seed, step, row0 + b, layer, i), +0.0 elsewhere (whatever x holds there).  key = (seed, step); layer in [0, 16): one number
    per dropout layer of a model; row0: the number of row 0 in the global batch (rank * B for a batch sharded by rank).
    rate <= 0 is the identity, rate >= 1 gives zeros."""
    rate, layer, row0 = float(rate), int(layer), int(row0)
    seed, step = int(key[0]), int(key[1])
    if not 0 <= layer < MAX_LAYERS:
        raise ValueError("dropout_keyed: layer %d outside [0, %d)" % (layer, MAX_LAYERS))
    if not rate >= 0.0 or rate > 1.0:
        raise ValueError("dropout_keyed: 0 <= rate <= 1 required, got %r" % rate)
    if rate == 0.0:
        return x
    if rate == 1.0:
        return torch.zeros_like(x)          # (nothing survives: no draw, and no gradient reaches x)
    return _DropoutKeyedFn.apply(x, rate, seed, step, layer, row0)
