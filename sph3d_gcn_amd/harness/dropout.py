"""Keyed dropout stated in numpy (csrc/dropout.hip, tf_dropout.dropout_keyed): the SPECIFICATION of the mask, no GPU.

Inverted dropout whose mask is a counter-based draw of harness/feed.py, like every other draw of a training run: a pure function
of (seed, step, row, layer, element), no generator state.  For x [B, ...] fp32, with L the number of elements of a row x[b]:

    ck    = feed.cloud_key(seed, step, row0 + b)
    w     = feed.draw(ck, DROPOUT + layer, i)             i < L < 2^32: the element's index inside row b
    keep  = feed._hi(w) >= threshold(rate)                threshold = min(2^32 - 1, ceil(rate 2^32)); rate 0.5: 0x80000000, P(keep) = 1/2
    y     = float32(x) * float32(1 / (1 - rate)) where kept, +0.0 where dropped, whatever x holds

rate <= 0 keeps everything unscaled, rate >= 1 drops everything (no draw is made).  `row0` is the row's number in a larger batch:
rank k of a sharded batch passes row0 = k B, so a batch's masks do not depend on how it is sharded.  The gradient is the same
function of grad_output.  The device result equals this statement bit for bit (tests/test_gpu_dropout.py)."""
import math

import numpy as np

from . import feed

DROPOUT = 16             # the `purpose` of a dropout draw: DROPOUT + layer (csrc/feed_draws.hpp: kFeedDropout); 1..15 are the feeds' and the sampler's
MAX_LAYERS = 16


def threshold(rate):
    """the 32-bit word a draw's high word must reach to keep its element"""
    return min(2 ** 32 - 1, int(math.ceil(float(rate) * 2.0 ** 32)))


def scale(rate):
    """float32(1 / (1 - rate)), the division in float64"""
    return np.float32(1.0 / (1.0 - float(rate)))


def check(row_len, layer, row0, B):
    if not 0 <= int(layer) < MAX_LAYERS:
        raise ValueError("dropout: layer %d outside [0, %d)" % (layer, MAX_LAYERS))
    if int(row_len) >= 2 ** 32:
        raise ValueError("dropout: rows of %d elements (< 2^32 required)" % row_len)
    if int(row0) < 0 or int(row0) + int(B) > 2 ** 32:
        raise ValueError("dropout: rows %d .. %d + %d do not fit 32 bits" % (row0, row0, B))


def keep_reference(shape, rate, key, layer, row0=0):
    """-> bool array of `shape` = (B, ...): the elements that survive"""
    shape = tuple(int(d) for d in shape)
    B, L = shape[0], int(np.prod(shape[1:], dtype=np.int64))
    check(L, layer, row0, B)
    if rate <= 0.0:
        return np.ones(shape, bool)
    if rate >= 1.0:
        return np.zeros(shape, bool)
    seed, step = key
    thr = np.uint32(threshold(rate))
    keep = np.empty((B, L), bool)
    counters = np.arange(L, dtype=np.uint64)
    for b in range(B):
        ck = feed.cloud_key(int(seed), int(step), int(row0) + b)
        keep[b] = feed._hi(feed.draw(ck, DROPOUT + int(layer), counters)) >= thr
    return keep.reshape(shape)


def dropout_reference(x, rate, key, layer, row0=0):
    """x [B, ...] -> y fp32 of the same shape"""
    x = np.asarray(x, dtype=np.float32)
    if rate <= 0.0:
        return x.copy()
    keep = keep_reference(x.shape, rate, key, layer, row0)
    y = np.zeros(x.shape, np.float32)
    if rate < 1.0:
        with np.errstate(invalid="ignore", over="ignore"):
            y[keep] = x[keep] * scale(rate)
    return y
