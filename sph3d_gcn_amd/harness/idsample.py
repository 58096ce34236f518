"""Keyed inverse-density sampling: the numpy STATEMENT of csrc/idsample.hip (include/sph3d.h: sph3d_ids_sample), no GPU.

The sample of a cloud is a pure function of (nn_dist, nn_count, seed, step, level); the kernel's output equals
``ids_reference`` bit for bit.  For cloud b, point i, K = nn_dist.shape[2]:

  weight    w = (((d[0] + d[1]) + ...) + d[c-1]) / float(c),  c = min(nn_count[b, i], K): sequential fp32 adds in slot order, one
            correctly rounded fp32 division; slots >= c are not read (the search leaves zeros there, so this is the
            reduce_sum(intra_dst, -1) / cnt of utils/sph3gcn_util.py:38).  The point is INVALID if c <= 0 or w is not finite or
            w <= 0;
  uniform   u = ((hi >> 8) + 1) * 2^-24 in (0, 1], hi = the high word of feed.draw(feed.cloud_key(seed, step, b), IDS + level, i);
  race      t = E / w in fp32, E = neglog32(u) (include/sph3d_log32.h); an invalid point has t = +inf.  The S smallest t are the
            Gumbel top-k of tf_sample.py:27-41: log p - log(-log u) is monotone in p / (-log u);
  key       (bits(t) << 32) | i as one unsigned 64-bit word: t >= +0, so unsigned order is numeric order and ties go to the lower
            index;
  output    the low words of the S smallest keys in ascending key order (tf.nn.top_k's order: best first); invalid points come
            last, by index.
"""
import os
import re

import numpy as np

from . import feed

_F32 = np.float32
_U64 = np.uint64
IDS = feed.IDS             # the `purpose` of the draws (csrc/feed_draws.hpp: kFeedIds); level l uses IDS + l
LEVELS = 8
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include", "sph3d_log32.h")
_consts = None


def _header():
    global _consts
    if _consts is None:
        text = open(_HEADER).read()
        body = re.search(r"#define\s+SPH3D_LOG32_COEFFS\s*\{([^}]*)\}", text).group(1)
        degree = int(re.search(r"#define\s+SPH3D_LOG32_DEGREE\s+(\d+)", text).group(1))
        vals = [_F32(t.strip().rstrip("f")) for t in body.split(",")]
        if len(vals) != degree + 1:
            raise ValueError("sph3d_log32.h: %d coefficients for degree %d" % (len(vals), degree))
        ln2 = _F32(re.search(r"#define\s+SPH3D_LOG32_LN2\s+(\S+?)f\b", text).group(1))
        sqrt2 = np.uint32(int(re.search(r"#define\s+SPH3D_LOG32_SQRT2_BITS\s+(0x[0-9a-fA-F]+)u", text).group(1), 16))
        _consts = (np.array(vals, dtype=_F32), ln2, sqrt2)
    return _consts


def neglog32_coefficients():
    """c0 .. c5 = 2/(2k+1) as float32, read from include/sph3d_log32.h (the list is written once, there)"""
    return _header()[0]


def neglog32(u):
    """sph3d_neglog32 on a float32 array of normal numbers in (0, 1]: every step one fp32 operation"""
    u = np.ascontiguousarray(u, dtype=_F32)
    c, ln2, sqrt2 = _header()
    bits = u.view(np.uint32)
    e = (bits >> np.uint32(23)).astype(np.int32) - np.int32(127)
    mbits = (bits & np.uint32(0x007fffff)) | np.uint32(0x3f800000)
    big = mbits > sqrt2
    mbits = np.where(big, mbits - np.uint32(0x00800000), mbits).astype(np.uint32)
    e = e + big.astype(np.int32)
    m = mbits.view(_F32)
    s = (m - _F32(1)) / (m + _F32(1))
    z = s * s
    q = np.full(u.shape, c[-1], dtype=_F32)
    for k in range(len(c) - 2, -1, -1):
        q = q * z
        q = q + c[k]
    r = e.astype(_F32) * ln2
    r = r + s * q
    return _F32(0) - r


def ids_weight(nn_dist, nn_count):
    """-> (w [B, N] float32, valid [B, N] bool): the weight of the statement above"""
    d = np.asarray(nn_dist, dtype=_F32)
    B, N, K = d.shape
    c = np.minimum(np.asarray(nn_count).reshape(B, N).astype(np.int64), K)
    acc = np.zeros((B, N), dtype=_F32)
    with np.errstate(all="ignore"):
        for k in range(K):
            live = k < c
            acc = np.where(live, acc + np.where(live, d[:, :, k], _F32(0)), acc)
        w = (acc / c.astype(_F32)).astype(_F32)
        valid = (c > 0) & np.isfinite(w) & (w > 0)
    return w, valid


def ids_keys(nn_dist, nn_count, seed, step, level):
    """-> the 64-bit keys [B, N] of the statement above"""
    if not 0 <= int(level) < LEVELS:
        raise ValueError("inverse density sampling: level %d outside 0..%d" % (level, LEVELS - 1))
    w, valid = ids_weight(nn_dist, nn_count)
    B, N = w.shape
    idx = np.arange(N, dtype=_U64)
    keys = np.empty((B, N), dtype=_U64)
    for b in range(B):
        hi = (feed.draw(feed.cloud_key(seed, step, b), IDS + int(level), idx) >> _U64(32)).astype(np.uint32)
        u = ((hi >> np.uint32(8)) + np.uint32(1)).astype(_F32) * _F32(2.0 ** -24)
        with np.errstate(all="ignore"):
            t = np.where(valid[b], neglog32(u) / np.where(valid[b], w[b], _F32(1)), _F32(np.inf)).astype(_F32)
        keys[b] = (t.view(np.uint32).astype(_U64) << _U64(32)) | idx
    return keys


def ids_reference(nn_dist, nn_count, S, seed, step, level=0):
    """nn_dist [B, N, K] float32, nn_count [B, N] -> [B, S] int32: the S smallest keys' points, best first"""
    S = int(S)
    N = np.asarray(nn_dist).shape[1]
    if S <= 0 or S > N:
        raise ValueError("inverse density sampling: 0 < S <= N required, got S=%d N=%d" % (S, N))
    keys = ids_keys(nn_dist, nn_count, seed, step, level)
    keys = np.sort(keys, axis=1)[:, :S]
    return (keys & _U64(0xffffffff)).astype(np.int32)
