"""The pooling / un-pooling family stated in float64 (plain numpy: no torch, no oracle), the per-element check the kernels
are held to, and the synthetic graphs the tests share.

Every op of the family is one of two sums over a neighbour graph (nn_index [B, M, K] ids of source points, nn_count [B, M]):
  gather   out[b, m, c]  = sum_{k < cnt[b, m]} w_k * x[b, idx[b, m, k], c]        avg / mean: w_k = 1 / cnt; weighted: weight[b, m, k]
  scatter  grad[b, n, c] = sum over edges (m, k) with idx[b, m, k] == n of w_k * go[b, m, c]
or the max scan of tf_pool3d_gpu.cu:17-29 and its one-term-per-output scatter.  Each sum comes with ``mag`` — the same sum over
absolute values, the quantity a floating-point sum's error is proportional to (tests/_errors.py) — and ``terms``, the number of
terms of each element.

The bound of assert_sum is derived, not measured.  An fp32 fmaf or add chain of n terms rounds at most n times; the kernels add
at most three more roundings — the rounded 1 / cnt, the multiplication by it, and the final adds: one add for the two half-waves,
or three adds for the split kernel's four partial sums, whose chains are each a quarter as long.  Every rounding is at most
2^-24 of a partial sum, and every partial sum is at most mag:  |got - ref| <= (terms + 3) * 2^-24 * mag.  At cnt = 1 that is
40 times tighter than the project's 1e-5 * mag: where a wrong reciprocal or a dropped tail shows."""
import numpy as np

from _errors import assert_per_element

U = 2.0 ** -24


def gather_ref(x, idx, cnt, weight=None, mean=False):
    """-> (out64, mag64, terms), each [B, M, C].  Accumulated slot by slot: nothing of shape [B, M, K, C] exists."""
    x = np.asarray(x)
    B, M, K = idx.shape
    C = x.shape[2]
    out = np.zeros((B, M, C), np.float64)
    mag = np.zeros((B, M, C), np.float64)
    for b in range(B):
        xb = x[b].astype(np.float64)
        for k in range(min(K, int(cnt[b].max()) if M else 0)):
            sel = np.nonzero(cnt[b] > k)[0]
            t = xb[idx[b, sel, k]]
            if weight is not None:
                t = t * weight[b, sel, k].astype(np.float64)[:, None]
            out[b, sel] += t
            mag[b, sel] += np.abs(t)
    if mean:
        inv = 1.0 / np.maximum(cnt, 1).astype(np.float64)
        out *= inv[:, :, None]
        mag *= inv[:, :, None]
    terms = np.broadcast_to(np.asarray(cnt, np.int64)[:, :, None], out.shape)
    return out, mag, terms


def scatter_ref(go, idx, cnt, n_src, weight=None, mean=False):
    """-> (grad64, mag64, terms), each [B, n_src, C]; terms = the in-degree of the source"""
    go = np.asarray(go)
    B, M, K = idx.shape
    C = go.shape[2]
    grad = np.zeros((B, n_src, C), np.float64)
    mag = np.zeros((B, n_src, C), np.float64)
    deg = np.zeros((B, n_src), np.int64)
    for b in range(B):
        gb = go[b].astype(np.float64)
        if mean:
            gb = gb * (1.0 / np.maximum(cnt[b], 1).astype(np.float64))[:, None]
        for k in range(min(K, int(cnt[b].max()) if M else 0)):
            sel = np.nonzero(cnt[b] > k)[0]
            t = gb[sel]
            if weight is not None:
                t = t * weight[b, sel, k].astype(np.float64)[:, None]
            np.add.at(grad[b], idx[b, sel, k], t)
            np.add.at(mag[b], idx[b, sel, k], np.abs(t))
            np.add.at(deg[b], idx[b, sel, k], 1)
    terms = np.broadcast_to(deg[:, :, None], grad.shape)
    return grad, mag, terms


def max_ref(x, idx, cnt):
    """the reference's scan (tf_pool3d_gpu.cu:17-29) -> (out32, arg32): slot 0 seeds unconditionally (a NaN there stays), a
    strict > replaces (a later NaN never wins, the first of equal values is kept, +0 and -0 are equal); cnt = 0 gives (0, 0)"""
    x = np.asarray(x, np.float32)
    B, M, K = idx.shape
    C = x.shape[2]
    out = np.zeros((B, M, C), np.float32)
    arg = np.zeros((B, M, C), np.int32)
    for b in range(B):
        has = cnt[b] > 0
        first = np.where(has, idx[b, :, 0], 0)
        o = x[b][first]
        a = np.broadcast_to(first[:, None].astype(np.int32), o.shape).copy()
        for k in range(1, min(K, int(cnt[b].max()) if M else 0)):
            sel = np.nonzero(cnt[b] > k)[0]
            n = idx[b, sel, k]
            v = x[b][n]
            with np.errstate(invalid="ignore"):
                rep = v > o[sel]
            o[sel] = np.where(rep, v, o[sel])
            a[sel] = np.where(rep, n[:, None].astype(np.int32), a[sel])
        o[~has] = 0.0
        a[~has] = 0
        out[b], arg[b] = o, a
    return out, arg


def max_grad_ref(go, arg, n_src):
    """grad[b, arg[b, m, c], c] += go[b, m, c]  (tf_pool3d_gpu.cu:38-50) -> (grad64, mag64, terms)"""
    go = np.asarray(go)
    B, M, C = go.shape
    grad = np.zeros((B, n_src, C), np.float64)
    mag = np.zeros((B, n_src, C), np.float64)
    terms = np.zeros((B, n_src, C), np.int64)
    cols = np.broadcast_to(np.arange(C)[None, :], (M, C))
    for b in range(B):
        gb = go[b].astype(np.float64)
        np.add.at(grad[b], (arg[b], cols), gb)
        np.add.at(mag[b], (arg[b], cols), np.abs(gb))
        np.add.at(terms[b], (arg[b], cols), 1)
    return grad, mag, terms


def assert_sum(got, ref, mag, terms, what):
    """got (fp32) against a float64 sum: no NaN left, tests/_errors.assert_per_element at its defaults (1e-5 * mag, 256 ULP, exact
    zeros where nothing contributes), and |got - ref| <= (terms + 3) * 2^-24 * mag per element.  Returns (and prints) the largest
    used fraction of that last bound."""
    got = np.asarray(got)
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, got.shape, ref.shape)
    nans = int(np.isnan(got).sum())
    assert nans == 0, "%s: %d elements are NaN (unwritten, or a non-finite product)" % (what, nans)
    bound = (np.asarray(terms, np.float64) + 3.0) * U * mag
    err = np.abs(got.astype(np.float64) - ref)
    live = bound > 0
    used = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print("%s: max |err| / ((terms + 3) 2^-24 mag) = %.3f" % (what, used))
    assert_per_element(got, ref, mag, what)
    worst = np.unravel_index(int(np.argmax(np.where(live, err / np.where(live, bound, 1.0), 0.0))), err.shape)
    assert used <= 1.0, ("%s: element %s is off by %.3e, %.2f of (terms + 3) * 2^-24 * mag (terms %d, mag %.3e)"
                         % (what, worst, err[worst], used, np.asarray(terms)[worst], mag[worst]))
    return used


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- synthetic graphs ----------------------------------------------------------------------------------------------------------
def make_graph(rng, B, n_src, M, K, unique=True, high_from=None, empty_rows=()):
    """nn_index [B, M, K] i32 (ascending ids without repeats per row when `unique`, else random ids; slots past the count hold
    0), nn_count [B, M] i32 drawn uniformly from 0..K with rows of count 0, 1, 2, K - 1 and K forced
    into every cloud.  high_from: every second row's count is drawn from high_from..K.  empty_rows: rows whose count is 0 in every cloud."""
    assert not unique or K <= n_src
    cnt = rng.randint(0, K + 1, size=(B, M)).astype(np.int32)
    if high_from is not None:
        cnt[:, ::2] = rng.randint(high_from, K + 1, size=cnt[:, ::2].shape)
    forced = [0, 1, 2, K - 1, K]
    empty_rows = np.asarray(empty_rows, np.int64)
    cnt[:, empty_rows] = 0
    for b in range(B):
        free = rng.permutation(M)
        free = free[~np.isin(free, empty_rows)]
        cnt[b, free[:len(forced)]] = forced
    if not unique:
        idx = rng.randint(0, n_src, size=(B, M, K)).astype(np.int32)
    elif B * M <= 4096:
        idx = np.zeros((B, M, K), np.int32)
        for b in range(B):
            for m in range(M):
                c = int(cnt[b, m])
                idx[b, m, :c] = np.sort(rng.permutation(n_src)[:c])
    else:       # many rows: ascending by construction, positive steps of at most n_src // K
        g = n_src // K
        step = rng.randint(1, g + 1, size=(B, M, K))
        step[:, :, 0] = rng.randint(0, g, size=(B, M))
        idx = np.cumsum(step, axis=2).astype(np.int32)
        assert int(idx.max()) < n_src
    idx[np.arange(K)[None, None, :] >= cnt[:, :, None]] = 0
    for v in forced:
        assert (cnt == v).any(axis=1).all()
    return idx, cnt


def make_values(rng, shape):
    """fp32 normal values; every third point rounded (ties for the arg-max rule), a few exact +0 and -0"""
    x = rng.randn(*shape).astype(np.float32)
    x[:, ::3] = np.round(x[:, ::3])
    flat = x.reshape(-1)
    where = rng.permutation(flat.size)[:max(4, flat.size // 50)]
    flat[where[0::2]] = 0.0
    flat[where[1::2]] = -0.0
    return x


def make_weights(rng, cnt, K):
    """[B, M, K] fp32 interpolation weights: positive, each row's live slots sum to 1, slots past the count are 0"""
    w = (rng.rand(*cnt.shape, K) + 0.05).astype(np.float32)
    w[np.arange(K)[None, None, :] >= cnt[:, :, None]] = 0
    s = w.sum(-1, keepdims=True)
    return (w / np.where(s > 0, s, 1)).astype(np.float32)
