"""The depthwise convolution and its gradient (csrc/conv3d.hip) stated in float64 (plain numpy: no torch, no oracle), and the
per-element check the kernels are held to.

With a neighbour graph nn_index / nn_count [B, M, K] over N source points, bin ids bin_index [B, M, K], a filter w [F, C, r],
clamp(f) = min(max(f, 0), F - 1) (all three forward kernels and the transposed graph clamp so) and, per live edge
e = (b, m, k < cnt[b, m]) with n = idx[e], f = clamp(bin[e]):
  out[b, m, c r + rho]    = (1 / cnt[b, m]) sum_k x[b, n, c] w[f, c, rho]                        rows with cnt = 0: exact 0
  grad_input[b, n, c]     = sum over the edges naming n, sum_rho  go[b, m, c r + rho] / cnt[b, m] * w[f, c, rho]
  grad_filter[f, c, rho]  = sum over all clouds' edges of bin f   go[b, m, c r + rho] / cnt[b, m] * x[b, n, c]
Each sum comes with ``mag``, the same sum over absolute values (tests/_errors.py), and with the counts its bound needs.

The bounds are derived, not measured: u = 2^-24, every fp32 rounding is at most u times a partial sum, every partial sum at
most mag.  Second-order terms are left out; the slack named below covers them.

forward  (cnt + 4) u mag
  cnt   the fmaf chain of dwconv_fwd_multi / dwconv_fwd_row (`acc = fmaf(x, w, acc)`); padding slots multiply by the zero row,
        which is exact; dwconv_fwd_multi splits the chain over EPL = 1, 2 or 4 lane groups, which only shortens it
  2     the cross-group adds (`acc[v] += __shfl_xor(acc[v], o)`, o = LPE .. 32: log2 EPL <= 2)
  1 + 1 `inv = 1.0f / (float)cnt` and `acc * inv`.  dwconv_fwd_generic divides instead (`acc[t] / (float)cnt`): cnt + 1.
  (An fp32 emulation of the 1-, 2- and 4-group orders over 4000 random rows, cnt 1..70, used at most 0.38 of it.)

grad_input, rows outside the hub launch  (2 deg + nseg + r + 2) u mag     deg: in-edges of the source, nseg: its non-empty bins
  deg   the fmaf chains `sg[v] = fmaf(g, sc, sg[v])`, one per segment: a chain of L edges rounds L times, each time at most
        u |w| mag(segment); summed over the segments, at most deg u mag
  deg   the rounded scales (`tg_packed_scale`: 1.0f / count, or ent_scale): u |term| each, u mag in all — deg is generous,
        and that slack pays for what the next line leaves out
  nseg  `gi[v] = fmaf(sg[v], wr[v], gi[v])`, once per segment — and once more per 64-edge chunk boundary that falls inside
        a segment (the chunk loop clips segments to a chunk): at most deg / 64 further roundings, inside the slack above
  r - 1 `s += gi[u * R + rr]`;  2: `gi[v] += __shfl_xor(gi[v], 32)` and `(…, 16)`, the half and quarter waves' partial sums
  dwconv_bwd_t_generic walks (segment, rho) with the same two fmaf and no cross-lane add: fewer.
grad_input, rows of the hub launch  + 4 kHubGroup = 32: `atomicAdd(&gp[u], s)`, one per wave that shares the source.

grad_filter  (2 E_f + S_f + 5 + depth) u mag     E_f: the bin's edges, S_f: its non-empty (cloud, source, bin) segments
  2 E_f  as 2 deg above (chains and scales), with the same slack for chunk boundaries
  S_f    `acc[fi][v] = fmaf(sg[v], xv[v], acc[fi][v])`, once per segment, whichever wave holds the accumulator
  5      the wave parts (`acc[i][v] += __shfl_xor(…, 32)`, `(…, 16)`) and the three turns `*p + acc[i][v]` of waves 1..3
  depth  reduce_filter_partials: each of 32 lanes adds ceil(slabs / 32) slabs in turn, then `s += red[k][cx]`, k = 1..31:
         ceil(slabs / 32) + 31, slabs = what the launcher passes as nparts (restated in tests/test_gpu_conv_forms.py).
         dwconv_bwd_t_generic has no slabs: one LDS atomic per segment (`sg * x`, rounded, then the add: 2 S_f, within
         2 E_f + S_f as S_f <= E_f) and one global atomic per workgroup: depth = B * ceil(N / 64), its workgroups per slice.

Left out on purpose: the 32-bit-offset fall-backs (N C or M C r near 2^32, N above 2^24) and neighbour ids outside [0, N)."""
import numpy as np

from _errors import assert_per_element
from _pool_ref import U, bits, make_graph  # noqa: F401  (re-exported: the conv tests draw their graphs with make_graph)

K_HUB_GROUP = 8          # conv3d.hip: kHubGroup


def clamp_bins(bins, F):
    return np.clip(np.asarray(bins).astype(np.int64), 0, F - 1)


def _slots(cnt_b, K):
    return range(min(K, int(cnt_b.max()) if cnt_b.size else 0))


def conv_ref(x, w, idx, cnt, bins):
    """-> (out64, mag64, terms), each [B, M, C r]; terms = cnt.  Slot by slot: nothing of shape [B, M, K, C] exists."""
    x, w = np.asarray(x), np.asarray(w)
    B, M, K = idx.shape
    F, C, r = w.shape
    w64 = w.astype(np.float64)
    out = np.zeros((B, M, C * r), np.float64)
    mag = np.zeros((B, M, C * r), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            xb = x[b].astype(np.float64)
            for k in _slots(cnt[b], K):
                sel = np.nonzero(cnt[b] > k)[0]
                t = (xb[idx[b, sel, k]][:, :, None] * w64[clamp_bins(bins[b, sel, k], F)]).reshape(sel.size, C * r)
                out[b, sel] += t
                mag[b, sel] += np.abs(t)
        inv = 1.0 / np.maximum(cnt, 1).astype(np.float64)
        out *= inv[:, :, None]
        mag *= inv[:, :, None]
    terms = np.broadcast_to(np.asarray(cnt, np.int64)[:, :, None], out.shape)
    return out, mag, terms


class ConvGrad:
    """grad_input [B, N, C] with gi_mag, deg [B, N], nseg [B, N]; grad_filter [F, C, r] with gf_mag, E_f [F], S_f [F]"""

    def __init__(self, B, N, F, C, r):
        self.gi, self.gi_mag = np.zeros((B, N, C), np.float64), np.zeros((B, N, C), np.float64)
        self.gf, self.gf_mag = np.zeros((F, C, r), np.float64), np.zeros((F, C, r), np.float64)
        self.seg = np.zeros((B, N, F), np.int64)           # edges per (cloud, source, bin)

    @property
    def deg(self):
        return self.seg.sum(axis=2)

    @property
    def nseg(self):
        return (self.seg > 0).sum(axis=2)

    @property
    def E_f(self):
        return self.seg.sum(axis=(0, 1))

    @property
    def S_f(self):
        return (self.seg > 0).sum(axis=(0, 1))

    def gi_terms(self, r, hub_rows=None):
        """[B, N, 1]: 2 deg + nseg + r + 2, and 4 kHubGroup more in the rows of hub_rows (bool [B, N])"""
        t = 2 * self.deg + self.nseg + r + 2
        if hub_rows is not None:
            t = t + 4 * K_HUB_GROUP * hub_rows
        return t[:, :, None]

    def gf_terms(self, depth):
        """[F, 1, 1]: 2 E_f + S_f + 5 + depth (vector kernels: depth = reduce_depth(slabs))"""
        return (2 * self.E_f + self.S_f + 5 + depth)[:, None, None]


def reduce_depth(slabs):
    return (slabs + 31) // 32 + 31


def conv_grad_ref(x, w, go, idx, cnt, bins):
    x, w, go = np.asarray(x), np.asarray(w), np.asarray(go)
    B, M, K = idx.shape
    N = x.shape[1]
    F, C, r = w.shape
    g = ConvGrad(B, N, F, C, r)
    w64 = w.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            xb = x[b].astype(np.float64)
            gb = go[b].astype(np.float64).reshape(M, C, r) * (1.0 / np.maximum(cnt[b], 1).astype(np.float64))[:, None, None]
            for k in _slots(cnt[b], K):
                sel = np.nonzero(cnt[b] > k)[0]
                n, f = idx[b, sel, k], clamp_bins(bins[b, sel, k], F)
                ti = gb[sel] * w64[f]                                  # [edges, C, r]
                np.add.at(g.gi[b], n, ti.sum(axis=2))
                np.add.at(g.gi_mag[b], n, np.abs(ti).sum(axis=2))
                tf = gb[sel] * xb[n][:, :, None]
                np.add.at(g.gf, f, tf)
                np.add.at(g.gf_mag, f, np.abs(tf))
                np.add.at(g.seg[b], (n, f), 1)
    return g


def assert_conv(got, ref, mag, bound_terms, what):
    """got (fp32) against a float64 sum: no NaN left, tests/_errors.assert_per_element at its defaults (1e-5 mag, 256 ULP on
    well-conditioned elements, exact zeros where nothing contributes), then |got - ref| <= bound_terms 2^-24 mag per element.
    Prints and returns the largest used fraction of that derived bound."""
    got = np.asarray(got)
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, got.shape, ref.shape)
    nans = int(np.isnan(got).sum())
    assert nans == 0, "%s: %d elements are NaN (unwritten, a stale slab, or a non-finite product)" % (what, nans)
    assert_per_element(got, ref, mag, what)
    bound = np.broadcast_to(np.asarray(bound_terms, np.float64), ref.shape) * U * mag
    err = np.abs(got.astype(np.float64) - ref)
    live = bound > 0
    frac = np.where(live, err / np.where(live, bound, 1.0), 0.0)
    used = float(frac.max()) if frac.size else 0.0
    print("%s: max |err| / (terms 2^-24 mag) = %.3f" % (what, used))
    if used > 1.0:
        worst = np.unravel_index(int(np.argmax(frac)), err.shape)
        raise AssertionError("%s: element %s is off by %.3e, %.2f of its derived bound (terms %d, mag %.3e)"
                             % (what, worst, err[worst], used, np.broadcast_to(bound_terms, ref.shape)[worst], mag[worst]))
    return used


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def make_bins(rng, idx, cnt, F, pool=None):
    """bin ids [B, M, K] from `pool` (default: all F bins); slots past the count hold F + 7 (garbage a kernel must not read as a bin)"""
    pool = np.arange(F) if pool is None else np.asarray(pool)
    b = pool[rng.randint(0, pool.size, size=idx.shape)].astype(np.int32)
    b[np.arange(idx.shape[2])[None, None, :] >= cnt[:, :, None]] = F + 7
    return b


def make_values(rng, shape):
    """fp32 normal values with a few exact zeros and a wide range of magnitudes (every fifth row scaled by 2^-10)"""
    v = rng.randn(*shape).astype(np.float32)
    if v.ndim >= 2 and v.shape[-2] >= 5:
        v[..., ::5, :] *= np.float32(2.0 ** -10)
    flat = v.reshape(-1)
    if flat.size >= 8:
        flat[rng.permutation(flat.size)[:max(2, flat.size // 60)]] = 0.0
    return v
