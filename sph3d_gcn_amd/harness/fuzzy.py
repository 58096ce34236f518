"""The fuzzy spherical kernel stated in numpy (csrc/fuzzy.hip): no torch, no library call.

``fuzzy_kernel_reference`` returns the two integer tensors of sph3d_fuzzy_spherical_kernel bit for bit: every float32 operation of
csrc/sphere_bin.hpp :49-68 is one numpy float32 operation, the double steps are float64, and include/sph3d_atan2f.h — plain
IEEE double arithmetic, no libm call — is restated line by line (``atan2f``).  ``fuzzy_conv_reference`` and
``fuzzy_conv_grad_reference`` are the convolution and its two gradients in float64, each with ``mag``, the same sum over absolute
values (tests/_errors.py), and the term counts the kernels' error bounds need.
"""
import numpy as np

_PI = 3.14159265358979323846            # csrc/sphere_bin.hpp: SPH3D_PI (== glibc M_PI)
_F32 = np.float32


# ---- include/sph3d_atan2f.h, vectorised --------------------------------------------------------------------------------------------
def _atan_pos(x):
    """sph3d_atan_pos: atan(x) for finite x >= 0, float64 in and out"""
    hi0, lo0 = 4.63647609000806093515e-01, 2.26987774529616870924e-17
    hi1, lo1 = 7.85398163397448278999e-01, 3.06161699786838301793e-17
    hi2, lo2 = 9.82793723247329054082e-01, 1.39033110312309984516e-17
    hi3, lo3 = 1.57079632679489655800e+00, 6.12323399573676603587e-17
    a0, a1 = 3.33333333333329318027e-01, -1.99999999998764832476e-01
    a2, a3 = 1.42857142725034663711e-01, -1.11111104054623557880e-01
    a4, a5 = 9.09088713343650656196e-02, -7.69187620504482999495e-02
    a6, a7 = 6.66107313738753120669e-02, -5.83357013379057348645e-02
    a8, a9 = 4.97687799461593236017e-02, -3.65315727442169155270e-02
    a10 = 1.62858201153657823623e-02
    x = np.asarray(x, np.float64)
    huge = x > 1.0e18
    r0 = x < 0.4375
    r1 = ~r0 & (x < 0.6875)
    r2 = ~r0 & ~r1 & (x < 1.1875)
    r3 = ~r0 & ~r1 & ~r2 & (x < 2.4375)
    with np.errstate(all="ignore"):
        xr = np.where(r0, x, np.where(r1, (2.0 * x - 1.0) / (2.0 + x), np.where(r2, (x - 1.0) / (x + 1.0),
                      np.where(r3, (x - 1.5) / (1.0 + 1.5 * x), -1.0 / x))))
        hi = np.where(r1, hi0, np.where(r2, hi1, np.where(r3, hi2, hi3)))
        lo = np.where(r1, lo0, np.where(r2, lo1, np.where(r3, lo2, lo3)))
        z = xr * xr
        w = z * z
        s1 = z * (a0 + w * (a2 + w * (a4 + w * (a6 + w * (a8 + w * a10)))))
        s2 = w * (a1 + w * (a3 + w * (a5 + w * (a7 + w * a9))))
        out = np.where(r0, xr - xr * (s1 + s2), hi - ((xr * (s1 + s2) - lo) - xr))
    return np.where(huge, hi3 + lo3, out)


def atan2f(yf, xf):
    """sph3d_atan2f(y, x) on float32 arrays -> float32, the same bits as the header on host and device"""
    pi, pi_lo = 3.14159265358979311600e+00, 1.22464679914735317720e-16
    pio2, pio4 = 1.57079632679489655800e+00, 7.85398163397448278999e-01
    yf, xf = np.broadcast_arrays(np.asarray(yf, _F32), np.asarray(xf, _F32))
    y, x = yf.astype(np.float64), xf.astype(np.float64)
    xneg, yneg = np.signbit(xf), np.signbit(yf)         # honours -0.0, as the header's 1 / -0 test does
    ay, ax = np.where(yneg, -y, y), np.where(xneg, -x, x)
    xinf, yinf = ax > 1.0e300, ay > 1.0e300
    with np.errstate(all="ignore"):
        z = _atan_pos(ay / ax)
        z = np.where(xneg, pi - (z - pi_lo), z)
        zinf = np.where(xinf & yinf, np.where(xneg, 3.0 * pio4, pio4), np.where(yinf, pio2, np.where(xneg, pi, 0.0)))
        z = np.where(xinf | yinf, zinf, z)
        z = np.where(ax == 0.0, pio2, z)
        z = np.where(ay == 0.0, np.where(xneg, pi, 0.0), z)
        out = np.where(yneg, -z, z).astype(_F32)
        nan = np.isnan(xf) | np.isnan(yf)
        return np.where(nan, xf + yf, out).astype(_F32)


# ---- csrc/sphere_bin.hpp :49-68 ----------------------------------------------------------------------------------------------------
def bin_coordinates(dx, dy, dz, dist, radius, kernel):
    """-> (alpha, beta, gamma float32, centre bool) of sphere_bin<false> for float32 arrays dx, dy, dz, dist"""
    n, p, q = (int(v) for v in kernel)
    dx, dy, dz, dist = (np.asarray(a, _F32) for a in (dx, dy, dz, dist))
    eps = _F32(1.01e-3)
    with np.errstate(all="ignore"):
        dist2d = np.sqrt((dx * dx + dy * dy).astype(_F32)).astype(_F32)
        centre = ~((dist > eps) & (np.abs((dist - eps).astype(_F32)).astype(np.float64) > 1e-6))
        theta = atan2f(dy, dx).astype(np.float64)
        phi = atan2f(dz, dist2d).astype(np.float64)
        theta = np.where(theta < _PI, theta, -_PI).astype(_F32).astype(np.float64)
        theta = np.where(theta > -_PI, theta, -_PI).astype(_F32).astype(np.float64)
        theta = (theta + _PI).astype(_F32)
        phi = np.where(phi < _PI / 2, phi, _PI / 2).astype(_F32).astype(np.float64)
        phi = np.where(phi > -_PI / 2, phi, -_PI / 2).astype(_F32).astype(np.float64)
        phi = (phi + _PI / 2).astype(_F32)
        alpha = (((theta * _F32(n)).astype(_F32) / _F32(2.0)).astype(_F32).astype(np.float64) / _PI).astype(_F32)
        beta = ((phi * _F32(p)).astype(_F32).astype(np.float64) / _PI).astype(_F32)
        gamma = ((dist * _F32(q)).astype(_F32) / (_F32(radius) + _F32(1e-6))).astype(_F32)
    return alpha, beta, gamma, centre


def hard_bins(alpha, beta, gamma, centre, kernel):
    """sphere_bin.hpp :70-74 on the coordinates above -> int32 bins (0 for a centre slot)"""
    n, p, q = (int(v) for v in kernel)
    nid = np.minimum(alpha.astype(np.int64), n - 1)
    pid = np.minimum(beta.astype(np.int64), p - 1)
    qid = np.minimum(np.minimum(gamma, _F32(1 << 20)).astype(np.int64), q - 1)
    return np.where(centre, 0, qid * p * n + pid * n + nid + 1).astype(np.int32)


def _frac8(a):
    """(floor(a), min(255, floor((a - floor(a)) * 256))) in float32 arithmetic"""
    fl = np.floor(a).astype(_F32)
    fr = (a - fl).astype(_F32)
    return fl, np.minimum(np.floor((fr * _F32(256.0)).astype(_F32)).astype(np.int64), 255)


def _clamped_axis(v, bins):
    fl, f8 = _frac8((v - _F32(0.5)).astype(_F32))
    low = ~(fl >= 0)
    high = fl >= _F32(bins - 1)
    lo = np.where(low, 0, np.where(high, bins - 1, np.clip(fl, 0, bins - 1).astype(np.int64)))
    return lo, np.where(low | high, 0, f8)


def fuzzy_words(alpha, beta, gamma, centre, kernel):
    """the slot's two words from its bin coordinates -> (filt_index, filt_frac) int32"""
    n, p, q = (int(v) for v in kernel)
    fl, fa8 = _frac8((alpha - _F32(0.5)).astype(_F32))
    i0 = np.mod(fl.astype(np.int64), n)
    j0, fb8 = _clamped_axis(beta, p)
    k0, fg8 = _clamped_axis(gamma, q)
    index = 1 + i0 + n * j0 + n * p * k0
    frac = fa8 | (fb8 << 8) | (fg8 << 16)
    return np.where(centre, 0, index).astype(np.int32), np.where(centre, 0, frac).astype(np.int32)


def slot_coordinates(database, query, nn_index, nn_count, nn_dist, radius, kernel):
    """-> (alpha, beta, gamma, centre, live) [B, M, K] for a graph; dead slots (k >= nn_count) carry garbage coordinates"""
    database, query = np.asarray(database, _F32)[:, :, :3], np.asarray(query, _F32)[:, :, :3]
    nn_index, nn_count = np.asarray(nn_index), np.asarray(nn_count)
    B, M, K = nn_index.shape
    live = np.arange(K)[None, None, :] < nn_count[:, :, None]
    idx = np.where(live, nn_index, 0)
    pt = database[np.arange(B)[:, None, None], idx]                    # [B, M, K, 3]
    d = (pt - query[:, :, None, :]).astype(_F32)
    dist = np.where(live, np.asarray(nn_dist, _F32), _F32(1.0))
    alpha, beta, gamma, centre = bin_coordinates(d[..., 0], d[..., 1], d[..., 2], dist, radius, kernel)
    return alpha, beta, gamma, centre, live


def fuzzy_kernel_reference(database, query, nn_index, nn_count, nn_dist, radius, kernel):
    """sph3d_fuzzy_spherical_kernel -> (filt_index, filt_frac) [B, M, K] int32, bit for bit"""
    alpha, beta, gamma, centre, live = slot_coordinates(database, query, nn_index, nn_count, nn_dist, radius, kernel)
    index, frac = fuzzy_words(alpha, beta, gamma, centre, kernel)
    return np.where(live, index, 0).astype(np.int32), np.where(live, frac, 0).astype(np.int32)


# ---- what every consumer derives from the two words --------------------------------------------------------------------------------
def corners(filt_index, filt_frac, kernel, num_bins):
    """-> (bins int64 [..., 8], weights int64 [..., 8]): corner t has bit 0 = upper sector, bit 1 = upper band, bit 2 = upper
    shell; its coefficient is weights * 2^-24 (the weights of a slot sum to 2^24).  filt_index <= 0: bin 0 with weight 2^24"""
    n, p, q = (int(v) for v in kernel)
    fi = np.asarray(filt_index).astype(np.int64)
    fr = np.asarray(filt_frac).astype(np.int64)
    centre = fi <= 0
    c = np.where(centre, 0, fi - 1)
    t = c // n
    i0, k0 = c - t * n, t // p
    j0 = t - k0 * p
    i = (i0, np.where(i0 + 1 == n, 0, i0 + 1))
    j = (j0, np.minimum(j0 + 1, p - 1))
    k = (k0, np.minimum(k0 + 1, q - 1))
    fa, fb, fg = fr & 255, (fr >> 8) & 255, (fr >> 16) & 255
    wa, wb, wg = (256 - fa, fa), (256 - fb, fb), (256 - fg, fg)
    bins, weights = [], []
    for tt in range(8):
        a, b, g = tt & 1, (tt >> 1) & 1, (tt >> 2) & 1
        f = np.clip(1 + i[a] + n * j[b] + n * p * k[g], 0, num_bins - 1)
        bins.append(np.where(centre, 0, f))
        weights.append(np.where(centre, (1 << 24) if tt == 0 else 0, wa[a] * wb[b] * wg[g]))
    return np.stack(bins, axis=-1), np.stack(weights, axis=-1)


def heaviest_corner(filt_index, filt_frac, kernel):
    """the bin of the corner with the largest weight per axis (ties at f8 = 128 go to the upper corner); 0 for a centre slot"""
    n, p, q = (int(v) for v in kernel)
    fi = np.asarray(filt_index).astype(np.int64)
    fr = np.asarray(filt_frac).astype(np.int64)
    c = np.maximum(fi - 1, 0)
    t = c // n
    i0, k0 = c - t * n, t // p
    j0 = t - k0 * p
    i = np.where((fr & 255) >= 128, np.where(i0 + 1 == n, 0, i0 + 1), i0)
    j = np.where(((fr >> 8) & 255) >= 128, np.minimum(j0 + 1, p - 1), j0)
    k = np.where(((fr >> 16) & 255) >= 128, np.minimum(k0 + 1, q - 1), k0)
    return np.where(fi <= 0, 0, 1 + i + n * j + n * p * k).astype(np.int32)


def _slots(cnt_b, K):
    return range(min(K, int(cnt_b.max()) if cnt_b.size else 0))


def fuzzy_conv_reference(x, w, idx, cnt, filt_index, filt_frac, kernel):
    """-> (out64, mag64, terms), each [B, M, C r]; terms = cnt.  Counts above K: the first K slots, divided by the count
    (the rule of tests/_conv_ref.py)"""
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
                bins, wts = corners(filt_index[b, sel, k], filt_frac[b, sel, k], kernel, F)
                weff = np.zeros((sel.size, C, r), np.float64)
                wmag = np.zeros((sel.size, C, r), np.float64)
                for t in range(8):
                    coef = (wts[:, t].astype(np.float64) * 2.0 ** -24)[:, None, None]
                    weff += coef * w64[bins[:, t]]
                    wmag += coef * np.abs(w64[bins[:, t]])
                xs = xb[idx[b, sel, k]][:, :, None]
                out[b, sel] += (xs * weff).reshape(sel.size, C * r)
                mag[b, sel] += (np.abs(xs) * wmag).reshape(sel.size, C * r)
        inv = 1.0 / np.maximum(cnt, 1).astype(np.float64)
        out *= inv[:, :, None]
        mag *= inv[:, :, None]
    terms = np.broadcast_to(np.asarray(cnt, np.int64)[:, :, None], out.shape)
    return out, mag, terms


class FuzzyGrad:
    """grad_input [B, N, C] with gi_mag and deg [B, N] (in-edges of the source); grad_filter [F, C, r] with gf_mag and
    gf_terms [F] (the (edge, corner) pairs of non-zero coefficient that name the bin)"""

    def __init__(self, B, N, F, C, r):
        self.gi, self.gi_mag = np.zeros((B, N, C), np.float64), np.zeros((B, N, C), np.float64)
        self.gf, self.gf_mag = np.zeros((F, C, r), np.float64), np.zeros((F, C, r), np.float64)
        self.deg = np.zeros((B, N), np.int64)
        self.gf_terms = np.zeros((F,), np.int64)


def fuzzy_conv_grad_reference(x, w, go, idx, cnt, filt_index, filt_frac, kernel):
    x, w, go = np.asarray(x), np.asarray(w), np.asarray(go)
    B, M, K = idx.shape
    N = x.shape[1]
    F, C, r = w.shape
    g = FuzzyGrad(B, N, F, C, r)
    w64 = w.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            xb = x[b].astype(np.float64)
            gb = go[b].astype(np.float64).reshape(M, C, r) * (1.0 / np.maximum(cnt[b], 1).astype(np.float64))[:, None, None]
            for k in _slots(cnt[b], K):
                sel = np.nonzero(cnt[b] > k)[0]
                nsrc = idx[b, sel, k]
                bins, wts = corners(filt_index[b, sel, k], filt_frac[b, sel, k], kernel, F)
                tf = gb[sel] * xb[nsrc][:, :, None]                      # [edges, C, r]
                weff = np.zeros((sel.size, C, r), np.float64)
                wmag = np.zeros((sel.size, C, r), np.float64)
                for t in range(8):
                    coef = (wts[:, t].astype(np.float64) * 2.0 ** -24)[:, None, None]
                    weff += coef * w64[bins[:, t]]
                    wmag += coef * np.abs(w64[bins[:, t]])
                    np.add.at(g.gf, bins[:, t], coef * tf)
                    np.add.at(g.gf_mag, bins[:, t], coef * np.abs(tf))
                    np.add.at(g.gf_terms, bins[:, t], (wts[:, t] != 0).astype(np.int64))
                np.add.at(g.gi[b], nsrc, (gb[sel] * weff).sum(axis=2))
                np.add.at(g.gi_mag[b], nsrc, (np.abs(gb[sel]) * wmag).sum(axis=2))
                np.add.at(g.deg[b], nsrc, 1)
    return g
