"""The augmentation stage in float64 with a bound on what csrc/augment.hip's fp32 evaluation may differ by, per element.

The bound is a running error analysis of the kernel's own operation order (the library is built without contraction, so every
fp32 operation rounds once): a number is a pair (v, e) — its float64 value and a bound on |fp32 result - v|.  An operation
propagates the operands' bounds to first order with the cross term kept, and every rounding step on the element's path adds
2^-24 times the magnitude of the result it rounds (the computed one: |v| + e):

    a + b    e = ea + eb                        a * b    e = |a| eb + |b| ea + ea eb
    a / b    e = (ea + |a / b| eb) / (|b| - eb)          sqrt(a)  e = ea / (2 sqrt(a - ea))

so the bound of an element is the rounding steps on its path times 2^-24 times the magnitudes of its terms, carried through the
later transforms.  Constants the kernel takes in fp32 (0.9, 0.2, 0.1, 0.01, the colour range, 1 / g, mag / FIELD_UNIT) enter
with their representation error.  Nothing here was fitted to a device result.

ELASTIC.  The blurred lattice is exact int32 on the device, and the displacement is a CONTINUOUS piecewise-trilinear function V
of the lattice coordinate t = x / g, so a kernel cell that differs from the float64 cell (a point within rounding of a node plane)
does not matter: |V(t') - V(t)| <= L sum_a |t'_a - t_a| with L = (2 / 3) FIELD_UNIT — along one axis the blurred field changes
by at most (1 + 1 + 1 + 1 + 1 + 1) / 9 of the raw range 2^21 between neighbouring nodes, times 81 for the two other blurs.  The
position error per axis is t's bound plus one rounding (of t - floor(t), magnitude below 1).  The blend itself: 1 - f rounds once
per axis and the product of three weights twice, five steps on a weight of at most 1, so 5 * 2^-24 |F_k| on each of 8 corners
(|F_k| <= Fmax, the largest lattice magnitude over the cloud's node box grown by one cell, since the kernel's corners lie within
one cell of the statement's); the int -> float conversion, the product with the weight and the eight additions are ten steps on
sum_k w_k |F_k|.

CJITTER.  The normal noise is feed_normal_pair's: as tests/test_gpu_feed.py does for the xyz jitter, the element gets 1e-5 times
the magnitudes of its terms, |c| + sigma ZMAX, where ZMAX = sqrt(2 * 24 ln 2) is the largest |z| Box-Muller makes of a 24-bit u1.
"""
import numpy as np

from sph3d_gcn_amd.harness import augment, feed

U = 2.0 ** -24
ZMAX = float(np.sqrt(2 * 24 * np.log(2.0)))
LIPSCHITZ = (2.0 / 3.0) * augment.FIELD_UNIT
FEED_NORMAL_BOUND = 1e-5


class T:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy()


def _rnd(v, e):
    return T(v, e + U * (np.abs(v) + e))


def const(c):
    """a constant the kernel holds in fp32"""
    return T(float(c), abs(float(c) - float(np.float32(c))))


def add(a, b):
    return _rnd(a.v + b.v, a.e + b.e)


def sub(a, b):
    return _rnd(a.v - b.v, a.e + b.e)


def mul(a, b):
    return _rnd(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def div(a, b):
    den = np.abs(b.v) - b.e
    v = a.v / b.v
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(den > 0, (a.e + np.abs(v) * b.e) / np.where(den > 0, den, 1.0), np.inf)
    return _rnd(v, e)


def sqrt(a):
    v = np.sqrt(a.v)
    low = a.v - a.e
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(low > 0, a.e / (2 * np.sqrt(np.where(low > 0, low, 1.0))), np.where(a.e > 0, np.inf, 0.0))
    return _rnd(v, e)


def clip(a, lo, hi):
    """min / max select: 1-Lipschitz, no rounding; the fp32 limits' own representation error joins the bound"""
    return T(np.clip(a.v, lo.v, hi.v), np.maximum(a.e, np.maximum(lo.e, hi.e)))


def elastic(x, ck, which, g, mag, max_nodes):
    """x: T [n, 3] -> (T [n, 3] after pass `which`, skipped)"""
    cell = augment.cell_index(x.v, g)
    cmin, cmax = cell.min(axis=0), cell.max(axis=0)
    if not augment.box_ok(cmin, cmax, max_nodes):
        return x, True
    t = mul(x, T(1.0 / g, abs(1.0 / g - float(np.float32(1.0 / g)))))
    pos = (t.e + U).sum(axis=1)                                   # lattice units, summed over the axes
    F = augment.lattice(ck, which, cmin - 1, cmax + 1).astype(np.float64)
    fmax = np.abs(F).max(axis=(0, 1, 2))
    f = x.v / g - cell
    l = cell - cmin + 1
    val = np.zeros(x.v.shape)
    mag_sum = np.zeros(x.v.shape)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                Fk = F[l[:, 0] + dx, l[:, 1] + dy, l[:, 2] + dz]
                val += w[:, None] * Fk
                mag_sum += w[:, None] * np.abs(Fk)
    acc = T(val, LIPSCHITZ * pos[:, None] + U * (8 * 5 * fmax[None, :] + 10 * mag_sum))
    scale = float(mag) / augment.FIELD_UNIT
    return add(x, mul(acc, T(scale, abs(scale - float(np.float32(scale)))))), False


def evaluate(points, label, inner, seed, step, opts):
    """points [B, N, C] float32 -> value [B, N, C] float64, bound [B, N, C], label', inner', Report — the statement's result
    (checked against augment.apply_reference by tests/test_augment.py) and the fp32 bound of every element"""
    points = np.asarray(points, dtype=np.float32)
    B, N, C = points.shape
    want, lab, inn, report = augment.apply_reference(points, label, inner, seed, step, opts)
    V, E = points.astype(np.float64), np.zeros(points.shape)
    gates, h = report.gates, N // 2
    ro, no = opts.rgb_offset, opts.normal_offset
    lo, hi = const(opts.rgb_range[0]), const(opts.rgb_range[1])
    for b in range(0, B - 1, 2):
        if not gates[b] & augment.MIX:
            continue
        for c in (b, b + 1):
            mn, mx = V[c, :, 0:3].min(axis=0), V[c, :, 0:3].max(axis=0)
            mid = add(T(mn[0:2]), T(mx[0:2]))
            ctr = T(np.concatenate([mid.v * 0.5, mn[2:3]]), np.concatenate([mid.e * 0.5, [0.0]]))
            x = sub(T(V[c, :, 0:3]), ctr)
            V[c, :, 0:3], E[c, :, 0:3] = x.v, x.e
        for t in (V, E):
            t[b, h:], t[b + 1, h:] = t[b + 1, h:].copy(), t[b, h:].copy()
    for b in range(B):
        g, ck = int(gates[b]), feed.cloud_key(seed, step, b)
        for bit, a in ((augment.FLIPX, 0), (augment.FLIPY, 1)):
            if g & bit:
                V[b, :, a] = np.negative(V[b, :, a])
                if no is not None:
                    V[b, :, no + a] = np.negative(V[b, :, no + a])
        x = T(V[b, :, 0:3], E[b, :, 0:3])
        if g & augment.ASCALE:
            u = np.array([float(feed.uniform(feed._hi(feed.draw(ck, augment.SCALE, a)))) for a in range(3)])
            s = add(const(0.9), mul(const(0.2), T(u)))
            x = mul(x, s)
            if no is not None:
                n = div(T(V[b, :, no:no + 3], E[b, :, no:no + 3]), s)
                sq = mul(n, n)
                length = sqrt(add(add(T(sq.v[:, 0], sq.e[:, 0]), T(sq.v[:, 1], sq.e[:, 1])), T(sq.v[:, 2], sq.e[:, 2])))
                ok = length.v > 0
                unit = div(n, T(np.where(ok, length.v, 1.0)[:, None], np.where(ok, length.e, 0.0)[:, None]))
                V[b, :, no:no + 3] = np.where(ok[:, None], unit.v, n.v)
                E[b, :, no:no + 3] = np.where(ok[:, None], unit.e, n.e)
        if g & augment.ELASTIC:
            for which, (gg, mag) in enumerate(opts.elastic):
                x, _skipped = elastic(x, ck, which, gg, mag, opts.max_nodes)
        V[b, :, 0:3], E[b, :, 0:3] = x.v, x.e
        if not g & augment.COLOUR:
            continue
        c = T(V[b, :, ro:ro + 3], E[b, :, ro:ro + 3])
        rng = sub(hi, lo)
        if g & augment.AUTOCONTRAST:
            alpha = T(float(feed.uniform(feed._hi(feed.draw(ck, augment.CONTRAST, 0)))))
            mn, mx = c.v.min(axis=0), c.v.max(axis=0)              # (selections of fp32 inputs: exact)
            live = mx > mn
            sc = div(rng, sub(T(np.where(live, mx, 1.0)), T(np.where(live, mn, 0.0))))
            cp = add(lo, mul(sub(c, T(mn)), sc))
            mixed = add(mul(sub(T(1.0), alpha), c), mul(alpha, cp))
            c = T(np.where(live, mixed.v, c.v), np.where(live, mixed.e, c.e))
        if g & augment.CTRANSLATE:
            u = feed.uniform(feed._hi(feed.draw(ck, augment.CTRANS, np.arange(3))))
            c = clip(add(c, mul(T(u - 0.5), mul(const(0.1), rng))), lo, hi)
        if g & augment.CJITTER:
            sigma = mul(const(0.01), rng)
            moved = add(c, mul(sigma, T(augment.colour_noise(ck, N))))
            moved.e += FEED_NORMAL_BOUND * (np.abs(c.v) + sigma.v * ZMAX)
            c = clip(moved, lo, hi)
        if g & augment.CDROP:
            half = add(lo, hi)
            c = T(np.broadcast_to(half.v * 0.5, c.v.shape), half.e * 0.5)
        V[b, :, ro:ro + 3], E[b, :, ro:ro + 3] = c.v, c.e
    return V, E, lab, inn, report, want
