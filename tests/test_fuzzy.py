"""The numpy statement of the fuzzy spherical kernel (sph3d_gcn_amd/harness/fuzzy.py), checked without a GPU: the restated
atan2f against the CPU oracle's hard bins, the format's identities, continuity across a sector boundary, and the two gradient
statements against central differences of the forward one."""
import numpy as np
import pytest

import oracle
from _fuzzy_ref import KERNELS, num_bins, planted_cloud, random_words
from _pool_ref import make_graph
from sph3d_gcn_amd.harness import fuzzy

RADIUS, K = 0.2, 32


@pytest.fixture(scope="module")
def cloud():
    xyz = planted_cloud(3)
    idx, cnt, dst = oracle.build_sphere_neighbor(xyz, xyz, RADIUS, None, K)
    live = np.arange(K)[None, None, :] < cnt[:, :, None]
    d = xyz[np.arange(2)[:, None, None], np.where(live, idx, 0)] - xyz[:, :, None, :]
    # what the clouds are planted for is there: zero deltas per axis, poles, coincident points
    others = live & (idx != np.arange(xyz.shape[1])[None, :, None])
    for axis in range(3):
        assert (others & (d[..., axis] == 0) & (dst > 0.01)).sum() >= 20
    assert (others & (d[..., 0] == 0) & (d[..., 1] == 0) & (d[..., 2] != 0)).sum() >= 8
    assert (others & (dst == 0)).sum() >= 8
    return xyz, idx, cnt, dst, live


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("radius", [RADIUS, 0.6 * RADIUS])          # the smaller one: neighbours with dist > radius
def test_restated_atan2_gives_the_oracles_hard_bins(cloud, kernel, radius):
    xyz, idx, cnt, dst, live = cloud
    if radius < RADIUS:
        assert (live & (dst > radius)).sum() >= 100
    alpha, beta, gamma, centre, live2 = fuzzy.slot_coordinates(xyz, xyz, idx, cnt, dst, radius, kernel)
    assert np.array_equal(live, live2)
    hard = np.where(live, fuzzy.hard_bins(alpha, beta, gamma, centre, kernel), 0)
    assert np.array_equal(hard, oracle.spherical_kernel(xyz, xyz, idx, cnt, dst, radius, kernel))


def test_restated_atan2_special_values():
    y = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 1e-30, 3.0, -2.5, 1.0], np.float32)
    x = np.array([1.0, 1.0, -1.0, -1.0, 0.0, -0.0, -1e30, 3.0, -2.5, 1e-20], np.float32)
    got = fuzzy.atan2f(y, x)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    rng = np.random.RandomState(0)
    y, x = rng.randn(200000).astype(np.float32), rng.randn(200000).astype(np.float32)
    got = fuzzy.atan2f(y, x)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)      # (the header's claim: correctly rounded)
    assert (got.view(np.int32) != want.view(np.int32)).sum() == 0


def _seam(alpha, kernel):
    """the slots on the seam of the periodic axis: theta = 2 pi gives alpha == n, theta = -pi rounds to a float below -M_PI and
    gives a tiny negative alpha; both name the direction between sector n - 1 and sector 0"""
    return (alpha == np.float32(kernel[0])) | (alpha < 0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_heaviest_corner_is_the_hard_bin(cloud, kernel):
    """per axis the heavier corner (ties at f8 = 128 to the upper one) is the hard bin, except on the seam of the azimuth, where
    the hard rule says sector 0 (alpha < 0) or n - 1 (alpha == n) and the fuzzy lower / upper corner the other one of the two:
    counted and shown.  On the cloud's slots and on 2 M random and boundary-planted coordinates."""
    n, p, q = kernel
    xyz, idx, cnt, dst, live = cloud
    alpha, beta, gamma, centre, _ = fuzzy.slot_coordinates(xyz, xyz, idx, cnt, dst, 0.6 * RADIUS, kernel)
    rng = np.random.RandomState(5)
    m = 2000000
    ra, rb, rg = (rng.rand(m) * n).astype(np.float32), (rng.rand(m) * p).astype(np.float32), (rng.rand(m) * q * 1.2).astype(np.float32)
    plant = np.arange(m) % 4 == 0                       # on and one ulp around every half-integer: bin boundaries and centres
    for arr in (ra, rb, rg):
        snapped = (np.round(arr * 2) / 2).astype(np.float32)
        nudged = np.nextafter(snapped, np.where(np.arange(m) % 3 == 0, np.float32(-1), np.float32(1000)).astype(np.float32))
        arr[plant] = np.where(np.arange(m) % 8 == 0, snapped, nudged)[plant]
    np.minimum(ra, np.float32(n), out=ra)               # (theta <= 2 pi and phi <= pi: alpha <= n, beta <= p)
    np.minimum(rb, np.float32(p), out=rb)
    ra[:4] = [n, 0.0, -1.2e-7, np.nextafter(np.float32(0.5), np.float32(0))]
    sets = [(alpha[live], beta[live], gamma[live], centre[live]), (ra, rb, rg, np.zeros(m, bool))]
    for a, b, g, c in sets:
        index, frac = fuzzy.fuzzy_words(a, b, g, c, kernel)
        assert ((frac >= 0) & (frac < (1 << 24))).all() and ((index >= 0) & (index < num_bins(kernel))).all()
        hard = fuzzy.hard_bins(a, b, g, c, kernel)
        heavy = fuzzy.heaviest_corner(index, frac, kernel)
        diff = heavy != hard
        seam = _seam(a, kernel) & ~c
        print("kernel %s: %d slots, %d on the seam (alpha == n: %d, alpha < 0: %d), %d differ"
              % (kernel, a.size, int(seam.sum()), int((a == n).sum()), int((a < 0).sum()), int(diff.sum())))
        assert not (diff & ~seam).any()
        # on the seam the two name adjacent sectors across it, same band and shell
        hs, fs = (hard[diff] - 1) % n, (heavy[diff] - 1) % n
        assert np.isin(hs, (0, n - 1)).all() and np.isin(fs, (0, n - 1)).all()
        assert np.array_equal((hard[diff] - 1) // n, (heavy[diff] - 1) // n)
    # without the clamp the fraction byte overflows just under alpha = 0.5
    a = np.nextafter(np.float32(0.5), np.float32(0)) - np.float32(0.5)
    assert np.floor((a - np.floor(a)).astype(np.float32) * np.float32(256)) == 256


@pytest.mark.parametrize("kernel", KERNELS)
def test_coefficients_are_exact_and_sum_to_one(kernel):
    rng = np.random.RandomState(9)
    cnt = np.full((4, 50), 40, np.int32)
    index, frac = random_words(rng, cnt, 40, kernel)
    bins, wts = fuzzy.corners(index, frac, kernel, num_bins(kernel))
    assert (wts >= 0).all() and (wts.sum(axis=-1) == 1 << 24).all()
    assert ((bins >= 0) & (bins < num_bins(kernel))).all()
    coef = wts.astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(coef.astype(np.float64), wts * 2.0 ** -24)              # exact in fp32
    for order in (np.arange(8), np.arange(8)[::-1], rng.permutation(8)):           # and their fp32 sum is 1 in any order
        s = np.zeros(coef.shape[:-1], np.float32)
        for t in order:
            s = (s + coef[..., t]).astype(np.float32)
        assert (s == 1).all()
    centre = index == 0
    assert centre.any() and (bins[centre] == 0).all() and (wts[centre][:, 0] == 1 << 24).all()


def _one_row(kernel, neighbours, radius):
    """a cloud of one query (the origin, point 0) and its neighbours -> the graph arrays of the query's row"""
    xyz = np.concatenate([np.zeros((1, 3), np.float32), np.asarray(neighbours, np.float32)])[None]
    N = xyz.shape[1]
    idx = np.arange(N, dtype=np.int32)[None, None, :]
    cnt = np.array([[N]], np.int32)
    d = xyz[0].astype(np.float32)
    dst = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float32)).astype(np.float32)[None, None, :]
    return xyz, xyz[:, :1], idx, cnt, dst


@pytest.mark.parametrize("kernel", KERNELS)
def test_continuity_across_a_sector_boundary(kernel):
    """a neighbour moved by +-1e-7 across a sector boundary: the fuzzy float64 output changes by at most 2/256 of mag, the hard
    op exchanges a whole filter row"""
    n, p, q = kernel
    F, C, r = num_bins(kernel), 6, 2
    rng = np.random.RandomState(11)
    w = rng.randn(F, C, r).astype(np.float32)
    others = (rng.rand(5, 3).astype(np.float32) - 0.5) * 0.15
    radius = 0.1
    for s in range(n):                                   # the boundary between sector s - 1 and s: theta + pi = 2 pi s / n
        ang = 2 * np.pi * s / n - np.pi
        if s == 0:
            continue                                     # (the seam: see test_heaviest_corner_is_the_hard_bin)
        outs, hards, mags = [], [], []
        for side in (-1.0, 1.0):
            t = np.array([np.cos(ang), np.sin(ang)]) * 0.05 + side * 1e-7 * np.array([-np.sin(ang), np.cos(ang)])
            nb = np.concatenate([np.array([[t[0], t[1], 0.013]], np.float32), others])
            xyz, query, idx, cnt, dst = _one_row(kernel, nb, radius)
            x = np.random.RandomState(100 + s).randn(1, xyz.shape[1], C).astype(np.float32)
            fi, fr = fuzzy.fuzzy_kernel_reference(xyz, query, idx, cnt, dst, radius, kernel)
            out, mag, _ = fuzzy.fuzzy_conv_reference(x, w, idx, cnt, fi, fr, kernel)
            a, b, g, c, live = fuzzy.slot_coordinates(xyz, query, idx, cnt, dst, radius, kernel)
            hard = fuzzy.hard_bins(a, b, g, c, kernel)
            hout = (x[0].astype(np.float64)[:, :, None] * w.astype(np.float64)[hard[0, 0]]).sum(axis=0).reshape(1, 1, C * r) / cnt[0, 0]
            outs.append(out), hards.append((hard, hout)), mags.append(mag)
        mag = np.minimum(mags[0], mags[1])
        assert (np.abs(outs[1] - outs[0]) <= 2.0 / 256 * mag).all(), (kernel, s)
        (h0, o0), (h1, o1) = hards
        assert h0[0, 0, 1] != h1[0, 0, 1] and np.array_equal(h0[0, 0, 2:], h1[0, 0, 2:]) and h0[0, 0, 0] == 0
        row = x[0, 1].astype(np.float64)[:, None] * (w[h1[0, 0, 1]].astype(np.float64) - w[h0[0, 0, 1]]) / cnt[0, 0]
        np.testing.assert_allclose(o1 - o0, row.reshape(1, 1, C * r), rtol=0, atol=1e-12)
        assert (np.abs(o1 - o0) > 2.0 / 256 * mag).any()


@pytest.mark.parametrize("kernel,r", [(KERNELS[0], 2), (KERNELS[1], 1), (KERNELS[2], 3)])
def test_gradient_statements_match_central_differences(kernel, r):
    rng = np.random.RandomState(13)
    B, N, M, Kk, C = 2, 20, 11, 6, 5
    F = num_bins(kernel)
    idx, cnt = make_graph(rng, B, N, M, Kk)
    fi, fr = random_words(rng, cnt, Kk, kernel)
    x, w = rng.randn(B, N, C), rng.randn(F, C, r)
    go = rng.randn(B, M, C * r)
    g = fuzzy.fuzzy_conv_grad_reference(x, w, go, idx, cnt, fi, fr, kernel)

    def loss(xx, ww):
        return float((fuzzy.fuzzy_conv_reference(xx, ww, idx, cnt, fi, fr, kernel)[0] * go).sum())

    h = 1e-3                                             # the loss is linear in x and in w: central differences are exact
    for _ in range(12):
        i = tuple(rng.randint(0, s) for s in x.shape)
        e = np.zeros_like(x)
        e[i] = h
        assert abs((loss(x + e, w) - loss(x - e, w)) / (2 * h) - g.gi[i]) <= 1e-9 * max(1.0, g.gi_mag[i])
        j = tuple(rng.randint(0, s) for s in w.shape)
        e = np.zeros_like(w)
        e[j] = h
        assert abs((loss(x, w + e) - loss(x, w - e)) / (2 * h) - g.gf[j]) <= 1e-9 * max(1.0, g.gf_mag[j])
    assert (g.gi_mag >= np.abs(g.gi) - 1e-12).all() and (g.gf_mag >= np.abs(g.gf) - 1e-12).all()
    assert g.deg.sum() == np.minimum(cnt, Kk).sum()
