"""What the fuzzy-kernel tests share: the planted clouds, random slot words, and the per-element bounds the kernels of
csrc/fuzzy.hip are held to against the float64 statement (sph3d_gcn_amd/harness/fuzzy.py).

The bounds are derived, not measured, in the manner of tests/_conv_ref.py: u = 2^-24, every fp32 rounding is at most u times a
partial sum, every partial sum at most mag (the same sum over absolute values).  A corner's coefficient is an integer of at
most 2^24 times 2^-24: exact, so it contributes no rounding of its own.

forward  (cnt + 12) u mag
  8     the blend `w = fmaf(coef[t], tab[..], w)` from w = 0 over the corners of non-zero coefficient: at most eight roundings,
        each at most u times the edge's sum of coef |W|; times |x| and summed over the edges that is 8 u mag in all, not per edge
  cnt   `acc = fmaf(x, w, acc)`, once per edge
  1 + 1 `inv = 1.0f / (float)cnt` and `acc * inv`;   2: slack for the second-order terms
grad_input  (deg + r + 12) u mag     deg: in-edges of the source
  8     the blend, as above;   r: `t = fmaf(go, w, t)` over rho, each at most u times the edge's term sum
  1     `inv`;   deg: `acc = fmaf(t, inv, acc)`, once per in-edge;   3: slack
grad_filter  (2 terms + 6) u mag     terms: the (edge, corner) pairs of non-zero coefficient that name the bin
  2 + 1  `g = go * inv` (inv and the product) and `gx = g * x`: three roundings of every term
  terms  `*cell = fmaf(coef, gx, *cell)`, once per pair
  terms  the group sums of a workgroup and fuzzy_gf_reduce's sum over the workgroups' tables: an add with a zero operand is
         exact, and at most `terms` tables (or groups) hold anything for the element
  3      slack
None of them exceeds (8 terms + 16) u mag (forward: terms = cnt; grad_input: terms = deg, for r <= 11) — asserted below."""
import numpy as np

from _conv_ref import assert_conv  # noqa: F401  (the per-element check itself is the hard op's)
from _pool_ref import U  # noqa: F401

from sph3d_gcn_amd.harness import fuzzy

KERNELS = ([8, 2, 2], [4, 2, 3], [8, 4, 1])


def num_bins(kernel):
    return kernel[0] * kernel[1] * kernel[2] + 1


def fwd_terms(cnt_terms):
    t = np.asarray(cnt_terms, np.int64) + 12
    assert (t <= 8 * np.asarray(cnt_terms, np.int64) + 16).all()
    return t


def gi_terms(deg, r):
    deg = np.asarray(deg, np.int64)
    t = deg + r + 12
    assert (t[deg > 0] <= 8 * deg[deg > 0] + 16).all()
    return t[:, :, None]


def gf_terms(terms):
    terms = np.asarray(terms, np.int64)
    t = 2 * terms + 6
    assert (t <= 8 * terms + 16).all()
    return t[:, None, None]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def planted_cloud(seed, B=2, N=256):
    """[B, N, 3] fp32 in a 0.5 box: 96 points on a lattice of pitch 1/8 (neighbours with dx, dy or dz exactly 0, pairs on one
    vertical line = the poles, and coincident points: 96 draws from 125 cells), eight forced copies, eight forced poles"""
    rng = np.random.RandomState(seed)
    xyz = (rng.rand(B, N, 3) * 0.5).astype(np.float32)
    xyz[:, :96] = rng.randint(0, 5, size=(B, 96, 3)).astype(np.float32) / np.float32(8.0)
    xyz[:, 96:104] = xyz[:, 120:128]                    # coincident with a random point
    xyz[:, 104:112, :2] = xyz[:, 128:136, :2]           # straight above / below a random point
    return xyz


def random_words(rng, cnt, K, kernel):
    """slot words [B, M, K] from random bin coordinates (a tenth planted on bin boundaries and centres, a few centre slots, a few
    beyond the last shell); slots past the count hold garbage a consumer must not read"""
    n, p, q = kernel
    shape = cnt.shape + (K,)
    alpha = (rng.rand(*shape) * n).astype(np.float32)
    beta = (rng.rand(*shape) * p).astype(np.float32)
    gamma = (rng.rand(*shape) * q * 1.1).astype(np.float32)
    snap = rng.rand(*shape) < 0.1
    alpha = np.where(snap, np.round(alpha * 2) / 2, alpha).astype(np.float32)
    beta = np.where(snap, np.round(beta * 2) / 2, beta).astype(np.float32)
    gamma = np.where(snap, np.round(gamma * 2) / 2, gamma).astype(np.float32)
    centre = rng.rand(*shape) < 0.05
    index, frac = fuzzy.fuzzy_words(alpha, beta, gamma, centre, kernel)
    dead = np.arange(K)[None, None, :] >= cnt[:, :, None]
    index[dead] = num_bins(kernel) + 7
    frac[dead] = -1
    return index, frac
