"""Inputs and bounds of the cross-entropy with class weights, label smoothing and an ignore label (csrc/xent.hip; the float64
statement is sph3d_gcn_amd/harness/xent.py: xent_reference).  numpy only.

INPUTS.  tests/_head_ref.py's xent_inputs (six kinds of logit rows; four blocks: no inner point, all inner, three inner points, a
mask drawn from 0, 1, 2.5, -1 and NaN) with, on top:
  * weights: classes alternate between a draw from {0, 0.25, 1, 3.5} and a uniform draw from (0, 4); class ZERO_CLASS = 0 has weight
    0 and class 1 % C a weight > 0;
  * block 2: EVERY row is labelled ZERO_CLASS, so with weights D = 0 under "weight" whether a mask is given or not;
  * about 5 % of the labels of blocks 1 and 3 are the ignore label: ignore_in(C) = C - 1, a class, or IGNORE_OUT = 255, outside;
  * row 0 of blocks 1 and 3 is never ignored and, in the mask, inner.
CONDITION (check_condition): every block other than the two designated empty ones — block 0 under a mask (no counted row) and block 2
(counted rows of zero weight only) — keeps at least one counted row after ignoring.

BOUNDS, first order in u = 2^-24, from the kernel's operation order (xent.hip: xent_kernel); C the number of classes.
  se      = the sum in ascending c of expf(x_c - m).  x_c - m is one rounding, an error of u |x_c - m| in the exponent; expf is good to
            one ulp = 2 u: term c is off by (|x_c - m| + 2) u relative.  Weighted by p_c = e_c / se: sum_c p_c |x_c - m| <= the entropy
            of p <= ln C (x_c - m = ln p_c + ln se and se >= 1).  The C - 1 additions of positive terms: (C - 1) u.
            se: (C + 1 + ln C) u relative.
  A       = (1 - eps) w_y + (eps / C) W.  1 - eps: 1 u; the product: 1 u; eps / C: 1 u; W = fp32(float64 sum of w): 1 u; the
            product: 1 u; the sum of two terms >= 0: 1 u.  A: 4 u.  inv = 1 / D with D one rounding of an exact value: 2 u.
  r       = (A inv) / se: 4 + 2 + 1 + 1 + (C + 1 + ln C) = (C + 9 + ln C) u.
  gradient element  expf(x_c - m) r - t_c inv.  First term: (|x_c - m| + 2) + (C + 9 + ln C) + 1 (product); t_c = [c = y] (1 - eps) w_y
            + (eps / C) w_c: 3 u, t_c inv: 3 + 2 + 1 = 6 u; the subtraction: 1 u of both.
                |error| <= u ((C + 13 + ln C + |x_c| + |m|) A p_c + 7 t_c) / D <= K_GRAD(C) u (A p_c (1 + |x_c| + |m|) + t_c) / D
            with K_GRAD(C) = C + 24 >= C + 13 + ln 4096 + 2 (the 2 for second-order terms), plus the float32 floor 2^-126 (a result
            below the smallest normal number, rounded to a subnormal or flushed: tests/_head_ref.py: F32_FLOOR).
  row loss  lse = m + logf(se): the error of se moves log se by (C + 1 + ln C) u, logf by 2 u |log se|, the addition by u (|m| +
            |log se|).  A term w_c (lse - x_c): the subtraction and the product, u (|m| + |log se| + |x_c|) each.  In all
            w_c u ((C + 1 + ln C) + 3 |m| + 5 |log se| + 2 |x_c|) <= (C + 10) u w_c (1 + |m| + |log se| + |x_c|).
            eps > 0: the C - 1 additions of the second sum, (C - 1) u; 1 - eps and eps / C and their products, 2 u each; the sum, 1 u.
                |error| <= K_ROW(C) u (A (|m| + |log se| + 1) + sum_c t_c |x_c|),   K_ROW(C) = 2 C + 16 >= (C + 10) + (C - 1) + 3 + 4
  loss part a thread adds its rows of the slice in order (trips - 1 additions), the workgroup's tree adds 6 + 15 levels, and the
            product with inv costs 2 + 1: (K_ROW(C) + trips + 26) u x the sum of the slice's row magnitudes / D (26 is
            tests/_head_ref.py's K_XENT_TREE, which counts the same tree).
The constants are these sums, not fitted to any output; the measured maxima are in DESIGN.md 2.
"""
import numpy as np

import _head_ref as H

U = H.U
ZERO_CLASS = 0
IGNORE_OUT = 255
EPS = float(np.float32(0.1))          # the smoothing the tests use: the float32 value, which the C ABI takes


def ignore_in(C):
    return C - 1


def k_grad(C):
    return C + 24


def k_row(C):
    return 2 * C + 16


def weights(C):
    rng = np.random.RandomState(77 + C)
    w = np.where(np.arange(C) % 2 == 0, rng.choice([0.0, 0.25, 1.0, 3.5], C), rng.uniform(0.01, 4.0, C)).astype(np.float32)
    w[ZERO_CLASS] = 0.0
    w[1 % C] = 3.5 if C <= 2 else 0.25
    return w


def inputs(N, C, ignore=None):
    """-> logits [4,N,C] float32, label [4,N] int64, inner [4,N] float32 (see the module text)"""
    x, label, inner = H.xent_inputs(4, N, C)
    label, inner = label.copy(), inner.copy()
    label[2] = ZERO_CLASS
    inner[3, 0] = 1.0
    if ignore is not None:
        rng = np.random.RandomState(5 * N + C)
        for b in (1, 3):
            label[b, rng.rand(N) < 0.05] = ignore
            if label[b, 0] == ignore:
                label[b, 0] = (ignore + 1) % C if 0 <= ignore < C else 1 % C
    return x, label, inner


def check_condition(label, inner, ignore):
    """every block but block 0 under a mask keeps a counted row (block 2's are of zero weight: the other designated empty block)"""
    counted = np.ones(label.shape, bool) if ignore is None else label != ignore
    if inner is not None:
        counted &= inner > 0
    n = counted.sum(1)
    return bool((n[1:] > 0).all() and (n[0] > 0 or inner is not None) and (label[2] == ZERO_CLASS).all())


def allowed(ref, C):
    """-> (loss part, gradient element) bounds in units of u x the element's magnitude"""
    return k_row(C) + ref["form"]["trips"] + H.K_XENT_TREE, k_grad(C)


def check(loss_part, dlogits, ref):
    """-> (worst loss part, worst gradient element) in units of u x magnitude (inf where NaN stands on one side only, or where an
    element of magnitude 0 is not exactly 0)"""
    return (H.xent_units(loss_part, ref["loss_part"], ref["part_mag"]),
            H.xent_units(dlogits, ref["dlogits"], ref["grad_mag"], H.F32_FLOOR))


# the shapes of tests/test_gpu_xent_ex.py
EQUAL_N, EQUAL_C = (1, 5, 1000, 1024, 1025, 4097, 16384), (2, 13, 21)
BOUND_N, BOUND_C = EQUAL_N + (16385, 40000), (2, 13, 50)
# on top of the issue's: the widest rows that are staged in LDS and the narrowest that are not (xent.hip: xent_stride), and a slice
# of two trips (more than 256 parts of 1024 rows: chunk 1029)
EXTRA_SHAPES = ((1025, 35), (1025, 36), (263169, 2))


def option_sets(C):
    """(name, dict of xent options) the bound tests run: each option alone at both normalisations where it matters, and all together"""
    w = weights(C)
    return [
        ("weights-count", dict(class_weight=w)),
        ("weights-weight", dict(class_weight=w, normalize="weight")),
        ("smoothing", dict(label_smoothing=EPS)),
        ("ignore-in", dict(ignore=ignore_in(C))),
        ("ignore-out", dict(ignore=IGNORE_OUT)),
        ("all-count", dict(class_weight=w, label_smoothing=EPS, ignore=ignore_in(C))),
        ("all-weight", dict(class_weight=w, label_smoothing=EPS, ignore=IGNORE_OUT, normalize="weight")),
    ]


# ---- D on the device: cases where the kernel's own D_b can be read off dlogits bit for bit ---------------------------------------------
# One block, C = 4, all logits 0, eps = 0, "weight": expf(0) = 1 and se = 4 are exact, so every gradient element is a short chain of
# correctly rounded float32 operations on inv = 1 / D_b (d_exact_gradient), and a D_b that is off by one ulp moves inv.  Each case
# names (weights, histogram) whose stated D — the float64 sum in ascending c, rounded once — differs from the sum in DESCENDING c
# (case "order": 1 + 2^-24 is a float32 tie, each 3 x 2^-55 alone is lost to the float64 sum, the two together are not) or from the
# sum formed in float32 (case "float32": found by a search over random weights for a D whose last bit also moves 1 / D).  tests/test_xent.py holds both properties on the CPU.
D_CASES = {
    "order": (np.array([1.0, 2.0 ** -24, 2.0 ** -55, 2.0 ** -55], np.float32), (1, 1, 3, 3)),
    "float32": (np.array([1.0, float.fromhex("0x1.192ae8p+1"), float.fromhex("0x1.9f335ep+0"), 1.0], np.float32), (1, 3, 3, 0)),
}


def d_case_inputs(name):
    """-> logits [1,N,4] zeros, label [1,N] int64 (class c h_c times, ascending), weights [4]"""
    w, h = D_CASES[name]
    label = np.repeat(np.arange(4), h)[None, :].astype(np.int64)
    return np.zeros((1, label.shape[1], 4), np.float32), label, w


def d_alternatives(w, h):
    """-> (D from the float64 sum in descending c, D from a float32 sum in ascending c): what a kernel with another order or another
    format would divide by"""
    f = np.float32
    down = 0.0
    for c in reversed(range(len(h))):
        down += float(h[c]) * float(w[c])
    single = f(0)
    for c in range(len(h)):
        single = f(single + f(f(h[c]) * w[c]))
    return f(down), single


def d_exact_gradient(label, w, D):
    """xent_kernel's gradient on all-zero logits with eps = 0, in float32 numpy, operation by operation:
    expf(0) * ((w_y * inv) / 4) - [c = y] w_y * inv with inv = 1 / D"""
    f = np.float32
    inv = f(1) / f(D)
    wy = w[label[0]].astype(f)
    r = (wy * inv).astype(f) / f(4)
    t = np.where(np.arange(4) == label[0][:, None], wy[:, None], f(0)).astype(f)
    return (r[:, None] - (t * inv).astype(f)).astype(f)[None]
