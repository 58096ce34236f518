"""The bounds the normal kernels (csrc/normals.hip) are held to against harness/normals.py, the seeded inputs of their tests,
and the one routine that applies the bounds.  Plain numpy.

What is compared for EQUALITY: the ten integer moments, the count and the skipped total.  Integer sums have no order.

What is bounded.  Kernel and statement form the float64 covariance c from identical integers with identical, separately
rounded operations, so they start from the same matrix.  They differ in the eigen-solve (cyclic Jacobi in the kernel,
np.linalg.eigh = LAPACK in the statement) and in the last rounding to fp32.  u = 2^-53, T = l0 + l1 + l2.

direction  Both solvers are backward stable: each returns the exact eigenvectors of c + E with ||E||_2 <= p u ||c||_2 for a
  modest p (a few units for a 3x3 matrix; p = 32 is taken below and is generous for either).  The eigenvector of l0 then moves
  by at most ||E||_2 / (l1 - l0) (Davis-Kahan, first order).  With the relative gap g = (l1 - l0) / T and ||c||_2 <= T for a
  positive semi-definite c that is p u / g per side: for g >= GAP = 2^-10 at most 2 * 32 * 2^-53 * 2^10 = 2^-37 for both.  Each
  side then rounds a component of magnitude <= 1 to fp32.  Two float64 values 2^-37 apart round to the same fp32 value or to
  neighbouring ones, and neighbouring fp32 values of magnitude <= 1 are at most 2^-24 apart: COMPONENT = 2^-24, with more than
  2^10 of room between the float64 term and the spacing.
  Rows with g < GAP are left out of the direction comparison (at most CAP of all rows, asserted); they must still be unit.

sign  is part of the answer.  The two sides decide it on float64 vectors that differ by the 2^-37 above, so a decision can
  differ only where its quantity is that close to zero: |n . (toward - q)| < SIGN ||toward - q||, or, without toward, where
  the two largest magnitudes differ by less than SIGN = 2^-20.  Such rows are left out as well (same cap, asserted).

variation  v = max(l0, 0) / T.  Each side's eigenvalues are those of c + E: |dl_i| <= p u ||c||_2 (Weyl).  Then
  |d(l0 / T)| <= |dl0| / T + l0 |dT| / T^2 <= p u s + (1/3) 3 p u s = 2 p u s per side, s = ||c||_2 / T (1 for a positive
  semi-definite c; the check takes max(1, |l|max / T) from the statement's own eigenvalues, so a matrix that rounding made
  indefinite is covered).  Both sides: 4 p u s = 2^-46 s.  The kernel ends its sweeps when the off-diagonal sum is below
  2^-70 of the diagonal's: a further 2^-69 s.  The float64 division rounds by u v, and each side rounds v to fp32: together
  2^-24 v_ref to first order.  So  |v - v_ref| <= 2^-24 v_ref + EPS s,  EPS = 2^-45 (twice the sum of the absolute terms).
"""
import numpy as np

COMPONENT = 2.0 ** -24
GAP = 2.0 ** -10
SIGN = 2.0 ** -20
UNIT = 2.0 ** -23
EPS = 2.0 ** -45
CAP = 0.01


def relative_gap(evals):
    """evals [..., 3] ascending -> g = (l1 - l0) / (l0 + l1 + l2), 0 where the sum is not positive"""
    e = np.asarray(evals, dtype=np.float64)
    t = (e[..., 0] + e[..., 1]) + e[..., 2]
    return np.where(t > 0, (e[..., 1] - e[..., 0]) / np.where(t > 0, t, 1.0), 0.0)


def sign_has_margin(ref, query, toward):
    """ref: the statement's namespace (normal64 [..., 3], dot); query [..., 3]; toward None or broadcastable to query"""
    n = np.asarray(ref.normal64)
    if toward is None:
        a = np.sort(np.abs(n), axis=-1)
        return (a[..., 2] - a[..., 1]) >= SIGN
    t = np.asarray(toward, dtype=np.float32).astype(np.float64) - np.asarray(query, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(ref.dot) >= SIGN * np.sqrt((t * t).sum(axis=-1))


def variation_bound(ref):
    e = np.asarray(ref.evals, dtype=np.float64)
    t = (e[..., 0] + e[..., 1]) + e[..., 2]
    s = np.where(t > 0, np.maximum(1.0, np.abs(e).max(axis=-1) / np.where(t > 0, t, 1.0)), 1.0)
    return 2.0 ** -24 * np.asarray(ref.variation, dtype=np.float64) + EPS * s


def check_rows(normals, variation, ref, query, toward, what=""):
    """normals [..., 3] fp32 and variation [...] fp32 (or None) of the kernel against the statement's namespace `ref`:
      * rows the statement sets to zero are exactly zero (variation too);
      * every other row is finite and of unit length within UNIT;
      * rows with g >= GAP and a sign decision with margin are within COMPONENT per component, sign included;
      * variation is within variation_bound on every row;
      * at most CAP of all rows is left out by the gap condition, and at most CAP by the sign condition.
    toward: None, or an array that broadcasts against query.  -> dict of the measured maxima"""
    got = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    zero = np.asarray(ref.zero).reshape(-1)
    R = zero.size
    want = np.asarray(ref.normals, dtype=np.float32).reshape(-1, 3)
    q = np.asarray(query, dtype=np.float32).reshape(-1, 3)
    tw = None if toward is None else np.broadcast_to(np.asarray(toward, dtype=np.float32), np.asarray(query).shape).reshape(-1, 3)
    flat = type(ref)(normal64=np.asarray(ref.normal64).reshape(-1, 3), dot=None if ref.dot is None else np.asarray(ref.dot).reshape(-1),
                     evals=np.asarray(ref.evals).reshape(-1, 3), variation=np.asarray(ref.variation).reshape(-1))
    assert np.isfinite(got).all(), what
    assert not got[zero].any(), "%s: rows the statement zeroes are not zero" % what
    length = np.sqrt((got.astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(length[~zero] - 1.0) <= UNIT).all(), "%s: a live row is not of unit length" % what
    g = relative_gap(flat.evals)
    margin = sign_has_margin(flat, q, tw)
    gap_out = ~zero & (g < GAP)
    sign_out = ~zero & ~gap_out & ~margin
    left_gap, left_sign = gap_out.sum() / max(R, 1), sign_out.sum() / max(R, 1)
    compare = ~zero & ~gap_out & ~sign_out
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = float(err[compare].max()) if compare.any() else 0.0
    stats = {"rows": R, "compared": int(compare.sum()), "left_gap": float(left_gap), "left_sign": float(left_sign),
             "component": worst / 2.0 ** -24, "variation": 0.0, "min_gap": float(g[~zero].min()) if (~zero).any() else None}
    if variation is not None:
        v = np.asarray(variation, dtype=np.float32).reshape(-1).astype(np.float64)
        assert np.isfinite(v).all() and not v[zero].any(), what
        over = np.abs(v - flat.variation.astype(np.float64)) / variation_bound(flat)
        stats["variation"] = float(over.max()) if R else 0.0
    print("%s: %s" % (what, stats))
    assert left_gap <= CAP, "%s: %.4f of the rows left out by the gap condition" % (what, left_gap)
    assert left_sign <= CAP, "%s: %.4f of the rows left out by the sign condition" % (what, left_sign)
    assert worst <= COMPONENT, "%s: component error %.3f of 2^-24" % (what, worst / 2.0 ** -24)
    assert stats["variation"] <= 1.0, "%s: variation error %.3f of its bound" % (what, stats["variation"])
    return stats


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def family(name, n, seed):
    """-> [n, 3] fp32.  "sphere": unit sphere, jitter sigma 0.01; "box": the surface of the unit cube, sigma 0.005; "volume":
    uniform in the unit cube"""
    rng = np.random.RandomState(seed)
    if name == "sphere":
        d = rng.randn(n, 3)
        p = d / np.linalg.norm(d, axis=1, keepdims=True) + 0.01 * rng.randn(n, 3)
    elif name == "box":
        p = rng.rand(n, 3) - 0.5
        axis, side = rng.randint(0, 3, n), rng.randint(0, 2, n) - 0.5
        p[np.arange(n), axis] = side
        p = p + 0.005 * rng.randn(n, 3)
    elif name == "volume":
        p = rng.rand(n, 3)
    else:
        raise ValueError(name)
    return p.astype(np.float32)


def plain_graph(database, query, radius, K):
    """strict radius, first K by index: nn_index [B, M, K] int32 (unused slots 0), nn_count [B, M] int32 — the graph of the
    searches' fixed radius mode, without its growth for a query that has no neighbour"""
    database, query = np.asarray(database, np.float32), np.asarray(query, np.float32)
    B, M = query.shape[0], query.shape[1]
    idx, cnt = np.zeros((B, M, K), np.int32), np.zeros((B, M), np.int32)
    r2 = np.float32(radius) * np.float32(radius)
    for b in range(B):
        with np.errstate(invalid="ignore", over="ignore"):
            d = query[b][:, None, :] - database[b][None, :, :]
            inside = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < r2
        for m in range(M):
            j = np.nonzero(inside[m])[0][:K]
            idx[b, m, :len(j)], cnt[b, m] = j, len(j)
    return idx, cnt
