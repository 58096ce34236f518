"""The category-conditioned logits layer stated in float64 (plain numpy: no torch, no oracle), with the bounds its kernels are held
to and the operands the tests share.

  y[b*P + p, :] = a1[b*P + p, :] w[0:K1] + a2[b*P + p, :] w[K1:K1+K2] + w[K1 + K2 + cat[b], :] + bias
which is pointwise_conv3d(concat(a1, a2, tile(one_hot(cat)))) of models/SPH3D_shapenet_onehot.py:105-119: a category outside
[0, T) has a zero one-hot row and contributes nothing.  Every value comes with ``mag``, the same sum over the magnitudes of its
terms (tests/_errors.py).  The bound, as in tests/_pool_ref.py: an fp32 sum of n terms in any order rounds at most n times on the
way to an element, each rounding at most 2^-24 of a partial sum that is at most mag, and three roundings are allowed for
the adds that join partial sums:  |got - ref| <= (terms + 3) * 2^-24 * mag.
  forward      terms = K1 + K2 + 2   (the products, the category row, the bias)
  dT, dbias    terms = the number of rows summed (the rows of the category's clouds; all rows)
An element with no term is exactly 0."""
import types

import numpy as np

U = 2.0 ** -24


def cond_reference(a1, a2, w, bias, cat, P, dy=None):
    """a1 [R, K1], a2 [R, K2] or None, w [K1 + K2 + T, N], bias [N] or None, cat [B] integers, R = B * P; dy [R, N] or None.
    -> namespace of float64 arrays: y, y_mag [R, N]; with dy also dt, dt_mag [T, N] and dt_terms [T] (the gradient of the category
    rows), db, db_mag [N] (of the bias: all rows), dw, dw_mag [K1 + K2, N] (of the operand rows) and da, da_mag [R, K1 + K2]."""
    a = np.asarray(a1, np.float64) if a2 is None else np.concatenate([np.asarray(a1, np.float64), np.asarray(a2, np.float64)], 1)
    w = np.asarray(w, np.float64)
    cat = np.asarray(cat).reshape(-1).astype(np.int64)
    R, K = a.shape
    T, N = w.shape[0] - K, w.shape[1]
    B = cat.shape[0]
    assert R == B * P and T >= 1
    live = (cat >= 0) & (cat < T)
    row = np.zeros((B, N))
    row[live] = w[K + cat[live]]
    row = np.repeat(row, P, axis=0)
    b64 = np.zeros((N,)) if bias is None else np.asarray(bias, np.float64)
    out = types.SimpleNamespace()
    out.y = a @ w[:K] + row + b64
    out.y_mag = np.abs(a) @ np.abs(w[:K]) + np.abs(row) + np.abs(b64)
    if dy is not None:
        dy = np.asarray(dy, np.float64)
        per_cloud = dy.reshape(B, P, N).sum(1)
        per_cloud_mag = np.abs(dy).reshape(B, P, N).sum(1)
        out.dt, out.dt_mag, out.dt_terms = np.zeros((T, N)), np.zeros((T, N)), np.zeros((T,), np.int64)
        for b in range(B):
            if live[b]:
                out.dt[cat[b]] += per_cloud[b]
                out.dt_mag[cat[b]] += per_cloud_mag[b]
                out.dt_terms[cat[b]] += P
        out.db, out.db_mag = dy.sum(0), np.abs(dy).sum(0)
        out.dw, out.dw_mag = a.T @ dy, np.abs(a).T @ np.abs(dy)
        out.da, out.da_mag = dy @ w[:K].T, np.abs(dy) @ np.abs(w[:K]).T
    return out


def assert_bound(got, ref, mag, terms, what):
    """|got - ref| <= (terms + 3) * 2^-24 * mag per element (terms: a scalar, or an array that broadcasts), no NaN, and exactly 0
    where nothing contributes.  Prints and returns the largest used fraction of the bound."""
    got = np.asarray(got)
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), "%s: NaN (unwritten, or a non-finite product)" % what
    bound = np.broadcast_to((np.asarray(terms, np.float64) + 3.0) * U * mag, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    live = mag > 0
    assert not got[~live].any(), "%s: elements with no contributing term must be exactly 0" % what
    used = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print("%s: max |err| / ((terms + 3) 2^-24 mag) = %.4f" % (what, used))
    assert used <= 1.0, "%s: %.3f of the bound" % (what, used)
    return used


def make_operands(seed, B, P, K1, K2, N, T, with_bias=True):
    """fp32 operands with mixed signs and magnitudes 2^-6 .. 2^6 (sums cancel), and a cotangent of the same kind"""
    rng = np.random.RandomState(seed)

    def vals(*shape):
        return (rng.choice([-1.0, 1.0], size=shape) * 2.0 ** rng.uniform(-6, 6, size=shape)).astype(np.float32)
    R = B * P
    a1 = vals(R, K1)
    a2 = vals(R, K2) if K2 > 0 else None
    w = vals(K1 + K2 + T, N)
    bias = vals(N) if with_bias else None
    dy = vals(R, N)
    return a1, a2, w, bias, dy


# the protocol case of tests/test_gpu_condlogits.py: six shapes around N = 256 rows, batches of 3; tests/test_condlogits.py asserts
# without a GPU that the evaluation's draws complete within the cap
PROTO_SIZES = [257, 256, 300, 130, 280, 256]
PROTO_CATEGORY = [10, 0, 15, 10, 4, 1]
PROTO_N, PROTO_BATCH, PROTO_SEED, PROTO_MIN_COUNT, PROTO_MAX_PASSES = 256, 3, 9, 1, 64


def proto_shapes(part_lo, part_n, seed=2):
    """-> shape_blocks rows per shape of PROTO_SIZES: xyz in the unit cube, labels inside the category's parts"""
    from sph3d_gcn_amd.harness import objfeed
    rng = np.random.RandomState(seed)
    out = []
    for n, c in zip(PROTO_SIZES, PROTO_CATEGORY):
        xyz = (rng.rand(n, 3) - 0.5).astype(np.float32)
        out.append(objfeed.shape_blocks(xyz, int(part_lo[c]) + rng.randint(0, int(part_n[c]), n)))
    return out


def make_categories(B, T):
    """[B] int32: a repeat, an unused category, and -1 and T among them as far as B allows"""
    base = [T - 1, -1, T - 1, T, 0, 0, min(2, T - 1)]
    return np.asarray((base * (B // len(base) + 1))[:B], dtype=np.int32)
