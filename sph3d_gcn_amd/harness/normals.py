"""Surface normals from order-free integer ball moments: the SPECIFICATION in numpy (no GPU) of csrc/normals.hip
(include/sph3d.h: sph3d_graph_normals, sph3d_ball_normals), and the two places the harness estimates normals on the device.

The statement
  * offsets: for a query q and a neighbour p (fp32 xyz) d_a = p_a - q_a, one fp32 subtraction per axis; Q = 262144.0 /
    (double)radius; t_a = rint((double)d_a * Q), ties to even.  A neighbour is VALID when fabs((double)d_a) * Q <= 2^21 on all
    three axes (a non-finite offset fails); the others are skipped.  A query with a non-finite coordinate has no valid neighbour;
  * moments: ten int64 per query over its valid neighbours — n, S1_x, S1_y, S1_z, S2_xx, S2_xy, S2_xz, S2_yy, S2_yz, S2_zz.
    Integer sums: the order of the neighbours cannot show, so the device's moments are compared for EQUALITY;
  * covariance in float64, every operation rounded once: m_a = S1_a / n, c_ab = S2_ab / n - m_a m_b;
  * normal: the unit eigenvector of the smallest eigenvalue l0 (np.linalg.eigh); variation = max(l0, 0) / (l0 + l1 + l2) as
    fp32.  A row with n < min_count (min_count >= 3) or with a trace (c_xx + c_yy) + c_zz that is not positive gets (0, 0, 0)
    and variation 0;
  * sign, decided in float64 before the rounding to fp32: the component of largest magnitude is positive (ties: the lowest
    axis); then, with `toward`, the normal is flipped when n . ((double)toward - (double)q) < 0 (exactly 0 keeps the sign).

``graph_normals_reference`` takes the first min(nn_count, K) entries of a row of a neighbour graph (an entry outside [0, N) is
skipped like an invalid one); ``ball_normals_reference`` takes every point with the fp32 predicate (dx*dx + dy*dy) + dz*dz < r2,
dx = p.x - q.x, r2 = fp32(radius * radius), the point itself included — brute force in chunks.

``estimate_pool`` and ``batch_normals`` run the kernels (tf_surface) for a feed.BlockPool and for a [B, N, >=3] batch.
"""
from types import SimpleNamespace

import numpy as np

LIMIT = 2097152.0            # 2^21
MOMENTS = 10
_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def check_args(radius, min_count):
    """-> (fp32 radius, min_count) or ValueError, as the C entries refuse them"""
    r = np.float32(radius)
    if not (r > 0 and np.isfinite(r)):
        raise ValueError("normals: finite radius>0 required, got %r" % (radius,))
    if int(min_count) < 3:
        raise ValueError("normals: min_count>=3 required, got %r" % (min_count,))
    return r, int(min_count)


def quantise(offsets, radius):
    """offsets [..., 3] fp32 -> (t [..., 3] int64, 0 where not valid; valid [...] bool)"""
    d = np.asarray(offsets)
    if d.dtype != np.float32:
        raise ValueError("quantise: fp32 offsets expected (the subtraction is an fp32 one)")
    q = 262144.0 / float(np.float32(radius))
    with np.errstate(invalid="ignore", over="ignore"):
        u = d.astype(np.float64) * q
        valid = (np.abs(u) <= LIMIT).all(axis=-1)                  # (a NaN fails)
    t = np.rint(np.where(valid[..., None], u, 0.0)).astype(np.int64)
    return t, valid


def moments_reference(offsets, listed, radius):
    """offsets [R, K, 3] fp32 (p - q of every candidate), listed [R, K] bool (the candidate is a neighbour of the row)
    -> (moments [R, 10] int64, skipped: the listed candidates that are not valid)"""
    t, valid = quantise(offsets, radius)
    listed = np.asarray(listed, dtype=bool)
    use = valid & listed
    t = t * use[..., None]
    out = np.zeros(t.shape[:-2] + (MOMENTS,), dtype=np.int64)
    out[..., 0] = use.sum(axis=-1)
    out[..., 1:4] = t.sum(axis=-2)
    for j, (a, b) in enumerate(_PAIRS):
        out[..., 4 + j] = (t[..., a] * t[..., b]).sum(axis=-1)
    return out, int((listed & ~valid).sum())


def covariance_reference(moments):
    """moments [R, 10] -> (c [R, 3, 3] float64, ok [R] bool: n > 0; rows that are not ok are zero)"""
    m = np.asarray(moments, dtype=np.int64).reshape(-1, MOMENTS)
    n = m[:, 0].astype(np.float64)
    ok = m[:, 0] > 0
    n = np.where(ok, n, 1.0)
    mean = m[:, 1:4].astype(np.float64) / n[:, None]
    c = np.zeros((m.shape[0], 3, 3), dtype=np.float64)
    for j, (a, b) in enumerate(_PAIRS):
        c[:, a, b] = c[:, b, a] = m[:, 4 + j].astype(np.float64) / n - mean[:, a] * mean[:, b]
    c[~ok] = 0.0
    return c, ok


def normals_from_moments_reference(moments, query, toward=None, min_count=3, full=False):
    """moments [R, 10] int64, query [R, 3] fp32, toward None or [R, 3] / [3] fp32 -> (normals [R, 3] fp32, variation [R] fp32).
    full: also a namespace with `evals` [R, 3] float64 ascending (0 for zero rows), `normal64` [R, 3] (the signed float64
    vector before its rounding), `zero` [R] bool (the rows the statement sets to zero) and `dot` [R] (the float64 product the
    toward rule looked at; None without toward)"""
    m = np.asarray(moments, dtype=np.int64).reshape(-1, MOMENTS)
    q = np.asarray(query, dtype=np.float32).reshape(-1, 3)
    R = m.shape[0]
    c, ok = covariance_reference(m)
    trace = (c[:, 0, 0] + c[:, 1, 1]) + c[:, 2, 2]
    live = ok & (m[:, 0] >= int(min_count)) & (trace > 0.0)
    evals = np.zeros((R, 3), dtype=np.float64)
    vec = np.zeros((R, 3), dtype=np.float64)
    if live.any():
        w, v = np.linalg.eigh(c[live])
        evals[live] = w
        vec[live] = v[:, :, 0]
    lead = np.argmax(np.abs(vec), axis=1)                          # (the first maximum: ties go to the lowest axis)
    flip = vec[np.arange(R), lead] < 0.0
    vec = np.where(flip[:, None], -vec, vec)
    dot = None
    if toward is not None:
        t = np.broadcast_to(np.asarray(toward, dtype=np.float32), (R, 3)).astype(np.float64) - q.astype(np.float64)
        with np.errstate(invalid="ignore"):
            dot = (vec[:, 0] * t[:, 0] + vec[:, 1] * t[:, 1]) + vec[:, 2] * t[:, 2]
            back = live & (dot < 0.0)
        vec = np.where(back[:, None], -vec, vec)
    vec[~live] = 0.0
    total = (evals[:, 0] + evals[:, 1]) + evals[:, 2]
    pos = live & (evals[:, 0] > 0.0)
    variation = np.zeros(R, dtype=np.float64)
    variation[pos] = evals[pos, 0] / total[pos]
    out = vec.astype(np.float32), variation.astype(np.float32)
    if full:
        return out + (SimpleNamespace(evals=evals, normal64=vec, zero=~live, dot=dot),)
    return out


def graph_normals_reference(database, query, nn_index, nn_count, radius, toward=None, min_count=3):
    """database [B, N, 3], query [B, M, 3] fp32, nn_index [B, M, K], nn_count [B, M] int, toward None or [B, 3]
    -> namespace: normals [B, M, 3] fp32, variation [B, M] fp32, count [B, M] int32, moments [B, M, 10] int64, skipped (int),
    and evals / normal64 / zero / dot of normals_from_moments_reference, shaped [B, M, ...]"""
    radius, min_count = check_args(radius, min_count)
    database = np.asarray(database, dtype=np.float32)
    query = np.asarray(query, dtype=np.float32)
    nn_index, nn_count = np.asarray(nn_index), np.asarray(nn_count)
    B, M, K = nn_index.shape
    N = database.shape[1]
    moments = np.zeros((B, M, MOMENTS), dtype=np.int64)
    skipped = 0
    for b in range(B):
        idx = nn_index[b].astype(np.int64)
        inside = (idx >= 0) & (idx < N)
        listed = np.arange(K)[None, :] < np.clip(nn_count[b].astype(np.int64), 0, K)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            off = (database[b][np.where(inside, idx, 0)] if N > 0 else np.zeros((M, K, 3), np.float32)) - query[b][:, None, :]
        moments[b], s = moments_reference(off.astype(np.float32), listed & inside, radius)
        skipped += s + int((listed & ~inside).sum())
    tw = None if toward is None else np.repeat(np.asarray(toward, dtype=np.float32).reshape(B, 1, 3), M, axis=1).reshape(-1, 3)
    nrm, var, f = normals_from_moments_reference(moments, query.reshape(-1, 3), tw, min_count, full=True)
    return SimpleNamespace(normals=nrm.reshape(B, M, 3), variation=var.reshape(B, M), count=moments[:, :, 0].astype(np.int32),
                           moments=moments, skipped=skipped, evals=f.evals.reshape(B, M, 3),
                           normal64=f.normal64.reshape(B, M, 3), zero=f.zero.reshape(B, M),
                           dot=None if f.dot is None else f.dot.reshape(B, M))


def ball_moments_reference(xyz, radius, rows=None, chunk_elems=1 << 22):
    """the ball form's moments of the queries `rows` (default: all) of xyz [V, 3] fp32 against ALL points -> [len(rows), 10]"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    V = xyz.shape[0]
    rows = np.arange(V) if rows is None else np.asarray(rows, dtype=np.int64)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    out = np.zeros((len(rows), MOMENTS), dtype=np.int64)
    if V == 0 or len(rows) == 0:
        return out
    step = max(1, chunk_elems // V)
    px, py, pz = xyz[:, 0][None, :], xyz[:, 1][None, :], xyz[:, 2][None, :]
    for lo in range(0, len(rows), step):
        q = xyz[rows[lo:lo + step]]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = px - q[:, 0:1], py - q[:, 1:2], pz - q[:, 2:3]
            d2 = (dx * dx + dy * dy) + dz * dz
            qi, pi = np.nonzero(d2 < r2)                               # row-major: grouped by query, ascending point
        t, valid = quantise(np.stack([dx[qi, pi], dy[qi, pi], dz[qi, pi]], axis=-1), r)
        cols = [valid.astype(np.int64), t[:, 0], t[:, 1], t[:, 2]] + [t[:, a] * t[:, b] for a, b in _PAIRS]
        ends = np.searchsorted(qi, np.arange(len(q) + 1))
        for j, col in enumerate(cols):
            cs = np.concatenate(([0], np.cumsum(col, dtype=np.int64)))
            out[lo:lo + len(q), j] = cs[ends[1:]] - cs[ends[:-1]]
    return out


def ball_normals_reference(xyz, radius, toward=None, min_count=3):
    """xyz [V, 3] fp32, toward None or [3] -> namespace as graph_normals_reference's, shaped [V, ...] (skipped is not reported:
    the ball form has no counter)"""
    radius, min_count = check_args(radius, min_count)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    moments = ball_moments_reference(xyz, radius)
    nrm, var, f = normals_from_moments_reference(moments, xyz, toward, min_count, full=True)
    return SimpleNamespace(normals=nrm, variation=var, count=moments[:, 0].astype(np.int32), moments=moments, evals=f.evals,
                           normal64=f.normal64, zero=f.zero, dot=f.dot)


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
def estimate_pool(pool, radius, toward=None, min_count=3):
    """normals of every row of a feed.BlockPool (or anything with its face: rows [T, 8] on the device, host_offsets): one
    ball_normals call per block — a block is a cloud of its own — on torch's current stream.  toward: None or [3].
    -> [T, 4] fp32 on the pool's device, in pool row order: nx, ny, nz, 0 (facadefeed.FacadePool's `normals` layout)"""
    import torch
    from .. import tf_surface
    out = torch.zeros((int(pool.rows.shape[0]), 4), dtype=torch.float32, device=pool.rows.device)
    off = [int(o) for o in pool.host_offsets]
    for lo, hi in zip(off[:-1], off[1:]):
        nrm = tf_surface.ball_normals(pool.rows[lo:hi, 0:3].contiguous(), radius, toward, min_count)[0]
        out[lo:hi, 0:3] = nrm
    return out


def batch_normals(points, radius, nnsample, toward=None, min_count=3):
    """points [B, N, >=3] on the device: the sphere search of the batch against itself (tf_nnquery.build_sphere_neighbor, in the
    radius mode that is set), then graph_normals over that graph.  toward: None or [B, 3].
    -> (normals [B, N, 3] fp32, variation [B, N] fp32, count [B, N] int32)"""
    from .. import tf_nnquery, tf_surface
    xyz = points[:, :, 0:3].contiguous()
    nn_index, nn_count, _ = tf_nnquery.build_sphere_neighbor(xyz, xyz, radius, None, nnsample)
    return tf_surface.graph_normals(xyz, xyz, nn_index, nn_count, radius, toward, min_count)
