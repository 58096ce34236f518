"""Exact k nearest neighbours: the numpy STATEMENT of csrc/knn.hip (include/sph3d.h: sph3d_build_nearest_neighbor), no GPU.

``knn_reference(database, query, k, radius=None, dist="root")`` -> nn_index [B, M, k] int32, nn_count [B, M] int32,
nn_dist [B, M, k] float32: the format of the range searches.  The kernels' outputs equal it bit for bit at every launch form.
Everything is float32 with one rounding per operation (the library is built without contraction):

  d2        dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;  d2 = (dx*dx + dy*dy) + dz*dz  (sph3d_nn1's d2)
  admitted  a database point is a candidate of a query iff d2 is finite and, with a radius, d2 < R2,
            R2 = float32(radius) * float32(radius).  ``radius=None`` and ``radius=inf`` say the same.  THIS PREDICATE IS THE OP'S
            OWN and deliberately simple: it is not the reference kernel's ``fabs(dist - radius) > 1e-6`` test
            (tf_nnquery_gpu.cu), and no radius grows.
  row       the admitted candidates in ascending (d2, index) order, the lowest index first among equal d2, cut at k.
            nn_count = min(k, admitted): it may be 0 with a radius, or for a query with a non-finite coordinate; a database
            point with a non-finite coordinate is never returned.  Unused slots hold index 0 and distance 0.
  nn_dist   "root" (the default): sqrt(sqrt(d2)), two correctly rounded float32 roots — the library's convention (the SQUARE
            ROOT of the Euclidean distance), so spherical_kernel and the 'weighted' un-pooling take the tensor as it is;
            "squared": d2 itself (what the 'idw' un-pooling weights are formed from).

1 <= k <= 64; radius > 0.
"""
import numpy as np

_F32 = np.float32
MAX_K = 64
AUTO, SCAN, GRID = 0, 1, 2               # include/sph3d.h: SPH3D_KNN_AUTO, _SCAN, _GRID
DIST = {"root": 0, "squared": 1}         # SPH3D_KNN_DIST_ROOT, _SQUARED


def squared_distances(database, query):
    """[N, 3], [M, 3] float32 -> d2 [M, N] float32, every operation rounded once"""
    p = np.ascontiguousarray(database, dtype=_F32)
    q = np.ascontiguousarray(query, dtype=_F32)
    with np.errstate(all="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def knn_reference(database, query, k, radius=None, dist="root"):
    database = np.ascontiguousarray(np.asarray(database)[:, :, 0:3], dtype=_F32)
    query = np.ascontiguousarray(np.asarray(query)[:, :, 0:3], dtype=_F32)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("1 <= k <= %d required, got %d" % (MAX_K, k))
    if dist not in DIST:
        raise ValueError("dist must be 'root' or 'squared'")
    r = _F32(np.inf) if radius is None else _F32(radius)
    if not r > 0:
        raise ValueError("radius > 0 required")
    with np.errstate(all="ignore"):
        R2 = r * r
    B, N, _ = database.shape
    M = query.shape[1]
    if query.shape[0] != B or N < 1:
        raise ValueError("database [B, N >= 1, 3] and query [B, M, 3] required")
    nn_index = np.zeros((B, M, k), np.int32)
    nn_count = np.zeros((B, M), np.int32)
    nn_dist = np.zeros((B, M, k), _F32)
    index = np.arange(N, dtype=np.uint64)
    chunk = max(1, (1 << 22) // N)
    for b in range(B):
        for m0 in range(0, M, chunk):
            d2 = squared_distances(database[b], query[b, m0:m0 + chunk])
            with np.errstate(all="ignore"):
                admitted = np.isfinite(d2) & (d2 < R2)
            # (bits(d2) << 32) | index: for non-negative finite floats the bit order is the value order
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[None, :]
            key[~admitted] = np.uint64(0xffffffffffffffff)
            kk = min(k, N)
            part = np.partition(key, kk - 1, axis=1)[:, :kk] if kk < N else key
            part = np.sort(part, axis=1)[:, :kk]
            ok = part != np.uint64(0xffffffffffffffff)
            rows = slice(m0, m0 + d2.shape[0])
            nn_count[b, rows] = ok.sum(axis=1)
            nn_index[b, rows, :kk] = np.where(ok, part & np.uint64(0xffffffff), 0).astype(np.int32)
            best = np.where(ok, (part >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(_F32)
            nn_dist[b, rows, :kk] = best if dist == "squared" else np.sqrt(np.sqrt(best))
    return nn_index, nn_count, nn_dist
