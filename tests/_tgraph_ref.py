"""The transposed neighbour graph (include/sph3d.h, csrc/graph.hip) stated in numpy: no torch, no library.

A neighbour graph is nn_index [B, M, K] (ids of the n_src source points of the row's cloud), nn_count [B, M] and, optionally,
bin_index [B, M, K] (F = num_bins filter bins) or weight [B, M, K].  Its live edges are the slots k < nn_count[b, m].  The
transposed graph lists, for every segment (cloud b, source n, bin f), the edges that name it:
  offsets [B * (L + 1)]   L = n_src * F; cloud b's part is b * M * K + the exclusive prefix sum of its L segment sizes, then
                          the cloud's end; cloud b's entries are [offsets[b, 0], offsets[b, L]) inside its slab of M * K
  entries                 per edge the row m and a factor: float32(1) / float32(nn_count[b, m]), or weight[b, m, k]
  active_bins             [count, the bins that occur among the live edges, ascending]; nothing behind 1 + count is defined
A bin id outside [0, F - 1] is clamped into it.  The order of the entries inside one segment is the arrival order of an atomic
on the device, so entries are compared as triples (segment, row, factor bits) sorted by all three: everything here is an
integer or a float's bit pattern, and every comparison made with it is exact."""
import numpy as np

ORDER_WINDOW = 2048          # graph.hip: kOrderWindow
DEGREE_CAP = 1 << 20         # graph.hip: balanced_order_window


def _sorted_triples(seg, key, scale_bits):
    t = np.stack([np.asarray(seg, np.int64), np.asarray(key, np.int64), np.asarray(scale_bits, np.int64)], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def transpose_reference(idx, cnt, n_src, bin_index=None, num_bins=1, weight=None):
    """-> (offsets int32 [B * (L + 1)], entries int64 [E, 3] = (segment b * L + n * F + f, row m, factor bits), sorted,
    active_bins int32 [1 + count])"""
    idx, cnt = np.asarray(idx), np.asarray(cnt)
    B, M, K = idx.shape
    F = int(num_bins) if bin_index is not None else 1
    L = n_src * F
    live = np.arange(K)[None, None, :] < cnt[:, :, None]
    b, m, k = np.nonzero(live)
    n = idx[b, m, k].astype(np.int64)
    assert n.size == 0 or (n.min() >= 0 and n.max() < n_src), "ids of live edges must name a source point"
    f = np.zeros(n.size, np.int64) if bin_index is None else np.clip(np.asarray(bin_index)[b, m, k].astype(np.int64), 0, F - 1)
    local = n * F + f
    offsets = np.zeros((B, L + 1), np.int64)
    for c in range(B):
        offsets[c, 0] = c * M * K
        offsets[c, 1:] = c * M * K + np.cumsum(np.bincount(local[b == c], minlength=L))
    assert offsets.max(initial=0) < 2 ** 31
    if weight is None:
        scale = np.float32(1) / cnt[b, m].astype(np.float32)
    else:
        scale = np.asarray(weight, np.float32)[b, m, k]
    bits = np.ascontiguousarray(scale, np.float32).view(np.uint32)
    occurring = np.unique(f)
    active = np.concatenate([[occurring.size], occurring]).astype(np.int32)
    return offsets.astype(np.int32).reshape(-1), _sorted_triples(b * L + local, m, bits), active


def device_entries(offsets, key, scale, B, L, MK):
    """arrays as the library writes them (scale None: packed entry words, decoded here in unsigned arithmetic) -> the sorted
    triples of transpose_reference.  The segment of an entry is where the offsets put it."""
    off = np.asarray(offsets).astype(np.int64).reshape(B, L + 1)
    key = np.ascontiguousarray(key).reshape(-1)
    segs, keys, bits = [], [], []
    for b in range(B):
        sizes = np.diff(off[b])
        assert (sizes >= 0).all() and b * MK <= off[b, 0] and off[b, L] <= (b + 1) * MK, "cloud %d: offsets leave its slab" % b
        segs.append(np.repeat(np.arange(L, dtype=np.int64) + b * L, sizes))
        lo, hi = int(off[b, 0]), int(off[b, L])
        if scale is None:
            w = key[lo:hi].view(np.uint32)
            keys.append(w & np.uint32(0xffffff))
            s = np.float32(1) / (w >> np.uint32(24)).astype(np.float32)
        else:
            keys.append(key[lo:hi])
            s = np.ascontiguousarray(scale, np.float32).reshape(-1)[lo:hi]
        bits.append(np.ascontiguousarray(s, np.float32).view(np.uint32))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return _sorted_triples(cat(segs), cat(keys), cat(bits))


def balanced_order_reference(offsets, B, N, F):
    """sph3d_graph_balanced_order: per cloud and window of 2048 consecutive sources, the sources sorted by the unique key
    (min(in-degree, 2^20) << 11 | index in the window) — descending in even windows, ascending in odd ones -> int32 [B, N]"""
    off = np.asarray(offsets).astype(np.int64).reshape(B, N * F + 1)
    order = np.zeros((B, N), np.int32)
    for b in range(B):
        deg = np.minimum(off[b, F::F] - off[b, :-1:F], DEGREE_CAP)
        for win, base in enumerate(range(0, N, ORDER_WINDOW)):
            d = deg[base:base + ORDER_WINDOW]
            keys = np.sort((d << 11) | np.arange(d.size))
            if win % 2 == 0:
                keys = keys[::-1]
            order[b, base:base + d.size] = base + (keys & (ORDER_WINDOW - 1))
    return order


def _spread3(v):
    v = v & np.uint32(0x3ff)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000ff)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300f00f)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030c30c3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def spatial_order_keys(xyz, N):
    """sph3d_spatial_order's sort key of every point, xyz [B, N, 3] float32 -> int64 [B, N]: the Morton code of the point's cell
    in a grid of 2^bpa cells per axis over the cloud's bounding box, cells sized by the longest axis; every operation float32"""
    xyz = np.asarray(xyz, np.float32)
    assert xyz.shape[1:] == (N, 3)
    bpa = 5 if 4096 < 4 * N else 4
    G = 1 << bpa
    keys = np.zeros(xyz.shape[:2], np.int64)
    for b in range(xyz.shape[0]):
        lo, hi = xyz[b].min(axis=0), xyz[b].max(axis=0)
        ext = np.float32((hi - lo).max())
        inv = np.float32(G) / ext if ext > 0 else np.float32(0)
        q = np.clip(((xyz[b] - lo) * inv).astype(np.int64), 0, G - 1).astype(np.uint32)
        k = np.zeros(N, np.uint32)
        for a in range(3):
            k |= _spread3(q[:, a]) << np.uint32(a)
        keys[b] = k
    return keys
