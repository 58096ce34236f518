"""Per-graph cache of transposed neighbour graphs (include/sph3d.h: sph3d_graph_transpose).

Every gradient of the path gathers over the transpose of its neighbour graph.  One graph feeds several
gradients per step (two depthwise convs per level share an intra graph), so the transpose is built once
per (nn_index, nn_count[, bin_index | weight]) and kept in a small LRU.  An entry holds strong references
to the tensors it was built from, so their storage (and therefore the data_ptr in the key) cannot be
recycled for a different graph while the entry is alive; in-place edits are caught by the version counter.
"""
import collections
import contextlib

import torch

from . import _lib

BALANCE_MIN_POINTS = 1024   # binned graphs with at least this many source points get a degree-balanced gradient order
PACK_ENTRIES = True     # (False: always separate key / scale arrays)
_MAX_ENTRIES = 24      # one S3DIS step builds 12 (8 binned intra graphs, 4 un-pooling graphs; deterministic and fuzzy plans: 4 pooling graphs more); entries pin ~150 MB each at level 0
_cache = collections.OrderedDict()


def _ident(t):
    return (0, 0) if t is None else (t.data_ptr(), t._version)


_generation = [0]      # bumped by clear(): entries attached to graph tensors (transpose's fast path) from before are ignored


def clear():
    """drop every cached transpose / order (and the per-stream call workspaces of _lib).  Plan tensors carved from one _lib.Arena
    share ONE autograd version counter (they are views of one buffer): an in-place edit of any tensor of a plan invalidates every
    cached transpose of that plan — correct, but the backward pass then rebuilds them on the main stream.  Graph tensors are
    outputs of the graph-building ops and are never edited in place by this package."""
    _lib.release_scratch()
    _cache.clear()
    _orders.clear()
    _unique.clear()
    _generation[0] += 1


# ---- deterministic mode (include/sph3d.h: sph3d_set_deterministic) ----
def is_deterministic():
    return bool(_lib.lib().sph3d_get_deterministic())


def set_deterministic(flag):
    """process-wide: every transposed graph built from now on is in canonical entry order, the conv gradient runs no hub
    launches, and what can only run with float atomics raises.  A change of the value empties this cache, so a transpose built
    in arrival order is never served while the mode is on -> the previous value"""
    flag = bool(flag)
    prev = bool(_lib.lib().sph3d_set_deterministic(1 if flag else 0))
    if prev != flag:
        clear()
    return prev


@contextlib.contextmanager
def deterministic(flag=True):
    prev = set_deterministic(flag)
    try:
        yield
    finally:
        set_deterministic(prev)


# processing order of the source points of a graph (a permutation per cloud, spatially sorted): optional hint for
# the convolution gradient (include/sph3d.h: source_order), registered by whoever knows the points' coordinates
_orders = collections.OrderedDict()


def set_source_order(nn_index, order):
    _orders[_ident(nn_index)] = (order, nn_index, set())
    while len(_orders) > _MAX_ENTRIES:
        _orders.popitem(last=False)


def source_order(nn_index):
    hit = _orders.get(_ident(nn_index))
    if hit is None:
        return None
    order = hit[0]
    if order.is_cuda:
        cur = _lib.current_raw_stream()
        if cur not in hit[2]:               # once per consuming stream: built on the graph stream, read by this stream's kernels
            order.record_stream(torch.cuda.current_stream())
            hit[2].add(cur)
    return order


_unique = set()        # keys of cached transposes whose builder promised rows without repeated neighbour ids


def peek(nn_index, nn_count, n_src, need_unique_rows=False):
    """the cached transpose of an un-binned, un-weighted graph, or None (never builds: for gradients that have a fallback).
    need_unique_rows: only a transpose whose builder promised that no row of nn_index lists a point twice (the max-pool
    gradient as a gather would add such a point's gradient once per repeat; the reference adds it once: ADVICE r3)"""
    key = (_ident(nn_index), _ident(nn_count), _ident(None), _ident(None), int(n_src), 1, tuple(nn_index.shape))
    if key not in _cache or (need_unique_rows and key not in _unique):
        return None
    return transpose(nn_index, nn_count, n_src)


def cached(nn_index, nn_count, n_src, bin_index=None, num_bins=1):
    """what transpose() with these arguments returns if that transpose is in the cache, else None (never builds)"""
    F = int(num_bins) if bin_index is not None else 1
    key = (_ident(nn_index), _ident(nn_count), _ident(bin_index), _ident(None), int(n_src), F, tuple(nn_index.shape))
    if key not in _cache:
        return None
    return transpose(nn_index, nn_count, n_src, bin_index=bin_index, num_bins=num_bins)


# ---- row link of a pooling graph (include/sph3d.h: sph3d_gather_rows_link) ----
# A pooling graph whose rows are rows of the level's intra graph needs no transposed graph of its own: the max-pool gradient walks
# the INTRA graph's transposed graph and this link (tf_pool3d).  The link hangs on the pooled nn_index tensor, as a transposed
# graph's fast-path entry does, and names the intra graph's tensors: the gradient asks cached() for their transpose when it runs.
def attach_row_link(pool_index, pool_count, first, next_, intra_index, intra_count, bin_index, num_bins):
    """record (on the current stream, which has just written them) the link first [B, N] / next [B, S] of the pooling graph
    (pool_index, pool_count) over the intra graph (intra_index, intra_count[, bin_index with num_bins bins])"""
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    pool_index._sph3d_rows = ((first, next_, intra_index, intra_count, bin_index, int(num_bins), ev, {_lib.current_raw_stream()}),
                              pool_count, (_generation[0], pool_index._version, pool_count._version))


def row_link(pool_index, pool_count):
    """-> (first, next, transposed intra graph, F) when (pool_index, pool_count) carry a row link whose intra graph's transposed
    graph is still cached, else None; orders the current stream behind the link's and the transpose's builders"""
    hung = pool_index.__dict__.get("_sph3d_rows")
    if hung is None or hung[1] is not pool_count or hung[2] != (_generation[0], pool_index._version, pool_count._version):
        return None
    first, next_, intra_index, intra_count, bin_index, num_bins, ev, synced = hung[0]
    tg = cached(intra_index, intra_count, intra_index.shape[1], bin_index=bin_index, num_bins=num_bins)
    if tg is None:
        return None
    cur_raw = _lib.current_raw_stream()
    if cur_raw not in synced:
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        first.record_stream(cur)
        next_.record_stream(cur)
        synced.add(cur_raw)
    return first, next_, tg, (num_bins if bin_index is not None else 1)


def _attach(nn_index, fkey, hit, nn_count, bin_index, weight):
    fast = nn_index.__dict__.get("_sph3d_tg")
    if fast is None:
        fast = nn_index._sph3d_tg = {}
    out, _keep, ev, synced = hit
    # (no reference back to nn_index: a cycle would keep a dropped graph's tensors until the cyclic collector runs)
    fast[fkey] = ((out, (nn_count, bin_index, weight), ev, synced),
                  (_generation[0], nn_index._version, nn_count._version, 0 if bin_index is None else bin_index._version,
                   0 if weight is None else weight._version))


def entries(tg):
    """(keys, scales) of a transposed graph returned by transpose(), decoded: int32 rows and float32 factors whether or not the
    entries are packed (tests, tools)"""
    _off, key, scale, _act = tg
    if scale is not None:
        return key, scale
    cnt = (key >> 24) & 0xff
    return key & 0xffffff, torch.where(cnt > 0, 1.0 / cnt.float().clamp(min=1.0), torch.zeros_like(cnt, dtype=torch.float32))


def transpose(nn_index, nn_count, n_src, bin_index=None, weight=None, num_bins=1, counted_workspace=None, unique_rows=False):
    """-> (offsets[B*(n_src*F+1)] i32, ent_key[B*M*K] i32, ent_scale[B*M*K] f32 | None (packed entries: see below), active_bins[F+1] i32 | None) on
    nn_index's device; F = num_bins (the filter's bin count when bin_index is given, else 1); active_bins (count, then
    the bins that occur) is produced for binned graphs only.  counted_workspace: a transpose workspace whose counting
    phase has already run (tf_nnquery.build_sphere_graph did it inside the neighbour search): only scan + fill remain.
    unique_rows: the caller's promise that no row lists a point twice (rows of the ball query and rows gathered from them)"""
    F = int(num_bins) if bin_index is not None else 1
    cur_raw = _lib.current_raw_stream()
    # fast path (the backward pass asks 50 times per step): the entry hangs on the nn_index tensor object itself, keyed by the
    # identities of the other tensors (which the entry keeps alive, so an id cannot be recycled under it); in-place edits are
    # caught by the version counters
    fkey = (id(nn_count), id(bin_index), id(weight), n_src, F)
    fast = nn_index.__dict__.get("_sph3d_tg")
    if fast is not None and not unique_rows:
        fhit = fast.get(fkey)
        if fhit is not None:
            hit, vers = fhit
            if vers == (_generation[0], nn_index._version, nn_count._version, 0 if bin_index is None else bin_index._version,
                        0 if weight is None else weight._version):
                out, _keep, ev, synced = hit
                if cur_raw not in synced:
                    cur = torch.cuda.current_stream()
                    cur.wait_event(ev)
                    for t in out:
                        if t is not None:
                            t.record_stream(cur)
                    synced.add(cur_raw)
                return out
    key = (_ident(nn_index), _ident(nn_count), _ident(bin_index), _ident(weight), int(n_src), F, tuple(nn_index.shape))
    if unique_rows:
        _unique.add(key)
    hit = _cache.get(key)
    if hit is not None:
        _cache.move_to_end(key)
        out, _keep, ev, synced = hit
        if cur_raw not in synced:                # built ahead of time on the graph stream: order this stream after it, ONCE
            cur = torch.cuda.current_stream()
            cur.wait_event(ev)
            for t in out:
                if t is not None:
                    t.record_stream(cur)
            synced.add(cur_raw)
        _attach(nn_index, fkey, hit, nn_count, bin_index, weight)
        return out
    cur = torch.cuda.current_stream()
    B, M, K = nn_index.shape
    dev = nn_index.device
    offsets = _lib.empty((B * (n_src * F + 1),), torch.int32, dev)
    ent_key = _lib.empty((B * M * K,), torch.int32, dev)
    # un-weighted graphs with at most 2^24 rows and K <= 255: PACKED entries (include/sph3d.h) — ent_key word = m | nn_count[m] << 24,
    # no ent_scale array (None here, NULL at the C ABI): one scattered store per edge in the fill pass instead of two
    packed = weight is None and M <= (1 << 24) and K <= 255 and PACK_ENTRIES
    ent_scale = None if packed else _lib.empty((B * M * K,), torch.float32, dev)
    active = _lib.empty((F + 1,), torch.int32, dev) if bin_index is not None else None
    l = _lib.lib()
    wsb = l.sph3d_graph_transpose_workspace(B, n_src, M, K, F)
    # processing order of the convolution gradient that evens out the in-edges per wave (sph3d_graph_balanced_order), written by
    # the fill launch itself; an order registered by the caller (set_source_order) wins
    order = None
    if bin_index is not None and n_src >= BALANCE_MIN_POINTS and _ident(nn_index) not in _orders:
        order = _lib.empty((B, n_src), torch.int32, dev)
    if counted_workspace is None:
        counted_workspace = torch.empty((max(wsb, 1),), dtype=torch.uint8, device=dev)
        _lib.check(l.sph3d_graph_transpose_count(B, n_src, M, K, F, _lib.ptr(nn_index), _lib.ptr(nn_count), _lib.ptr(bin_index),
                                                 1 if bin_index is not None else 0, _lib.ptr(counted_workspace), wsb,
                                                 _lib.stream_ptr()))
    _lib.check(l.sph3d_graph_transpose_finish_ordered(B, n_src, M, K, F, _lib.ptr(nn_index), _lib.ptr(nn_count),
                                                      _lib.ptr(bin_index), _lib.ptr(weight), _lib.ptr(offsets), _lib.ptr(ent_key),
                                                      _lib.ptr(ent_scale), _lib.ptr(active), _lib.ptr(order),
                                                      _lib.ptr(counted_workspace), wsb, _lib.stream_ptr()))
    if order is not None:
        set_source_order(nn_index, order)
    out = (offsets, ent_key, ent_scale, active)
    ev = torch.cuda.Event()
    ev.record(cur)
    _cache[key] = (out, (nn_index, nn_count, bin_index, weight), ev, {cur_raw})
    _attach(nn_index, fkey, _cache[key], nn_count, bin_index, weight)
    while len(_cache) > _MAX_ENTRIES:
        _unique.discard(_cache.popitem(last=False)[0])
    return out


def transpose_edges(nn_index, nn_count, n_src, counted_workspace=None):
    """-> (offsets[B*(n_src+1)] i32, ent_edge[B*M*K] i32): the un-binned transpose whose entries name the edge m*K + k
    (include/sph3d.h: sph3d_graph_transpose_finish_edges), for the fuzzy convolution's gradient.  Cached under a key of its own
    ("edges"), in the same LRU and with the same stream rules as transpose()."""
    cur_raw = _lib.current_raw_stream()
    key = ("edges", _ident(nn_index), _ident(nn_count), int(n_src), tuple(nn_index.shape))
    hit = _cache.get(key)
    if hit is not None:
        _cache.move_to_end(key)
        out, _keep, ev, synced = hit
        if cur_raw not in synced:
            cur = torch.cuda.current_stream()
            cur.wait_event(ev)
            for t in out:
                t.record_stream(cur)
            synced.add(cur_raw)
        return out
    cur = torch.cuda.current_stream()
    B, M, K = nn_index.shape
    dev = nn_index.device
    offsets = _lib.empty((B * (n_src + 1),), torch.int32, dev)
    ent_edge = _lib.empty((B * M * K,), torch.int32, dev)
    l = _lib.lib()
    wsb = l.sph3d_graph_transpose_workspace(B, n_src, M, K, 1)
    if counted_workspace is None:
        counted_workspace = torch.empty((max(wsb, 1),), dtype=torch.uint8, device=dev)
        _lib.check(l.sph3d_graph_transpose_count(B, n_src, M, K, 1, _lib.ptr(nn_index), _lib.ptr(nn_count), None, 0,
                                                 _lib.ptr(counted_workspace), wsb, _lib.stream_ptr()))
    _lib.check(l.sph3d_graph_transpose_finish_edges(B, n_src, M, K, _lib.ptr(nn_index), _lib.ptr(nn_count), _lib.ptr(offsets),
                                                    _lib.ptr(ent_edge), _lib.ptr(counted_workspace), wsb, _lib.stream_ptr()))
    out = (offsets, ent_edge)
    ev = torch.cuda.Event()
    ev.record(cur)
    _cache[key] = (out, (nn_index, nn_count), ev, {cur_raw})
    while len(_cache) > _MAX_ENTRIES:
        _unique.discard(_cache.popitem(last=False)[0])
    return out
