"""The transposed neighbour graph (csrc/graph.hip) against its numpy statement (tests/_tgraph_ref.py), at every build form.

Every gradient of the path gathers over this structure; the older tests compare one device build of it with another, and both
sides share the scan and the fill pass.  Here each case restates the rule that puts it on its form as an assertion (the _plan,
_zero_fill_form and _packable functions are the launcher's rules, copied from common.hpp and graph.hip), calls the C ABI on
outputs pre-filled with sentinels and a workspace pre-filled with 0xFF bytes, and compares offsets, the active-bin list and the
balanced order with assert_array_equal and the entries as sorted (segment, row, factor bits) triples: integers and float bit
patterns only, no tolerance.  What the header leaves open is asserted as the kernels have it: the words of a cloud's entry slab
behind offsets[b, L] and of active_bins behind 1 + count are not written."""
import numpy as np
import pytest
import torch

from _tgraph_ref import balanced_order_reference, device_entries, spatial_order_keys, transpose_reference
from sph3d_gcn_amd import _lib, _tgraph, tf_nnquery

pytestmark = pytest.mark.gpu

KEY_SENTINEL, NAN_BITS, EINVAL = 0x7f7f7f7f, 0x7fc00000, -1
P, S = _lib.ptr, _lib.stream_ptr


# ---- the launcher's rules -----------------------------------------------------------------------------------------------------------
def _plan(B, N, M, K, F):
    """common.hpp: tg_ws -> (L, chunks of the scan, words of the one zero fill, words of the workspace)"""
    L = N * F
    chunks = (L + 2047) // 2048
    head = (B * L + F + 1) & ~1
    zero_words = head + 2 * B * chunks
    return L, chunks, zero_words, zero_words + B * M * K


def _zero_fill_form(address, zero_words):
    """graph.hip: zero_async -> None (the runtime's memset, under 256 KiB) or zero_fill_kernel's (head words, tail words)"""
    if 4 * zero_words < (256 << 10):
        return None
    head = ((16 - (address & 15)) & 15) >> 2
    return head, (zero_words - head) % 4


def _packable(M, K, weight):
    """common.hpp: tg_packable"""
    return weight is None and M <= (1 << 24) and K <= 255


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _fresh_transposes():
    _tgraph.clear()
    yield
    _tgraph.clear()


def _t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to(dev) if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype, device=dev)


def _n(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Graph:
    """a neighbour graph on the host and on the device, with the statement of its transposed graph (computed once per form)"""

    def __init__(self, dev, idx, cnt, n_src, bins=None, F=1, weight=None):
        self.dev, self.idx, self.cnt, self.n_src, self.bins, self.w = dev, idx, cnt, n_src, bins, weight
        self.B, self.M, self.K = idx.shape
        self.F = F if bins is not None else 1
        self.it, self.ct = _t(idx, dev), _t(cnt, dev)
        self.bt = None if bins is None else _t(bins, dev)
        self.wt = None if weight is None else _t(weight, dev)
        self._ref = {}
        assert _plan(self.B, n_src, self.M, self.K, self.F)[3] * 4 == self.workspace_bytes()

    def workspace_bytes(self):
        return _lib.lib().sph3d_graph_transpose_workspace(self.B, self.n_src, self.M, self.K, self.F)

    def ref(self, weighted=False):
        if weighted not in self._ref:
            self._ref[weighted] = transpose_reference(self.idx, self.cnt, self.n_src, self.bins, self.F,
                                                      self.w if weighted else None)
        return self._ref[weighted]

    def in_degree(self):
        o = self.ref()[0].astype(np.int64).reshape(self.B, -1)
        return o[:, self.F::self.F] - o[:, :-1:self.F]


def _draw(dev, seed, B, n_src, M, K, F=1, bins_from=None, hub=False, high_from=None, skip_sources=True):
    """ids in range (repeats inside a row allowed), ragged counts with rows of 0 and of K, slots past the count holding ids and
    bins that would count if they were read, every seventh source without in-edge, with `hub` one source that most rows list"""
    rng = np.random.RandomState(seed)
    sources = np.arange(n_src)
    if skip_sources and n_src >= 8:
        sources = sources[sources % 7 != 3]
    idx = sources[rng.randint(0, sources.size, size=(B, M, K))].astype(np.int32)
    cnt = rng.randint(0, K + 1, size=(B, M)).astype(np.int32)
    if high_from is not None:
        cnt[:, ::2] = rng.randint(high_from, K + 1, size=cnt[:, ::2].shape)
    cnt[:, 1::6] = 0
    cnt[:, 2::6] = K
    if hub:
        idx[:, rng.rand(M) < 0.8, 0] = sources[-1]
    bins = None
    if F > 1 or bins_from is not None:
        pool = np.arange(F) if bins_from is None else np.asarray(bins_from)
        bins = pool[rng.randint(0, pool.size, size=(B, M, K))].astype(np.int32)
    w = (rng.rand(B, M, K) + 0.05).astype(np.float32)
    g = Graph(dev, idx, cnt, n_src, bins, F, w)
    if M:
        deg = g.in_degree()
        assert (cnt == 0).any() and (cnt == K).any() and (not skip_sources or (deg == 0).any())
        assert not hub or deg.max() >= M // 3
    return g


# ---- calls ------------------------------------------------------------------------------------------------------------------------
class Out:
    """the outputs of one build, pre-filled: offsets and ent_key 0x7f7f7f7f, ent_scale a NaN, active_bins and order -1"""

    def __init__(self, g, form, active, order=False):
        n_ent = max(g.B * g.M * g.K, 16)
        full = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=g.dev)
        self.form = form
        self.off = full(g.B * (g.n_src * g.F + 1), KEY_SENTINEL)
        self.key = full(n_ent, KEY_SENTINEL)
        self.scale = None if form == "packed" else full(n_ent, NAN_BITS).view(torch.float32)
        self.act = full(g.F + 1, -1) if active else None
        self.order = full(g.B * g.n_src, -1) if order else None

    def host(self):
        for name in ("off", "key", "scale", "act", "order"):
            t = getattr(self, name)
            setattr(self, name, None if t is None else _n(t))
        return self

    def untouched(self):
        return ((self.off == KEY_SENTINEL).all() and (self.key == KEY_SENTINEL).all()
                and (self.scale is None or (_bits(self.scale) == NAN_BITS).all())
                and (self.act is None or (self.act == -1).all()) and (self.order is None or (self.order == -1).all()))


def _workspace(g, shift=0):
    """-> (tensor of 0xFF bytes, address inside it, bytes): the address is `shift` bytes behind a 256-byte boundary"""
    nbytes = g.workspace_bytes()
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=g.dev)
    assert ws.data_ptr() % 256 == 0
    return ws, ws.data_ptr() + shift, nbytes


def _build(g, form="arrays", split=False, active=None, order=False, ws=None):
    """one build through the C ABI -> (status, Out on the host).  form: "arrays" (ent_key + ent_scale), "packed" (ent_scale NULL),
    "weighted" (ent_scale = the weights); split: sph3d_graph_transpose_count, then _finish[_ordered], on one workspace"""
    l = _lib.lib()
    active = (g.bins is not None) if active is None else active
    out = Out(g, form, active, order)
    keep, address, nbytes = ws if ws is not None else _workspace(g)
    dims = (g.B, g.n_src, g.M, g.K, g.F)
    wt = g.wt if form == "weighted" else None
    tail = (P(g.it), P(g.ct), P(g.bt), P(wt), P(out.off), P(out.key), P(out.scale), P(out.act))
    if not split and not order:
        rc = l.sph3d_graph_transpose(*dims, *tail, address, nbytes, S())
    else:
        rc = l.sph3d_graph_transpose_count(*dims, P(g.it), P(g.ct), P(g.bt), 1 if active else 0, address, nbytes, S())
        assert rc == 0, l.sph3d_last_error()
        if order:
            rc = l.sph3d_graph_transpose_finish_ordered(*dims, *tail, P(out.order), address, nbytes, S())
        else:
            rc = l.sph3d_graph_transpose_finish(*dims, *tail, address, nbytes, S())
    torch.cuda.synchronize()
    del keep
    return rc, out.host()


def _assert_equals_statement(g, out, what, sentinels=True):
    B, M, K, L = g.B, g.M, g.K, g.n_src * g.F
    off_ref, ent_ref, act_ref = g.ref(weighted=out.form == "weighted")
    np.testing.assert_array_equal(out.off, off_ref, err_msg=what + ": offsets")
    if sentinels:                                  # behind every cloud's end the slab is as it was
        o = off_ref.astype(np.int64).reshape(B, L + 1)
        behind = np.ones(out.key.size, bool)
        for b in range(B):
            behind[o[b, 0]:o[b, L]] = False
        np.testing.assert_array_equal(out.key[behind], KEY_SENTINEL, err_msg=what + ": ent_key behind a cloud's end")
        if out.scale is not None:
            np.testing.assert_array_equal(_bits(out.scale)[behind], NAN_BITS, err_msg=what + ": ent_scale behind a cloud's end")
    np.testing.assert_array_equal(device_entries(out.off, out.key, out.scale, B, L, M * K), ent_ref, err_msg=what + ": entries")
    if out.act is not None:
        n = 1 + int(act_ref[0])
        np.testing.assert_array_equal(out.act[:n], act_ref, err_msg=what + ": active bins")
        if sentinels:
            np.testing.assert_array_equal(out.act[n:], -1, err_msg=what + ": active_bins behind 1 + count")


def _check(g, what, forms=("arrays",), splits=(False, True), **kw):
    for form in forms:
        assert form != "packed" or _packable(g.M, g.K, None)
        for split in splits:
            rc, out = _build(g, form, split, **kw)
            assert rc == 0, _lib.lib().sph3d_last_error()
            _assert_equals_statement(g, out, "%s, %s, %s" % (what, form, "count + finish" if split else "one call"))
    return out


ALL_FORMS = ("arrays", "packed", "weighted")


# ---- count + scan + fill ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 33])
def test_plain(dev, F):
    B, N, M, K = 3, 77, 50, 8
    g = _draw(dev, 1, B, N, M, K, F)
    L, chunks, zero_words, _ = _plan(B, N, M, K, F)
    assert chunks == {1: 1, 33: 2}[F] and _zero_fill_form(0, zero_words) is None        # (77 * 33 = 2541 counters per cloud)
    _check(g, "plain F=%d" % F, ALL_FORMS)


@pytest.mark.parametrize("N,F,chunks", [(2047, 1, 1), (2048, 1, 1), (2049, 1, 2), (63, 33, 2)])
def test_chunk_edges(dev, N, F, chunks):
    """the scan's last chunk is one counter short of full, full, one counter long, or 31 counters long: off[L] is the last
    thread's running sum, and cloud 1 starts at M * K whatever cloud 0 holds"""
    B, M, K = 2, 300, 8
    g = _draw(dev, 2 + N, B, N, M, K, F)
    L, got_chunks, _, _ = _plan(B, N, M, K, F)
    assert got_chunks == chunks and L % 2048 == {2047: 2047, 2048: 0, 2049: 1, 63: 31}[N]
    off = g.ref()[0].reshape(B, L + 1)
    assert off[0, L] < M * K == off[1, 0] < off[1, L]
    _check(g, "N=%d F=%d" % (N, F), ("arrays", "packed"))


@pytest.mark.parametrize("B,N,M,K,F,chunks", [(2, 4100, 4100, 8, 33, 67), (1, 8200, 8200, 4, 33, 133), (1, 140000, 2000, 16, 1, 69)])
def test_look_back_over_more_than_64_chunks(dev, B, N, M, K, F, chunks):
    """a chunk behind the 65th has more predecessors than one trip of the wave-wide look-back reads"""
    g = _draw(dev, 5, B, N, M, K, F, hub=True)
    L, got_chunks, _, _ = _plan(B, N, M, K, F)
    assert got_chunks == chunks > 65 and L % 2048 != 0
    _check(g, "%d chunks" % chunks, ("packed",))


@pytest.mark.parametrize("K", [70, 200])
def test_fill_loop_with_more_than_64_slots(dev, K):
    B, N, M = 2, 300, 60
    g = _draw(dev, 7, B, N, M, K, F=3, high_from=65)
    assert (g.cnt > 64).any() and (K < 129 or (g.cnt > 128).any())                    # a second (and a third, fourth) lane trip
    _check(g, "K=%d" % K, ALL_FORMS)


def test_entry_forms(dev):
    """separate arrays, packed words (counts up to 255: the word's sign bit) and weights describe one graph; what cannot be
    packed is refused before anything is written"""
    B, N, M, K = 2, 300, 40, 255
    g = _draw(dev, 11, B, N, M, K, F=2, high_from=120)
    assert {127, 128, 255} <= set(g.cnt.ravel().tolist()) or (g.cnt >= 128).sum() >= 10
    assert (g.cnt == 255).any() and _packable(M, K, None)
    out = _check(g, "K=255", ("arrays", "weighted", "packed"))
    live = out.key[:int(out.off[N * 2])]
    assert (live < 0).any() and (live >= 0).any()                                       # words with and without bit 31
    # packed with a weight: not packable
    assert not _packable(M, K, g.w)
    l = _lib.lib()
    o = Out(g, "packed", True)
    keep, address, nbytes = _workspace(g)
    args = lambda gr, o: (gr.B, gr.n_src, gr.M, gr.K, gr.F, P(gr.it), P(gr.ct), P(gr.bt), P(gr.wt), P(o.off), P(o.key), None, P(o.act))
    assert l.sph3d_graph_transpose(*args(g, o), address, nbytes, S()) == EINVAL
    assert l.sph3d_graph_transpose_finish(*args(g, o), address, nbytes, S()) == EINVAL
    torch.cuda.synchronize()
    assert o.host().untouched()
    # packed with K = 256: the count does not fit the word's eight bits
    g256 = _draw(dev, 13, 1, 40, 10, 256)
    g256.wt = None
    assert not _packable(g256.M, 256, None)
    o = Out(g256, "packed", False)
    keep, address, nbytes = _workspace(g256)
    assert l.sph3d_graph_transpose(*args(g256, o), address, nbytes, S()) == EINVAL
    assert l.sph3d_graph_transpose_finish(*args(g256, o), address, nbytes, S()) == EINVAL
    torch.cuda.synchronize()
    assert o.host().untouched()
    _check(g256, "K=256", ("arrays",))                                                   # with a scale array it is a graph like any other


ACTIVE_CASES = [(33, [0, 4, 9, 17, 32]), (33, list(range(0, 33, 2))), (33, list(range(0, 33, 2)) + [31]), (33, list(range(33))),
                (300, [0, 3, 200, 255, 256, 257, 299])]


@pytest.mark.parametrize("F,occurring", ACTIVE_CASES, ids=["F%d-%dbins" % (F, len(o)) for F, o in ACTIVE_CASES])
def test_active_bins(dev, F, occurring):
    """5, 17, 18 (the two sides of the convolution gradient's compact form) and all 33 bins; with F = 300 the list is made in two
    trips of 256 bins and the second one goes on where the first one stopped"""
    B, N, M, K = 2, 40, 120, 6
    g = _draw(dev, 17, B, N, M, K, F, bins_from=occurring)
    np.testing.assert_array_equal(g.ref()[2], [len(occurring)] + sorted(occurring))
    assert F <= 256 or (min(occurring) < 256 <= max(occurring))
    _check(g, "F=%d, %d bins" % (F, len(occurring)), ("arrays", "packed"))
    # active_bins == NULL with bins given: accepted, the same graph
    _check(g, "F=%d without the list" % F, ("packed",), active=False)


def test_clamped_bins(dev):
    """bin ids outside [0, F - 1] on live edges count for the nearest bin, and the list names the bins they were clamped to"""
    B, N, M, K, F = 2, 40, 120, 6, 9
    g = _draw(dev, 19, B, N, M, K, F, bins_from=[-3, 2, 5, F + 5])
    live = np.arange(K)[None, None, :] < g.cnt[:, :, None]
    assert (g.bins[live] == -3).any() and (g.bins[live] == F + 5).any()
    np.testing.assert_array_equal(g.ref()[2], [4, 0, 2, 5, F - 1])
    _check(g, "clamped bins", ("arrays", "packed"))


def test_repeated_ids_in_a_row(dev):
    B, N, M, K = 2, 5, 30, 12
    g = _draw(dev, 23, B, N, M, K, skip_sources=False)
    g.idx[0, 2] = [4, 4, 1, 4, 1, 0, 4, 4, 4, 4, 4, 4]                                   # count K (every row 2 mod 6)
    g = Graph(dev, g.idx, g.cnt, N, None, 1, g.w)
    assert g.cnt[0, 2] == K
    out = _check(g, "repeated ids", ALL_FORMS)
    lo, hi = int(out.off[4]), int(out.off[5])
    assert int(((out.key[lo:hi] & 0xffffff) == 2).sum()) == 9                              # row 2 names source 4 nine times


def test_no_rows(dev):
    """M = 0: every cloud's slab is empty and starts at 0; nothing but the offsets is written"""
    B, N, K = 2, 50, 4
    g = Graph(dev, np.zeros((B, 0, K), np.int32), np.zeros((B, 0), np.int32), N)
    for form in ("arrays", "packed"):
        for split in (False, True):
            rc, out = _build(g, form, split)
            assert rc == 0, _lib.lib().sph3d_last_error()
            np.testing.assert_array_equal(out.off, np.zeros(B * (N + 1), np.int32))
            out.off[:] = KEY_SENTINEL
            assert out.untouched()


def test_zero_fill_kernel_and_a_reused_workspace(dev):
    """from 256 KiB the counters, bin flags and status words are zeroed by the library's own kernel: 16-byte stores between a
    head and a tail of single words.  The same workspace serves three builds in a row — the graph twice, then another graph
    with fewer bins — without being touched in between: counters, flags and status words of a previous build must not show"""
    B, N, M, K, F = 2, 1000, 300, 8, 33
    g = _draw(dev, 29, B, N, M, K, F)
    g2 = _draw(dev, 31, B, N, M, K, F, bins_from=[1, 7, 30])
    _, _, zero_words, _ = _plan(B, N, M, K, F)
    assert 4 * zero_words >= (256 << 10)
    for shift, form in ((0, (0, 2)), (8, (2, 0))):
        ws = _workspace(g, shift)
        assert _zero_fill_form(ws[1], zero_words) == form
        for graph, what in ((g, "first build"), (g, "second build"), (g2, "another graph")):
            rc, out = _build(graph, "packed", split=shift == 8, ws=ws)
            assert rc == 0, _lib.lib().sph3d_last_error()
            _assert_equals_statement(graph, out, "workspace at +%d, %s" % (shift, what))


# ---- the other producers of the counting phase --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,Sn,K", [(3, 700, 100, 16), (2, 300, 50, 70)])
def test_gather_rows_count(dev, B, N, Sn, K):
    """the pooling graph = rows of a level's graph at the sampled points, copied by the kernel that also counts the in-edges of
    its transposed graph"""
    src = _draw(dev, 37, B, N, N, K, high_from=65 if K > 64 else None)
    rng = np.random.RandomState(41)
    pick = np.stack([rng.permutation(N)[:Sn] for _ in range(B)]).astype(np.int32)
    pairs = np.stack([np.broadcast_to(np.arange(B, dtype=np.int32)[:, None], (B, Sn)), pick], axis=2)
    want_idx = np.stack([src.idx[b, pick[b]] for b in range(B)])
    want_cnt = np.stack([src.cnt[b, pick[b]] for b in range(B)])
    assert (want_cnt == 0).any() and (want_cnt == K).any()
    l, pt = _lib.lib(), _t(pairs, dev)
    full = lambda shape: torch.full(shape, KEY_SENTINEL, dtype=torch.int32, device=dev)
    # copy only
    oi, oc = full((B, Sn, K)), full((B, Sn))
    _lib.check(l.sph3d_gather_rows_count(B, N, Sn, K, P(pt), P(src.it), P(src.ct), P(oi), P(oc), None, 0, S()))
    np.testing.assert_array_equal(_n(oi), want_idx)
    np.testing.assert_array_equal(_n(oc), want_cnt)
    # with the counting phase, finished on the same workspace
    pool = Graph(dev, want_idx, want_cnt, N)
    for form in ("arrays", "packed"):
        oi, oc = full((B, Sn, K)), full((B, Sn))
        keep, address, nbytes = _workspace(pool)
        _lib.check(l.sph3d_gather_rows_count(B, N, Sn, K, P(pt), P(src.it), P(src.ct), P(oi), P(oc), address, nbytes, S()))
        out = Out(pool, form, False)
        _lib.check(l.sph3d_graph_transpose_finish(B, N, Sn, K, 1, P(oi), P(oc), None, None, P(out.off), P(out.key), P(out.scale),
                                                  None, address, nbytes, S()))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_n(oi), want_idx)
        np.testing.assert_array_equal(_n(oc), want_cnt)
        _assert_equals_statement(pool, out.host(), "gather_rows_count K=%d, %s" % (K, form))


def _assert_cached_equals_statement(tg, idx, cnt, n_src, bins, F, what):
    """a transposed graph as _tgraph returns it (torch.empty outputs: what lies behind a cloud's end is not looked at)"""
    g = Graph(idx.device, _n(idx), _n(cnt), n_src, None if bins is None else _n(bins), F)
    out = Out.__new__(Out)
    out.form, out.off, out.key, out.act = "cached", _n(tg[0]), _n(tg[1]), None if tg[3] is None else _n(tg[3])
    out.scale = None if tg[2] is None else _n(tg[2])
    _assert_equals_statement(g, out, what, sentinels=False)
    return g


def _only_cached():
    assert len(_tgraph._cache) == 1
    return next(iter(_tgraph._cache.values()))[0]


def test_fused_search_with_bins(dev):
    B, N, K, kernel = 2, 300, 16, (8, 2, 2)
    xyz = _t(np.random.RandomState(43).rand(B, N, 3).astype(np.float32), dev)
    idx, cnt, _dst, filt = tf_nnquery.build_sphere_graph(xyz, 0.2, K, kernel)
    built = _only_cached()
    tg = _tgraph.transpose(idx, cnt, N, bin_index=filt, num_bins=33)
    assert tg is built                                                                 # the one finished from the search's own counts
    g = _assert_cached_equals_statement(tg, idx, cnt, N, filt, 33, "build_sphere_graph")
    assert np.unique(g.cnt).size > 3 and g.ref()[2][0] > 1


def test_counted_inter_level_search(dev):
    B, N, M, K = 2, 300, 500, 24
    rng = np.random.RandomState(47)
    db, q = _t(rng.rand(B, N, 3).astype(np.float32), dev), _t(rng.rand(B, M, 3).astype(np.float32), dev)
    idx, cnt, _dst = tf_nnquery.build_sphere_neighbor_counted(db, q, 0.15, K)
    built = _only_cached()
    tg = _tgraph.peek(idx, cnt, N)
    assert tg is built
    g = _assert_cached_equals_statement(tg, idx, cnt, N, None, 1, "build_sphere_neighbor_counted")
    assert np.unique(g.cnt).size > 3 and (g.in_degree() > 0).any()


def test_cell_grid_search_with_bins(dev):
    """csrc/nngrid.hip counts the in-edges from inside its own search kernels"""
    B, N, K, kernel = 2, 2048, 16, (8, 2, 2)
    xyz = _t(np.random.RandomState(53).rand(B, N, 3).astype(np.float32), dev)
    before = _lib.lib().sph3d_nngrid_launches()
    idx, cnt, _dst, filt = tf_nnquery.build_sphere_graph(xyz, 0.07, K, kernel)
    assert _lib.lib().sph3d_nngrid_launches() == before + 1
    built = _only_cached()
    tg = _tgraph.transpose(idx, cnt, N, bin_index=filt, num_bins=33)
    assert tg is built
    _assert_cached_equals_statement(tg, idx, cnt, N, filt, 33, "build_sphere_graph over the cell grid")
    # N >= _tgraph.BALANCE_MIN_POINTS: the fill launch wrote the gradient's order as well
    order = _tgraph.source_order(idx)
    assert order is not None
    np.testing.assert_array_equal(_n(order), balanced_order_reference(_n(tg[0]), B, N, 33))


# ---- the balanced order -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 33])
@pytest.mark.parametrize("N", [1500, 2048, 2049, 4097])
def test_balanced_order(dev, N, F):
    """one window short of 2048, one full window, a second window of one source, a third window of one source; in-degrees of a
    few units (many ties, decided by the index) and one hub"""
    B, M, K = 2, N, 4
    g = _draw(dev, 59 + N, B, N, M, K, F, hub=True)
    deg = g.in_degree()
    assert all(np.unique(d).size < 40 for d in deg)
    want = balanced_order_reference(g.ref()[0], B, N, F)
    for b in range(B):
        np.testing.assert_array_equal(np.sort(want[b]), np.arange(N))
    rc, out = _build(g, "packed", order=True)
    assert rc == 0, _lib.lib().sph3d_last_error()
    _assert_equals_statement(g, out, "finish_ordered N=%d F=%d" % (N, F))
    np.testing.assert_array_equal(out.order.reshape(B, N), want)
    # the stand-alone kernel on the same offsets
    off, order = _t(out.off, dev), torch.full((B * N,), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().sph3d_graph_balanced_order(B, N, F, P(off), P(order), S()))
    np.testing.assert_array_equal(_n(order).reshape(B, N), want)


def test_balanced_order_caps_the_degree(dev):
    """in-degrees of 2^20 + 5 and 2^20 + 1 both count as 2^20 (the key keeps 11 bits for the index): the index decides"""
    big = 1 << 20
    B, N, K, M = 1, 4, 1, 2 * big + 8
    idx = np.concatenate([np.zeros(big + 5, np.int32), np.full(big + 1, 2, np.int32), np.full(2, 3, np.int32)]).reshape(B, M, K)
    g = Graph(dev, idx, np.ones((B, M), np.int32), N)
    deg = np.bincount(idx.ravel(), minlength=N)
    np.testing.assert_array_equal(deg, [big + 5, 0, big + 1, 2])
    want = balanced_order_reference(np.concatenate([[0], np.cumsum(deg)]), B, N, 1)
    np.testing.assert_array_equal(want, [[2, 0, 3, 1]])                                # (uncapped: 0, 2, 3, 1)
    rc, out = _build(g, "packed", order=True)
    assert rc == 0, _lib.lib().sph3d_last_error()
    _assert_equals_statement(g, out, "2 M rows on two sources")
    np.testing.assert_array_equal(out.order.reshape(B, N), want)


# ---- the spatial order --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 1023, 1024, 1025, 5000])
def test_spatial_order(dev, N):
    """a counting sort by the Morton code of the point's cell: every cloud's order is a permutation along which the codes do not
    decrease; 16 cells per axis up to 1024 points, 32 from 1025; a cloud of equal points has one cell"""
    B = 3
    rng = np.random.RandomState(61 + N)
    xyz = (rng.rand(B, N, 3) * [2.0, 1.0, 0.5] - 0.3).astype(np.float32)
    xyz[1] = xyz[1, 0]                                                                  # no extent
    xyz[2, :, 2] = 0.25                                                                 # a plane
    keys = spatial_order_keys(xyz, N)
    assert (keys[1] == 0).all() and (N < 1000 or (np.unique(keys[0]).size > 200 and (keys[0].max() >= (1 << 12)) == (N > 1024)))
    xt, seqs = _t(xyz, dev), []
    for _ in range(2):
        order = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().sph3d_spatial_order(B, N, P(xt), P(order), S()))
        order = _n(order)
        for b in range(B):
            np.testing.assert_array_equal(np.sort(order[b]), np.arange(N))
        seqs.append(np.take_along_axis(keys, order.astype(np.int64), axis=1))
        assert (np.diff(seqs[-1], axis=1) >= 0).all()
    np.testing.assert_array_equal(seqs[0], seqs[1])


# ---- the cache ----------------------------------------------------------------------------------------------------------------------
def test_cache_follows_in_place_edits_clear_and_the_packing_switch(dev):
    B, N, M, K, F = 2, 60, 80, 6, 5
    g = _draw(dev, 67, B, N, M, K, F)
    call = lambda: _tgraph.transpose(g.it, g.ct, N, bin_index=g.bt, num_bins=F)
    old = _tgraph.PACK_ENTRIES
    try:
        _tgraph.PACK_ENTRIES = True
        tg = call()
        assert tg[2] is None and call() is tg
        _assert_cached_equals_statement(tg, g.it, g.ct, N, g.bt, F, "first build")
        g.ct.copy_(torch.roll(g.ct, 1, dims=1))                                         # other counts in the same storage
        assert not np.array_equal(_n(g.ct), g.cnt)
        tg2 = call()
        assert tg2 is not tg
        _assert_cached_equals_statement(tg2, g.it, g.ct, N, g.bt, F, "after an in-place edit of nn_count")
        _tgraph.clear()
        tg3 = call()
        assert tg3 is not tg2 and tg3[0] is not tg2[0]
        _assert_cached_equals_statement(tg3, g.it, g.ct, N, g.bt, F, "after clear()")
        _tgraph.clear()
        _tgraph.PACK_ENTRIES = False
        tg4 = call()
        assert tg4[2] is not None
        _assert_cached_equals_statement(tg4, g.it, g.ct, N, g.bt, F, "PACK_ENTRIES = False")
    finally:
        _tgraph.PACK_ENTRIES = old
        _tgraph.clear()
