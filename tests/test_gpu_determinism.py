"""Deterministic mode on the device: the canonical-order pass against its numpy statement (tests/_det_ref.py) on
host-shuffled graphs and behind every build form of the transposed graph, gradients that repeat bit for bit over rebuilt graphs,
the entries that refuse, and a Trainer whose runs from one seed — a resumed one included — end with the same bits.

Every comparison of integers and bit patterns is exact.  The switch is off after every test (the fixture below)."""
import numpy as np
import pytest
import torch

import _det_ref as D
from _conv_forms import bwd_layout, cat_ok, grad_form
from _conv_ref import assert_conv, conv_grad_ref
from _pool_ref import assert_sum, make_graph, scatter_ref
from _tgraph_ref import balanced_order_reference, transpose_reference
import sph3d_gcn_amd as pkg
from sph3d_gcn_amd import _lib, _tgraph, tf_conv3d, tf_nnquery, tf_pool3d, tf_unpool3d
from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd.harness import feed, optim, s3dis_net, train

pytestmark = pytest.mark.gpu

FILL, EUNSUPPORTED = 0x7f7f7f7f, -4
P, S = _lib.ptr, _lib.stream_ptr
WINDOW = 64          # graph.hip: tg_canonical_order ranks a window of 64 entries in registers; longer segments go in strips of 64


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    pkg.set_deterministic(False)
    _tgraph.clear()
    yield
    pkg.set_deterministic(False)
    _tgraph.clear()
    assert _lib.lib().sph3d_get_deterministic() == 0


def _t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to(dev) if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype, device=dev)


def _n(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _n(t.contiguous()).view(np.int32)


# ---- graphs on the host ---------------------------------------------------------------------------------------------------------------
class HostGraph:
    def __init__(self, idx, cnt, n_src, bins=None, F=1, weight=None):
        self.idx, self.cnt, self.n_src, self.bins, self.w = idx, cnt, n_src, bins, weight
        self.B, self.M, self.K = idx.shape
        self.F = F if bins is not None else 1
        self.L = n_src * self.F
        self._ref = {}

    def ref(self, weighted=False):
        if weighted not in self._ref:
            self._ref[weighted] = transpose_reference(self.idx, self.cnt, self.n_src, self.bins, self.F, self.w if weighted else None)
        return self._ref[weighted]

    def canonical(self, form):
        """-> (offsets, key int32, scale bits uint32 | None, active): the numpy canonical arrays of one entry form"""
        off, ent, act = self.ref(form == "weighted")
        key, sb = D.arrays_from_reference(off, ent, self.cnt, self.B, self.M, self.K, self.L, form == "packed", FILL)
        return off, key, sb, act

    def sizes(self):
        off = self.ref()[0].astype(np.int64).reshape(self.B, self.L + 1)
        return np.diff(off, axis=1)


def _draw(seed, B, n_src, M, K, F=1, high_from=None):
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, n_src, size=(B, M, K)).astype(np.int32)
    cnt = rng.randint(0, K + 1, size=(B, M)).astype(np.int32)
    if high_from is not None:
        cnt = rng.randint(high_from, K + 1, size=(B, M)).astype(np.int32)
    else:
        cnt[:, 1::6] = 0
        cnt[:, 2::6] = K
    bins = rng.randint(0, F, size=(B, M, K)).astype(np.int32) if F > 1 else None
    w = (rng.rand(B, M, K) + 0.05).astype(np.float32)
    return HostGraph(idx, cnt, n_src, bins, F, w)


def _canonical_order_call(g, dev, off, key, sb):
    """sph3d_graph_canonical_order on device copies, workspace pre-filled with 0xFF -> (status, key, scale bits | None) on the host"""
    l = _lib.lib()
    need = l.sph3d_graph_canonical_order_workspace(g.B, g.n_src, g.M, g.K, g.F)
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=dev)
    ot, kt = _t(off, dev), _t(key, dev)
    st = None if sb is None else _t(sb.view(np.int32), dev)
    rc = l.sph3d_graph_canonical_order(g.B, g.n_src, g.M, g.K, g.F, P(ot), P(kt), None if st is None else P(st), P(ws), need, S())
    torch.cuda.synchronize()
    return rc, _n(kt), None if st is None else _n(st).view(np.uint32)


def _pass_on_shuffled(g, dev, form, seed, what):
    off, key, sb, _ = g.canonical(form)
    rng = np.random.RandomState(seed)
    ks, ss = D.shuffle_segments(off, key, sb, g.B, g.L, rng)
    assert (ks != key).any() or (ss is not None and (ss != sb).any()), what + ": the shuffle moved nothing"
    rc, kd, sd = _canonical_order_call(g, dev, off, ks, ss)
    assert rc == 0, _lib.lib().sph3d_last_error()
    np.testing.assert_array_equal(kd, key, err_msg=what + ": ent_key")          # (the sentinels outside the segments included)
    if sb is not None:
        np.testing.assert_array_equal(sd, sb, err_msg=what + ": ent_scale bits")
    # the pass on its own output changes nothing
    rc, kd2, sd2 = _canonical_order_call(g, dev, off, kd, sd)
    assert rc == 0
    np.testing.assert_array_equal(kd2, key, err_msg=what + ": second pass")
    if sb is not None:
        np.testing.assert_array_equal(sd2, sb, err_msg=what + ": second pass, scale bits")


# ---- 1. the pass alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 17])
def test_pass_on_shuffled_packed_graph(dev, F):
    """F = 1: segments of ~48 entries, some longer than a window; F = 17: many short segments per window, empty ones among them"""
    g = _draw(3 + F, 2, 50, 300, 16, F)
    sizes = g.sizes()
    assert (sizes == 0).any() or F == 1
    assert (sizes.max() > WINDOW) == (F == 1) and (sizes > 1).sum() > 40
    _pass_on_shuffled(g, dev, "packed", 5, "packed F=%d" % F)
    _pass_on_shuffled(g, dev, "arrays", 6, "arrays F=%d" % F)


def test_pass_on_weighted_graph_with_repeats_and_special_factors(dev):
    g = _draw(7, 2, 9, 60, 12, F=3)
    g.idx[0, 2, :] = 4                                                  # row 2 (count K) names source 4 in every slot, in one bin
    g.bins[0, 2, :] = 1
    g.idx[1, 8, :] = [4, 4, 1, 4, 1, 0, 4, 4, 4, 4, 4, 4]
    wb = D.fbits(g.w).reshape(g.w.shape)
    wb[0, 2, :7] = [0x80000000, 0x7fc00000, 0x00000000, 0xffc00001, 0x3f800000, 0x80000000, 0x7fc00000]
    wb[0, 2, 7:] = wb[0, 2, 7]                                          # and five entries that tie on both fields
    g = HostGraph(g.idx, g.cnt, 9, g.bins, 3, wb.view(np.float32))
    assert g.cnt[0, 2] == 12 and g.cnt[1, 8] == 12
    off, key, sb, _ = g.canonical("weighted")
    lo, hi = int(off[4 * 3 + 1]), int(off[4 * 3 + 2])
    seg_bits = sb[lo:hi][key[lo:hi] == 2].tolist()
    assert len(seg_bits) == 12 and seg_bits == sorted(seg_bits) and seg_bits.count(0x80000000) == 2 and seg_bits[-1] == 0xffc00001
    for form, seed in (("weighted", 11), ("arrays", 12), ("packed", 13)):
        _pass_on_shuffled(g, dev, form, seed, form + " with repeated ids")


@pytest.mark.parametrize("form", ["packed", "arrays"])
def test_pass_on_a_star(dev, form):
    """every row names source 0 in bin 1, plus three random sources: one segment of 5000 entries — 79 strips of 64, far above the
    64-entry window that the kernel holds in registers (it has no other size: no LDS, the staging words are the workspace)"""
    B, N, M, K, F = 1, 200, 5000, 4, 3
    rng = np.random.RandomState(17)
    idx = rng.randint(1, N, size=(B, M, K)).astype(np.int32)
    idx[:, :, 0] = 0
    bins = rng.randint(0, F, size=(B, M, K)).astype(np.int32)
    bins[:, :, 0] = 1
    g = HostGraph(idx, np.full((B, M), K, np.int32), N, bins, F, (rng.rand(B, M, K) + 0.05).astype(np.float32))
    sizes = g.sizes()
    assert sizes[0, 1] == M > 64 * WINDOW and sizes[0, 0] == 0 and sizes[0, 2] == 0
    _pass_on_shuffled(g, dev, form, 19, "star, " + form)


def test_pass_with_an_empty_cloud(dev):
    g = _draw(23, 3, 40, 100, 8, F=5)
    g.cnt[1] = 0
    g = HostGraph(g.idx, g.cnt, 40, g.bins, 5, g.w)
    off = g.ref()[0].reshape(3, -1)
    assert off[1, 0] == off[1, -1] == 100 * 8 and off[2, -1] > off[2, 0]
    _pass_on_shuffled(g, dev, "packed", 29, "cloud 1 empty, packed")
    _pass_on_shuffled(g, dev, "weighted", 31, "cloud 1 empty, weighted")


def test_pass_with_counts_that_reach_bit_31(dev):
    g = _draw(37, 2, 300, 40, 255, F=2, high_from=128)
    assert g.cnt.min() >= 128 and (g.cnt == 255).any()
    off, key, _sb, _ = g.canonical("packed")
    assert (key[:int(off[g.L])] < 0).all()                                # every live word has bit 31 set
    _pass_on_shuffled(g, dev, "packed", 41, "K=255")


# ---- 2. every build form, mode on -------------------------------------------------------------------------------------------------------
class Built:
    pass


def _build(g, dev, form, how):
    """how: "plain" (sph3d_graph_transpose), "split" (count + finish), "ordered" (count + finish_ordered) -> outputs on the host"""
    l = _lib.lib()
    it, ct = _t(g.idx, dev), _t(g.cnt, dev)
    bt = None if g.bins is None else _t(g.bins, dev)
    wt = _t(g.w, dev) if form == "weighted" else None
    n_ent = max(g.B * g.M * g.K, 16)
    full = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=dev)
    off, key = full(g.B * (g.L + 1), FILL), full(n_ent, FILL)
    scale = None if form == "packed" else full(n_ent, FILL)
    act = full(g.F + 1, -1) if g.bins is not None else None
    order = full(g.B * g.n_src, -1) if how == "ordered" else None
    nbytes = l.sph3d_graph_transpose_workspace(g.B, g.n_src, g.M, g.K, g.F)
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=dev)
    dims = (g.B, g.n_src, g.M, g.K, g.F)
    tail = (P(it), P(ct), P(bt), P(wt), P(off), P(key), P(scale), P(act))
    if how == "plain":
        _lib.check(l.sph3d_graph_transpose(*dims, *tail, P(ws), nbytes, S()))
    else:
        _lib.check(l.sph3d_graph_transpose_count(*dims, P(it), P(ct), P(bt), 1 if act is not None else 0, P(ws), nbytes, S()))
        if how == "ordered":
            _lib.check(l.sph3d_graph_transpose_finish_ordered(*dims, *tail, P(order), P(ws), nbytes, S()))
        else:
            _lib.check(l.sph3d_graph_transpose_finish(*dims, *tail, P(ws), nbytes, S()))
    torch.cuda.synchronize()
    out = Built()
    out.off, out.key = _n(off), _n(key)
    out.scale = None if scale is None else _n(scale).view(np.uint32)
    out.act = None if act is None else _n(act)
    out.order = None if order is None else _n(order)
    return out


def _assert_canonical(g, out, form, what, sentinels=True):
    off, key, sb, act = g.canonical(form)
    np.testing.assert_array_equal(out.off, off, err_msg=what + ": offsets")
    if sentinels:
        np.testing.assert_array_equal(out.key, key, err_msg=what + ": ent_key in device order")
        if sb is not None:
            np.testing.assert_array_equal(out.scale, sb, err_msg=what + ": ent_scale bits in device order")
    else:                                                               # torch.empty outputs: only the entries are defined
        pos, _seg = D.segment_positions(off, g.B, g.L)
        np.testing.assert_array_equal(out.key.reshape(-1)[pos], key[pos], err_msg=what + ": ent_key in device order")
        if sb is not None:
            np.testing.assert_array_equal(out.scale.reshape(-1)[pos], sb[pos], err_msg=what + ": ent_scale bits in device order")
    if out.act is not None:
        np.testing.assert_array_equal(out.act[:1 + int(act[0])], act, err_msg=what + ": active bins")


@pytest.mark.parametrize("how", ["plain", "split", "ordered"])
def test_build_forms_leave_canonical_entries(dev, how):
    cases = [("F=1", _draw(43, 3, 77, 50, 8)), ("F=33", _draw(47, 3, 77, 50, 8, 33)), ("long segments", _draw(53, 2, 6, 400, 8, 2)),
             ("K=200", _draw(59, 2, 300, 60, 200, 3, high_from=65))]
    assert cases[2][1].sizes().max() > 2 * WINDOW
    off_words = {}
    for name, g in cases:
        off_words[name] = _lib.lib().sph3d_graph_transpose_workspace(g.B, g.n_src, g.M, g.K, g.F)
    with pkg.deterministic():
        for name, g in cases:
            assert (_lib.lib().sph3d_graph_transpose_workspace(g.B, g.n_src, g.M, g.K, g.F)
                    == off_words[name] + 4 * g.B * g.M * g.K)
            for form in ("arrays", "packed", "weighted"):
                out = _build(g, dev, form, how)
                _assert_canonical(g, out, form, "%s, %s, %s" % (how, name, form))


@pytest.mark.parametrize("N,F", [(1500, 1), (2049, 33)])
def test_finish_ordered_writes_the_balanced_order_as_before(dev, N, F):
    g = _draw(61 + N, 2, N, N, 4, F)
    with pkg.deterministic():
        out = _build(g, dev, "packed", "ordered")
    _assert_canonical(g, out, "packed", "finish_ordered N=%d" % N)
    np.testing.assert_array_equal(out.order.reshape(2, N), balanced_order_reference(g.ref()[0], 2, N, F))


def _cached_as_built(tg):
    out = Built()
    out.off, out.key = _n(tg[0]), _n(tg[1])
    out.scale = None if tg[2] is None else _n(tg[2]).view(np.uint32)
    out.act = None if tg[3] is None else _n(tg[3])
    return out


def _only_cached():
    assert len(_tgraph._cache) == 1
    return next(iter(_tgraph._cache.values()))[0]


@pytest.mark.parametrize("N,radius", [(300, 0.2), (2048, 0.07)], ids=["wave-per-query search", "cell-grid search"])
def test_fused_search_leaves_canonical_entries(dev, N, radius):
    B, K, kernel = 2, 16, (8, 2, 2)
    xyz = _t(np.random.RandomState(67).rand(B, N, 3).astype(np.float32), dev)
    with pkg.deterministic():
        idx, cnt, _dst, filt = tf_nnquery.build_sphere_graph(xyz, radius, K, kernel)
        tg = _only_cached()
        assert _tgraph.transpose(idx, cnt, N, bin_index=filt, num_bins=33) is tg
        order = _tgraph.source_order(idx)                               # (leaving the mode empties the cache, the orders with it)
        torch.cuda.synchronize()
    g = HostGraph(_n(idx), _n(cnt), N, _n(filt), 33)
    assert (g.sizes() > 1).sum() > 100
    _assert_canonical(g, _cached_as_built(tg), "packed", "build_sphere_graph N=%d" % N, sentinels=False)
    if N >= _tgraph.BALANCE_MIN_POINTS:
        np.testing.assert_array_equal(_n(order), balanced_order_reference(_n(tg[0]), B, N, 33))


def test_counted_inter_level_search_leaves_canonical_entries(dev):
    B, N, M, K = 2, 300, 500, 24
    rng = np.random.RandomState(71)
    db, q = _t(rng.rand(B, N, 3).astype(np.float32), dev), _t(rng.rand(B, M, 3).astype(np.float32), dev)
    with pkg.deterministic():
        idx, cnt, _dst = tf_nnquery.build_sphere_neighbor_counted(db, q, 0.15, K)
        tg = _only_cached()
        torch.cuda.synchronize()
    g = HostGraph(_n(idx), _n(cnt), N)
    assert g.sizes().max() > 8
    _assert_canonical(g, _cached_as_built(tg), "packed", "build_sphere_neighbor_counted", sentinels=False)


def test_gather_rows_count_leaves_canonical_entries(dev):
    B, N, Sn, K = 3, 700, 100, 16
    src = _draw(73, B, N, N, K)
    rng = np.random.RandomState(79)
    pick = np.stack([rng.permutation(N)[:Sn] for _ in range(B)]).astype(np.int32)
    pairs = np.stack([np.broadcast_to(np.arange(B, dtype=np.int32)[:, None], (B, Sn)), pick], axis=2)
    pool = HostGraph(np.stack([src.idx[b, pick[b]] for b in range(B)]), np.stack([src.cnt[b, pick[b]] for b in range(B)]), N)
    l = _lib.lib()
    it, ct, pt = _t(src.idx, dev), _t(src.cnt, dev), _t(pairs, dev)
    full = lambda shape: torch.full(shape, FILL, dtype=torch.int32, device=dev)
    with pkg.deterministic():
        for form in ("arrays", "packed"):
            oi, oc = full((B, Sn, K)), full((B, Sn))
            nbytes = l.sph3d_graph_transpose_workspace(B, N, Sn, K, 1)
            ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=dev)
            _lib.check(l.sph3d_gather_rows_count(B, N, Sn, K, P(pt), P(it), P(ct), P(oi), P(oc), P(ws), nbytes, S()))
            off, key = full((B * (N + 1),)), full((B * Sn * K,))
            scale = None if form == "packed" else full((B * Sn * K,))
            _lib.check(l.sph3d_graph_transpose_finish(B, N, Sn, K, 1, P(oi), P(oc), None, None, P(off), P(key), P(scale), None,
                                                      P(ws), nbytes, S()))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_n(oi), pool.idx)
            out = Built()
            out.off, out.key, out.act = _n(off), _n(key), None
            out.scale = None if scale is None else _n(scale).view(np.uint32)
            _assert_canonical(pool, out, form, "gather_rows_count, " + form)
        # and through the package: the cached transposed pooling graph with its unique-rows promise
        oi, oc = s3g_util.gather_pooling_graph(it, ct, pt)
        tg = _tgraph.peek(oi, oc, N, need_unique_rows=True)
        assert tg is not None
        torch.cuda.synchronize()
    _assert_canonical(pool, _cached_as_built(tg), "packed", "gather_pooling_graph", sentinels=False)


# ---- 3 .. 5: gradients ----------------------------------------------------------------------------------------------------------------
N_PTS, K_NN, KERNEL, F_BINS = 4096, 32, (8, 2, 2), 33


@pytest.fixture(scope="module")
def ball(dev):
    """B = 2 clouds of 4096 points and their ball-query graph with 33 bins, built once with the mode off (the tensors are inputs:
    every test rebuilds the transposed graph itself); `bins17` folds the bin ids onto 17 bins (the conv gradient's compact table)"""
    rng = np.random.RandomState(83)
    xyz = _t(rng.rand(2, N_PTS, 3).astype(np.float32), dev)
    idx, cnt, _dst, filt = tf_nnquery.build_sphere_graph(xyz, 0.12, K_NN, KERNEL, with_transpose=False)
    torch.cuda.synchronize()
    b = Built()
    # (a uniform cloud leaves some of the kernel's 33 bins empty: the ids are spread over all of them with the neighbour's id)
    spread = filt + idx
    b.xyz, b.idx, b.cnt, b.bins33, b.bins17 = xyz, idx, cnt, (spread % 33).contiguous(), (spread % 17).contiguous()
    b.h_idx, b.h_cnt = _n(idx), _n(cnt)
    live = np.arange(K_NN)[None, None, :] < b.h_cnt[:, :, None]
    assert len(np.unique(_n(b.bins33)[live])) == 33 and len(np.unique(_n(b.bins17)[live])) == 17
    assert b.h_cnt.min() >= 1 and b.h_cnt.mean() > 12 and (b.h_cnt == K_NN).any()
    return b


def _conv_inputs(dev, seed, C, r):
    rng = np.random.RandomState(seed)
    x = _t(rng.randn(2, N_PTS, C).astype(np.float32), dev)
    w = _t(rng.randn(F_BINS, C, r).astype(np.float32), dev)
    go = _t(rng.randn(2, N_PTS, C * r).astype(np.float32), dev)
    return x, w, go


def _conv_grad(ball, bins, x, w, go, cat=None):
    if cat is not None:
        ga, gb, gf = tf_conv3d._depthwise_conv3d_cat_grad_impl(x[:, :, :cat].contiguous(), x[:, :, cat:].contiguous(), w, go, ball.idx,
                                                               ball.cnt, bins)
        torch.cuda.synchronize()
        return [_bits(ga), _bits(gb), _bits(gf)]
    gi, gf = tf_conv3d.depthwise_conv3d_grad(x, w, go, ball.idx, ball.cnt, bins)
    torch.cuda.synchronize()
    return [_bits(gi), _bits(gf)]


def _repeats(fn, runs=5):
    """fn() after a _tgraph.clear(), `runs` times: every result must have the first one's bits -> the first"""
    first = None
    for i in range(runs):
        _tgraph.clear()
        got = fn()
        assert len(_tgraph._cache) >= 1                                 # the call built its transposed graph
        if first is None:
            first = got
        else:
            for a, b in zip(first, got):
                np.testing.assert_array_equal(a, b, err_msg="run %d differs from run 0" % i)
    return first


CONV_FORMS = [(32, 2, 4, 4), (64, 2, 4, 2), (128, 2, 4, 1), (6, 1, 2, 1)]     # C, r -> V, PARTS


@pytest.mark.parametrize("active", [17, 33])
@pytest.mark.parametrize("C,r,V,parts", CONV_FORMS, ids=["quarter-waves", "half-waves", "four-per-lane", "two-per-lane"])
def test_conv_gradient_repeats_bit_for_bit(dev, ball, C, r, V, parts, active):
    bins = ball.bins17 if active == 17 else ball.bins33
    form = grad_form(2, N_PTS, N_PTS, F_BINS, C, r, True, active)
    assert form["V"] == V and form["PARTS"] == parts and form["compact"] == (V == 4 and active == 17) and not form["hub"]
    x, w, go = _conv_inputs(dev, 89 + C, C, r)
    with pkg.deterministic():
        _repeats(lambda: _conv_grad(ball, bins, x, w, go))


def test_two_input_conv_gradient_repeats_bit_for_bit(dev, ball):
    Ca, Cb, r = 128, 4, 2
    assert cat_ok(F_BINS, Ca, Cb, r)
    x, w, go = _conv_inputs(dev, 97, Ca + Cb, r)
    with pkg.deterministic():
        cat = _repeats(lambda: _conv_grad(ball, ball.bins17, x, w, go, cat=Ca))
        _tgraph.clear()
        one = _conv_grad(ball, ball.bins17, x, w, go)
    np.testing.assert_array_equal(np.concatenate([cat[0], cat[1]], axis=2), one[0])     # the same gradient as of the concatenation
    np.testing.assert_array_equal(cat[2], one[1])


def test_packed_and_separate_entries_give_the_same_bits(dev, ball):
    C, r = 64, 2
    x, w, go = _conv_inputs(dev, 101, C, r)
    old = _tgraph.PACK_ENTRIES
    got = {}
    try:
        with pkg.deterministic():
            for pack in (True, False):
                _tgraph.PACK_ENTRIES = pack
                _tgraph.clear()
                got[pack] = _conv_grad(ball, ball.bins33, x, w, go)
                tg = _only_cached()
                assert (tg[2] is None) == pack
    finally:
        _tgraph.PACK_ENTRIES = old
    np.testing.assert_array_equal(got[True][0], got[False][0], err_msg="grad_input")
    np.testing.assert_array_equal(got[True][1], got[False][1], err_msg="grad_filter")


def test_conv_gradient_in_the_mode_holds_its_float64_bound(dev, ball):
    """the mode must not cost accuracy: the half-wave form at 33 bins under tests/_conv_ref.py's derived per-element bound"""
    C, r = 64, 2
    x, w, go = _conv_inputs(dev, 103, C, r)
    with pkg.deterministic():
        _tgraph.clear()
        gi, gf = tf_conv3d.depthwise_conv3d_grad(x, w, go, ball.idx, ball.cnt, ball.bins33)
        torch.cuda.synchronize()
    form = grad_form(2, N_PTS, N_PTS, F_BINS, C, r, True, 33)
    ref = conv_grad_ref(_n(x), _n(w), _n(go), ball.h_idx, ball.h_cnt, _n(ball.bins33))
    assert_conv(_n(gi), ref.gi, ref.gi_mag, ref.gi_terms(r), "[%s] deterministic: grad_input" % form["tag"])
    assert_conv(_n(gf), ref.gf, ref.gf_mag, ref.gf_terms(form["depth"]), "[%s] deterministic: grad_filter" % form["tag"])


def _pool_graph(dev, ball, S_pts=1024):
    """the pooling graph of the ball graph at S_pts sampled points per cloud, through the package (unique rows promised)"""
    rng = np.random.RandomState(107)
    pick = np.stack([np.sort(rng.permutation(N_PTS)[:S_pts]) for _ in range(2)]).astype(np.int32)
    pairs = np.stack([np.broadcast_to(np.arange(2, dtype=np.int32)[:, None], (2, S_pts)), pick], axis=2)
    return _t(pairs, dev)


def test_pool_and_interpolation_gradients_repeat_bit_for_bit(dev, ball):
    C = 64
    rng = np.random.RandomState(109)
    x = _t(rng.randn(2, N_PTS, C).astype(np.float32), dev)
    go = _t(rng.randn(2, N_PTS, C).astype(np.float32), dev)
    wt = _t((rng.rand(2, N_PTS, K_NN) + 0.05).astype(np.float32), dev)

    def sync(t):
        torch.cuda.synchronize()
        return [_bits(t)]
    with pkg.deterministic():
        avg = _repeats(lambda: sync(tf_pool3d.avg_pool3d_grad(x, go, ball.idx, ball.cnt)))
        _repeats(lambda: sync(tf_unpool3d.mean_interpolate_grad(x, go, ball.idx, ball.cnt)))
        _repeats(lambda: sync(tf_unpool3d.weighted_interpolate_grad(x, go, wt, ball.idx, ball.cnt)))
    # the avg-pool gradient once under tests/_pool_ref.py's bound: the mode must not cost accuracy
    ref, mag, terms = scatter_ref(_n(go), ball.h_idx, ball.h_cnt, N_PTS, mean=True)
    assert_sum(avg[0].view(np.float32), ref, mag, terms, "deterministic avg_pool3d gradient")


@pytest.mark.parametrize("skip", [False, True], ids=["max_pool3d", "max_pool3d_with_skip"])
def test_max_pool_gradient_repeats_bit_for_bit(dev, ball, skip):
    C, S_pts = 64, 1024
    pairs = _pool_graph(dev, ball, S_pts)
    rng = np.random.RandomState(113)
    x0 = _t(np.round(rng.randn(2, N_PTS, C) * 2).astype(np.float32), dev)      # many ties: several rows pick one point
    go = _t(rng.randn(2, S_pts, C).astype(np.float32), dev)
    gs = _t(rng.randn(2, N_PTS, C).astype(np.float32), dev)

    def run():
        pi, pc = s3g_util.gather_pooling_graph(ball.idx, ball.cnt, pairs)
        assert _tgraph.peek(pi, pc, N_PTS, need_unique_rows=True) is not None
        x = x0.clone().requires_grad_(True)
        if skip:
            out, _arg, sk = tf_pool3d.max_pool3d_with_skip(x, pi, pc)
            torch.autograd.backward([out, sk], [go, gs])
        else:
            out, _arg = tf_pool3d.max_pool3d(x, pi, pc)
            out.backward(go)
        torch.cuda.synchronize()
        return [_bits(x.grad)]
    with pkg.deterministic():
        got = _repeats(run)
    assert np.isfinite(got[0].view(np.float32)).all() and got[0].any()


def test_hub_hooks_are_ignored_in_the_mode(dev, ball, monkeypatch):
    """with the hooks the parent's launcher would send this cloud's busy sources through the hub launches (float atomics); in the
    mode the result has the bits of the run without hooks, every time: no hub launch ran"""
    C, r = 128, 2
    x, w, go = _conv_inputs(dev, 127, C, r)
    with pkg.deterministic():
        _tgraph.clear()
        plain = _conv_grad(ball, ball.bins17, x, w, go)
        monkeypatch.setenv("SPH3D_BWD_HUB_MIN_N", "1024")
        monkeypatch.setenv("SPH3D_BWD_HUB_T", "8")
        assert grad_form(2, N_PTS, N_PTS, F_BINS, C, r, True, 17)["hub"]       # what the hooks mean with the mode off
        deg = np.bincount(ball.h_idx[0][np.arange(K_NN)[None, :] < ball.h_cnt[0][:, None]], minlength=N_PTS)
        assert (deg > 8).sum() > 1000                                           # and there are sources above the threshold
        hooked = _repeats(lambda: _conv_grad(ball, ball.bins17, x, w, go), runs=3)
    np.testing.assert_array_equal(hooked[0], plain[0], err_msg="grad_input")
    np.testing.assert_array_equal(hooked[1], plain[1], err_msg="grad_filter")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_entries_that_need_float_atomics_refuse_in_the_mode(dev):
    B, N, M, K, F, C, r = 2, 60, 80, 6, 5, 5, 3
    assert (C * r) % 4 != 0 and bwd_layout(B, N, F, C, r)["V"] == 0                  # the generic kernel's shape
    rng = np.random.RandomState(131)
    idx, cnt = make_graph(rng, B, N, M, K)
    it, ct = _t(idx, dev), _t(cnt, dev)
    bt = _t(rng.randint(0, F, size=idx.shape).astype(np.int32), dev)
    x, w = _t(rng.randn(B, N, C).astype(np.float32), dev), _t(rng.randn(F, C, r).astype(np.float32), dev)
    go = _t(rng.randn(B, M, C * r).astype(np.float32), dev)
    pool_go = _t(rng.randn(B, M, C).astype(np.float32), dev)
    l = _lib.lib()

    def wrapper_call():
        need = l.sph3d_depthwise_conv3d_grad_workspace(B, N, M, F, C, r, K)
        ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        gi, gf = torch.empty_like(x), torch.empty_like(w)
        rc = l.sph3d_depthwise_conv3d_grad(B, N, M, F, C, r, K, P(it), P(ct), P(bt), P(x), P(w), P(go), P(gi), P(gf), P(ws), need, S())
        torch.cuda.synchronize()
        return rc

    def max_backward():
        xr = x.clone().requires_grad_(True)
        out, arg = tf_pool3d.max_pool3d(xr, it, ct)
        out.backward(pool_go)
        torch.cuda.synchronize()
        return xr.grad, arg
    # mode off: all three succeed as today
    gi0, gf0 = tf_conv3d.depthwise_conv3d_grad(x, w, go, it, ct, bt)
    assert wrapper_call() == 0
    g0, arg = max_backward()
    assert torch.allclose(tf_pool3d.max_pool3d_grad(x, pool_go, arg), g0, rtol=1e-6, atol=1e-6)       # (the scatter's own order varies)
    assert torch.isfinite(gi0).all() and torch.isfinite(gf0).all()
    with pkg.deterministic():
        with pytest.raises(_lib.Sph3dError) as e:
            tf_conv3d.depthwise_conv3d_grad(x, w, go, it, ct, bt)
        assert "deterministic mode" in str(e.value) and "float atomics" in str(e.value) and "status -4" in str(e.value)
        assert wrapper_call() == EUNSUPPORTED
        text = l.sph3d_last_error().decode()
        assert "deterministic mode" in text and "float atomics" in text
        gi = torch.empty_like(x)
        rc = l.sph3d_max_pool3d_grad(B, N, M, C, P(arg), P(pool_go), P(gi), S())
        assert rc == EUNSUPPORTED
        text = l.sph3d_last_error().decode()
        assert "deterministic mode" in text and "float atomics" in text
        with pytest.raises(RuntimeError, match="unique_rows=True"):
            max_backward()
        # with the promised transposed graph the same backward is the gather, and equals the scatter's sums here (unique rows)
        _tgraph.transpose(it, ct, N, unique_rows=True)
        g1, _ = max_backward()
    # one term per (row, channel) and at most a few rows per point: the two orders agree to the last bits
    assert torch.allclose(g1, g0, rtol=1e-6, atol=1e-6)


# ---- 7. the Trainer -------------------------------------------------------------------------------------------------------------------
T_PTS, BATCH, SEED = 1024, 3, 21


def _pool(dev):
    rng = np.random.RandomState(3)
    blocks = []
    for n in (1500, 1024, 900, 2000, 3000, 1100, 1300, 700, 2500):
        b = np.empty((n, 8), np.float32)
        b[:, 0:3] = rng.rand(n, 3) * np.array([1.0, 1.0, 1.5])
        b[:, 3:6] = rng.rand(n, 3)
        b[:, 6] = rng.randint(0, 13, n)
        b[:, 7] = rng.randint(0, 2, n)
        blocks.append(b)
    return feed.BlockPool.from_blocks(blocks, dev)


def _trainer(pool, dev, deterministic=True):
    model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(T_PTS), device=dev, seed=3)
    prime = feed.assemble(pool.rows, pool.offsets, torch.from_numpy(np.asarray([0, 1, 2], np.int32)).to(dev), T_PTS, SEED, 0, True)
    return train.Trainer(model, model.loss, lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4),
                         train.Schedule(1e-3, BATCH, decay_step=9, decay_rate=0.7), 13, prime=prime, seed=SEED, log=lambda s: None,
                         log_every=3, deterministic=deterministic)


def _snapshot(tr):
    torch.cuda.synchronize()
    s = {"flat_param": tr.flat.flat_param.detach().clone(), "opt.m": tr.opt.m.clone(), "opt.v": tr.opt.v.clone()}
    for k, v in tr.model.state_dict().items():
        if "moving" in k:
            s[k] = v.detach().clone()
    return s


def _first_difference(a, b):
    assert set(a) == set(b)
    for k in a:
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            return k
    return None


def _run(pool, dev, ckpt=None):
    """two epochs of three batches -> the state after every step (six snapshots); ckpt: a checkpoint is written after epoch 0"""
    tr = _trainer(pool, dev)
    states = []
    for epoch in range(2):
        f = feed.DeviceFeed(pool, BATCH, T_PTS, seed=SEED, augment=True)
        f.epoch = epoch
        for item in f:
            tr.train_step(item, f)
            states.append(_snapshot(tr))
        tr.epoch = epoch
        if ckpt is not None and epoch == 0:
            tr.save(ckpt)
    assert tr.global_step == 6 and not pkg.is_deterministic()
    return states


def test_trainer_runs_from_one_seed_end_with_the_same_bits(dev, tmp_path):
    pool = _pool(dev)
    ckpt = str(tmp_path)
    a = _run(pool, dev, ckpt)
    b = _run(pool, dev)
    assert any("moving_mean" in k for k in a[-1]) and any("moving_variance" in k for k in a[-1])
    assert not torch.equal(a[0]["flat_param"], a[-1]["flat_param"]) and torch.isfinite(a[-1]["flat_param"]).all()
    for step, (sa, sb) in enumerate(zip(a, b)):
        assert _first_difference(sa, sb) is None, "two fresh runs differ after step %d in %s" % (step, _first_difference(sa, sb))
    # the resumed run: the checkpoint written after three steps, then fit() to the end of epoch 1
    tr = _trainer(pool, dev)
    tr.load(train.latest_checkpoint(ckpt))
    assert tr.global_step == 3 and _first_difference(_snapshot(tr), a[2]) is None
    tr.fit(lambda epoch: feed.DeviceFeed(pool, BATCH, T_PTS, seed=SEED, augment=True), 2)
    assert tr.global_step == 6 and not pkg.is_deterministic()
    assert _first_difference(_snapshot(tr), a[-1]) is None, "the resumed run differs in %s" % _first_difference(_snapshot(tr), a[-1])
