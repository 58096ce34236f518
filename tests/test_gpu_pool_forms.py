"""Pooling and un-pooling (csrc/pool3d.hip) per element against float64 (tests/_pool_ref.py), at every launch form.

The launchers pick a kernel form from the dimensions alone (csrc/pool_plan.hpp); every case here asserts the form it is there
for, read from the library's own query (tests/_pool_forms.py: the *_form functions ask sph3d_pool3d_plan; tests/test_pool_forms.py
holds that query to the rules restated in Python, and the cases listed in plan_cases() below to the full set of kernels), calls
the C ABI on outputs pre-filled with NaN (ids: -1) — the gradient kernels promise "each element written exactly once, no memset" —
and compares max-pool values and ids bit for bit with the reference's scan and every sum under
|got - ref| <= (terms + 3) * 2^-24 * mag (assert_sum, which prints the used fraction of that bound: DESIGN.md §2 quotes the
maxima per form)."""
import numpy as np
import pytest
import torch

import _pool_forms as PF
from _pool_forms import bwd_t_form as _bwd_t_form, fwd_form as _fwd_form, max_t_form as _max_t_form, scatter_blocks as _scatter_blocks
from _pool_ref import (U, assert_sum, bits, gather_ref, make_graph, make_values, make_weights, max_grad_ref, max_ref,
                       scatter_ref)
from sph3d_gcn_amd import _lib, _tgraph, tf_pool3d

pytestmark = pytest.mark.gpu


# ---- calls ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _fresh_transposes():
    _tgraph.clear()
    yield
    _tgraph.clear()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


class Graph:
    """a neighbour graph on the host and on the device: idx [B, M, K] ids of the n_src source points, cnt [B, M], w [B, M, K]"""

    def __init__(self, dev, idx, cnt, n_src, rng):
        self.dev, self.idx, self.cnt, self.n_src = dev, idx, cnt, n_src
        self.B, self.M, self.K = idx.shape
        self.w = make_weights(rng, cnt, self.K)
        self.it, self.ct, self.wt = _t(idx, dev), _t(cnt, dev), _t(self.w, dev)

    def in_degree(self):
        live = np.arange(self.K)[None, None, :] < self.cnt[:, :, None]
        return np.stack([np.bincount(self.idx[b][live[b]], minlength=self.n_src) for b in range(self.B)])


P, S = _lib.ptr, _lib.stream_ptr


def _forward(g, mode, x):
    """-> out [B, M, C] (and the ids for max) of the C ABI's forward op on x [B, n_src, C]"""
    B, M, K, N, C = g.B, g.M, g.K, g.n_src, x.shape[2]
    xt, out, l = _t(x, g.dev), _nan((B, M, C), g.dev), _lib.lib()
    if mode == "max":
        mi = torch.full((B, M, C), -1, dtype=torch.int32, device=g.dev)
        _lib.check(l.sph3d_max_pool3d(B, N, M, C, K, P(g.it), P(g.ct), P(xt), P(out), P(mi), S()))
        return _n(out), _n(mi)
    if mode == "avg":
        _lib.check(l.sph3d_avg_pool3d(B, N, M, C, K, P(g.it), P(g.ct), P(xt), P(out), S()))
    else:       # (un-pooling names the rows N and the sources M)
        _lib.check(l.sph3d_weighted_interpolate(B, M, N, C, K, P(g.it), P(g.ct), P(xt), P(g.wt), P(out), S()))
    return _n(out)


def _sum_grad(g, go, weighted, launches=1):
    """gradient of avg / mean (packed entries) or weighted (key + scale arrays) as the gather over the transposed graph; with
    launches = 2 the second launch, over the same transposed graph, must give the first one's bits"""
    B, M, N, C = g.B, g.M, g.n_src, go.shape[2]
    tg = _tgraph.transpose(g.it, g.ct, N, weight=g.wt if weighted else None)
    assert (tg[2] is None) == (not weighted)              # packed entries exactly for the un-weighted graph
    got, outs = _t(go, g.dev), []
    for _ in range(launches):
        gi = _nan((B, N, C), g.dev)
        _lib.check(_lib.lib().sph3d_scatter_grad_t(B, N, M, C, P(tg[0]), P(tg[1]), P(tg[2]), P(got), P(gi), S()))
        outs.append(_n(gi))
    for o in outs[1:]:
        np.testing.assert_array_equal(bits(o), bits(outs[0]))
    return outs[0]


def _max_grad_t(g, go, mi, addend=None, launches=1):
    B, M, N, C = g.B, g.M, g.n_src, go.shape[2]
    tg = _tgraph.transpose(g.it, g.ct, N)
    got, mit, at, outs = _t(go, g.dev), _t(mi, g.dev), (None if addend is None else _t(addend, g.dev)), []
    for _ in range(launches):
        gi = _nan((B, N, C), g.dev)
        _lib.check(_lib.lib().sph3d_max_pool3d_grad_t(B, N, M, C, P(tg[0]), P(tg[1]), P(g.ct), P(mit), P(got), P(at), P(gi), S()))
        outs.append(_n(gi))
    for o in outs[1:]:
        np.testing.assert_array_equal(bits(o), bits(outs[0]))
    return outs[0]


def _max_grad_scatter(g, go, mi):
    B, M, N, C = g.B, g.M, g.n_src, go.shape[2]
    mit, got, gi = _t(mi, g.dev), _t(go, g.dev), _nan((B, N, C), g.dev)      # (named: alive until the result has been read)
    _lib.check(_lib.lib().sph3d_max_pool3d_grad(B, N, M, C, P(mit), P(got), P(gi), S()))
    return _n(gi)


def _check_max(g, x, what):
    out, mi = _forward(g, "max", x)
    ro, ra = max_ref(x, g.idx, g.cnt)
    np.testing.assert_array_equal(mi, ra, err_msg=what + ": ids")
    np.testing.assert_array_equal(bits(out), bits(ro), err_msg=what + ": values")
    return ra


def _check_forward(g, x, what):
    """max, avg and weighted on x; -> the arg-max ids"""
    form = "%s ppwg %d" % _fwd_form(g.B, g.M, x.shape[2])
    ra = _check_max(g, x, "%s max %s" % (form, what))
    assert_sum(_forward(g, "avg", x), *gather_ref(x, g.idx, g.cnt, mean=True), "%s avg %s" % (form, what))
    assert_sum(_forward(g, "weighted", x), *gather_ref(x, g.idx, g.cnt, weight=g.w), "%s weighted %s" % (form, what))
    return ra


def _check_sum_grads(g, go, what, launches=2):
    form = _bwd_t_form(g.B, g.n_src, g.M, go.shape[2])
    assert_sum(_sum_grad(g, go, False, launches), *scatter_ref(go, g.idx, g.cnt, g.n_src, mean=True),
               "%s mean, packed %s" % (form, what))
    assert_sum(_sum_grad(g, go, True, launches), *scatter_ref(go, g.idx, g.cnt, g.n_src, weight=g.w),
               "%s weighted, scale array %s" % (form, what))


def _graph(dev, seed, B, n_src, M, K, **kw):
    rng = np.random.RandomState(seed)
    idx, cnt = make_graph(rng, B, n_src, M, K, **kw)
    assert {0, 1, 2, K - 1, K} <= set(cnt.ravel().tolist())
    return Graph(dev, idx, cnt, n_src, rng), rng


# ---- a. the three forward kernels, four points per workgroup; d. the plain transposed gather ------------------------------------
A_DIMS = (2, 96, 150, 19)             # B, Nin, Mout, K
FWD_C = {"gather_fwd_half": [4, 8, 64, 124, 128], "gather_fwd<4>": [132, 256, 260, 516], "gather_fwd<1>": [1, 3, 63, 65, 67, 129, 131]}
FWD_CASES = [(k, C) for k, cs in FWD_C.items() for C in cs]


def _a_graph(dev, repeats):
    B, N, M, K = A_DIMS
    return _graph(dev, 31 + repeats, B, N, M, K, unique=not repeats)


@pytest.mark.parametrize("repeats", [False, True], ids=["unique", "repeated-ids"])
@pytest.mark.parametrize("kernel,C", FWD_CASES, ids=["%s-C%d" % kc for kc in FWD_CASES])
def test_forward_kernel_forms(dev, kernel, C, repeats):
    g, rng = _a_graph(dev, repeats)
    assert _fwd_form(g.B, g.M, C) == (kernel, 4)
    _check_forward(g, make_values(rng, (g.B, g.n_src, C)), "C=%d" % C)


PLAIN_C = [4, 128, 132, 260, 3, 67, 129]


@pytest.mark.parametrize("repeats", [False, True], ids=["unique", "repeated-ids"])
@pytest.mark.parametrize("C", PLAIN_C)
def test_plain_transposed_gather(dev, C, repeats):
    """the graphs of the forward cases in the pooling direction: 150 rows over 96 sources is short of the split rule"""
    g, rng = _a_graph(dev, repeats)
    assert _bwd_t_form(g.B, g.n_src, g.M, C) == ("gather_bwd_t<4>" if C % 4 == 0 else "gather_bwd_t<1>")
    _check_sum_grads(g, make_values(rng, (g.B, g.M, C)), "C=%d" % C)


# ---- b. sixteen points per workgroup --------------------------------------------------------------------------------------------
FWD16_DIMS, FWD16_C = (2, 64, 32771, 5), [8, 132, 3]             # B, Nin, Mout, K
MAX16_DIMS, MAX16_C = (2, 32771, 200, 8), [8, 3]


@pytest.mark.parametrize("C", FWD16_C)
def test_forward_sixteen_points_per_workgroup(dev, C):
    B, N, M, K = FWD16_DIMS
    g, rng = _graph(dev, 41, B, N, M, K)
    assert B * M == 65542 and M % 16 != 0                                   # over the threshold, a ragged last workgroup
    assert _fwd_form(B, M, C) == ({8: "gather_fwd_half", 132: "gather_fwd<4>", 3: "gather_fwd<1>"}[C], 16)
    _check_forward(g, make_values(rng, (B, N, C)), "C=%d" % C)


@pytest.mark.parametrize("C", MAX16_C)
def test_max_gradient_gather_sixteen_points_per_workgroup(dev, C):
    B, N, M, K = MAX16_DIMS
    g, rng = _graph(dev, 43, B, N, M, K)
    assert _max_t_form(B, N, C) == ("maxpool_bwd_t<4>" if C == 8 else "maxpool_bwd_t<1>", 16) and N % 16 != 0
    x, go = make_values(rng, (B, N, C)), make_values(rng, (B, M, C))
    ra = _check_max(g, x, "max C=%d" % C)
    assert_sum(_max_grad_t(g, go, ra, launches=2), *max_grad_ref(go, ra, N), "%s ppwg %d C=%d" % (_max_t_form(B, N, C) + (C,)))


# ---- c. counts of 128 and above in packed entries ------------------------------------------------------------------------------
PACKED_DIMS, PACKED_C = (1, 256, 40, 200), [8, 67]


@pytest.mark.parametrize("C", PACKED_C)
def test_packed_entries_with_counts_from_128(dev, C):
    B, N, M, K = PACKED_DIMS
    g, rng = _graph(dev, 47, B, N, M, K, high_from=128)
    assert int((g.cnt >= 128).sum()) >= M // 2
    x, go = make_values(rng, (B, N, C)), make_values(rng, (B, M, C))
    assert_sum(_forward(g, "avg", x), *gather_ref(x, g.idx, g.cnt, mean=True), "%s ppwg %d avg K=200 C=%d" % (_fwd_form(B, M, C) + (C,)))
    _check_sum_grads(g, go, "K=200 C=%d" % C)
    ra = _check_max(g, x, "max K=200 C=%d" % C)
    assert_sum(_max_grad_t(g, go, ra, launches=2), *max_grad_ref(go, ra, N), "%s ppwg %d K=200 C=%d" % (_max_t_form(B, N, C) + (C,)))
    # the packed words decode to the transpose numpy makes: per source, the multiset of (row, 1 / count)
    tg = _tgraph.transpose(g.it, g.ct, N)
    assert tg[2] is None
    assert bool((tg[1][: int(tg[0][N])] < 0).any())                       # counts from 128 reach the word's sign bit
    keys, scales = (_n(a) for a in _tgraph.entries(tg))
    off = _n(tg[0]).reshape(B, N + 1)
    for b in range(B):
        rows, slots = np.nonzero(np.arange(K)[None, :] < g.cnt[b][:, None])
        src = g.idx[b, rows, slots]
        for n in range(N):
            want = sorted((int(m), float(np.float32(1) / np.float32(g.cnt[b, m]))) for m in rows[src == n])
            e0, e1 = int(off[b, n]), int(off[b, n + 1])
            assert sorted(zip(keys[e0:e1].tolist(), scales[e0:e1].tolist())) == want, "source %d" % n


# ---- e. the split gather's three bodies ------------------------------------------------------------------------------------------
SPLIT_DIMS = (2, 40, 500, 9)


def _split_graph(dev):
    """2 clouds, 40 sources, 500 rows of up to 9: source 0 without in-edge, source j with j in-edges (1..17), the others share
    the rest, and source 39 — a hub — closes at least 300 rows"""
    B, N, M, K = SPLIT_DIMS
    rng = np.random.RandomState(53)
    idx, cnt = make_graph(rng, B, 22, M, K)
    live = np.arange(K)[None, None, :] < cnt[:, :, None]
    idx = np.where(live, idx + 18, 0).astype(np.int32)
    for b in range(B):
        has = np.nonzero(cnt[b] >= 1)[0][:330]
        idx[b, has, cnt[b, has] - 1] = N - 1                                  # the largest id: rows stay ascending and unique
        two = rng.permutation(np.nonzero(cnt[b] >= 2)[0])
        at = 0
        for j in range(1, 18):
            idx[b, two[at:at + j], 0] = j                                     # the smallest id of its row
            at += j
    g = Graph(dev, idx, cnt, N, rng)
    assert {0, 1, 2, K - 1, K} <= set(cnt.ravel().tolist())
    for deg in g.in_degree():
        assert set(range(18)) <= set(deg.tolist()) and deg.max() >= 300
    return g, rng


SPLIT_C = {"split pairs": [4, 64, 128], "split<4> 1 passes": [132], "split<4> 2 passes": [260], "split<4> 3 passes": [516],
           "split<1> 1 passes": [1], "split<1> 2 passes": [67], "split<1> 3 passes": [129]}
SPLIT_CASES = [(k, C) for k, cs in SPLIT_C.items() for C in cs]


@pytest.mark.parametrize("body,C", SPLIT_CASES, ids=["C%d" % kc[1] for kc in SPLIT_CASES])
def test_split_gather_bodies(dev, body, C):
    g, rng = _split_graph(dev)
    assert _bwd_t_form(g.B, g.n_src, g.M, C) == body
    _check_sum_grads(g, make_values(rng, (g.B, g.M, C)), "C=%d" % C)


# ---- f. the selection boundary ------------------------------------------------------------------------------------------------------
ROW_BOUNDARY, ROW_BOUNDARY_C = [(100, 199), (100, 200)], [8, 67]         # B = 2
SOURCE_BOUNDARY = [(65536, 131072), (65537, 131074)]                    # B = 1, C = 4


@pytest.mark.parametrize("C", ROW_BOUNDARY_C)
@pytest.mark.parametrize("Nin,Mout", ROW_BOUNDARY)
def test_split_rule_boundary_on_the_row_count(dev, Nin, Mout, C):
    B, K = 2, 9
    g, rng = _graph(dev, 59 + Mout, B, Nin, Mout, K)
    assert _bwd_t_form(B, Nin, Mout, C).startswith("split") == (Mout == 200)
    _check_sum_grads(g, make_values(rng, (B, Mout, C)), "Nin=%d Mout=%d C=%d" % (Nin, Mout, C))


@pytest.mark.parametrize("Nin,Mout", SOURCE_BOUNDARY)
def test_split_rule_boundary_on_the_source_count(dev, Nin, Mout):
    B, K, C = 1, 2, 4
    g, rng = _graph(dev, 61, B, Nin, Mout, K)
    assert _bwd_t_form(B, Nin, Mout, C) == ("split pairs" if Nin == 65536 else "gather_bwd_t<4>")     # 65 536 workgroups | plain
    _check_sum_grads(g, make_values(rng, (B, Mout, C)), "Nin=%d Mout=%d" % (Nin, Mout))


# ---- g. the max-pool scatter with a capped grid ------------------------------------------------------------------------------------
SCATTER_CASES = [(64, 40, 300, 131, 4), (1, 64, 4100, 512, 3)]          # B, N, M, C, K


@pytest.mark.parametrize("B,N,M,C,K", SCATTER_CASES)
def test_max_gradient_scatter_capped_grid(dev, B, N, M, C, K):
    blocks, cap = _scatter_blocks(B, M, C)
    assert blocks > cap and cap == {64: 128, 1: 8192}[B]                   # 39 300 > 256 * 128; 2 099 200 > 256 * 8192
    assert M * C > 256 * cap                                                 # grid-stride trips: the channel is carried across them
    g, rng = _graph(dev, 67, B, N, M, K)
    x, go = make_values(rng, (B, N, C)), make_values(rng, (B, M, C))
    ra = _check_max(g, x, "max")
    assert_sum(_max_grad_scatter(g, go, ra), *max_grad_ref(go, ra, N), "maxpool_bwd capped grid B=%d C=%d" % (B, C))


# ---- h. the gather form of the max-pool gradient ----------------------------------------------------------------------------------
H_DIMS, H_C = (2, 96, 150, 19), [4, 128, 260, 3, 67]


def _h_graph(dev):
    B, N, M, K = H_DIMS
    empty = np.unique(np.concatenate([[64, 149], np.random.RandomState(71).permutation(M)[:75]]))
    g, rng = _graph(dev, 73, B, N, M, K, empty_rows=empty)
    for b in range(B):                                                         # past the first 64-row sweep, and the last row
        assert (g.cnt[b] == 0).sum() >= 70 and g.cnt[b, 64] == 0 and g.cnt[b, 149] == 0 and (g.cnt[b, :64] == 0).any()
    assert M % 64 != 0
    return g, rng


@pytest.mark.parametrize("C", H_C)
def test_max_gradient_gather_form(dev, C):
    g, rng = _h_graph(dev)
    B, N, M = g.B, g.n_src, g.M
    form = "%s ppwg %d" % _max_t_form(B, N, C)
    assert form == ("maxpool_bwd_t<4> ppwg 4" if C % 4 == 0 else "maxpool_bwd_t<1> ppwg 4")
    blocks, cap = _scatter_blocks(B, M, C)
    assert blocks <= cap                                                       # the scatter form: every element has its own thread
    x, go, skip = make_values(rng, (B, N, C)), make_values(rng, (B, M, C)), make_values(rng, (B, N, C))
    ra = _check_max(g, x, "max C=%d" % C)
    ref, mag, terms = max_grad_ref(go, ra, N)
    assert (ref[:, 0] != 0).any() and terms[:, 0].max() >= 70                  # the empty rows' gradient goes to point 0
    plain = _max_grad_t(g, go, ra, launches=2)
    assert_sum(plain, ref, mag, terms, "%s C=%d" % (form, C))
    scat = _max_grad_scatter(g, go, ra)
    assert_sum(scat, ref, mag, terms, "maxpool_bwd C=%d" % C)
    assert (np.abs(plain.astype(np.float64) - scat) <= 2 * (terms + 3) * U * mag).all()
    # with an addend: one more term, one more rounding
    s64 = skip.astype(np.float64)
    assert_sum(_max_grad_t(g, go, ra, addend=skip, launches=2), ref + s64, mag + np.abs(s64), terms + 1,
               "%s with addend C=%d" % (form, C))
    # the autograd path of a pooled tensor that a skip connection also reads: both gradients meet in the gather kernel
    _tgraph.clear()
    _tgraph.transpose(g.it, g.ct, N, unique_rows=True)
    xt = _t(x, dev).requires_grad_(True)
    out, mi, sk = tf_pool3d.max_pool3d_with_skip(xt, g.it, g.ct)
    np.testing.assert_array_equal(_n(mi), ra)
    assert _tgraph.peek(g.it, g.ct, N, need_unique_rows=True) is not None        # (else the op falls back to the scatter)
    ((out * _t(go, dev)).sum() + (sk * _t(skip, dev)).sum()).backward()
    assert_sum(_n(xt.grad), ref + s64, mag + np.abs(s64), terms + 1, "%s through max_pool3d_with_skip C=%d" % (form, C))


# ---- i. non-finite inputs ------------------------------------------------------------------------------------------------------------
def _poisoned(a, points, kinds):
    a = a.copy()
    for p, v in zip(points, kinds):
        a[:, p] = v
    return a


def _check_confined(got, clean, dirty_elements, what):
    """elements all of whose terms are finite carry the bits of the run without the non-finite points; the others are non-finite
    (which kind is not asserted: three kernels read an odd tail's row a second time with weight 0, and 0 * inf is NaN)"""
    assert dirty_elements.any() and not dirty_elements.all(), what
    np.testing.assert_array_equal(bits(got)[~dirty_elements], bits(clean)[~dirty_elements], err_msg=what)
    assert not np.isfinite(got[dirty_elements]).any(), what + ": a non-finite term left a finite element"


def _roles(g):
    """three distinct points: one in slot 0 of a row, one in a later slot of a row, one last in a row of odd count (>= 3)"""
    idx, cnt = g.idx[0], g.cnt[0]
    first = int(idx[np.nonzero(cnt >= 2)[0][0], 0])
    odd = np.nonzero((cnt % 2 == 1) & (cnt >= 3))[0]
    last = next(int(idx[m, cnt[m] - 1]) for m in odd if idx[m, cnt[m] - 1] != first)
    later = next(int(idx[m, 1]) for m in np.nonzero(cnt >= 3)[0] if idx[m, 1] not in (first, last))
    return first, later, last


def _roles_rows(g):
    """three rows with neighbours in every cloud, one of them with an odd count: their sources' sums get a non-finite term"""
    ok = (g.cnt >= 1).all(axis=0)
    odd = np.nonzero(ok & (g.cnt[0] % 2 == 1))[0]
    rest = [int(m) for m in np.nonzero(ok)[0] if m != odd[0]]
    return int(odd[0]), rest[0], rest[len(rest) // 2]


NON_FINITE_CASES = [(0, 8), (1, 132), (2, 67)]


@pytest.mark.parametrize("turn,C", NON_FINITE_CASES)
def test_non_finite_inputs_stay_in_their_rows(dev, turn, C):
    g, rng = _graph(dev, 79, *A_DIMS)
    B, N, M = g.B, g.n_src, g.M
    kinds = np.roll(np.array([np.nan, np.inf, -np.inf], np.float32), turn)        # each role meets each kind over the three cases
    points = _roles(g)
    x = make_values(rng, (B, N, C))
    xp, x0 = _poisoned(x, points, kinds), _poisoned(x, points, (0, 0, 0))
    live = np.arange(g.K)[None, None, :] < g.cnt[:, :, None]
    dirty_rows = (np.isin(g.idx, points) & live).any(axis=2)                       # [B, M]
    dirty = np.broadcast_to(dirty_rows[:, :, None], (B, M, C))
    _check_max(g, xp, "max, non-finite C=%d" % C)
    for mode in ("avg", "weighted"):
        _check_confined(_forward(g, mode, xp), _forward(g, mode, x0), dirty, "%s %s C=%d" % (_fwd_form(B, M, C)[0], mode, C))
    # gradients with three non-finite grad_output rows, on this graph (plain gather) and on the split graph
    for gg in (g, _split_graph(dev)[0]):
        rows = _roles_rows(gg)
        go = make_values(rng, (gg.B, gg.M, C))
        gp, g0 = _poisoned(go, rows, kinds), _poisoned(go, rows, (0, 0, 0))
        lv = np.arange(gg.K)[None, None, :] < gg.cnt[:, :, None]
        hit = np.zeros((gg.B, gg.n_src), bool)
        for b in range(gg.B):
            for m in rows:
                hit[b, gg.idx[b, m][lv[b, m]]] = True
        dirty_src = np.broadcast_to(hit[:, :, None], (gg.B, gg.n_src, C))
        for weighted in (False, True):
            _check_confined(_sum_grad(gg, gp, weighted), _sum_grad(gg, g0, weighted), dirty_src,
                            "%s weighted=%s C=%d" % (_bwd_t_form(gg.B, gg.n_src, gg.M, C), weighted, C))
    # the max gradient (gather form): an element is touched where a non-finite row's arg-max id names it
    ra = max_ref(x, g.idx, g.cnt)[1]
    rows = _roles_rows(g)
    go = make_values(rng, (B, M, C))
    gp, g0 = _poisoned(go, rows, kinds), _poisoned(go, rows, (0, 0, 0))
    touched = np.zeros((B, N, C), bool)
    for b in range(B):
        for m in rows:
            touched[b, ra[b, m], np.arange(C)] = True
    _check_confined(_max_grad_t(g, gp, ra), _max_grad_t(g, g0, ra), touched, "%s C=%d" % (_max_t_form(B, N, C)[0], C))


# ---- the calls of the cases above, for tests/test_pool_forms.py ---------------------------------------------------------------------
def plan_cases():
    """-> [(op, B, Nin, Mout, C, K, forward modes)] of the parametrize lists above: the library calls their tests make"""
    out = []

    def add(op, dims, C, modes=PF.MODES):
        B, N, M, K = dims
        out.append((op, B, N, M, C, K, modes))

    for _, C in FWD_CASES:
        add(PF.FWD, A_DIMS, C)
    for C in PLAIN_C:
        add(PF.SUM_GRAD_T, A_DIMS, C)
    for C in FWD16_C:
        add(PF.FWD, FWD16_DIMS, C)
    for C in MAX16_C:
        add(PF.FWD, MAX16_DIMS, C, ("max",))
        add(PF.MAX_GRAD_T, MAX16_DIMS, C)
    for C in PACKED_C:
        add(PF.FWD, PACKED_DIMS, C, ("max", "avg"))
        add(PF.SUM_GRAD_T, PACKED_DIMS, C)
        add(PF.MAX_GRAD_T, PACKED_DIMS, C)
    for _, C in SPLIT_CASES:
        add(PF.SUM_GRAD_T, SPLIT_DIMS, C)
    for C in ROW_BOUNDARY_C:
        for Nin, Mout in ROW_BOUNDARY:
            add(PF.SUM_GRAD_T, (2, Nin, Mout, 9), C)
    for Nin, Mout in SOURCE_BOUNDARY:
        add(PF.SUM_GRAD_T, (1, Nin, Mout, 2), 4)
    for B, N, M, C, K in SCATTER_CASES:
        add(PF.FWD, (B, N, M, K), C, ("max",))
        add(PF.MAX_GRAD, (B, N, M, K), C)
    for C in H_C:
        add(PF.FWD, H_DIMS, C, ("max",))
        add(PF.MAX_GRAD_T, H_DIMS, C)
        add(PF.MAX_GRAD, H_DIMS, C)
    for _, C in NON_FINITE_CASES:
        add(PF.FWD, A_DIMS, C)
        add(PF.SUM_GRAD_T, A_DIMS, C)
        add(PF.SUM_GRAD_T, SPLIT_DIMS, C)
        add(PF.MAX_GRAD_T, A_DIMS, C)
    return out
