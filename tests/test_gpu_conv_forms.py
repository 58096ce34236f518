"""The depthwise convolution and its gradient (csrc/conv3d.hip) per element against float64 (tests/_conv_ref.py), at every launch
form, through the C ABI.

The launchers pick kernels from the dimensions (and, on the device, from the active-bin count); every case restates the rule
that selects its form as an assertion — the functions of tests/_conv_forms.py are copied from the launchers conv3d.hip had before
csrc/conv_plan.hpp stated the choice once; tests/test_conv_forms.py holds the library's own plan to them on the host, and here
the gradient's workspace size and the two-input predicate are compared with the library's answer.  Outputs are pre-filled with NaN (grad_input and grad_filter are promised "fully
written"), the gradient's workspace — slabs and hub list — with 0xFF bytes (NaN as floats: a slab that is read but was not
written this call shows), transposed graphs are built with sph3d_graph_transpose itself.  assert_conv prints the used fraction
of each derived bound behind a [form] tag: DESIGN.md §2 quotes the maxima.

Left out on purpose: neighbour ids outside [0, N), and launches at the 32-bit-offset fall-backs (N C or M C r near 2^32, N above
2^24: no small device input reaches them; tests/test_conv_forms.py holds the plan's choice there on the host).  The
separable kernels (sepconv.hip, sepring.hip) are held the same way in tests/test_gpu_sep_forms.py."""
import os

import numpy as np
import pytest
import torch

from _conv_forms import (FWD_CASES, HUB_CASES, K_COMPACT_BINS, K_SLICE, PLAN_CASES, V2_CASES, bwd_layout, cat_ok, dims_ok, fwd_form,
                         grad_form, hub_threshold, vec_plan)
from _conv_ref import assert_conv, bits, clamp_bins, conv_grad_ref, conv_ref, make_bins, make_graph, make_values
from sph3d_gcn_amd import _lib

pytestmark = pytest.mark.gpu
P, S = _lib.ptr, _lib.stream_ptr
EWORKSPACE, EUNSUPPORTED = -2, -4


# ---- graphs and calls -------------------------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _ff(nbytes, dev):
    return torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=dev)


class Graph:
    """nn_index / nn_count / bin_index [B, M, K] over N sources and F bins, on the host and on the device, with its transposed
    graphs (built once per form by sph3d_graph_transpose, into pre-filled outputs and a 0xFF workspace)"""

    def __init__(self, dev, idx, cnt, bins, N, F):
        self.dev, self.idx, self.cnt, self.bins, self.N, self.F = dev, idx, cnt, bins, N, F
        self.B, self.M, self.K = idx.shape
        self.it, self.ct, self.bt = _t(idx, dev), _t(cnt, dev), _t(bins, dev)
        self.live = np.arange(self.K)[None, None, :] < cnt[:, :, None]
        self.A = int(np.unique(clamp_bins(bins[self.live], F)).size)
        self._tg = {}

    def transposed(self, entries="packed", active=True):
        """-> (offsets, ent_key, ent_scale | None, active_bins | None)"""
        if (entries, active) not in self._tg:
            B, N, M, K, F, dev = self.B, self.N, self.M, self.K, self.F, self.dev
            n_ent = max(B * M * K, 16)
            off = torch.full((B * (N * F + 1),), 0x7f7f7f7f, dtype=torch.int32, device=dev)
            key = torch.full((n_ent,), 0x7f7f7f7f, dtype=torch.int32, device=dev)
            scale = None if entries == "packed" else _nan((n_ent,), dev)
            act = torch.full((F + 1,), -1, dtype=torch.int32, device=dev) if active else None
            l = _lib.lib()
            wsb = l.sph3d_graph_transpose_workspace(B, N, M, K, F)
            ws = _ff(wsb, dev)
            _lib.check(l.sph3d_graph_transpose(B, N, M, K, F, P(self.it), P(self.ct), P(self.bt), None, P(off), P(key), P(scale),
                                               P(act), P(ws), wsb, S()))
            torch.cuda.synchronize()
            if active:
                assert int(act[0]) == self.A
            self._tg[(entries, active)] = (off, key, scale, act)
        return self._tg[(entries, active)]


def _random_graph(dev, seed, B, N, M, K, F, pool=None, unique=True, hub=False, **kw):
    rng = np.random.RandomState(seed)
    if hub:                                                   # source N - 1 closes five of six rows that have a neighbour
        idx, cnt = make_graph(rng, B, N - 1, M, K, unique=unique, **kw)
        for b in range(B):
            has = np.nonzero(cnt[b] >= 1)[0]
            has = has[has % 6 != 0]
            idx[b, has, cnt[b, has] - 1] = N - 1
    else:
        idx, cnt = make_graph(rng, B, N, M, K, unique=unique, **kw)
    return Graph(dev, idx, cnt, make_bins(rng, idx, cnt, F, pool), N, F), rng


def _graph_from_segments(dev, seed, B, N, F, seglens, K):
    """a graph whose transposed graph has exactly seglens[(n, f)] in-edges in segment (source n, bin f) of every cloud: the edges
    are shuffled and dealt to rows of 1, 2 .. K, 1 .. slots (a source may appear twice in a row), then two empty rows"""
    rng = np.random.RandomState(seed)
    edges = np.array([(n, f) for (n, f), ln in sorted(seglens.items()) for _ in range(ln)], np.int64).reshape(-1, 2)
    E, counts, c = len(edges), [], 1
    while sum(counts) < E:
        counts.append(min(c, E - sum(counts)))
        c = c % K + 1
    M = len(counts) + 2
    idx, cnt, bins = np.zeros((B, M, K), np.int32), np.zeros((B, M), np.int32), np.full((B, M, K), F + 7, np.int32)
    for b in range(B):
        e = edges[rng.permutation(E)]
        rows, at = rng.permutation(M)[:len(counts)], 0
        for m, c in zip(rows, counts):
            idx[b, m, :c], bins[b, m, :c], cnt[b, m] = e[at:at + c, 0], e[at:at + c, 1], c
            at += c
    g = Graph(dev, idx, cnt, bins, N, F)
    return g, rng


def _forward(g, x, w, clamp_ids=None, cat=None):
    """sph3d_depthwise_conv3d (cat = Ca: sph3d_depthwise_conv3d_cat on x[..., :Ca] | x[..., Ca:]) -> out [B, M, C r]"""
    (F, C, r), l = w.shape, _lib.lib()
    bt = g.bt if clamp_ids is None else _t(clamp_ids, g.dev)
    wt, out = _t(w, g.dev), _nan((g.B, g.M, C * r), g.dev)
    if cat is None:
        xt = _t(x, g.dev)
        _lib.check(l.sph3d_depthwise_conv3d(g.B, g.N, g.M, F, C, r, g.K, P(g.it), P(g.ct), P(bt), P(xt), P(wt), P(out), S()))
    else:
        xa, xb = _t(x[:, :, :cat], g.dev), _t(x[:, :, cat:], g.dev)
        _lib.check(l.sph3d_depthwise_conv3d_cat(g.B, g.N, g.M, F, cat, C - cat, r, g.K, P(g.it), P(g.ct), P(bt), P(xa), P(xb), P(wt),
                                                P(out), S()))
    return _n(out)


def _grad(g, x, w, go, entries="packed", active=True, order=None, launches=1, cat=None):
    """sph3d_depthwise_conv3d_grad_t[_cat] on NaN outputs and a 0xFF workspace -> (grad_input, grad_filter); with launches = 2 the
    second launch, on the same transposed graph and the workspace as the first left it, must give the first one's bits"""
    (F, C, r), l, dev = w.shape, _lib.lib(), g.dev
    B, N, M = g.B, g.N, g.M
    off, key, scale, act = g.transposed(entries, active)
    wsb = l.sph3d_depthwise_conv3d_grad_t_workspace(B, N, F, C, r)
    assert wsb == bwd_layout(B, N, F, C, r)["bytes"]                       # vec_plan and bwd_plan, as the library computes them
    ws = _ff(wsb, dev)
    xt, wt, got, outs = _t(x, dev), _t(w, dev), _t(go, dev), []
    if cat is not None:
        xa, xb = _t(x[:, :, :cat], dev), _t(x[:, :, cat:], dev)
    for _ in range(launches):
        gf = _nan((F, C, r), dev)
        if cat is None:
            gi = _nan((B, N, C), dev)
            _lib.check(l.sph3d_depthwise_conv3d_grad_t(B, N, M, F, C, r, P(off), P(key), P(scale), P(order), P(act), P(xt), P(wt), P(got),
                                                       P(gi), P(gf), P(ws) if wsb else None, wsb, S()))
        else:
            ga, gb = _nan((B, N, cat), dev), _nan((B, N, C - cat), dev)
            _lib.check(l.sph3d_depthwise_conv3d_grad_t_cat(B, N, M, F, cat, C - cat, r, P(off), P(key), P(scale), P(order), P(act), P(xa),
                                                           P(xb), P(wt), P(got), P(ga), P(gb), P(gf), P(ws), wsb, S()))
            gi = torch.cat((ga, gb), 2)
        outs.append((_n(gi), _n(gf)))
    for o in outs[1:]:
        np.testing.assert_array_equal(bits(o[0]), bits(outs[0][0]), err_msg="grad_input of a second launch")
        np.testing.assert_array_equal(bits(o[1]), bits(outs[0][1]), err_msg="grad_filter of a second launch")
    return outs[0]


def _inputs(rng, g, C, r):
    return make_values(rng, (g.B, g.N, C)), make_values(rng, (g.F, C, r)), make_values(rng, (g.B, g.M, C * r))


def _assert_grad(got, ref, form, r, what, hub_rows=None):
    tag = "[%s] %s" % (form["tag"], what)
    return (assert_conv(got[0], ref.gi, ref.gi_mag, ref.gi_terms(r, hub_rows), tag + ": grad_input"),
            assert_conv(got[1], ref.gf, ref.gf_mag, ref.gf_terms(form["depth"]), tag + ": grad_filter"))


def _check_grad(g, x, w, go, what, expect, active=True, ref=None, **kw):
    """one gradient case: the form the rules give must be the `expect`ed one, then the call and both per-element checks"""
    F, C, r = w.shape
    form = grad_form(g.B, g.N, g.M, F, C, r, active, g.A)
    for k, v in expect.items():
        assert form[k] == v, "%s: rule gives %s = %s, the case is meant for %s" % (what, k, form[k], v)
    ref = conv_grad_ref(x, w, go, g.idx, g.cnt, g.bins) if ref is None else ref
    hub_rows = ref.deg > hub_threshold() if form["hub"] else None
    got = _grad(g, x, w, go, active=active, **kw)
    _assert_grad(got, ref, form, r, what, hub_rows)
    return got, ref


@pytest.fixture
def hub_env():
    old = {k: os.environ.get(k) for k in ("SPH3D_BWD_HUB_MIN_N", "SPH3D_BWD_HUB_T")}
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _hubs(min_n, T):
    os.environ["SPH3D_BWD_HUB_MIN_N"], os.environ["SPH3D_BWD_HUB_T"] = str(min_n), str(T)


# ---- forward -----------------------------------------------------------------------------------------------------------------------
FWD_COUNTS = [0, 1, 3, 4, 15, 16, 17, 63, 64]
FWD_GEOMS = [(1, 33, 70), (3, 31, 200), (9, 1, 70)]        # B, M, K: 32 points per workgroup; second and fourth 64-slot chunks


def _fwd_graph(dev, B, M, K, F, seed=0, N=40):
    """random ids (repeats inside a row), counts 0..K with FWD_COUNTS, K - 1 and K forced in; dead slots hold bin F + 7"""
    rng = np.random.RandomState(1000 + 7 * B + M + K + seed)
    idx = rng.randint(0, N, size=(B, M, K)).astype(np.int32)
    cnt = rng.randint(0, K + 1, size=(B, M)).astype(np.int32)
    forced = (FWD_COUNTS + [K - 1, K])[:B * M]
    cnt.reshape(-1)[np.linspace(0, B * M - 1, len(forced)).astype(np.int64)] = forced
    assert set(FWD_COUNTS) <= set(cnt.ravel().tolist())
    return Graph(dev, idx, cnt, make_bins(rng, idx, cnt, F), N, F), rng


@pytest.mark.parametrize("kernel,C,r,F", FWD_CASES, ids=["C%d-r%d-F%d" % c[1:] for c in FWD_CASES])
def test_forward_kernel_forms(dev, kernel, C, r, F):
    for B, M, K in FWD_GEOMS:
        g, rng = _fwd_graph(dev, B, M, K, F)
        assert dims_ok(F, C, r) and fwd_form(g.N, F, C, r) == kernel
        assert (C, r) not in ((132, 2), (100, 3)) or C * r - K_SLICE in (8, 44)        # two slices, the second 8 and 44 outputs wide
        x, w = make_values(rng, (B, g.N, C)), make_values(rng, (F, C, r))
        ref, mag, terms = conv_ref(x, w, g.idx, g.cnt, g.bins)
        assert_conv(_forward(g, x, w), ref, mag, terms + 4, "[%s] C=%d r=%d F=%d B=%d M=%d K=%d" % (kernel, C, r, F, B, M, K))


@pytest.mark.parametrize("C,r", [(64, 2), (132, 2), (35, 2)], ids=["multi", "row", "generic"])
def test_forward_out_of_range_bin_ids(dev, C, r):
    B, M, K, F = 3, 31, 70, 33
    g, rng = _fwd_graph(dev, B, M, K, F)
    assert fwd_form(g.N, F, C, r) == {64: "dwconv_fwd_multi<2,16>", 132: "dwconv_fwd_row<2>", 35: "dwconv_fwd_generic"}[C]
    bad = g.bins.copy()
    sel = g.live & (rng.rand(*bad.shape) < 0.3)
    bad[sel] = np.array([-3, F, F + 5], np.int32)[rng.randint(0, 3, size=int(sel.sum()))]
    assert {-3, F, F + 5} <= set(bad[g.live].tolist())
    x, w = make_values(rng, (B, g.N, C)), make_values(rng, (F, C, r))
    out = _forward(g, x, w, clamp_ids=bad)
    clamped = np.where(g.live, clamp_bins(bad, F), bad).astype(np.int32)
    np.testing.assert_array_equal(bits(out), bits(_forward(g, x, w, clamp_ids=clamped)))
    # garbage ids in dead slots change nothing
    dead = np.where(g.live, bad, rng.randint(-(1 << 30), 1 << 30, size=bad.shape)).astype(np.int32)
    np.testing.assert_array_equal(bits(out), bits(_forward(g, x, w, clamp_ids=dead)))
    ref, mag, terms = conv_ref(x, w, g.idx, g.cnt, bad)
    assert_conv(out, ref, mag, terms + 4, "[%s] out-of-range bin ids" % fwd_form(g.N, F, C, r))


CAT_SHAPES = [(128, 4, 2), (128, 128, 2), (256, 128, 1)]


@pytest.mark.parametrize("Ca,Cb,r", CAT_SHAPES)
def test_forward_two_inputs(dev, Ca, Cb, r):
    B, M, K, F = 3, 31, 70, 33
    g, rng = _fwd_graph(dev, B, M, K, F)
    C = Ca + Cb
    assert cat_ok(F, Ca, Cb, r) and _lib.lib().sph3d_depthwise_conv3d_cat_supported(F, Ca, Cb, r) == 1
    assert fwd_form(g.N, F, C, r) == "dwconv_fwd_row<%d>" % r                # the plain op's kernel on the concatenation
    x, w = make_values(rng, (B, g.N, C)), make_values(rng, (F, C, r))
    out = _forward(g, x, w, cat=Ca)
    np.testing.assert_array_equal(bits(out), bits(_forward(g, x, w)))
    ref, mag, terms = conv_ref(x, w, g.idx, g.cnt, g.bins)
    assert_conv(out, ref, mag, terms + 4, "[dwconv_fwd_row<%d> two inputs] Ca=%d Cb=%d" % (r, Ca, Cb))


def test_two_inputs_unsupported_shape(dev):
    B, M, K, F, Ca, Cb, r = 1, 33, 70, 33, 64, 64, 2                            # Ca r = 128: a slice would straddle the two tensors
    g, rng = _fwd_graph(dev, B, M, K, F)
    l = _lib.lib()
    assert not cat_ok(F, Ca, Cb, r) and l.sph3d_depthwise_conv3d_cat_supported(F, Ca, Cb, r) == 0
    assert not cat_ok(34, 128, 128, 2) and l.sph3d_depthwise_conv3d_cat_supported(34, 128, 128, 2) == 0       # V = 2 plan
    xa, xb, wt = _nan((B, g.N, Ca), dev), _nan((B, g.N, Cb), dev), _nan((F, Ca + Cb, r), dev)
    out = _nan((B, M, (Ca + Cb) * r), dev)
    assert l.sph3d_depthwise_conv3d_cat(B, g.N, M, F, Ca, Cb, r, K, P(g.it), P(g.ct), P(g.bt), P(xa), P(xb), P(wt), P(out), S()) == EUNSUPPORTED
    off, key, scale, act = g.transposed()
    ga, gb, gf, ws = _nan((B, g.N, Ca), dev), _nan((B, g.N, Cb), dev), _nan((F, Ca + Cb, r), dev), _ff(1 << 20, dev)
    assert l.sph3d_depthwise_conv3d_grad_t_cat(B, g.N, M, F, Ca, Cb, r, P(off), P(key), P(scale), None, P(act), P(xa), P(xb), P(wt), P(out),
                                               P(ga), P(gb), P(gf), P(ws), 1 << 20, S()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (out, ga, gb, gf))           # nothing was written


# ---- gradient: plans and segments -----------------------------------------------------------------------------------------------------
def _segment_graph(dev, B=2):
    """40 sources, 33 bins of which 8 occur.  Source j < 10: a segment of j in-edges in bin 3 (the full wave's remainders 1..3,
    the half waves' batch of 6, the quarter waves' batch of 8) between segments in bins 0 and 7; sources 10..15: 61, 64, 65, 127,
    130 and 200 in-edges in bin 5 alone (the half waves' last batch of six starts at lane 60 and wraps; chunks of 64); source 16:
    60 + 10 + 3 in bins 1, 2, 7 (the chunk boundary falls inside the second segment); source 17: 3 + 61 (the last batch of six
    starts at lane 63); source 18: no in-edge; the others: short segments in random bins of the eight"""
    rng = np.random.RandomState(211)
    seg = {}
    for j in range(10):
        seg[(j, 0)], seg[(j, 3)], seg[(j, 7)] = 1 + j % 3, j, 2
    for n, ln in zip(range(10, 16), (61, 64, 65, 127, 130, 200)):
        seg[(n, 5)] = ln
    seg[(16, 1)], seg[(16, 2)], seg[(16, 7)] = 60, 10, 3
    seg[(17, 0)], seg[(17, 5)] = 3, 61
    pool = [0, 1, 2, 3, 5, 7, 20, 32]
    for n in range(19, 40):
        for f in rng.permutation(pool)[:rng.randint(1, 6)]:
            seg[(n, int(f))] = int(rng.randint(1, 10))
    g, rng = _graph_from_segments(dev, 223, B, 40, 33, {k: v for k, v in seg.items() if v}, K=8)
    assert g.A == 8 and g.M != g.N
    return g, rng, seg


def _assert_segments(ref, seg, B):
    want = np.zeros(ref.seg.shape[1:], np.int64)
    for (n, f), ln in seg.items():
        want[n, f] = ln
    for b in range(B):
        np.testing.assert_array_equal(ref.seg[b], want)


@pytest.mark.parametrize("C,r,parts", PLAN_CASES, ids=["C%d-r%d" % c[:2] for c in PLAN_CASES])
def test_gradient_plans_tables_and_segments(dev, C, r, parts):
    g, rng, seg = _segment_graph(dev)
    x, w, go = _inputs(rng, g, C, r)
    assert dims_ok(g.F, C, r) and vec_plan(g.F, C * r, r) == 4
    expect = dict(kernel="vec", V=4, PARTS=parts, hub=False)
    got, ref = _check_grad(g, x, w, go, "segments, active_bins given", dict(expect, compact=True), active=True, launches=2)
    _assert_segments(ref, seg, g.B)
    # active_bins == NULL: the full table, whatever occurs
    _check_grad(g, x, w, go, "segments, active_bins NULL", dict(expect, compact=False), active=False, ref=ref, launches=2)


@pytest.mark.parametrize("C,r,F", V2_CASES, ids=["C%d-r%d-F%d" % c for c in V2_CASES])
def test_gradient_two_channels_per_lane(dev, C, r, F):
    g, rng = _random_graph(dev, 227 + F, 2, 70, 150, 9, F, hub=True)
    used = set(clamp_bins(g.bins[g.live], F).tolist())
    assert F - 1 in used and (F < 65 or {63, 64} <= used)                       # F = 65: bounds in the second register
    assert vec_plan(F, C * r, r) == 2 and (F > 33 or (C * r) % 4 == 2) and dims_ok(F, C, r)
    x, w, go = _inputs(rng, g, C, r)
    got, ref = _check_grad(g, x, w, go, "F=%d" % F, dict(kernel="vec", V=2, PARTS=1, compact=False, hub=False), launches=2)
    assert ref.deg.max() > 64


GENERIC_CASES = [(3, 1, 33), (5, 3, 33), (64, 2, 66), (100, 3, 17)]


@pytest.mark.parametrize("C,r,F", GENERIC_CASES, ids=["C%d-r%d-F%d" % c for c in GENERIC_CASES])
def test_gradient_generic_kernel(dev, C, r, F):
    g, rng = _random_graph(dev, 229 + F, 2, 70, 150, 9, F, hub=True)
    if F == 66:           # F alone sends it to the generic kernel: the same channels take V = 4 at 33 bins and V = 2 at 65
        assert vec_plan(33, C * r, r) == 4 and vec_plan(65, C * r, r) == 2
    assert vec_plan(F, C * r, r) == 0 and dims_ok(F, C, r)
    x, w, go = _inputs(rng, g, C, r)
    _check_grad(g, x, w, go, "C=%d r=%d F=%d" % (C, r, F), dict(kernel="generic"))
    _check_grad(g, x, w, go, "C=%d r=%d F=%d key + scale" % (C, r, F), dict(kernel="generic"), entries="arrays")


# ---- gradient: compact and full tables ----------------------------------------------------------------------------------------------
_BIN_ORDER = np.random.RandomState(233).permutation(33)


@pytest.mark.parametrize("C,r", [(8, 2), (128, 2)], ids=["quarter-waves", "full-wave"])
@pytest.mark.parametrize("A", [1, 17, 18, 33])
def test_gradient_table_choice_by_active_bins(dev, A, C, r):
    F = 33
    pool = np.sort(np.concatenate([[32], _BIN_ORDER[_BIN_ORDER != 32][:A - 1]]))
    g, rng = _random_graph(dev, 239 + A, 2, 70, 150, 9, F, pool=pool, hub=True)
    assert g.A == A
    x, w, go = _inputs(rng, g, C, r)
    got, ref = _check_grad(g, x, w, go, "A=%d" % A, dict(kernel="vec", V=4, compact=A <= K_COMPACT_BINS, hub=False), launches=2)
    never = np.setdiff1d(np.arange(F), pool)
    assert (ref.E_f[never] == 0).all() and (bits(got[1][never]) == 0).all()          # bins that never occur: exact +0
    _check_grad(g, x, w, go, "A=%d, active_bins NULL" % A, dict(compact=False), active=False, ref=ref)


@pytest.mark.parametrize("C,r", [(8, 2), (34, 2), (132, 1)])
def test_gradient_fewer_bins_than_compact_rows(dev, C, r):
    F = 8
    g, rng = _random_graph(dev, 241, 2, 70, 150, 9, F, hub=True)
    assert F < K_COMPACT_BINS and g.A == F
    x, w, go = _inputs(rng, g, C, r)
    _check_grad(g, x, w, go, "F=8", dict(kernel="vec", V=4, compact=True), launches=2)
    _check_grad(g, x, w, go, "F=8, active_bins NULL", dict(kernel="vec", V=4, compact=False), active=False)


@pytest.mark.parametrize("C,r,F", [(8, 2, 33), (128, 2, 33), (6, 1, 33), (3, 1, 33)])
def test_gradient_of_an_empty_graph(dev, C, r, F):
    B, N, M, K = 2, 70, 50, 9
    rng = np.random.RandomState(251)
    idx = rng.randint(0, N, size=(B, M, K)).astype(np.int32)
    g = Graph(dev, idx, np.zeros((B, M), np.int32), rng.randint(0, F, size=(B, M, K)).astype(np.int32), N, F)
    assert g.A == 0
    x, w, go = _inputs(rng, g, C, r)
    for active in (True, False):
        form = grad_form(B, N, M, F, C, r, active, 0)
        assert form["kernel"] == "generic" or form["compact"] == (active and form["V"] == 4)
        gi, gf = _grad(g, x, w, go, active=active)
        assert (bits(gi) == 0).all() and (bits(gf) == 0).all(), "every cnt = 0: both gradients are exact zeros, fully written"


# ---- gradient: the sweep over clouds and sources -----------------------------------------------------------------------------------
SWEEP_N = [1, 5, 8, 63, 64, 65, 300]
SWEEP_CR = [(4, 2), (34, 2), (132, 1), (6, 1), (3, 1)]         # quarter, half and full waves, two channels per lane, generic


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 8, 9, 16])
def test_gradient_sweep_of_clouds_and_sources(dev, B):
    F, K = 33, 4
    for i, N in enumerate(SWEEP_N):
        C, r = SWEEP_CR[(B + i) % len(SWEEP_CR)]
        M = N + 5                                                           # M != N; rows of 0, 1, 2, K - 1 and K slots
        g, rng = _random_graph(dev, 257 + 31 * B + N, B, N, M, K, F, pool=np.arange(0, F, 3), unique=False)
        active = (B + i) % 3 != 0                                           # every third cell: active_bins NULL
        form = grad_form(B, N, M, F, C, r, active, g.A)
        if form["kernel"] == "vec":
            gcd = max(d for d in (1, 2, 4, 8) if B % d == 0)
            # parts = 8 / gcd(B, 8), or 1 when N < parts, written a second way: a cross-check of the restated bwd_plan, not of
            # the launcher — the library's own plan enters through the workspace byte count that _grad compares
            assert form["plan"][0] == (8 // gcd if N >= 8 // gcd else 1)
            assert form["plan"][2] == 8 * form["plan"][1] and form["plan"][1] >= 1
        x, w, go = _inputs(rng, g, C, r)
        _check_grad(g, x, w, go, "B=%d N=%d M=%d C=%d r=%d" % (B, N, M, C, r), {}, active=active)


# ---- gradient: source_order, entries -------------------------------------------------------------------------------------------------
def test_gradient_source_orders(dev):
    B, N, M, K, F, C, r = 3, 300, 320, 9, 33, 64, 2
    g, rng = _random_graph(dev, 263, B, N, M, K, F, hub=True)
    x, w, go = _inputs(rng, g, C, r)
    off = g.transposed()[0]
    l = _lib.lib()
    balanced = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    _lib.check(l.sph3d_graph_balanced_order(B, N, F, P(off), P(balanced), S()))
    xyz, spatial = _t(rng.rand(B, N, 3).astype(np.float32), dev), torch.full((B, N), -1, dtype=torch.int32, device=dev)
    _lib.check(l.sph3d_spatial_order(B, N, P(xyz), P(spatial), S()))
    rev = _t(np.broadcast_to(np.arange(N - 1, -1, -1, dtype=np.int32), (B, N)), dev)
    ref, first = None, None
    for name, order in (("NULL", None), ("balanced", balanced), ("spatial", spatial), ("reversed", rev)):
        if order is not None:
            assert (np.sort(_n(order), axis=1) == np.arange(N)).all(), name + ": a permutation per cloud"
        got, ref = _check_grad(g, x, w, go, "source_order " + name, dict(kernel="vec", PARTS=2, compact=False), ref=ref, order=order,
                               launches=2)
        first = got if first is None else first
        np.testing.assert_array_equal(bits(got[0]), bits(first[0]), err_msg="grad_input does not depend on the order: " + name)


@pytest.mark.parametrize("C,r", [(8, 2), (128, 2), (6, 1)])
def test_gradient_packed_and_key_scale_entries(dev, C, r):
    g, rng = _random_graph(dev, 269, 2, 70, 150, 9, 33, hub=True)
    x, w, go = _inputs(rng, g, C, r)
    got, ref = _check_grad(g, x, w, go, "packed", dict(kernel="vec"), entries="packed", launches=2)
    _check_grad(g, x, w, go, "key + scale", dict(kernel="vec"), entries="arrays", ref=ref, launches=2)
    assert g.transposed("packed")[2] is None and g.transposed("arrays")[2] is not None


@pytest.mark.parametrize("C,r", [(8, 2), (132, 1)])
def test_gradient_packed_entries_with_counts_to_200(dev, C, r):
    B, N, M, K, F = 1, 256, 40, 200, 33
    g, rng = _random_graph(dev, 271, B, N, M, K, F, high_from=128)
    assert int((g.cnt >= 128).sum()) >= M // 2 and g.cnt.max() == 200
    assert bool((g.transposed("packed")[1][: int(g.cnt.sum())] < 0).any())        # counts from 128 reach the word's sign bit
    x, w, go = _inputs(rng, g, C, r)
    _check_grad(g, x, w, go, "K=200 packed", dict(kernel="vec"), launches=2)


# ---- gradient: the hub path ---------------------------------------------------------------------------------------------------------------
def _many_hubs_graph(dev, T, B=2):
    """200 sources: source 0 has exactly T in-edges, source 1 T + 1, sources 2..141 between T + 1 and 5 T (more than 128 hubs: the
    hub launch's item loop runs twice), the others at most T; 12 bins occur"""
    rng = np.random.RandomState(277)
    pool, seg = [0, 2, 3, 5, 8, 13, 21, 22, 23, 30, 31, 32], {}

    def spread(n, deg):
        for _ in range(deg):
            k = (n, int(pool[rng.randint(0, 3 if n % 2 else len(pool))]))
            seg[k] = seg.get(k, 0) + 1
    spread(0, T)
    spread(1, T + 1)
    for n in range(2, 142):
        spread(n, int(rng.randint(T + 1, 5 * T + 1)))
    for n in range(142, 200):
        spread(n, int(rng.randint(0, T + 1)))
    g, rng = _graph_from_segments(dev, 281, B, 200, 33, seg, K=8)
    assert g.A == 12
    return g, rng


@pytest.mark.parametrize("active", [True, False], ids=["compact", "full"])
@pytest.mark.parametrize("C,r,parts", HUB_CASES, ids=["C%d-r%d" % c[:2] for c in HUB_CASES])
def test_gradient_hub_path(dev, hub_env, C, r, parts, active):
    T = 8
    g, rng = _many_hubs_graph(dev, T)
    x, w, go = _inputs(rng, g, C, r)
    _hubs(1 << 30, T)
    plain, ref = _check_grad(g, x, w, go, "ordinary path", dict(kernel="vec", PARTS=parts, hub=False, compact=active), active=active)
    deg = ref.deg
    assert (deg[:, 0] == T).all() and (deg[:, 1] == T + 1).all() and ((deg > T).sum(axis=1) > 128).all()
    _hubs(1, T)
    hub, _ = _check_grad(g, x, w, go, "hub path T=%d" % T, dict(kernel="vec", PARTS=parts, hub=True, compact=active), active=active, ref=ref)
    rows = deg <= T                                                              # source 0 among them: exactly T is no hub
    np.testing.assert_array_equal(bits(hub[0])[rows], bits(plain[0])[rows], err_msg="non-hub rows are the ordinary path's")


@pytest.mark.parametrize("C,r,active", [(8, 2, True), (64, 2, False), (132, 1, True)])
def test_gradient_hub_of_more_than_2048_in_edges(dev, hub_env, C, r, active):
    B, N, M, K, F, T = 2, 64, 2304, 4, 33, 256
    rng = np.random.RandomState(283)
    idx = rng.randint(1, N, size=(B, M, K)).astype(np.int32)
    idx[:, :, :2] = 0                                                            # source 0 twice in every row
    cnt = rng.randint(2, K + 1, size=(B, M)).astype(np.int32)
    g = Graph(dev, idx, cnt, make_bins(rng, idx, cnt, F, pool=[1, 4, 9, 16, 25]), N, F)
    x, w, go = _inputs(rng, g, C, r)
    _hubs(1, T)
    got, ref = _check_grad(g, x, w, go, "one source of 4608 in-edges", dict(kernel="vec", hub=True, compact=active), active=active)
    assert (ref.deg[:, 0] == 2 * M).all() and 2 * M > 2 * 64 * 32 and (ref.deg[:, 1:] <= T).all()       # every wave of the group: 2+ chunks


def test_gradient_hub_path_two_inputs(dev, hub_env):
    T, (Ca, Cb, r) = 8, CAT_SHAPES[0]
    g, rng = _many_hubs_graph(dev, T, B=1)
    x, w, go = _inputs(rng, g, Ca + Cb, r)
    _hubs(1, T)
    form = grad_form(g.B, g.N, g.M, g.F, Ca + Cb, r, True, g.A)
    assert form["hub"] and form["compact"] and form["PARTS"] == 1 and cat_ok(g.F, Ca, Cb, r)
    ref = conv_grad_ref(x, w, go, g.idx, g.cnt, g.bins)
    form["tag"] += " two inputs"
    _assert_grad(_grad(g, x, w, go, cat=Ca), ref, form, r, "Ca=%d Cb=%d" % (Ca, Cb), ref.deg > T)


# ---- gradient: two inputs, the wrapper, empty dimensions ------------------------------------------------------------------------------
@pytest.mark.parametrize("Ca,Cb,r", CAT_SHAPES)
def test_gradient_two_inputs(dev, Ca, Cb, r):
    g, rng, seg = _segment_graph(dev)
    C = Ca + Cb
    assert cat_ok(g.F, Ca, Cb, r) and _lib.lib().sph3d_depthwise_conv3d_cat_supported(g.F, Ca, Cb, r) == 1
    x, w, go = _inputs(rng, g, C, r)
    plain, ref = _check_grad(g, x, w, go, "plain op on the concatenation", dict(kernel="vec", V=4, PARTS=1, hub=False, compact=True))
    two = _grad(g, x, w, go, cat=Ca, launches=2)
    np.testing.assert_array_equal(bits(two[0]), bits(plain[0]))
    np.testing.assert_array_equal(bits(two[1]), bits(plain[1]))


@pytest.mark.parametrize("C,r", [(8, 2), (3, 1)], ids=["vec", "generic"])
def test_gradient_wrapper_builds_its_own_transpose(dev, C, r):
    g, rng = _random_graph(dev, 293, 3, 70, 150, 9, 33, hub=True)
    B, N, M, K, F = g.B, g.N, g.M, g.K, g.F
    x, w, go = _inputs(rng, g, C, r)
    l = _lib.lib()
    need = l.sph3d_depthwise_conv3d_grad_workspace(B, N, M, F, C, r, K)
    assert need > bwd_layout(B, N, F, C, r)["bytes"]
    xt, wt, got, ws = _t(x, dev), _t(w, dev), _t(go, dev), _ff(need, dev)

    def call(nbytes):
        gi, gf = _nan((B, N, C), dev), _nan((F, C, r), dev)
        rc = l.sph3d_depthwise_conv3d_grad(B, N, M, F, C, r, K, P(g.it), P(g.ct), P(g.bt), P(xt), P(wt), P(got), P(gi), P(gf), P(ws), nbytes, S())
        return rc, _n(gi), _n(gf)
    rc, gi, gf = call(need - 1)
    assert rc == EWORKSPACE and np.isnan(gi).all() and np.isnan(gf).all()
    rc, gi, gf = call(need)
    assert rc == 0
    form = grad_form(B, N, M, F, C, r, True, g.A)
    form["tag"] += " wrapper"
    _assert_grad((gi, gf), conv_grad_ref(x, w, go, g.idx, g.cnt, g.bins), form, r, "sph3d_depthwise_conv3d_grad")


def test_empty_batch_and_no_rows(dev):
    """B = 0: the forward writes nothing, the gradient zeroes grad_filter (grad_input has no element); M = 0: the forward writes
    nothing (there is no output row), the gradients are fully written: zeros"""
    l, F, N, K = _lib.lib(), 33, 20, 4
    one = torch.zeros((16,), dtype=torch.int32, device=dev)
    for C, r in ((8, 2), (3, 1)):
        x, w = _t(make_values(np.random.RandomState(1), (2, N, C)), dev), _t(make_values(np.random.RandomState(2), (F, C, r)), dev)
        out = _nan((4, C * r), dev)
        for B, M in ((0, 5), (2, 0)):
            assert l.sph3d_depthwise_conv3d(B, N, M, F, C, r, K, P(one), P(one), P(one), P(x), P(w), P(out), S()) == 0
        assert bool(torch.isnan(out).all())
        gi, gf = _nan((2, N, C), dev), _nan((F, C, r), dev)
        assert l.sph3d_depthwise_conv3d_grad_t(0, N, 5, F, C, r, None, None, None, None, None, P(x), P(w), P(out), P(gi), P(gf), None, 0, S()) == 0
        assert bool(torch.isnan(gi).all()) and (bits(_n(gf)) == 0).all()
        # M = 0: a transposed graph without entries (offsets[b, :] = b M K = 0)
        gi, gf = _nan((2, N, C), dev), _nan((F, C, r), dev)
        off = torch.zeros((2 * (N * F + 1),), dtype=torch.int32, device=dev)
        wsb = l.sph3d_depthwise_conv3d_grad_t_workspace(2, N, F, C, r)
        ws = _ff(wsb, dev)
        assert l.sph3d_depthwise_conv3d_grad_t(2, N, 0, F, C, r, P(off), P(one), None, None, None, P(x), P(w), P(out), P(gi), P(gf), P(ws), wsb,
                                               S()) == 0
        assert (bits(_n(gi)) == 0).all() and (bits(_n(gf)) == 0).all()


# ---- non-finite gradients -------------------------------------------------------------------------------------------------------------
def conv_seg(g):
    """edges per (cloud, source, bin) [B, N, F]"""
    seg = np.zeros((g.B, g.N, g.F), np.int64)
    b, m, k = np.nonzero(g.live)
    np.add.at(seg, (b, g.idx[b, m, k], clamp_bins(g.bins[b, m, k], g.F)), 1)
    return seg


NONFINITE_CASES = [(8, 2, 33, 4), (34, 2, 33, 2), (132, 1, 33, 1), (6, 1, 33, 1), (3, 1, 33, 0)]


@pytest.mark.parametrize("C,r,F,parts", NONFINITE_CASES, ids=["quarter-waves", "half-waves", "full-wave", "two-per-lane", "generic"])
def test_non_finite_grad_output(dev, C, r, F, parts):
    """+inf, -inf and NaN in single grad_output elements (include/sph3d.h at sph3d_depthwise_conv3d_grad_t).  grad_input is
    non-finite exactly where the float64 statement is.  grad_filter is non-finite at least there and, in the half- and
    quarter-wave forms — whose batches of 6 or 8 edges run past a segment's end and multiply the extra rows, in-edges of the same
    source in other bins, by a scale of exactly 0 —, at most in the bad channel of the bins in which a source fed by the bad row
    has an in-edge.  The full-wave bodies (V = 4 with C r > 128, V = 2) and the generic kernel take exact remainders: for them
    the two sets are equal.  Finite elements stay within the derived bounds."""
    g, rng, seg = _segment_graph(dev)
    x, w, go = _inputs(rng, g, C, r)
    CR = C * r
    form = grad_form(g.B, g.N, g.M, F, C, r, True, g.A)
    assert (form["kernel"] == "generic") == (parts == 0) and (parts == 0 or form["PARTS"] == parts)
    rows = [int(m) for m in np.nonzero((g.cnt >= 2).all(axis=0))[0][[0, 7, 19]]]
    bad = [(0, rows[0], 0, np.inf), (1, rows[1], CR - 1, -np.inf), (g.B - 1, rows[2], CR // 2, np.nan)]
    allowed, seg_edges = np.zeros((F, CR), bool), conv_seg(g)
    for b, m, j, v in bad:
        go[b, m, j] = v
        fed = np.unique(g.idx[b, m, :g.cnt[b, m]])
        allowed[:, j] |= (seg_edges[b, fed] > 0).any(axis=0)
    ref = conv_grad_ref(x, w, go, g.idx, g.cnt, g.bins)
    gi, gf = _grad(g, x, w, go)
    bad_i, bad_f = ~np.isfinite(gi), ~np.isfinite(gf)
    ref_i, ref_f = ~np.isfinite(ref.gi), ~np.isfinite(ref.gf)
    assert ref_i.any() and ref_f.any() and not ref_f.reshape(F, CR)[~allowed].any()
    np.testing.assert_array_equal(bad_i, ref_i, err_msg="grad_input: non-finite exactly where the statement is")
    assert not (ref_f & ~bad_f).any(), "grad_filter: finite where the statement is not"
    assert not (bad_f.reshape(F, CR) & ~allowed).any(), "grad_filter: non-finite outside the bad channel of the fed sources' bins"
    extra = int((bad_f & ~ref_f).sum())
    print("[%s] grad_filter elements non-finite beyond the statement's: %d of %d allowed" % (form["tag"], extra, int(allowed.sum() - ref_f.sum())))
    if parts in (0, 1):
        assert extra == 0, "exact remainders: no row is read with a scale of 0"
    z = lambda a, m: np.where(m, 0, a)
    _assert_grad((z(gi, bad_i), z(gf, bad_f)), _Masked(ref, bad_i, bad_f), form, r, "finite elements")


class _Masked:
    """a ConvGrad with the given elements taken out of the comparison (value and magnitude 0)"""

    def __init__(self, ref, bad_i, bad_f):
        self.gi, self.gi_mag = np.where(bad_i, 0, ref.gi), np.where(bad_i, 0, ref.gi_mag)
        self.gf, self.gf_mag = np.where(bad_f, 0, ref.gf), np.where(bad_f, 0, ref.gf_mag)
        self.gi_terms, self.gf_terms = ref.gi_terms, ref.gf_terms
