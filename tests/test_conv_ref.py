"""tests/_conv_ref.py proved on the CPU: the float64 statement of the depthwise convolution and its gradient gives the answers
worked out by hand on small graphs, agrees with the fp32 C oracle (the reference's behaviour), equals itself in the gather form
the gradient kernel uses (over tests/_tgraph_ref.py's transposed graph), and its checker catches the defects that a chunked,
segment-wise kernel with a slab workspace can have."""
import numpy as np
import pytest

import oracle
from _conv_forms import FWD_CASES, HUB_CASES, PLAN_CASES, V2_CASES, grad_form
from _conv_ref import (U, assert_conv, conv_grad_ref, conv_ref, clamp_bins, make_bins, make_graph, make_values, reduce_depth)
from _errors import assert_per_element
from _tgraph_ref import transpose_reference


# ---- hand graphs ----------------------------------------------------------------------------------------------------------------
def test_hand_graphs():
    F, C, r = 4, 2, 2
    w = np.arange(1, F * C * r + 1, dtype=np.float32).reshape(F, C, r)            # w[f, c, rho] = 1 + 4 f + 2 c + rho
    x = np.array([[[1, 2], [3, 5], [7, 11], [13, 17]]], np.float32)               # B = 1, N = 4 (source 3: no in-edge)
    go = np.array([[[1, 10, 100, 1000], [2, 20, 200, 2000], [4, 40, 400, 4000], [8, 80, 800, 8000]]], np.float32)
    #   row 0: one edge, source 1, bin 2       row 1: empty (its slots hold ids and bins that must not be read)
    #   row 2: source 2 twice (bins 1 and 1)   row 3: sources 0 and 1, bin ids -3 (-> 0) and F + 5 (-> F - 1)
    idx = np.array([[[1, 0, 0], [2, 2, 2], [2, 2, 0], [0, 1, 3]]], np.int32)
    cnt = np.array([[1, 0, 2, 2]], np.int32)
    bins = np.array([[[2, 9, 9], [1, 1, 1], [1, 1, 9], [-3, F + 5, 2]]], np.int32)
    out, mag, terms = conv_ref(x, w, idx, cnt, bins)
    want = np.zeros((1, 4, 4))
    want[0, 0] = [3 * 9, 3 * 10, 5 * 11, 5 * 12]                                     # x[1] * w[2]
    want[0, 2] = [7 * 5, 7 * 6, 11 * 7, 11 * 8]                                      # (2 x[2] * w[1]) / 2
    want[0, 3] = [(1 * 1 + 3 * 13) / 2, (1 * 2 + 3 * 14) / 2, (2 * 3 + 5 * 15) / 2, (2 * 4 + 5 * 16) / 2]
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(mag, want)                                         # every operand is positive
    np.testing.assert_array_equal(terms[0, :, 0], cnt[0])
    assert (out[0, 1] == 0).all() and (mag[0, 1] == 0).all()

    g = conv_grad_ref(x, w, go, idx, cnt, bins)
    np.testing.assert_array_equal(g.deg, [[1, 2, 2, 0]])
    np.testing.assert_array_equal(g.nseg, [[1, 2, 1, 0]])                            # source 1: bins 2 and 3; source 2: bin 1 twice
    np.testing.assert_array_equal(g.E_f, [1, 2, 1, 1])
    np.testing.assert_array_equal(g.S_f, [1, 1, 1, 1])
    gi = np.zeros((1, 4, 2))
    gi[0, 0] = [(8 * 1 + 80 * 2) / 2, (800 * 3 + 8000 * 4) / 2]                      # row 3, bin 0
    gi[0, 1] = [1 * 9 + 10 * 10 + (8 * 13 + 80 * 14) / 2, 100 * 11 + 1000 * 12 + (800 * 15 + 8000 * 16) / 2]
    gi[0, 2] = [4 * 5 + 40 * 6, 400 * 7 + 4000 * 8]                                  # two edges of weight 1 / 2 each
    np.testing.assert_array_equal(g.gi, gi)
    assert (g.gi[0, 3] == 0).all() and (g.gi_mag[0, 3] == 0).all()
    gf = np.zeros((F, C, r))
    gf[0] = [[8 * 1 / 2, 80 * 1 / 2], [800 * 2 / 2, 8000 * 2 / 2]]                   # row 3 -> source 0
    gf[1] = [[4 * 7, 40 * 7], [400 * 11, 4000 * 11]]                                 # row 2 -> source 2, twice a half
    gf[2] = [[1 * 3, 10 * 3], [100 * 5, 1000 * 5]]                                   # row 0 -> source 1
    gf[3] = [[8 * 3 / 2, 80 * 3 / 2], [800 * 5 / 2, 8000 * 5 / 2]]                   # row 3 -> source 1
    np.testing.assert_array_equal(g.gf, gf)
    np.testing.assert_array_equal(g.gf_mag, gf)
    np.testing.assert_array_equal(g.gi_terms(r)[0, :, 0], [2 + 1 + 4, 4 + 2 + 4, 4 + 1 + 4, 4])
    np.testing.assert_array_equal(g.gf_terms(reduce_depth(8))[:, 0, 0], np.array([2, 4, 2, 2]) + 1 + 5 + 32)


# ---- the statement against the oracle ----------------------------------------------------------------------------------------------
def _hub(rng, B, N, M, K):
    """source N - 1 closes 5 of 6 rows that have a neighbour; the other rows list ascending ids below it"""
    idx, cnt = make_graph(rng, B, N - 1, M, K)
    for b in range(B):
        has = np.nonzero(cnt[b] >= 1)[0]
        has = has[has % 6 != 0]
        idx[b, has, cnt[b, has] - 1] = N - 1
    return idx, cnt


#          name     B  N    M    K   F   C  r  unique
GRAPHS = [("intra", 2, 96, 96, 19, 33, 8, 2, True), ("inter", 2, 120, 50, 12, 17, 6, 1, True),
          ("K70", 1, 80, 40, 70, 33, 4, 2, False), ("hub", 2, 64, 600, 6, 5, 4, 2, True)]


def _case(name, seed=0, out_of_range=False):
    _n, B, N, M, K, F, C, r, unique = next(g for g in GRAPHS if g[0] == name)
    rng = np.random.RandomState(97 * seed + N + K)
    idx, cnt = _hub(rng, B, N, M, K) if name == "hub" else make_graph(rng, B, N, M, K, unique=unique)
    bins = make_bins(rng, idx, cnt, F)
    if out_of_range:
        live = np.arange(K)[None, None, :] < cnt[:, :, None]
        bins = np.where(live & (rng.rand(*bins.shape) < 0.2), F + 5, bins).astype(np.int32)
        assert (bins[live] == F + 5).sum() > 20
    return (make_values(rng, (B, N, C)), make_values(rng, (F, C, r)), make_values(rng, (B, M, C * r)), idx, cnt, bins)


@pytest.mark.parametrize("name", [g[0] for g in GRAPHS])
def test_statement_equals_the_oracle(name):
    x, w, go, idx, cnt, bins = _case(name)
    r = w.shape[2]
    ref, mag, terms = conv_ref(x, w, idx, cnt, bins)
    got = oracle.depthwise_conv3d(x, w, idx, cnt, bins)
    assert_per_element(got, ref, mag, "oracle forward, " + name)
    g = conv_grad_ref(x, w, go, idx, cnt, bins)
    if name == "hub":
        assert g.deg.max() >= 400
    gi_o, gf_o = oracle.depthwise_conv3d_grad(x, w, go, idx, cnt, bins)
    assert_per_element(gi_o, g.gi, g.gi_mag, "oracle grad_input, " + name)
    assert_per_element(gf_o, g.gf, g.gf_mag, "oracle grad_filter, " + name)
    # for information: the oracle divides every term, so its rounding count is not the kernels'
    for what, a, ref64, m, t in (("forward", got, ref, mag, terms + 4), ("grad_input", gi_o, g.gi, g.gi_mag, g.gi_terms(r)),
                                 ("grad_filter", gf_o, g.gf, g.gf_mag, g.gf_terms(reduce_depth(8)))):
        bound = np.broadcast_to(t, ref64.shape) * U * m
        err = np.abs(a.astype(np.float64) - ref64)
        print("oracle %s, %s: used %.3f of the derived bound" % (what, name, float((err[bound > 0] / bound[bound > 0]).max())))


# ---- the gather form over the transposed graph ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["inter", "hub"])
def test_gather_form_equals_scatter_form(name):
    x, w, go, idx, cnt, bins = _case(name, out_of_range=True)
    B, M, K = idx.shape
    N, (F, C, r) = x.shape[1], w.shape
    L = N * F
    offsets, entries, _active = transpose_reference(idx, cnt, N, bins, F)
    off = offsets.astype(np.int64).reshape(B, L + 1)
    # the segment of a position is where the offsets put it: that must be the segment the entry list names
    seg_of_pos = np.concatenate([np.repeat(np.arange(L) + b * L, np.diff(off[b])) for b in range(B)])
    np.testing.assert_array_equal(seg_of_pos, entries[:, 0])
    gb, gl, gm = entries[:, 0] // L, entries[:, 0] % L, entries[:, 1]
    gn, gf_ = gl // F, gl % F
    # scatter form: the live slots in row order
    sb, sm, sk = np.nonzero(np.arange(K)[None, None, :] < cnt[:, :, None])
    sn, sf = idx[sb, sm, sk].astype(np.int64), clamp_bins(bins[sb, sm, sk], F)

    def terms(b, m, n, f):
        order = np.lexsort((m, f, n, b))
        b, m, n, f = b[order], m[order], n[order], f[order]
        g64 = go[b, m].astype(np.float64).reshape(-1, C, r) / cnt[b, m].astype(np.float64)[:, None, None]
        return (b * N + n, f), g64 * w[f].astype(np.float64), g64 * x[b, n].astype(np.float64)[:, :, None]

    (ks, fs), ti_s, tf_s = terms(sb, sm, sn, sf)
    (kg, fg), ti_g, tf_g = terms(gb, gm, gn, gf_)
    np.testing.assert_array_equal(ks, kg)
    np.testing.assert_array_equal(fs, fg)
    np.testing.assert_array_equal(ti_s, ti_g)                       # the same multiset of float64 terms, element for element
    np.testing.assert_array_equal(tf_s, tf_g)
    # ... and their sums are the statement's
    g = conv_grad_ref(x, w, go, idx, cnt, bins)
    gi = np.zeros((B * N, C))
    np.add.at(gi, kg, ti_g.sum(axis=2))
    gf = np.zeros((F, C, r))
    np.add.at(gf, fg, tf_g)
    assert (np.abs(gi.reshape(B, N, C) - g.gi) <= 1e-12 * g.gi_mag).all()
    assert (np.abs(gf - g.gf) <= 1e-12 * g.gf_mag).all()
    # the entries' factor is the correctly rounded fp32 quotient
    np.testing.assert_array_equal(entries[:, 2], (np.float32(1) / cnt[gb, gm].astype(np.float32)).view(np.uint32))


# ---- planted defects: fp32 numpy restatements of the kernels' sums, each with a switch that breaks it -------------------------------
def _fwd32(x, w, idx, cnt, bins, inv_of_cnt_minus_one=False, clamp_to_F=False):
    B, M, K = idx.shape
    F, C, r = w.shape
    wz = np.concatenate([w, np.zeros((1, C, r), np.float32)])              # row F: the padding slots' zero row
    acc = np.zeros((B, M, C * r), np.float32)
    for b in range(B):
        for k in range(int(cnt[b].max())):
            sel = np.nonzero(cnt[b] > k)[0]
            f = np.clip(bins[b, sel, k], 0, F if clamp_to_F else F - 1)
            acc[b, sel] += (x[b][idx[b, sel, k]][:, :, None] * wz[f]).reshape(sel.size, C * r)
    div = np.where(cnt >= 2, cnt - 1, cnt) if inv_of_cnt_minus_one else cnt
    inv = np.where(cnt > 0, np.float32(1) / np.maximum(div, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return acc * inv[:, :, None]


def _grad32(x, w, go, idx, cnt, bins, drop_last_of_six=False, chunk_first_twice=False):
    """the gather form: edges sorted by (cloud, source, bin), fp32 segment sums, then one product per segment for each gradient"""
    B, M, K = idx.shape
    N, (F, C, r) = x.shape[1], w.shape
    b, m, k = np.nonzero(np.arange(K)[None, None, :] < cnt[:, :, None])
    n, f = idx[b, m, k].astype(np.int64), clamp_bins(bins[b, m, k], F)
    order = np.lexsort((m, f, n, b))
    b, m, n, f = b[order], m[order], n[order], f[order]
    src, seg, pos = b * N + n, (b * N + n) * F + f, np.arange(b.size)
    pos_src = pos - np.searchsorted(src, src, "left")
    seg_len = np.searchsorted(seg, seg, "right") - np.searchsorted(seg, seg, "left")
    last_of_seg = pos == np.searchsorted(seg, seg, "right") - 1
    times = np.ones(b.size, np.float32)
    hit = 0
    if drop_last_of_six:
        sel = (seg_len == 6) & last_of_seg
        times[sel], hit = 0, int(sel.sum())
    if chunk_first_twice:
        sel = (pos_src > 0) & (pos_src % 64 == 0)
        times[sel], hit = 2, int(sel.sum())
    t = go[b, m] * ((np.float32(1) / cnt[b, m].astype(np.float32)) * times)[:, None]
    useg, inv = np.unique(seg, return_inverse=True)
    sg = np.zeros((useg.size, C, r), np.float32)
    np.add.at(sg, inv, t.reshape(-1, C, r))
    s_src, s_f = useg // F, useg % F
    gir = np.zeros((B * N, C, r), np.float32)
    np.add.at(gir, s_src, sg * w[s_f])
    gi = gir[:, :, 0].copy()
    for rho in range(1, r):
        gi += gir[:, :, rho]
    gf = np.zeros((F, C, r), np.float32)
    np.add.at(gf, s_f, sg * x.reshape(B * N, C)[s_src][:, :, None])
    return gi.reshape(B, N, C), gf, hit


def _assert_grad(gi, gf, g, r, what):
    return (assert_conv(gi, g.gi, g.gi_mag, g.gi_terms(r), what + ": grad_input"),
            assert_conv(gf, g.gf, g.gf_mag, g.gf_terms(reduce_depth(8)), what + ": grad_filter"))


@pytest.mark.parametrize("name", [g[0] for g in GRAPHS])
def test_the_restatements_pass_without_a_defect(name):
    x, w, go, idx, cnt, bins = _case(name, out_of_range=True)
    ref, mag, terms = conv_ref(x, w, idx, cnt, bins)
    assert_conv(_fwd32(x, w, idx, cnt, bins), ref, mag, terms + 4, "fp32 forward")
    gi, gf, _ = _grad32(x, w, go, idx, cnt, bins)
    _assert_grad(gi, gf, conv_grad_ref(x, w, go, idx, cnt, bins), w.shape[2], "fp32 gradient")


def test_a_reciprocal_of_the_count_less_one_is_caught():
    x, w, go, idx, cnt, bins = _case("intra")
    with pytest.raises(AssertionError):
        assert_conv(_fwd32(x, w, idx, cnt, bins, inv_of_cnt_minus_one=True), *conv_ref(x, w, idx, cnt, bins)[:2],
                    cnt[:, :, None] + 4, "1 / (cnt - 1)")


def test_a_clamp_to_F_is_caught():
    x, w, go, idx, cnt, bins = _case("intra", out_of_range=True)
    ref, mag, terms = conv_ref(x, w, idx, cnt, bins)
    with pytest.raises(AssertionError):
        assert_conv(_fwd32(x, w, idx, cnt, bins, clamp_to_F=True), ref, mag, terms + 4, "clamp to F: the zero row")


def test_a_dropped_last_edge_of_a_segment_of_six_is_caught():
    x, w, go, idx, cnt, bins = _case("hub")
    g = conv_grad_ref(x, w, go, idx, cnt, bins)
    gi, gf, hit = _grad32(x, w, go, idx, cnt, bins, drop_last_of_six=True)
    assert hit >= 1 and (g.seg == 6).sum() == hit
    with pytest.raises(AssertionError):
        assert_conv(gi, g.gi, g.gi_mag, g.gi_terms(2), "last of six dropped: grad_input")
    with pytest.raises(AssertionError):
        assert_conv(gf, g.gf, g.gf_mag, g.gf_terms(reduce_depth(8)), "last of six dropped: grad_filter")


def test_the_first_edge_of_a_chunk_counted_twice_is_caught():
    x, w, go, idx, cnt, bins = _case("hub")
    g = conv_grad_ref(x, w, go, idx, cnt, bins)
    gi, gf, hit = _grad32(x, w, go, idx, cnt, bins, chunk_first_twice=True)
    assert hit >= 6                                                        # the hub of each cloud: 400+ in-edges
    with pytest.raises(AssertionError):
        assert_conv(gi, g.gi, g.gi_mag, g.gi_terms(2), "chunk's first edge twice: grad_input")
    with pytest.raises(AssertionError):
        assert_conv(gf, g.gf, g.gf_mag, g.gf_terms(reduce_depth(8)), "chunk's first edge twice: grad_filter")


def test_an_unwritten_grad_input_row_is_caught():
    x, w, go, idx, cnt, bins = _case("inter")
    g = conv_grad_ref(x, w, go, idx, cnt, bins)
    gi, gf, _ = _grad32(x, w, go, idx, cnt, bins)
    assert_conv(gi, g.gi, g.gi_mag, g.gi_terms(1), "grad_input")
    row = int(np.nonzero(g.deg[1] == 0)[0][0]) if (g.deg[1] == 0).any() else 7
    gi[1, row] = np.nan                      # what a skipped store leaves of the caller's NaN fill — also in a row whose sum is 0
    with pytest.raises(AssertionError):
        assert_conv(gi, g.gi, g.gi_mag, g.gi_terms(1), "one row unwritten")


def test_a_stale_slab_is_caught():
    x, w, go, idx, cnt, bins = _case("intra")
    g = conv_grad_ref(x, w, go, idx, cnt, bins)
    gi, gf, _ = _grad32(x, w, go, idx, cnt, bins)
    assert_conv(gf, g.gf, g.gf_mag, g.gf_terms(reduce_depth(8)), "grad_filter")
    # an earlier call's partial table: one workgroup's share (a sixteenth) of another grad_output's filter gradient
    stale = _grad32(x, w, make_values(np.random.RandomState(5), go.shape), idx, cnt, bins)[1] / np.float32(16)
    with pytest.raises(AssertionError):
        assert_conv(gf + stale, g.gf, g.gf_mag, g.gf_terms(reduce_depth(8)), "a stale slab added")
    # ... and what the GPU tests' 0xFF workspace fill makes of it
    with pytest.raises(AssertionError):
        assert_conv(gf + np.float32(np.nan), g.gf, g.gf_mag, g.gf_terms(reduce_depth(8)), "a 0xFF slab added")


# ---- the GPU cases' lists name every launch form (the rules are restated in tests/_conv_forms.py) ----------
def test_every_launch_form_has_a_gpu_case(monkeypatch):
    """dwconv_bwd_t_vec at r in {1, 2}: V = 4 as R x PARTS x {compact, full} x HUB {0, 1, 2} = 36 instantiations, V = 2 as R = 2
    more (full wave, full table, no hubs).  The hub path launches HUB = 1 and HUB = 2 together, so they are 26 launch forms;
    the case lists of the GPU tests, through the restated rules, name each of them, and the forward list each forward kernel."""
    def tags(cases, hub):
        monkeypatch.setenv("SPH3D_BWD_HUB_MIN_N", "1" if hub else str(1 << 30))
        return {grad_form(2, 40, 250, 33, C, r, active, 8)["tag"] for C, r, *_ in cases for active in (True, False)}
    got = tags(PLAN_CASES, False) | tags(HUB_CASES, True) | tags([c for c in V2_CASES if c[2] == 33], False)
    want = {"bwd R%d V4 PARTS%d %s%s" % (r, p, t, h) for r in (1, 2) for p in (1, 2, 4) for t in ("compact", "full") for h in ("", " hub")}
    want |= {"bwd R1 V2 PARTS1 full", "bwd R2 V2 PARTS1 full"}
    assert got == want and len(want) == 26
    assert {c[0] for c in FWD_CASES} == ({"dwconv_fwd_multi<%d,%d>" % (r, l) for r in (1, 2) for l in (16, 32)}
                                        | {"dwconv_fwd_row<1>", "dwconv_fwd_row<2>", "dwconv_fwd_generic"})
