"""The conv gradient for odd row widths (r = 1, odd C: dwconv_bwd_t_odd of csrc/conv3d.hip), the fixed-order kernel that
deterministic mode runs where dwconv_bwd_t_generic would add with float atomics — per element against float64
(tests/_conv_ref.py: the project's derived bounds, nothing new), through the C ABI like tests/test_gpu_conv_forms.py, whose host
graph makers and device helpers it uses.  tests/_conv_forms.py restates the launch plan; the workspace bytes it gives are
compared with the library's answer in the mode, and outside it the same shapes must still ask for no workspace and run.

Outputs are pre-filled with NaN, the workspace with 0xFF bytes.  Every comparison of bit patterns is exact.  The switch is off
after every test."""
import numpy as np
import pytest
import torch

from _conv_forms import ODD_CHANNELS as CHANNELS, dims_ok, odd_form, odd_layout, vec_plan
from _conv_ref import assert_conv, bits, conv_grad_ref, make_bins, make_graph, make_values
from test_gpu_conv_forms import Graph, _ff, _graph_from_segments, _n, _nan, _random_graph, _t
import sph3d_gcn_amd as pkg
from sph3d_gcn_amd import _lib, _tgraph

pytestmark = pytest.mark.gpu
P, S = _lib.ptr, _lib.stream_ptr
EUNSUPPORTED = -4
B, N, M = 3, 300, 77                     # three clouds: a ragged deal of (cloud, part) items to the 8 XCDs; N != M


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    pkg.set_deterministic(False)
    _tgraph.clear()
    yield
    pkg.set_deterministic(False)
    _tgraph.clear()
    assert _lib.lib().sph3d_get_deterministic() == 0


def _grad(g, x, w, go, form, entries="packed", order=None, launches=1):
    """sph3d_depthwise_conv3d_grad_t at the mode's current value, on a transposed graph built at that value -> (gi, gf); the
    library's workspace answer must be the restated plan's; a second launch on the workspace as the first left it: the same bits"""
    (F, C, r), l, dev = w.shape, _lib.lib(), g.dev
    g._tg = {}                                                            # (a graph built at the mode's other value is not reused)
    off, key, scale, act = g.transposed(entries, True)
    wsb = l.sph3d_depthwise_conv3d_grad_t_workspace(g.B, g.N, F, C, r)
    assert wsb == form["bytes"], "workspace: the library says %d B, the restated plan %d B" % (wsb, form["bytes"])
    ws = _ff(wsb, dev)
    xt, wt, got, outs = _t(x, dev), _t(w, dev), _t(go, dev), []
    for _ in range(launches):
        gi, gf = _nan((g.B, g.N, C), dev), _nan((F, C, r), dev)
        _lib.check(l.sph3d_depthwise_conv3d_grad_t(g.B, g.N, g.M, F, C, r, P(off), P(key), P(scale), P(order), P(act), P(xt), P(wt), P(got),
                                                   P(gi), P(gf), P(ws) if wsb else None, wsb, S()))
        outs.append((_n(gi), _n(gf)))
    for o in outs[1:]:
        np.testing.assert_array_equal(bits(o[0]), bits(outs[0][0]), err_msg="grad_input of a second launch")
        np.testing.assert_array_equal(bits(o[1]), bits(outs[0][1]), err_msg="grad_filter of a second launch")
    return outs[0]


def _assert(got, ref, form, what):
    tag = "[%s] %s" % (form["tag"], what)
    assert_conv(got[0], ref.gi, ref.gi_mag, ref.gi_terms(1), tag + ": grad_input")
    assert_conv(got[1], ref.gf, ref.gf_mag, ref.gf_terms(form["depth"]), tag + ": grad_filter")


def _inputs(rng, g, C):
    return make_values(rng, (g.B, g.N, C)), make_values(rng, (g.F, C, 1)), make_values(rng, (g.B, g.M, C))


def _check(g, x, w, go, what, T=None, orders=False):
    """one shape, in the mode (the odd-width kernel, both entry forms) and out of it (the generic kernel, no workspace) -> ref"""
    F, C, r = w.shape
    assert r == 1 and vec_plan(F, C, 1) == 0 and dims_ok(F, C, 1)
    ref = conv_grad_ref(x, w, go, g.idx, g.cnt, g.bins)
    with pkg.deterministic():
        form = odd_form(g.B, g.N, g.M, F, C, 1, True)
        assert form["kernel"] == "odd" and (T is None or form["T"] == T) and form["bytes"] == 4 * form["slabs"] * F * C > 0
        packed = _grad(g, x, w, go, form, launches=2)
        _assert(packed, ref, form, what)
        arrays = _grad(g, x, w, go, form, entries="arrays")
        np.testing.assert_array_equal(bits(arrays[0]), bits(packed[0]), err_msg=what + ": grad_input, key + scale entries")
        np.testing.assert_array_equal(bits(arrays[1]), bits(packed[1]), err_msg=what + ": grad_filter, key + scale entries")
        if orders:
            rev = _t(np.broadcast_to(np.arange(g.N - 1, -1, -1, dtype=np.int32), (g.B, g.N)), g.dev)
            swept = _grad(g, x, w, go, form, order=rev, launches=2)
            np.testing.assert_array_equal(bits(swept[0]), bits(packed[0]), err_msg=what + ": grad_input does not depend on the order")
            _assert(swept, ref, form, what + ", reversed source_order")
    off = odd_form(g.B, g.N, g.M, F, C, 1, False)
    assert off["kernel"] == "generic" and off["bytes"] == 0
    _assert(_grad(g, x, w, go, off), ref, off, what + ", mode off")
    return ref


# ---- small graphs, every channel count ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CHANNELS)
def test_odd_widths_hold_the_float64_bounds(dev, C):
    F = 33
    T = {1: 1, 3: 1, 35: 1, 63: 1, 65: 2, 67: 2, 131: 3, 255: 4, 257: 4}[C]
    assert odd_layout(B, N, F, C, 1)["nslices"] == (2 if C == 257 else 1)
    # K = 6: ~230 edges per cloud over 300 sources, every bin live; K = 64: long rows, 17 of the 33 bins live
    g6, rng = _random_graph(dev, 307 + C, B, N, M, 6, F)
    assert g6.A == 33
    ref = _check(g6, *_inputs(rng, g6, C), "C=%d K=6, 33 bins live" % C, T=T)
    assert (ref.deg == 0).any() and (ref.deg > 0).any(), "sources without in-edges get a zero row"
    g64, rng = _random_graph(dev, 311 + C, B, N, M, 64, F, pool=np.arange(0, F, 2))
    assert g64.A == 17
    ref = _check(g64, *_inputs(rng, g64, C), "C=%d K=64, 17 bins live" % C, T=T, orders=C in (67, 257))
    assert ref.deg.max() > 8 and (ref.seg > 1).any()                      # mean in-degree 8 (batches of four, chunk boundaries: test_a_star)


@pytest.mark.parametrize("C,F", [(3, 49), (67, 49), (67, 65)])
def test_odd_widths_at_more_than_33_bins(dev, C, F):
    """the 65-row table: T <= 2 (C = 67: two channels per lane, one slice); F = 65: bounds 64 and 65 live in the second register"""
    g, rng = _random_graph(dev, 313 + F, B, N, M, 64, F)
    assert g.A == F and odd_layout(B, N, F, C, 1)["MAXF"] == 65
    _check(g, *_inputs(rng, g, C), "C=%d F=%d" % (C, F), T=1 if C == 3 else 2)


@pytest.mark.parametrize("C", [3, 131])
def test_odd_widths_in_131_channels_at_49_bins_take_two_slices(dev, C):
    g, rng = _random_graph(dev, 317, B, N, M, 6, 49)
    L = odd_layout(B, N, 49, C, 1)
    assert (L["T"], L["nslices"]) == ((1, 1) if C == 3 else (2, 2))        # 131 = 128 + 3
    _check(g, *_inputs(rng, g, C), "C=%d F=49 K=6" % C)


@pytest.mark.parametrize("C", [3, 67, 131])
def test_an_extra_cloud_without_edges(dev, C):
    F, K = 33, 6
    rng = np.random.RandomState(331)
    idx, cnt = make_graph(rng, B + 1, N, M, K)
    cnt[B] = 0
    g = Graph(dev, idx, cnt, make_bins(rng, idx, cnt, F), N, F)
    ref = _check(g, *_inputs(rng, g, C), "C=%d, cloud %d empty" % (C, B))
    assert (ref.deg[B] == 0).all() and (ref.deg[:B] > 0).any()


@pytest.mark.parametrize("C", [3, 67, 257])
def test_a_star(dev, C):
    """source 5: 150 in-edges in bin 4 (three 64-edge chunks, the chunk boundaries inside the segment) and 3 in bin 7; sources of
    61, 64 and 65 in-edges in one bin; most of the 40 sources have none"""
    seg = {(5, 4): 150, (5, 7): 3, (1, 0): 2, (2, 32): 1, (7, 4): 64, (8, 4): 65, (9, 10): 61, (30, 31): 7, (30, 32): 5}
    g, rng = _graph_from_segments(dev, 337, 2, 40, 33, seg, K=8)
    ref = _check(g, *_inputs(rng, g, C), "C=%d star" % C)
    assert ref.seg[0, 5, 4] == 150 and ref.deg.max() == 153 and (ref.deg == 0).sum() > 40


# ---- rebuilt graphs, entry forms, the wrapper ---------------------------------------------------------------------------------------
def _package_grad(g, xt, wt, got):
    """the C entry on the package's transposed graph (_tgraph.transpose, its source order) -> bits of (grad_input, grad_filter)"""
    (F, C, r), l = wt.shape, _lib.lib()
    off, key, scale, act = _tgraph.transpose(g.it, g.ct, g.N, bin_index=g.bt, num_bins=F)
    wsb = l.sph3d_depthwise_conv3d_grad_t_workspace(g.B, g.N, F, C, r)
    ws = _ff(wsb, g.dev)
    gi, gf = _nan((g.B, g.N, C), g.dev), _nan((F, C, r), g.dev)
    _lib.check(l.sph3d_depthwise_conv3d_grad_t(g.B, g.N, g.M, F, C, r, P(off), P(key), P(scale), P(_tgraph.source_order(g.it)), P(act),
                                               P(xt), P(wt), P(got), P(gi), P(gf), P(ws), wsb, S()))
    torch.cuda.synchronize()
    return bits(_n(gi)), bits(_n(gf))


@pytest.mark.parametrize("C", [67, 131])
def test_rebuilt_graphs_and_both_entry_forms_give_the_same_bits(dev, C):
    g, rng = _random_graph(dev, 347, B, N, M, 64, 33)
    x, w, go = _inputs(rng, g, C)
    xt, wt, got = _t(x, dev), _t(w, dev), _t(go, dev)
    old = _tgraph.PACK_ENTRIES
    try:
        with pkg.deterministic():
            first = None
            for run in range(5):
                _tgraph.clear()
                now = _package_grad(g, xt, wt, got)
                assert len(_tgraph._cache) >= 1
                first = now if first is None else first
                np.testing.assert_array_equal(now[0], first[0], err_msg="grad_input, rebuild %d" % run)
                np.testing.assert_array_equal(now[1], first[1], err_msg="grad_filter, rebuild %d" % run)
            _tgraph.PACK_ENTRIES = not old
            _tgraph.clear()
            other = _package_grad(g, xt, wt, got)
            assert (next(iter(_tgraph._cache.values()))[0][2] is None) == _tgraph.PACK_ENTRIES
    finally:
        _tgraph.PACK_ENTRIES = old
    np.testing.assert_array_equal(other[0], first[0], err_msg="grad_input, packed against separate entries")
    np.testing.assert_array_equal(other[1], first[1], err_msg="grad_filter, packed against separate entries")


def test_the_wrapper_reaches_the_kernel(dev):
    """sph3d_depthwise_conv3d_grad builds its transposed graph itself: in the mode its workspace is the graph's plus the slabs,
    and its result has the bits of the prebuilt-graph entry in index order"""
    C, F, K = 67, 33, 6
    g, rng = _random_graph(dev, 349, B, N, M, K, F)
    x, w, go = _inputs(rng, g, C)
    l = _lib.lib()
    xt, wt, got = _t(x, dev), _t(w, dev), _t(go, dev)
    # (C = 5, r = 3: a shape of the generic kernel in and out of the mode, so its answer is the transposed graph's bytes alone)
    assert l.sph3d_depthwise_conv3d_grad_workspace(B, N, M, F, C, 1, K) == l.sph3d_depthwise_conv3d_grad_workspace(B, N, M, F, 5, 3, K)
    with pkg.deterministic():
        form = odd_form(B, N, M, F, C, 1, True)
        need = l.sph3d_depthwise_conv3d_grad_workspace(B, N, M, F, C, 1, K)
        assert need == l.sph3d_depthwise_conv3d_grad_workspace(B, N, M, F, 5, 3, K) + form["bytes"]
        ws = _ff(need, dev)
        gi, gf = _nan((B, N, C), dev), _nan((F, C, 1), dev)
        _lib.check(l.sph3d_depthwise_conv3d_grad(B, N, M, F, C, 1, K, P(g.it), P(g.ct), P(g.bt), P(xt), P(wt), P(got), P(gi), P(gf), P(ws),
                                                 need, S()))
        direct = _grad(g, x, w, go, form)
    np.testing.assert_array_equal(bits(_n(gi)), bits(direct[0]))
    np.testing.assert_array_equal(bits(_n(gf)), bits(direct[1]))
    _assert((_n(gi), _n(gf)), conv_grad_ref(x, w, go, g.idx, g.cnt, g.bins), dict(form, tag=form["tag"] + " wrapper"), "C=67")


@pytest.mark.parametrize("C,r,F", [(67, 1, 66), (5, 3, 33), (3, 3, 5)])
def test_shapes_outside_the_plan_still_refuse(dev, C, r, F):
    g, rng = _random_graph(dev, 353, 2, 60, 80, 6, F)
    x, w, go = make_values(rng, (2, 60, C)), make_values(rng, (F, C, r)), make_values(rng, (2, 80, C * r))
    assert vec_plan(F, C * r, r) == 0 and odd_layout(2, 60, F, C, r)["T"] == 0
    l = _lib.lib()
    with pkg.deterministic():
        assert odd_form(2, 60, 80, F, C, r, True)["kernel"] == "refused"
        assert l.sph3d_depthwise_conv3d_grad_t_workspace(2, 60, F, C, r) == 0
        off, key, scale, act = g.transposed()
        gi, gf = _nan((2, 60, C), dev), _nan((F, C, r), dev)
        rc = l.sph3d_depthwise_conv3d_grad_t(2, 60, 80, F, C, r, P(off), P(key), P(scale), None, P(act), P(_t(x, dev)), P(_t(w, dev)),
                                             P(_t(go, dev)), P(gi), P(gf), None, 0, S())
        torch.cuda.synchronize()
        text = l.sph3d_last_error().decode()
    assert rc == EUNSUPPORTED and "deterministic mode" in text and "float atomics" in text
    assert bool(torch.isnan(gi).all()) and bool(torch.isnan(gf).all())          # nothing was written
