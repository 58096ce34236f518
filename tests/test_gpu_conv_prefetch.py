"""The conv gradient's index chain runs one source ahead of the walk (dwconv_bwd_t_vec of csrc/conv3d.hip, HUB = 0 and 1): while a
wave walks the source at position p it already holds the bounds row and the first 64 keys of the source one step on, and the
scalar loads for the sources two and three steps on are in flight.  Which wave takes which source and the order of every sum are
what they were, so nothing here is a new bound: grad_input and grad_filter per element against float64 (tests/_conv_ref.py) with
the bounds and helpers of tests/test_gpu_conv_forms.py, at the shapes where such a pipeline goes wrong —

  a wave with no source, one source, or two (the first prefetch has no successor, the last source prefetches nothing);
  clouds that are no multiple of 8 with N no multiple of `parts` (the interleaved positions run past N at different steps);
  sources without in-edges first, last, two in a row and between two busy ones in a wave's walk (their keys must not be read);
  sources of more than 64 and more than 128 in-edges (the prefetch covers the first chunk only);
  the quarter-, half- and full-wave forms and two channel slices; the compact and the full table; with and without a source
  order; packed and key + scale entries; two inputs;

and one repeat in deterministic mode on a canonical transposed graph: a register read before its load has landed shows as bits
that differ between two runs.  F = 33 throughout."""
import numpy as np
import pytest

from _conv_forms import K_BWD_WAVES, K_COMPACT_BINS, cat_ok, grad_form
from _conv_ref import bits, conv_grad_ref, make_bins
from test_gpu_conv_forms import Graph, _assert_grad, _check_grad, _grad, _inputs, _random_graph, _t
import sph3d_gcn_amd as pkg
from sph3d_gcn_amd import _lib, _tgraph

pytestmark = pytest.mark.gpu
F = 33
FEW_BINS = [0, 2, 3, 5, 8, 13, 21, 32]                               # 8 <= 17 bins: the compact table does the work
#          C r = 64 (PARTS 4), 128 (PARTS 2), 256 (PARTS 1), 512 (PARTS 1, two slices), for r = 1 and 2
WIDTHS = {1: [(64, 4), (128, 2), (256, 1), (512, 1)], 2: [(32, 4), (64, 2), (128, 1), (256, 1)]}


def _reversed(g):
    return _t(np.broadcast_to(np.arange(g.N - 1, -1, -1, dtype=np.int32), (g.B, g.N)), g.dev)


def _tables(g_few, g_all):
    """(graph, active_bins given, compact table expected): <= 17 bins named, more than 17 named, active_bins NULL"""
    assert g_few.A <= K_COMPACT_BINS < g_all.A
    return [(g_few, True, True), (g_all, True, False), (g_few, False, False)]


# ---- waves with no source, one, or two ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2])
def test_few_sources(dev, r):
    for N in (1, 3, 5):
        M, K = N + 5, 4
        g_few, rng = _random_graph(dev, 401 + N, 1, N, M, K, F, pool=FEW_BINS, unique=False)
        g_all, _ = _random_graph(dev, 431 + N, 1, N, M, 40, F, unique=False)
        for C, parts in WIDTHS[r][:3]:
            for g, active, compact in _tables(g_few, g_all):
                x, w, go = _inputs(rng, g, C, r)
                form = grad_form(1, N, g.M, F, C, r, active, g.A)
                assert form["plan"][0] == 1                           # parts = 8 > N: one part, a single wave per source at most
                _check_grad(g, x, w, go, "N=%d C=%d r=%d active=%s" % (N, C, r, active),
                            dict(kernel="vec", V=4, PARTS=parts, compact=compact, hub=False), active=active)
    # exactly two sources on some waves: B = 8 gives one part per cloud and W = ceil(N / 8) workgroups, 4 W waves for N sources
    N = 61
    g, rng = _random_graph(dev, 443, 8, N, N + 5, 4, F, pool=FEW_BINS, unique=False)
    for C, parts in WIDTHS[r][:3]:
        form = grad_form(8, N, g.M, F, C, r, True, g.A)
        stride = K_BWD_WAVES * form["plan"][1]
        assert form["plan"][0] == 1 and stride < N < 2 * stride       # waves 0 .. N - stride - 1 walk two sources, the others one
        x, w, go = _inputs(rng, g, C, r)
        _check_grad(g, x, w, go, "N=61 B=8 C=%d r=%d" % (C, r), dict(kernel="vec", PARTS=parts, compact=True), launches=2)


# ---- clouds that are no multiple of 8, N no multiple of parts ----------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 5])
def test_ragged_batches(dev, B):
    N, M, K = 301, 120, 9
    g_few, rng = _random_graph(dev, 457 + B, B, N, M, K, F, pool=FEW_BINS)
    g_all, _ = _random_graph(dev, 461 + B, B, N, M, K, F)
    for i, (C, r, parts) in enumerate([(C, r, p) for r in (1, 2) for C, p in WIDTHS[r]]):
        g, active, compact = _tables(g_few, g_all)[i % 3]
        form = grad_form(B, N, M, F, C, r, active, g.A)
        assert form["plan"][0] == 8 and N % 8 != 0                    # eight interleaved parts per cloud, the last ones one position short
        x, w, go = _inputs(rng, g, C, r)
        order = _reversed(g) if i % 2 else None
        _check_grad(g, x, w, go, "B=%d C=%d r=%d order=%s" % (B, C, r, "reversed" if i % 2 else "NULL"),
                    dict(kernel="vec", V=4, PARTS=parts, compact=compact, hub=False), active=active, order=order)


# ---- sources without in-edges --------------------------------------------------------------------------------------------------------
# a wave's walk of three sources: empty ones first, last, two in a row, between two busy ones (1 = no in-edge); wave gw takes
# pattern gw % 4
WALKS = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1]])


def _graph_with_empty_sources(dev, B, N, stride, M, K, pool, seed):
    """neighbour lists by hand: position p = gw + stride j (one part per cloud, no source order: source p) has no in-edge where
    WALKS[gw % 4, j] says so; every other source is named by at least one row"""
    rng = np.random.RandomState(seed)
    p = np.arange(N)
    empty = WALKS[(p % stride) % 4, p // stride] == 1
    busy = p[~empty]
    assert M >= len(busy)
    idx = busy[rng.randint(0, len(busy), size=(B, M, K))].astype(np.int32)
    idx[:, :len(busy), 0] = busy                                      # row m < len(busy) names busy[m] in its first slot
    cnt = rng.randint(1, K + 1, size=(B, M)).astype(np.int32)
    cnt[:, len(busy):][:, ::3] = 0
    return Graph(dev, idx, cnt, make_bins(rng, idx, cnt, F, pool), N, F), rng, empty


@pytest.mark.parametrize("table", ["compact", "full"])
def test_sources_without_in_edges(dev, table):
    B, C, r, K = 8, 256, 2, 4                                         # C r = 512: two slices, W = 64 (compact) or 32 (full) per XCD
    compact = table == "compact"
    N = 96
    for _ in range(12):                                               # the N at which every wave walks exactly three sources
        W = grad_form(B, N, N, F, C, r, compact, 8)["plan"][1]
        N = 3 * K_BWD_WAVES * W
    stride = K_BWD_WAVES * W
    g, rng, empty = _graph_with_empty_sources(dev, B, N, stride, N, K, FEW_BINS, 467)
    form = grad_form(B, N, g.M, F, C, r, compact, g.A)
    assert form["plan"][:2] == (1, W) and form["compact"] == compact and not form["hub"]
    x, w, go = _inputs(rng, g, C, r)
    got, ref = _check_grad(g, x, w, go, "empty sources, " + table, dict(kernel="vec", PARTS=1), active=compact, launches=2)
    assert (ref.deg[:, empty] == 0).all() and (ref.deg[:, ~empty] > 0).all()
    assert (bits(got[0])[:, empty] == 0).all(), "a source without in-edges: exact +0"
    # (the last source of the last cloud is one of them: its E0 is the end of the entries)  The same through key + scale entries
    assert empty[N - 1] and empty[0]
    _check_grad(g, x, w, go, "empty sources, key + scale, " + table, dict(kernel="vec", PARTS=1), active=compact, ref=ref, entries="arrays")


# ---- sources of more than one chunk ---------------------------------------------------------------------------------------------------
def _multi_chunk_graph(dev, pool, seed):
    """N = 200, K = 64, 150 rows: every row with a neighbour names source 0, rows 0..99 with two also source 1"""
    B, N, M, K = 2, 200, 150, 64
    g, rng = _random_graph(dev, seed, B, N, M, K, F, pool=pool)
    idx, cnt = g.idx.copy(), g.cnt
    idx[:, :, 0] = 0
    idx[:, :100, 1] = np.where(cnt[:, :100] >= 2, 1, idx[:, :100, 1])
    return Graph(dev, idx, cnt, g.bins, N, F), rng


@pytest.fixture(scope="module")
def chunk_graphs(dev):
    return _multi_chunk_graph(dev, FEW_BINS, 479)[0], _multi_chunk_graph(dev, None, 487)[0]


@pytest.mark.parametrize("C,r,parts", [(32, 2, 4), (128, 1, 2), (128, 2, 1), (512, 1, 1)], ids=["quarter", "half", "full", "two-slices"])
def test_sources_of_several_chunks(dev, chunk_graphs, C, r, parts):
    rng = np.random.RandomState(491 + C)
    for g, active, compact in _tables(*chunk_graphs):
        x, w, go = _inputs(rng, g, C, r)
        expect = dict(kernel="vec", V=4, PARTS=parts, compact=compact, hub=False)
        got, ref = _check_grad(g, x, w, go, "K=64 packed active=%s" % active, expect, active=active, launches=2)
        deg = ref.deg
        assert (deg[:, 0] > 128).all() and (deg[:, 1] > 64).all() and (deg[:, 1] <= 128).all()
        _check_grad(g, x, w, go, "K=64 key + scale, reversed order", expect, active=active, ref=ref, entries="arrays", order=_reversed(g))


def test_two_inputs(dev, chunk_graphs):
    Ca, Cb, r = 128, 4, 2                                             # Ca r = 256: the first slice is the first tensor's
    g = chunk_graphs[0]
    assert cat_ok(F, Ca, Cb, r)
    rng = np.random.RandomState(499)
    x, w, go = _inputs(rng, g, Ca + Cb, r)
    plain, ref = _check_grad(g, x, w, go, "plain op on the concatenation", dict(kernel="vec", V=4, PARTS=1, compact=True, hub=False))
    for order in (None, _reversed(g)):
        two = _grad(g, x, w, go, cat=Ca, order=order)
        np.testing.assert_array_equal(bits(two[0]), bits(plain[0]))
        form = grad_form(g.B, g.N, g.M, F, Ca + Cb, r, True, g.A)
        form["tag"] += " two inputs"
        _assert_grad(two, ref, form, r, "Ca=%d Cb=%d" % (Ca, Cb))


# ---- deterministic repeat --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def deterministic_mode():
    pkg.set_deterministic(False)
    _tgraph.clear()
    pkg.set_deterministic(True)
    yield
    pkg.set_deterministic(False)
    _tgraph.clear()
    assert _lib.lib().sph3d_get_deterministic() == 0


@pytest.mark.parametrize("C,r", [(32, 2), (64, 2), (128, 2)], ids=["quarter", "half", "full"])
def test_deterministic_repeat(dev, deterministic_mode, C, r):
    """the same call twice — separate outputs and workspaces — on one canonical transposed graph: the same bits"""
    B, N, M, K = 3, 301, 320, 9
    g, rng = _random_graph(dev, 503, B, N, M, K, F, pool=FEW_BINS, hub=True)
    x, w, go = _inputs(rng, g, C, r)
    ref = conv_grad_ref(x, w, go, g.idx, g.cnt, g.bins)
    first, _ = _check_grad(g, x, w, go, "deterministic, first call", dict(kernel="vec", compact=True), ref=ref, order=_reversed(g))
    again, _ = _check_grad(g, x, w, go, "deterministic, second call", dict(kernel="vec", compact=True), ref=ref, order=_reversed(g))
    np.testing.assert_array_equal(bits(again[0]), bits(first[0]), err_msg="grad_input differs between two runs")
    np.testing.assert_array_equal(bits(again[1]), bits(first[1]), err_msg="grad_filter differs between two runs")
