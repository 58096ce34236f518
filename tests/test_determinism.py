"""Deterministic mode without a device: the process-wide switch, the host-side validation of sph3d_graph_canonical_order, the
workspace sizes with the mode off and on, the cache rule of the Python switch, and the numpy statement of the canonical order
(tests/_det_ref.py) against tests/_tgraph_ref.py::transpose_reference."""
import ctypes

import numpy as np
import pytest

import _det_ref as D
from _tgraph_ref import transpose_reference
from sph3d_gcn_amd import _lib

EINVAL, EWORKSPACE = -1, -2
WS_DIMS = [(1, 1, 1, 1, 1), (2, 50, 300, 16, 17), (3, 77, 50, 8, 33), (2, 2049, 300, 8, 1), (16, 8192, 8192, 64, 65), (1, 40, 0, 4, 1)]
# taken when this module is imported: before any test here has touched the switch
WS_BEFORE = {d: _lib.lib().sph3d_graph_transpose_workspace(*d) for d in WS_DIMS}
MODE_AT_IMPORT = _lib.lib().sph3d_get_deterministic()


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    yield
    import sph3d_gcn_amd
    sph3d_gcn_amd.set_deterministic(False)
    assert _lib.lib().sph3d_get_deterministic() == 0


def _tg_ws_words(B, N, M, K, F):
    """common.hpp: tg_ws (as tests/test_gpu_tgraph.py::_plan restates it)"""
    L = N * F
    chunks = (L + 2047) // 2048
    return ((B * L + F + 1) & ~1) + 2 * B * chunks + B * M * K


def test_switch_round_trips_and_returns_the_previous_value():
    l = _lib.lib()
    assert MODE_AT_IMPORT == 0 and l.sph3d_get_deterministic() == 0           # off by default
    assert l.sph3d_set_deterministic(1) == 0 and l.sph3d_get_deterministic() == 1
    assert l.sph3d_set_deterministic(1) == 1 and l.sph3d_get_deterministic() == 1
    assert l.sph3d_set_deterministic(7) == 1 and l.sph3d_get_deterministic() == 1      # any non-zero value is "on"
    assert l.sph3d_set_deterministic(0) == 1 and l.sph3d_get_deterministic() == 0
    assert l.sph3d_set_deterministic(0) == 0
    assert l.sph3d_abi_version() == 2                                           # symbols were added, none changed


def test_new_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sph3d_set_deterministic", "sph3d_get_deterministic", "sph3d_graph_canonical_order",
                 "sph3d_graph_canonical_order_workspace"):
        assert hasattr(raw, name), "libsph3d.so does not export %s" % name
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["sph3d_set_deterministic"] == (ctypes.c_int, [ctypes.c_int])
    assert _lib.SIGNATURES["sph3d_get_deterministic"] == (ctypes.c_int, [])
    assert len(_lib.SIGNATURES["sph3d_graph_canonical_order"][1]) == 11


def test_python_switch_and_context_manager():
    import sph3d_gcn_amd as pkg
    assert pkg.is_deterministic() is False
    assert pkg.set_deterministic(True) is False and pkg.is_deterministic() is True
    with pkg.deterministic(False):
        assert pkg.is_deterministic() is False
        with pkg.deterministic():
            assert pkg.is_deterministic() is True
        assert pkg.is_deterministic() is False
    assert pkg.is_deterministic() is True
    assert pkg.set_deterministic(False) is True
    with pytest.raises(KeyError):
        with pkg.deterministic():
            assert _lib.lib().sph3d_get_deterministic() == 1
            raise KeyError("leaves the block")
    assert pkg.is_deterministic() is False


def test_flipping_the_switch_empties_the_transpose_cache():
    import sph3d_gcn_amd as pkg
    from sph3d_gcn_amd import _tgraph
    for first, second in ((True, False), (False, True)):
        pkg.set_deterministic(first)
        gen = _tgraph._generation[0]
        _tgraph._cache["stale"] = ("a transposed graph in the other mode's order",)
        _tgraph._unique.add("stale")
        pkg.set_deterministic(first)                                    # no change of value: the cache is kept
        assert "stale" in _tgraph._cache and _tgraph._generation[0] == gen
        pkg.set_deterministic(second)
        assert len(_tgraph._cache) == 0 and len(_tgraph._unique) == 0 and _tgraph._generation[0] == gen + 1
    pkg.set_deterministic(False)
    _tgraph._cache["stale"] = ("x",)
    with pkg.deterministic(True):
        assert len(_tgraph._cache) == 0
        _tgraph._cache["canonical"] = ("y",)
    assert len(_tgraph._cache) == 0
    pkg.set_deterministic(False)


def test_workspace_sizes_are_the_parents_with_the_mode_off():
    l = _lib.lib()
    for d in WS_DIMS:
        assert WS_BEFORE[d] == 4 * _tg_ws_words(*d), d
    assert l.sph3d_set_deterministic(1) == 0
    try:
        for d in WS_DIMS:
            B, N, M, K, F = d
            on = l.sph3d_graph_transpose_workspace(*d)
            assert on == WS_BEFORE[d] + 4 * B * M * K, d                # staging for the factors of separate entry arrays
            assert l.sph3d_graph_canonical_order_workspace(*d) == 8 * B * M * K
    finally:
        l.sph3d_set_deterministic(0)
    for d in WS_DIMS:
        assert l.sph3d_graph_transpose_workspace(*d) == WS_BEFORE[d], d
        assert l.sph3d_graph_canonical_order_workspace(*d) == 8 * d[0] * d[2] * d[3]      # (the pass is the same in either mode)
    # the wrappers' sizes contain the transpose's scratch and follow it
    off = (l.sph3d_scatter_grad_workspace(2, 50, 300, 16), l.sph3d_depthwise_conv3d_grad_workspace(2, 50, 300, 17, 8, 2, 16))
    l.sph3d_set_deterministic(1)
    on = (l.sph3d_scatter_grad_workspace(2, 50, 300, 16), l.sph3d_depthwise_conv3d_grad_workspace(2, 50, 300, 17, 8, 2, 16))
    tv = l.sph3d_depthwise_conv3d_grad_t_workspace(2, 50, 17, 8, 2)
    l.sph3d_set_deterministic(0)
    assert all(0 < b - a <= 4 * 2 * 300 * 16 + 256 for a, b in zip(off, on))
    assert tv == l.sph3d_depthwise_conv3d_grad_t_workspace(2, 50, 17, 8, 2)             # no transposed graph inside: unchanged


def test_canonical_order_validates_on_the_host():
    l = _lib.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)
    good = dict(B=1, N=2, M=2, K=2, F=1)
    need = l.sph3d_graph_canonical_order_workspace(1, 2, 2, 2, 1)
    assert need == 32

    def call(offsets=p, key=p, scale=p, ws=p, nbytes=need, **dims):
        d = dict(good, **dims)
        return l.sph3d_graph_canonical_order(d["B"], d["N"], d["M"], d["K"], d["F"], offsets, key, scale, ws, nbytes, None)
    for name in good:
        for bad in (0, -3):
            assert call(**{name: bad}) == EINVAL, (name, bad)
            assert b"canonical_order" in l.sph3d_last_error()
    assert call(offsets=None) == EINVAL and call(key=None) == EINVAL
    assert call(N=1 << 30, F=4) == EINVAL                               # N * F does not fit int32
    assert call(ws=None) == EWORKSPACE and call(nbytes=need - 1) == EWORKSPACE and call(scale=None, nbytes=0) == EWORKSPACE
    assert b"workspace" in l.sph3d_last_error()
    with pytest.raises(ValueError):
        _lib.check(call(B=0))
    assert not any(buf)                                                 # nothing was written
    assert l.sph3d_graph_canonical_order_workspace(0, 2, 2, 2, 1) == 0


# ---- the numpy statement ------------------------------------------------------------------------------------------------------------
def _graph(seed, B, n_src, M, K, F=1, special=False, high=False):
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, n_src, size=(B, M, K)).astype(np.int32)
    cnt = rng.randint(0, K + 1, size=(B, M)).astype(np.int32)
    if high:
        cnt[:, ::2] = rng.randint(128, K + 1, size=cnt[:, ::2].shape)
    cnt[:, 1::6] = 0
    cnt[:, 2::6] = K
    bins = rng.randint(0, F, size=(B, M, K)).astype(np.int32) if F > 1 else None
    w = (rng.rand(B, M, K) + 0.05).astype(np.float32)
    if special:
        idx[0, 2, :] = 1                                                # row 2 (count K) names source 1 in every slot
        if bins is not None:
            bins[0, 2, :] = 0
        wb = D.fbits(w).reshape(B, M, K)
        wb[0, 2, :6] = [0x80000000, 0x7fc00000, 0x00000000, 0xffc00001, 0x3f800000, 0x80000000]    # -0, NaN, +0, a negative NaN, 1, -0
        w = wb.view(np.float32)
    return idx, cnt, bins, w


@pytest.mark.parametrize("form", ["packed", "arrays", "weighted"])
@pytest.mark.parametrize("F", [1, 5])
def test_statement_of_the_canonical_order(form, F):
    """step 1: the rows of transpose_reference, laid out by its offsets, ARE in canonical order (re-sorting changes nothing);
    step 2: shuffling inside the segments and sorting again gives them back"""
    B, N, M, K = 2, 7, 40, 9
    idx, cnt, bins, w = _graph(5 + F, B, N, M, K, F, special=True)
    L = N * F
    off, ent, _act = transpose_reference(idx, cnt, N, bins, F, w if form == "weighted" else None)
    key, sb = D.arrays_from_reference(off, ent, cnt, B, M, K, L, form == "packed")
    k2, s2 = D.canonical_order(off, key, sb, B, L)
    np.testing.assert_array_equal(k2, key)
    assert (sb is None) == (s2 is None) and (sb is None or np.array_equal(s2, sb))
    # the segment of (cloud 0, source 1, bin 0) holds row 2 nine times
    lo, hi = int(off[1 * F]), int(off[1 * F + 1])
    m, f = D.entry_fields(key[lo:hi], None if sb is None else sb[lo:hi])
    assert int((m == 2).sum()) == K and (np.diff(m) >= 0).all()
    if form == "weighted":
        got = f[m == 2].tolist()
        assert got == sorted(got) and {0x80000000, 0x7fc00000, 0, 0xffc00001} <= set(got) and got.count(0x80000000) == 2
        assert got[0] == 0 and got[-1] == 0xffc00001                   # unsigned order: +0 first, the negative NaN last
    rng = np.random.RandomState(11)
    moved = 0
    for _ in range(3):
        ks, ss = D.shuffle_segments(off, key, sb, B, L, rng)
        moved += int((ks != key).sum())
        kc, sc = D.canonical_order(off, ks, ss, B, L)
        np.testing.assert_array_equal(kc, key)
        if sb is not None:
            np.testing.assert_array_equal(sc, sb)
    assert moved > 0


def test_statement_with_counts_that_reach_bit_31():
    B, N, M, K = 2, 6, 30, 255
    idx, cnt, _bins, _w = _graph(13, B, N, M, K, high=True)
    assert (cnt >= 128).sum() > 10 and (cnt == 255).any() and ((cnt > 0) & (cnt < 128)).any()
    off, ent, _ = transpose_reference(idx, cnt, N)
    key, _ = D.arrays_from_reference(off, ent, cnt, B, M, K, N, True)
    live = key[:int(off[N])]
    assert (live < 0).any() and (live >= 0).any()                       # words with and without the sign bit
    ks, _ = D.shuffle_segments(off, key, None, B, N, np.random.RandomState(17))
    assert (ks != key).any()
    kc, _ = D.canonical_order(off, ks, None, B, N)
    np.testing.assert_array_equal(kc, key)
    # packed and separate arrays list the same (m, factor) sequence
    ka, sa = D.arrays_from_reference(off, ent, cnt, B, M, K, N, False)
    pos, _seg = D.segment_positions(off, B, N)
    mp, fp = D.entry_fields(key[pos], None)
    ma, fa = D.entry_fields(ka[pos], sa[pos])
    np.testing.assert_array_equal(mp, ma)
    np.testing.assert_array_equal(fp, fa)
