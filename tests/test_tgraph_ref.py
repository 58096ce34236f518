"""tests/_tgraph_ref.py — the numpy statement of the transposed neighbour graph that tests/test_gpu_tgraph.py holds the
kernels to — checked on the CPU: against arrays written out by hand, against the scatter it replaces, and (packed entry words)
against _tgraph.entries()."""
import numpy as np
import torch

from _tgraph_ref import balanced_order_reference, device_entries, spatial_order_keys, transpose_reference
from sph3d_gcn_amd import _tgraph

THIRD, HALF, ONE = 0x3eaaaaab, 0x3f000000, 0x3f800000          # float32 bits of 1/3, 1/2, 1


def _hand_graph():
    """B = 2, three sources, two rows of up to three slots, two bins: cloud 0 has a row that lists source 2 twice and an empty
    row (whose slots hold ids that must not count), cloud 1 two rows that share source 1"""
    idx = np.array([[[2, 2, 0], [1, 1, 1]], [[0, 1, 2], [1, 0, 0]]], np.int32)
    cnt = np.array([[3, 0], [2, 1]], np.int32)
    bins = np.array([[[1, 1, 0], [0, 1, 0]], [[0, 1, 1], [1, 0, 0]]], np.int32)
    return idx, cnt, bins


def test_hand_written_graph_with_bins():
    idx, cnt, bins = _hand_graph()
    off, ent, act = transpose_reference(idx, cnt, 3, bin_index=bins, num_bins=2)
    assert off.dtype == np.int32 and act.dtype == np.int32
    np.testing.assert_array_equal(off, [0, 1, 1, 1, 1, 1, 3, 6, 7, 7, 7, 9, 9, 9])
    np.testing.assert_array_equal(ent, [[0, 0, THIRD], [5, 0, THIRD], [5, 0, THIRD], [6, 0, HALF], [9, 0, HALF], [9, 1, ONE]])
    np.testing.assert_array_equal(act, [2, 0, 1])


def test_hand_written_graph_without_bins_and_with_weights():
    idx, cnt, _bins = _hand_graph()
    off, ent, act = transpose_reference(idx, cnt, 3)
    np.testing.assert_array_equal(off, [0, 1, 1, 3, 6, 7, 9, 9])
    np.testing.assert_array_equal(ent, [[0, 0, THIRD], [2, 0, THIRD], [2, 0, THIRD], [3, 0, HALF], [4, 0, HALF], [4, 1, ONE]])
    np.testing.assert_array_equal(act, [1, 0])
    w = np.arange(12, dtype=np.float32).reshape(2, 2, 3) + np.float32(0.25)
    wb = lambda b, m, k: int(w[b, m, k].view(np.uint32))
    off_w, ent_w, _ = transpose_reference(idx, cnt, 3, weight=w)
    np.testing.assert_array_equal(off_w, off)
    np.testing.assert_array_equal(ent_w, [[0, 0, wb(0, 0, 2)], [2, 0, wb(0, 0, 0)], [2, 0, wb(0, 0, 1)], [3, 0, wb(1, 0, 0)],
                                          [4, 0, wb(1, 0, 1)], [4, 1, wb(1, 1, 0)]])


def test_out_of_range_bins_are_clamped():
    idx, cnt, bins = _hand_graph()
    bins = bins.copy()
    bins[0, 0] = [-3, 7, 0]                   # live edges: bins 0, 1, 0 after clamping
    bins[0, 1] = [-9, 9, 9]                   # an empty row: no edge, no bin
    off, ent, act = transpose_reference(idx, cnt, 3, bin_index=bins, num_bins=2)
    np.testing.assert_array_equal(off[:7], [0, 1, 1, 1, 1, 2, 3])
    np.testing.assert_array_equal(ent[:3], [[0, 0, THIRD], [4, 0, THIRD], [5, 0, THIRD]])
    np.testing.assert_array_equal(act, [2, 0, 1])


def test_device_form_of_the_hand_graph_gives_the_same_triples():
    """entries laid out as the library writes them (any order inside a segment, untouched words behind a cloud's end), as
    separate arrays and as packed words"""
    idx, cnt, bins = _hand_graph()
    off, ent, _ = transpose_reference(idx, cnt, 3, bin_index=bins, num_bins=2)
    junk = 0x7f7f7f7f
    key = np.array([0, 0, 0, junk, junk, junk, 0, 1, 0, junk, junk, junk], np.int32)
    scale = np.array([THIRD, THIRD, THIRD, 0, 0, 0, HALF, ONE, HALF, 0, 0, 0], np.uint32).view(np.float32)
    np.testing.assert_array_equal(device_entries(off, key, scale, 2, 6, 6), ent)
    packed = np.array([3 << 24, 3 << 24, 3 << 24, junk, junk, junk, 2 << 24, 1 | 1 << 24, 2 << 24, junk, junk, junk], np.uint32)
    np.testing.assert_array_equal(device_entries(off, packed.view(np.int32), None, 2, 6, 6), ent)


def _random_graph(rng, B, n_src, M, K, F):
    idx = rng.randint(0, n_src, size=(B, M, K)).astype(np.int32)
    cnt = rng.randint(0, K + 1, size=(B, M)).astype(np.int32)
    cnt[:, ::5] = 0
    bins = rng.randint(-2, F + 2, size=(B, M, K)).astype(np.int32)
    return idx, cnt, bins


def _terms_by_segment(seg, term, segments):
    """-> per segment the sorted list of its float64 terms"""
    out = [[] for _ in range(segments)]
    for s, t in zip(seg.tolist(), term.tolist()):
        out[s].append(t)
    return [sorted(v) for v in out]


def test_gather_over_the_transposed_graph_is_the_scatter_over_the_graph():
    """per (source, bin) the gather's terms go[m] * scale are the scatter's terms, as multisets of float64 values — with the
    factor 1 / count and with weights"""
    for seed, (B, n_src, M, K, F) in enumerate([(2, 13, 40, 5, 1), (3, 7, 25, 9, 4), (1, 30, 60, 70, 3)]):
        rng = np.random.RandomState(seed)
        idx, cnt, bins = _random_graph(rng, B, n_src, M, K, F)
        go = rng.randn(B, M)
        w = rng.rand(B, M, K).astype(np.float32)
        L = n_src * F
        for weight in (None, w):
            off, ent, act = transpose_reference(idx, cnt, n_src, bin_index=bins if F > 1 else None, num_bins=F, weight=weight)
            got = _terms_by_segment(ent[:, 0], go.reshape(-1)[ent[:, 0] // L * M + ent[:, 1]]
                                    * ent[:, 2].astype(np.uint32).view(np.float32).astype(np.float64), B * L)
            seg, term, used = [], [], set()
            for b in range(B):
                for m in range(M):
                    for k in range(int(cnt[b, m])):
                        f = min(max(int(bins[b, m, k]), 0), F - 1) if F > 1 else 0
                        s = np.float32(1) / np.float32(cnt[b, m]) if weight is None else weight[b, m, k]
                        seg.append(b * L + int(idx[b, m, k]) * F + f)
                        term.append(go[b, m] * np.float64(s))
                        used.add(f)
            want = _terms_by_segment(np.array(seg), np.array(term), B * L)
            assert got == want
            # the offsets delimit exactly these lists, cloud after cloud in slabs of M * K
            o = off.reshape(B, L + 1)
            np.testing.assert_array_equal(o[:, 0], np.arange(B) * M * K)
            np.testing.assert_array_equal(np.diff(o, axis=1).reshape(-1), [len(v) for v in want])
            np.testing.assert_array_equal(act, [len(used)] + sorted(used))


def test_balanced_order_of_a_short_window_with_ties():
    # in-degrees 2 0 2 1 0: heaviest first, equal degrees by descending index (the keys are unique: degree << 11 | index)
    off = np.cumsum([0, 2, 0, 2, 1, 0])
    np.testing.assert_array_equal(balanced_order_reference(off, 1, 5, 1), [[2, 0, 3, 4, 1]])
    # the same degrees spread over F = 2 segments per source, in two clouds (the second one's offsets start at its slab)
    sizes = [1, 1, 0, 0, 2, 0, 0, 1, 0, 0]
    off2 = np.concatenate([np.cumsum([0] + sizes), 40 + np.cumsum([0] + sizes[::-1])])
    np.testing.assert_array_equal(balanced_order_reference(off2, 2, 5, 2), [[2, 0, 3, 4, 1], [4, 2, 1, 3, 0]])


def test_balanced_order_alternates_the_direction_from_window_to_window():
    N = 2048 + 4
    deg = np.zeros(N, np.int64)
    deg[2048:] = [1, 0, 1, 0]
    deg[7] = (1 << 20) + 5                      # capped: ties with source 9 on the degree, the index decides
    deg[9] = 1 << 20
    order = balanced_order_reference(np.concatenate([[0], np.cumsum(deg)]), 1, N, 1)[0]
    np.testing.assert_array_equal(order[:2], [9, 7])
    np.testing.assert_array_equal(order[2:2048], [i for i in range(2047, -1, -1) if i not in (7, 9)])
    np.testing.assert_array_equal(order[2048:], [2049, 2051, 2048, 2050])       # an odd window: lightest first
    np.testing.assert_array_equal(np.sort(order), np.arange(N))


def test_packed_words_decode_as_tgraph_entries_decodes_them():
    counts, rows = [1, 64, 127, 128, 200, 255], [0, (1 << 24) - 1]
    words = np.array([m | c << 24 for c in counts for m in rows], np.uint32)
    assert (words.view(np.int32) < 0).sum() == 6                                 # counts from 128 set the sign bit
    key, scale = _tgraph.entries((None, torch.from_numpy(words.view(np.int32).copy()), None, None))
    assert key.dtype == torch.int32 and scale.dtype == torch.float32
    got = device_entries(np.array([0, words.size], np.int32), words.view(np.int32), None, 1, 1, words.size)
    want = device_entries(np.array([0, words.size], np.int32), key.numpy(), scale.numpy(), 1, 1, words.size)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(np.unique(got[:, 1]), rows)
    np.testing.assert_array_equal(np.unique(got[:, 2]), np.sort((np.float32(1) / np.array(counts, np.float32)).view(np.uint32)))


def test_spatial_order_keys_of_a_hand_cloud():
    # bounding box [0, 4]^3 scaled to 16 cells per axis: cell = 4 * coordinate, clamped to 15; x is the lowest bit of the code
    xyz = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4], [0.25, 0.5, 0.75], [1, 1, 1]]], np.float32)
    np.testing.assert_array_equal(spatial_order_keys(xyz, 6)[0], [0, 0x249, 0x492, 0x924, 1 | 8 << 1 | 9 << 2, 0x1c0])
    # all points equal: no extent, one cell
    np.testing.assert_array_equal(spatial_order_keys(np.ones((1, 5, 3), np.float32), 5), np.zeros((1, 5)))
