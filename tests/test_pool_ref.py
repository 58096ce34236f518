"""tests/_pool_ref.py proved on the CPU: the float64 statement of the pooling / un-pooling family agrees with the fp32 C oracle
(the reference's behaviour), and its checker catches the defects a pair-wise, chunked gather kernel can have."""
import numpy as np
import pytest

import oracle
from _pool_ref import (assert_sum, bits, gather_ref, make_graph, make_values, make_weights, max_grad_ref, max_ref,
                       scatter_ref)

# (B, sources, rows, C, K, unique ids per row, counts of every second row from)
GRAPHS = [(2, 96, 300, 67, 19, True, None), (1, 40, 500, 8, 200, False, 128), (2, 320, 300, 132, 6, True, None),
          (2, 64, 4000, 12, 9, True, None)]
_IDS = ["B%d-N%d-M%d-C%d-K%d" % g[:5] for g in GRAPHS]


def _case(g, seed=0):
    B, N, M, C, K, unique, high = g
    rng = np.random.RandomState(1000 * seed + N + K)
    idx, cnt = make_graph(rng, B, N, M, K, unique=unique, high_from=high)
    return idx, cnt, make_values(rng, (B, N, C)), make_values(rng, (B, M, C)), make_weights(rng, cnt, K)


def _edge_inputs():
    """rows with every edge of the max scan: empty, NaN in slot 0, NaN in a later slot, an all -inf channel, +0 / -0 ties in
    both orders, next to ordinary rows with rounded (tying) values"""
    rng = np.random.RandomState(7)
    B, N, M, C, K = 2, 50, 40, 9, 7
    idx, cnt = make_graph(rng, B, N, M, K)
    x = make_values(rng, (B, N, C))
    rows = [(40, 41, 42),        # NaN in slot 0
            (41, 40, 42),        # NaN in a later slot
            (43, 44),            # +0 then -0
            (44, 43),            # -0 then +0
            (45, 46, 47),        # channel 0 is -inf in all three
            ()]                  # empty
    for b in range(B):
        for m, ids in enumerate(rows):
            idx[b, m] = 0
            idx[b, m, :len(ids)] = ids
            cnt[b, m] = len(ids)
        x[b, 40] = np.nan
        x[b, 43] = 0.0
        x[b, 44] = -0.0
        x[b, 45:48, 0] = -np.inf
    return idx, cnt, x


def test_max_ref_equals_the_oracle_bit_for_bit():
    idx, cnt, x = _edge_inputs()
    out, arg = max_ref(x, idx, cnt)
    out_o, arg_o = oracle.max_pool3d(x, idx, cnt)
    np.testing.assert_array_equal(bits(out), bits(out_o))
    np.testing.assert_array_equal(arg, arg_o)
    # what the oracle does at the edges, stated: (the reference's behaviour)
    assert np.isnan(out[0, 0]).all() and (arg[0, 0] == 40).all()                 # a NaN in slot 0 stays, with slot 0's id
    assert not np.isnan(out[0, 1]).any() and (arg[0, 1] != 40).all()             # a NaN in a later slot is ignored
    assert (bits(out[0, 2]) == 0).all() and (arg[0, 2] == 43).all()              # +0 first: kept
    assert (bits(out[0, 3]) == bits(np.float32(-0.0))).all() and (arg[0, 3] == 44).all()
    assert out[0, 4, 0] == -np.inf and arg[0, 4, 0] == 45                        # all -inf: -inf with slot 0's id
    assert (bits(out[0, 5]) == 0).all() and (arg[0, 5] == 0).all()               # an empty row: value 0, id 0


@pytest.mark.parametrize("g", GRAPHS, ids=_IDS)
def test_max_ref_and_the_oracle_sums_on_the_four_graphs(g):
    idx, cnt, x, go, w = _case(g)
    N = x.shape[1]
    out, arg = max_ref(x, idx, cnt)
    out_o, arg_o = oracle.max_pool3d(x, idx, cnt)
    np.testing.assert_array_equal(bits(out), bits(out_o))
    np.testing.assert_array_equal(arg, arg_o)
    used = [assert_sum(oracle.avg_pool3d(x, idx, cnt), *gather_ref(x, idx, cnt, mean=True), "oracle avg_pool3d"),
            assert_sum(oracle.mean_interpolate(x, idx, cnt), *gather_ref(x, idx, cnt, mean=True), "oracle mean_interpolate"),
            assert_sum(oracle.weighted_interpolate(x, w, idx, cnt), *gather_ref(x, idx, cnt, weight=w), "oracle weighted_interpolate"),
            assert_sum(oracle.avg_pool3d_grad(x, go, idx, cnt), *scatter_ref(go, idx, cnt, N, mean=True), "oracle avg_pool3d_grad"),
            assert_sum(oracle.mean_interpolate_grad(x, go, idx, cnt), *scatter_ref(go, idx, cnt, N, mean=True),
                       "oracle mean_interpolate_grad"),
            assert_sum(oracle.weighted_interpolate_grad(x, go, w, idx, cnt), *scatter_ref(go, idx, cnt, N, weight=w),
                       "oracle weighted_interpolate_grad"),
            assert_sum(oracle.max_pool3d_grad(x, go, arg_o), *max_grad_ref(go, arg_o, N), "oracle max_pool3d_grad")]
    assert max(used) <= 1.0


# ---- planted defects: fp32 numpy restatements of the kernels' sums, each with one switch that breaks it ------------------------
def _avg32(x, idx, cnt, drop_odd_tail=False, wrong_inv_at_one=False):
    B, M, K = idx.shape
    out = np.zeros((B, M, x.shape[2]), np.float32)
    for b in range(B):
        lim = cnt[b] - (cnt[b] & 1) if drop_odd_tail else cnt[b]
        for k in range(K):
            sel = np.nonzero(lim > k)[0]
            out[b, sel] += x[b][idx[b, sel, k]]
        div = cnt[b] + 1 if wrong_inv_at_one else cnt[b]
        div = np.where(cnt[b] == 1, div, cnt[b])
        inv = np.where(cnt[b] > 0, np.float32(1) / np.maximum(div, 1).astype(np.float32), np.float32(0)).astype(np.float32)
        out[b] *= inv[:, None]
    return out


def _avg_grad32(go, idx, cnt, n_src, chunk_cap=None):
    """chunk_cap: a source keeps only its first chunk_cap in-edges (rows ascending)"""
    B, M, K = idx.shape
    grad = np.zeros((B, n_src, go.shape[2]), np.float32)
    for b in range(B):
        live = np.arange(K)[None, :] < cnt[b][:, None]
        m, k = np.nonzero(live)
        n = idx[b, m, k]
        t = go[b][m] * (np.float32(1) / cnt[b][m].astype(np.float32))[:, None]
        if chunk_cap is not None:
            order = np.argsort(n, kind="stable")
            start = np.searchsorted(n[order], n[order], side="left")
            rank = np.empty_like(order)
            rank[order] = np.arange(order.size) - start
            keep = rank < chunk_cap
            n, t = n[keep], t[keep]
        np.add.at(grad[b], n, t)
    return grad


def _max32(x, idx, cnt, later_tie_wins=False):
    B, M, K = idx.shape
    out = np.zeros((B, M, x.shape[2]), np.float32)
    arg = np.zeros((B, M, x.shape[2]), np.int32)
    for b in range(B):
        for m in range(M):
            for k in range(int(cnt[b, m])):
                v = x[b, idx[b, m, k]]
                rep = np.ones_like(v, bool) if k == 0 else ((v >= out[b, m]) if later_tie_wins else (v > out[b, m]))
                out[b, m] = np.where(rep, v, out[b, m])
                arg[b, m] = np.where(rep, idx[b, m, k], arg[b, m])
    return out, arg


def test_the_restatements_pass_without_a_defect():
    idx, cnt, x, go, w = _case(GRAPHS[0])
    assert_sum(_avg32(x, idx, cnt), *gather_ref(x, idx, cnt, mean=True), "fp32 avg")
    out, arg = _max32(x, idx, cnt)
    ro, ra = max_ref(x, idx, cnt)
    np.testing.assert_array_equal(bits(out), bits(ro))
    np.testing.assert_array_equal(arg, ra)
    idx, cnt, x, go, w = _case(GRAPHS[3])
    ref = scatter_ref(go, idx, cnt, x.shape[1], mean=True)
    assert int(ref[2].max()) > 64
    assert_sum(_avg_grad32(go, idx, cnt, x.shape[1]), *ref, "fp32 avg gradient")
    assert_sum(_avg_grad32(go, idx, cnt, x.shape[1], chunk_cap=1 << 20), *ref, "fp32 avg gradient, cap never reached")


def test_a_dropped_odd_tail_is_caught():
    idx, cnt, x, go, w = _case(GRAPHS[0])
    with pytest.raises(AssertionError):
        assert_sum(_avg32(x, idx, cnt, drop_odd_tail=True), *gather_ref(x, idx, cnt, mean=True), "odd tail dropped")


def test_a_wrong_reciprocal_at_count_one_is_caught():
    idx, cnt, x, go, w = _case(GRAPHS[0])
    assert (cnt == 1).any()
    with pytest.raises(AssertionError):
        assert_sum(_avg32(x, idx, cnt, wrong_inv_at_one=True), *gather_ref(x, idx, cnt, mean=True), "1 / (cnt + 1) at cnt = 1")


def test_in_edges_dropped_beyond_the_64th_are_caught():
    idx, cnt, x, go, w = _case(GRAPHS[3])
    with pytest.raises(AssertionError):
        assert_sum(_avg_grad32(go, idx, cnt, x.shape[1], chunk_cap=64), *scatter_ref(go, idx, cnt, x.shape[1], mean=True),
                   "in-edges past the 64th dropped")


def test_a_tie_resolved_to_the_later_slot_is_caught():
    idx, cnt, x, go, w = _case(GRAPHS[0])
    out, arg = _max32(x, idx, cnt, later_tie_wins=True)
    ro, ra = max_ref(x, idx, cnt)
    np.testing.assert_array_equal(out, ro)            # the values agree (but for the sign of a zero) ...
    assert (arg != ra).any()                          # ... the ids do not


def test_an_unwritten_element_is_caught():
    idx, cnt, x, go, w = _case(GRAPHS[0])
    ref = gather_ref(x, idx, cnt, mean=True)
    got = _avg32(x, idx, cnt)
    assert_sum(got, *ref, "fp32 avg")
    got[1, 17, 5] = np.nan                # what torch.empty + a skipped store leaves, with the caller's NaN fill
    with pytest.raises(AssertionError):
        assert_sum(got, *ref, "one element unwritten")
