"""Exact k nearest neighbours on the device (csrc/knn.hip) against the numpy statement harness/knn.py: nn_index, nn_count and the
bit patterns of nn_dist, in the AUTO, SCAN and GRID modes and in both `dist` forms, on the smallest clouds where the kernels can
go wrong (tests/_knn_ref.py; tests/test_knn_forms.py pins each case to the launch form its id names and holds the statement
itself to exact integers and to float64).  Then the graph's consumers over a k-NN graph: the interpolations and their gradients
against tests/_pool_ref.py's float64 statements, the 'idw' weights, and the transposed graph."""
import numpy as np
import pytest
import torch

import _knn_ref as R
import _pool_ref as P
import _tgraph_ref as T
from sph3d_gcn_amd import _lib, _tgraph, tf_nnquery, tf_unpool3d
from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd.harness import knn

pytestmark = pytest.mark.gpu

MODES = (("auto", tf_nnquery.KNN_AUTO), ("scan", tf_nnquery.KNN_SCAN), ("grid", tf_nnquery.KNN_GRID))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _search(dev, db, q, k, radius, dist, mode):
    """one call through the C entry with outputs and a workspace of the test's own, filled with ones: what the kernels leave
    unwritten shows"""
    l = _lib.lib()
    B, N, M = db.shape[0], db.shape[1], q.shape[1]
    need = l.sph3d_build_nearest_neighbor_workspace(B, N, M, k, mode)
    idx = torch.full((B, M, k), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((B, M), -1, dtype=torch.int32, device=dev)
    dst = torch.full((B, M, k), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.full((max(need, 16),), 0xff, dtype=torch.uint8, device=dev)
    _lib.check(l.sph3d_build_nearest_neighbor(B, N, M, k, float("inf") if radius is None else radius, mode, tf_nnquery._KNN_DIST[dist],
                                              _lib.ptr(db), _lib.ptr(q), _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(dst),
                                              _lib.ptr(ws) if need else None, need, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), cnt.cpu().numpy(), dst.cpu().numpy()


def _assert_equal(got, want, what):
    for name, g, w in zip(("nn_index", "nn_count", "nn_dist"), got, want):
        if name == "nn_dist":
            g, w = _bits(g), _bits(w)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s %s: %d elements differ, first at %s: got %s, expected %s" % (
            what, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("name", list(R.CASES))
def test_knn_equals_the_statement(dev, name):
    db, q, k, radius = R.case(name)
    dbt, qt = torch.from_numpy(db).to(dev), torch.from_numpy(q).to(dev)
    for dist in ("root", "squared"):
        want = R.expected(name, dist)
        for mname, mode in MODES:
            _assert_equal(_search(dev, dbt, qt, k, radius, dist, mode), want, "%s %s %s" % (name, dist, mname))
    # what the case is there for, said of the expected rows themselves
    idx, cnt, _ = R.expected(name, "squared")
    N = db.shape[1]
    if radius is None and "nonfinite" not in name:
        assert (cnt == min(k, N)).all() and (idx[:, :, min(k, N):] == 0).all()
    if "nonfinite" in name:
        bad = ~np.isfinite(db).all(axis=2)
        assert bad.sum(axis=1).tolist() == [3, 3] and not bad[np.arange(2)[:, None, None], idx][cnt[:, :, None] > np.arange(k)].any()
        assert cnt[0, 5] == 0 and cnt[1, 77] == 0 and cnt[1, 129] == 0 and (cnt > 0).sum() == cnt.size - 3
    if name.startswith("radius"):
        classes = [int((cnt == 0).sum()), int(((cnt > 0) & (cnt < k)).sum()), int((cnt == k).sum())]
        print("\n%s: rows with count 0 / between / k: %s" % (name, classes))
        assert min(classes) >= 100
    if name.startswith("duplicates"):
        d2 = R.expected(name, "squared")[2]
        assert (d2[0, :200, :min(k, 8)] == 0).all() and (np.diff(idx[0, :200, :min(k, 8)], axis=1) > 0).all()


def test_knn_through_the_op(dev):
    """the public op: slices x, y, z, takes its workspace from the scratch and its outputs from _lib.empty; empty batches and
    empty query sets launch nothing and give empty tensors; CPU tensors and bad arguments are refused"""
    db, q, k, radius = R.case("radius-k8-scan")
    wide = torch.cat([torch.from_numpy(db), torch.ones(2, 1500, 2)], dim=2).to(dev)
    qt = torch.from_numpy(q).to(dev)
    for dist in ("root", "squared"):
        got = tf_nnquery.build_nearest_neighbor(wide, qt, k, radius=radius, dist=dist)
        torch.cuda.synchronize()
        _assert_equal([t.cpu().numpy() for t in got], R.expected("radius-k8-scan", dist), "op " + dist)
    got = torch.ops.sph3d.build_nearest_neighbor(wide[:, :, 0:3], qt, 16, float("inf"), 0, 0)
    _assert_equal([t.cpu().numpy() for t in got], knn.knn_reference(db, q, 16), "custom op")
    for B, M in ((0, 7), (2, 0), (0, 0)):
        idx, cnt, dst = tf_nnquery.build_nearest_neighbor(torch.zeros(B, 9, 3, device=dev), torch.zeros(B, M, 3, device=dev), 4)
        assert idx.shape == (B, M, 4) and cnt.shape == (B, M) and dst.shape == (B, M, 4) and idx.dtype == torch.int32
    with pytest.raises(_lib.Sph3dError):
        tf_nnquery.build_nearest_neighbor(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), 3)
    for kw in (dict(k=0), dict(k=65), dict(k=3, radius=0.0), dict(k=3, radius=-1.0), dict(k=3, dist="euclid")):
        with pytest.raises((ValueError, _lib.Sph3dError)):
            tf_nnquery.build_nearest_neighbor(wide, qt, **kw)


@pytest.fixture(scope="module")
def knn_graph(dev):
    """k = 3, 2 x 256 coarse points -> 2 x 1024 fine points (the coarse points are among them: d2 = 0 occurs), C = 32"""
    rng = np.random.RandomState(3)
    fine = rng.rand(2, 1024, 3).astype(np.float32)
    coarse = np.ascontiguousarray(fine[:, ::4])
    idx, cnt, d2 = tf_nnquery.build_nearest_neighbor(torch.from_numpy(coarse).to(dev), torch.from_numpy(fine).to(dev), 3, dist="squared")
    torch.cuda.synchronize()
    _assert_equal([t.cpu().numpy() for t in (idx, cnt, d2)], knn.knn_reference(coarse, fine, 3, dist="squared"), "k-NN un-pooling graph")
    x = P.make_values(rng, (2, 256, 32))
    go = P.make_values(rng, (2, 1024, 32))
    return dict(idx=idx, cnt=cnt, d2=d2, x=x, go=go, idx_h=idx.cpu().numpy(), cnt_h=cnt.cpu().numpy(), d2_h=d2.cpu().numpy())


def test_idw_weights(dev, knn_graph):
    """w_i = (1 / (d2_i + e)) / sum_j (1 / (d2_j + e)), e = float32(1e-8), against float64 within (k + 4) * 2^-24 relative: the
    numerator carries the add's and the reciprocal's rounding (2), the denominator those two and k - 1 for its sum (k + 1), the
    division one more: k + 4 to first order.  Rows of a coarse point's own fine point (d2 = 0) are in the graph."""
    g, k = knn_graph, 3
    w = s3g_util._idw_weights(g["d2"], g["cnt"]).cpu().numpy().astype(np.float64)
    r = 1.0 / (g["d2_h"].astype(np.float64) + np.float64(np.float32(1e-8)))
    want = r / r.sum(axis=-1, keepdims=True)
    assert (g["cnt_h"] == k).all() and (g["d2_h"] == 0).any() and (want > 0).all()
    rel = np.abs(w - want) / want
    print("\nidw weights: max relative error %.3e, bound %.3e" % (rel.max(), (k + 4) * P.U))
    assert rel.max() <= (k + 4) * P.U
    # a row with fewer neighbours than slots, and one with none: the dead slots and the empty row are exact zeros
    d2 = torch.tensor([[[0.25, 0.5, 9.0], [1.0, 2.0, 3.0]]], device=dev)
    w = s3g_util._idw_weights(d2, torch.tensor([[2, 0]], dtype=torch.int32, device=dev)).cpu().numpy()
    assert w[0, 1].tolist() == [0, 0, 0] and w[0, 0, 2] == 0 and abs(w[0, 0, 0] - 2 / 3) < 1e-6 and abs(w[0, 0, 1] - 1 / 3) < 1e-6


def test_interpolations_over_a_knn_graph(dev, knn_graph):
    g = knn_graph
    x, go = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["go"]).to(dev)
    idx, cnt = g["idx"], g["cnt"]
    w = s3g_util._idw_weights(g["d2"], cnt)
    w_h = w.cpu().numpy()
    P.assert_sum(tf_unpool3d.mean_interpolate(x, idx, cnt).cpu().numpy(), *P.gather_ref(g["x"], g["idx_h"], g["cnt_h"], mean=True),
                 "mean_interpolate over k-NN")
    P.assert_sum(tf_unpool3d.mean_interpolate_grad(x, go, idx, cnt).cpu().numpy(),
                 *P.scatter_ref(g["go"], g["idx_h"], g["cnt_h"], 256, mean=True), "mean_interpolate_grad over k-NN")
    P.assert_sum(tf_unpool3d.weighted_interpolate(x, w, idx, cnt).cpu().numpy(),
                 *P.gather_ref(g["x"], g["idx_h"], g["cnt_h"], weight=w_h), "weighted_interpolate over k-NN")
    P.assert_sum(tf_unpool3d.weighted_interpolate_grad(x, go, w, idx, cnt).cpu().numpy(),
                 *P.scatter_ref(g["go"], g["idx_h"], g["cnt_h"], 256, weight=w_h), "weighted_interpolate_grad over k-NN")
    # and through unpool3d's 'idw'
    out = s3g_util.unpool3d(x, idx, cnt, g["d2"], scope="u", method="idw")
    assert torch.equal(out, tf_unpool3d.weighted_interpolate(x, w, idx, cnt))


def test_transposed_knn_graph(dev, knn_graph):
    g = knn_graph
    B, M, K, n_src = 2, 1024, 3, 256
    assert all(len(set(row)) == K for row in g["idx_h"].reshape(-1, K).tolist())           # unique_rows is a true promise
    off, key, scale, _ = _tgraph.transpose(g["idx"], g["cnt"], n_src, unique_rows=True)
    torch.cuda.synchronize()
    want_off, want_ent, _ = T.transpose_reference(g["idx_h"], g["cnt_h"], n_src)
    assert (off.cpu().numpy() == want_off).all()
    got = T.device_entries(off.cpu().numpy(), key.cpu().numpy(), None if scale is None else scale.cpu().numpy(), B, n_src, M * K)
    assert (got == want_ent).all()
    assert _tgraph.peek(g["idx"], g["cnt"], n_src, need_unique_rows=True) is not None
