"""Neighbour search on clouds of at most 1024 points (csrc/nngrid.hip, nnsmall_search): no cell grid — a prepare launch writes
the thresholds of the chain positions and one header per cloud, and the early-stopping scan (nndense_kernel) takes every query
as an independent wave.  The yardstick is the chain kernel itself: the same `_ws` entry point with workspace = NULL computes
the call with nnquery_sphere_kernel, and the two must agree exactly — indices and counts as integers, distances bit for bit,
bins for both angle functions, the transposed graph's segment totals.  The launch counter shows which path ran."""
import numpy as np
import pytest
import torch

import oracle
from sph3d_gcn_amd import _lib, tf_sample
from sph3d_gcn_amd.harness import synth

pytestmark = pytest.mark.gpu

B = 3
KERNEL = (8, 2, 2)
F = KERNEL[0] * KERNEL[1] * KERNEL[2] + 1

# radius of an intra graph on the first N points of the sampling order, per (N, K): some rows reach K, some do not
# (asserted on the counts; the spacing of N farthest-point samples of an S3DIS-like block goes with 1 / sqrt(N))
INTRA_RADIUS = {
    (65, 8): 0.9, (65, 64): 2.6,
    (128, 8): 0.65, (128, 64): 2.0,
    (384, 8): 0.4, (384, 64): 1.2,
    (768, 8): 0.3, (768, 64): 0.9,
    (1023, 8): 0.25, (1023, 64): 0.8,
    (1024, 8): 0.25, (1024, 64): 0.8,
}
# (N, M, radius): queries = the first M points of the sampling order, or (M > 1024) of the block itself; every query has a
# database point inside the radius
INTER = [(128, 384, 0.6), (384, 768, 0.4), (768, 2048, 0.3), (768, 1500, 0.3), (64, 1, 0.5)]

_cache = {}


def _points(dev):
    """-> (block [B, 2048, 3], the same points in farthest-point order [B, 1024, 3]), numpy, computed once: planes, and
    exact zeros in dx, dy, dz between neighbours"""
    if "pts" not in _cache:
        block = synth.s3dis_batch(5, B, 2048)[0][:, :, :3].copy()
        order = tf_sample.farthest_point_sample(1024, torch.from_numpy(block).to(dev)).cpu().numpy().astype(np.int64)
        fps = np.ascontiguousarray(np.take_along_axis(block, order[:, :, None], axis=1))
        block.setflags(write=False)
        fps.setflags(write=False)
        _cache["pts"] = (block, fps)
    return _cache["pts"]


def _db_query(dev, N, M):
    block, fps = _points(dev)
    db = np.ascontiguousarray(fps[:, :N])
    q = np.ascontiguousarray(fps[:, :M] if M <= 1024 else block[:, :M])
    return db, q


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(dev)          # (the shared points are read-only)


def _workspace(l, dev, nb, N, M):
    need = l.sph3d_build_sphere_neighbor_workspace(nb, N, M)
    assert need > 0, "clouds of at most 1024 points size a workspace (flag, thresholds, one header per cloud)"
    return torch.zeros((need,), dtype=torch.uint8, device=dev)


def _search(l, dev, db, q, K, radius, ws, fixed=False):
    """-> rc, (nn_index, nn_count, nn_dist as int32 bit patterns), numpy"""
    nb, N, _ = db.shape
    M = q.shape[1]
    idx = torch.full((nb, M, K), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((nb, M), -1, dtype=torch.int32, device=dev)
    dst = torch.full((nb, M, K), -1.0, dtype=torch.float32, device=dev)
    fn = l.sph3d_build_sphere_neighbor_fixed_ws if fixed else l.sph3d_build_sphere_neighbor_ws
    rc = fn(nb, N, M, K, radius, _lib.ptr(db), _lib.ptr(q), _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(dst), _lib.ptr(ws),
            0 if ws is None else ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, (idx.cpu().numpy(), cnt.cpu().numpy(), dst.cpu().numpy().view(np.int32))


def _graph(l, dev, db, q, K, radius, ws, ocml, binned):
    """the fused construction (bins when `binned`, segment counts of the transposed graph)
    -> rc, (nn_index, nn_count, nn_dist bits, filt_index or None, segment totals [B, N * F'])"""
    nb, N, _ = db.shape
    M = q.shape[1]
    Fb = F if binned else 1
    idx = torch.full((nb, M, K), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((nb, M), -1, dtype=torch.int32, device=dev)
    dst = torch.full((nb, M, K), -1.0, dtype=torch.float32, device=dev)
    filt = torch.full((nb, M, K), -1, dtype=torch.int32, device=dev) if binned else None
    twsb = l.sph3d_graph_transpose_workspace(nb, N, M, K, Fb)
    tws = torch.empty((twsb,), dtype=torch.uint8, device=dev)
    n, p, qq = KERNEL if binned else (0, 0, 0)
    rc = l.sph3d_build_sphere_graph_ws(nb, N, M, K, radius, n, p, qq, ocml, _lib.ptr(db), _lib.ptr(q), _lib.ptr(idx), _lib.ptr(cnt),
                                       _lib.ptr(dst), _lib.ptr(filt), _lib.ptr(tws), twsb, _lib.ptr(ws),
                                       0 if ws is None else ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    seg = tws[:nb * N * Fb * 4].view(torch.int32).reshape(nb, N * Fb).cpu().numpy()      # (common.hpp tg_ws: the counters lead)
    return rc, (idx.cpu().numpy(), cnt.cpu().numpy(), dst.cpu().numpy().view(np.int32),
                filt.cpu().numpy() if binned else None, seg)


def _flag(ws):
    return int(ws[:4].view(torch.int32).item())          # the gate: the workspace's first word


def _equal(got, want):
    for g, w in zip(got, want):
        if w is None:
            assert g is None
        else:
            np.testing.assert_array_equal(g, w)


def _both_paths(l, dev, call, ws, expect_gate=0):
    """call(ws) with and without the workspace: the new path ran (counter), the gate reads as expected, everything is equal"""
    before = l.sph3d_nngrid_launches()
    rc0, want = call(None)
    assert rc0 == 0 and l.sph3d_nngrid_launches() == before, "workspace = NULL: the chain kernel"
    rc1, got = call(ws)
    assert rc1 == 0
    assert l.sph3d_nngrid_launches() == before + 1, "a workspace: the early-stopping scan over every query"
    assert _flag(ws) == expect_gate
    _equal(got, want)
    return want


def _has_neighbour(db, q, radius):
    d = np.linalg.norm(q[:, :, None, :].astype(np.float64) - db[:, None, :, :].astype(np.float64), axis=-1)
    return d.min(axis=2) < 0.999 * radius


@pytest.mark.parametrize("K", [8, 64])
@pytest.mark.parametrize("N", [65, 128, 384, 768, 1023, 1024])
def test_intra_graphs_equal_the_chain_kernel(dev, N, K):
    """query = database; less than one trip of 256 points, N no multiple of 64, the largest cloud; plain search, then the fused
    construction with bins (both angle functions) and segment counts"""
    l = _lib.lib()
    dbn, _ = _db_query(dev, N, N)
    db = _t(dbn, dev)
    radius = INTRA_RADIUS[(N, K)]
    ws = _workspace(l, dev, B, N, N)
    _, cnt, _ = _both_paths(l, dev, lambda w: _search(l, dev, db, db, K, radius, w), ws)
    assert cnt.min() >= 1 and (cnt == K).any() and (cnt < K).any()
    for ocml in (0, 1):
        want = _both_paths(l, dev, lambda w: _graph(l, dev, db, db, K, radius, w, ocml, True), ws)
        assert want[4].sum() == want[1].sum() and len(np.unique(want[3])) > 8


@pytest.mark.parametrize("shape", INTER, ids=lambda s: "N%d-M%d" % s[:2])
def test_inter_graphs_equal_the_chain_kernel(dev, shape):
    """un-pooling graphs: more queries than points; 2048 queries are two full chain positions (r0, r0 + 0.05), 1500 a ragged
    second one; one query"""
    N, M, radius = shape
    l = _lib.lib()
    dbn, qn = _db_query(dev, N, M)
    assert _has_neighbour(dbn, qn, radius).all()
    db, q = _t(dbn, dev), _t(qn, dev)
    ws = _workspace(l, dev, B, N, M)
    for K in (8, 64):
        _both_paths(l, dev, lambda w: _search(l, dev, db, q, K, radius, w), ws)
        want = _both_paths(l, dev, lambda w: _graph(l, dev, db, q, K, radius, w, 0, False), ws)      # counted, no bins
        assert want[4].sum() == want[1].sum()
    if M > 1024:
        # the second position searches with the grown radius: it finds more
        _, cnt, _ = _search(l, dev, db, q, 1024, radius, None)[1]
        assert cnt[:, 1024:].mean() > cnt[:, :1024].mean()


def test_an_isolated_query_raises_the_gate_and_the_chain_kernel_recomputes(dev):
    """compat mode: a query without a neighbour inside its radius takes a second pass in the reference, and the radius it grew
    is what the next query of its chain starts from — the one case in which queries depend on each other.  At position 0 and
    at position 1."""
    l = _lib.lib()
    N, M, radius, K = 768, 2048, 0.3, 8
    dbn, qn = _db_query(dev, N, M)
    db = _t(dbn, dev)
    ws = _workspace(l, dev, B, N, M)
    for j in (5, 1024 + 77):
        far = qn.copy()
        far[1, j] += np.float32(0.45)            # beyond its radius, found after growth: its chain's later query changes too
        assert not _has_neighbour(dbn, far, radius + (0.05 if j >= 1024 else 0.0))[1, j]
        q = _t(far, dev)
        _, cnt, _ = _both_paths(l, dev, lambda w: _search(l, dev, db, q, K, radius, w), ws, expect_gate=1)
        assert cnt[1, j] >= 1                   # (the chain kernel grew the radius until it found one)
        _both_paths(l, dev, lambda w: _graph(l, dev, db, q, K, radius, w, 0, False), ws, expect_gate=1)
    # and the flag does not stick: the next call without an isolated query is the scan's alone
    _both_paths(l, dev, lambda w: _search(l, dev, db, _t(qn, dev), K, radius, w), ws)


def test_fixed_radius_mode(dev):
    """every query at the nominal radius, whatever its chain position"""
    l = _lib.lib()
    for N, M, radius in ((384, 384, 0.4), (768, 2048, 0.3)):
        dbn, qn = _db_query(dev, N, M)
        db, q = _t(dbn, dev), _t(qn, dev)
        ws = _workspace(l, dev, B, N, M)
        _, cnt, _ = _both_paths(l, dev, lambda w: _search(l, dev, db, q, 8, radius, w, fixed=True), ws)
        assert cnt.min() >= 1
    far = qn.copy()
    far[2, 1500] += np.float32(5.0)
    _both_paths(l, dev, lambda w: _search(l, dev, db, _t(far, dev), 8, radius, w, fixed=True), ws, expect_gate=1)


@pytest.mark.parametrize("fixed", [False, True], ids=["compat", "fixed"])
def test_rows_equal_the_oracle(dev, fixed):
    l = _lib.lib()
    N, M, radius, K = 768, 2048, 0.3, 8
    dbn, qn = _db_query(dev, N, M)
    idx_o, cnt_o, dst_o = oracle.build_sphere_neighbor(dbn, qn, radius, None, K, fixed=fixed)
    ws = _workspace(l, dev, B, N, M)
    before = l.sph3d_nngrid_launches()
    rc, (idx, cnt, dst) = _search(l, dev, _t(dbn, dev), _t(qn, dev), K, radius, ws, fixed=fixed)
    assert rc == 0 and l.sph3d_nngrid_launches() == before + 1 and _flag(ws) == 0
    np.testing.assert_array_equal(cnt, cnt_o)
    np.testing.assert_array_equal(idx, idx_o)
    np.testing.assert_array_equal(dst, dst_o.view(np.int32))


def test_batches_outside_3_to_32_clouds_keep_the_chain_kernel(dev):
    """clouds b and b + 32 share a reference block and its chains: not taken (no workspace is sized, and one that is given
    anyway is left alone); neither are one or two clouds"""
    l = _lib.lib()
    N, K, radius = 128, 8, 0.65
    dbn, _ = _db_query(dev, N, N)
    db33 = _t(np.concatenate([dbn] * 11, axis=0), dev)                     # 33 clouds
    assert l.sph3d_build_sphere_neighbor_workspace(33, N, N) == 0
    assert l.sph3d_build_sphere_neighbor_workspace(32, N, N) > 0
    before = l.sph3d_nngrid_launches()
    rc0, want = _search(l, dev, db33, db33, K, radius, None)
    ws = torch.zeros((1 << 16,), dtype=torch.uint8, device=dev)
    rc1, got = _search(l, dev, db33, db33, K, radius, ws)
    assert rc0 == 0 and rc1 == 0 and l.sph3d_nngrid_launches() == before
    _equal(got, want)
    # cloud 32 continues cloud 0's chains: the same points, a larger radius
    assert want[1][32].sum() > want[1][0].sum()
    # the lower bound: batches of one or two clouds stay with the chain kernel as well (tests/test_abi.py and
    # tests/test_gpu_nngrid.py pin them to "no workspace, no launch counted")
    assert l.sph3d_build_sphere_neighbor_workspace(2, N, N) == 0 and l.sph3d_build_sphere_neighbor_workspace(3, N, N) > 0
    db2 = _t(dbn[:2], dev)
    rc0, want = _search(l, dev, db2, db2, K, radius, None)
    rc1, got = _search(l, dev, db2, db2, K, radius, ws)
    assert rc0 == 0 and rc1 == 0 and l.sph3d_nngrid_launches() == before
    _equal(got, want)


def test_a_workspace_that_is_too_small_is_refused(dev):
    l = _lib.lib()
    dbn, _ = _db_query(dev, 128, 128)
    db = _t(dbn, dev)
    need = l.sph3d_build_sphere_neighbor_workspace(B, 128, 128)
    ws = torch.zeros((need - 16,), dtype=torch.uint8, device=dev)
    rc, _ = _search(l, dev, db, db, 8, 0.65, ws)
    assert rc == -2 and b"workspace" in l.sph3d_last_error()


def test_the_search_runs_under_stream_capture(dev):
    """nothing allocates or synchronises: one call captured into a graph (a single chain of nodes) and replayed once"""
    l = _lib.lib()
    N, M, K, radius = 384, 768, 8, 0.4
    dbn, qn = _db_query(dev, N, M)
    db, q = _t(dbn, dev), _t(qn, dev)
    ws = _workspace(l, dev, B, N, M)
    rc, want = _search(l, dev, db, q, K, radius, ws)
    assert rc == 0
    idx = torch.zeros((B, M, K), dtype=torch.int32, device=dev)
    cnt = torch.zeros((B, M), dtype=torch.int32, device=dev)
    dst = torch.zeros((B, M, K), dtype=torch.float32, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    before = l.sph3d_nngrid_launches()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            rc = l.sph3d_build_sphere_neighbor_ws(B, N, M, K, radius, _lib.ptr(db), _lib.ptr(q), _lib.ptr(idx), _lib.ptr(cnt),
                                                  _lib.ptr(dst), _lib.ptr(ws), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and l.sph3d_nngrid_launches() == before + 1
    assert int(cnt.abs().sum()) == 0                               # captured, not run
    g.replay()
    torch.cuda.synchronize()
    _equal((idx.cpu().numpy(), cnt.cpu().numpy(), dst.cpu().numpy().view(np.int32)), want)
