"""The paths of the range search's plan (csrc/nn_plan.hpp) that no other GPU case list reaches, on the device: each case is pinned
to its path by the plan query, compared with the CPU oracle (indices and counts as integers, distances bit for bit), and the
launch counter moves exactly when the plan has a front.  The lists of test_gpu_nngrid, test_gpu_nnsmall, test_gpu_boundary,
test_gpu_parity and test_gpu_tgraph reach the chain kernel at one and four chains per wave and in its multi-chunk form with
deferred hit lists, at one chain per wave without them, the grid alone (both radius modes) and with the early-stopping scan, and
the small clouds (both modes) — decided on the host from the plan query over those lists, DESIGN.md 4.23.  Left out there: two
chains per wave, the other three forms without deferred lists, a grid that takes one position in front of the scan, and the graph
construction falling back to the separate kernels."""
import numpy as np
import pytest
import torch

import _nn_forms as S
import oracle
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import synth

pytestmark = pytest.mark.gpu

KERNEL = (8, 2, 2)
F = KERNEL[0] * KERNEL[1] * KERNEL[2] + 1

# (id, fixed, B, N, M, K, radius, workspace given, the plan's fields that name the path)
CASES = [
    ("chain-cpw2-defer", 0, 8, 256, 1024, 8, 0.15, False, dict(front=S.NONE, CPW=2, MULTI=0, DEFER=1)),
    ("chain-cpw2-inline", 0, 8, 256, 1024, 321, 0.8, False, dict(front=S.NONE, CPW=2, MULTI=0, DEFER=0)),
    ("chain-cpw4-inline", 0, 16, 256, 1024, 161, 0.6, False, dict(front=S.NONE, CPW=4, MULTI=0, DEFER=0)),
    ("chain-multi-inline", 0, 1, 12289, 64, 641, 0.25, False, dict(front=S.NONE, CPW=1, MULTI=1, DEFER=0, chunkN=12288)),
    # a front, for the counter: the grid takes position 0 alone and leaves the second thousand queries to the scan (the lists
    # reach grid + scan only with two or more positions in the grid)
    ("grid-one-position-and-scan", 0, 1, 2048, 2048, 16, 0.02, True, dict(front=S.GRID, npos=1, j0=1024, dparts=64)),
]


def _plan(fixed, B, N, M, K, radius, fuse, memory):
    out = np.zeros(len(S.FIELDS), dtype=np.int64)
    assert _lib.lib().sph3d_build_sphere_neighbor_plan(fixed, B, N, M, K, radius, fuse, memory, out.ctypes.data) == 0
    return dict(zip(S.FIELDS, (int(v) for v in out)))


def _points(B, N, M, front):
    """database; queries: with a front its own first points (every query has itself as a neighbour: the flag stays down), else
    points of their own (some find nothing at the nominal radius: the chains grow)"""
    db = synth.uniform_cloud(7, B, N, 1.0)
    if front or M <= N:
        return db, np.ascontiguousarray(db[:, :M])
    return db, synth.uniform_cloud(8, B, M, 1.0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_each_path_of_the_plan_equals_the_oracle(dev, case):
    _, fixed, B, N, M, K, radius, with_ws, path = case
    l = _lib.lib()
    need = l.sph3d_build_sphere_neighbor_workspace(B, N, M)
    p = _plan(fixed, B, N, M, K, radius, 0, S.MEM_CALLER if with_ws else S.MEM_NONE)
    assert {k: p[k] for k in path} == path, p
    assert (need > 0) == (p["front"] != S.NONE) or not with_ws
    dbn, qn = _points(B, N, M, p["front"] != S.NONE)
    db, q = _t(dbn, dev), _t(qn, dev)
    ws = torch.zeros((max(need, 16),), dtype=torch.uint8, device=dev) if with_ws else None
    idx = torch.full((B, M, K), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((B, M), -1, dtype=torch.int32, device=dev)
    dst = torch.full((B, M, K), -1.0, dtype=torch.float32, device=dev)
    fn = l.sph3d_build_sphere_neighbor_fixed_ws if fixed else l.sph3d_build_sphere_neighbor_ws
    before = l.sph3d_nngrid_launches()
    rc = fn(B, N, M, K, radius, _lib.ptr(db), _lib.ptr(q), _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(dst), _lib.ptr(ws),
            0 if ws is None else ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and l.sph3d_nngrid_launches() - before == int(p["front"] != S.NONE)
    if p["front"] != S.NONE:
        assert int(ws[:4].view(torch.int32).item()) == 0          # the flag stayed down: the rows are the front's
    idx_o, cnt_o, dst_o = oracle.build_sphere_neighbor(dbn, qn, radius, None, K, fixed=bool(fixed))
    np.testing.assert_array_equal(cnt.cpu().numpy(), cnt_o)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_o)
    np.testing.assert_array_equal(dst.cpu().numpy().view(np.int32), dst_o.view(np.int32))
    assert cnt_o.min() >= 1 and (cnt_o < K).any()


def test_graph_construction_without_deferred_lists_runs_the_separate_kernels(dev):
    """K = 641: the hit lists of one chain per wave do not fit LDS, so nothing is fused — sph3d_build_sphere_graph_ws runs the
    bins and the segment counts behind the search, and the result is that of the separate ops"""
    B, N, M, K, radius = 1, 700, 70, 641, 0.6
    l = _lib.lib()
    p = _plan(0, B, N, M, K, radius, 1, S.MEM_NONE)
    assert (p["front"], p["DEFER"], p["fused"], p["clear_counts"]) == (S.NONE, 0, 0, 0)
    assert _plan(0, B, N, M, 640, radius, 1, S.MEM_NONE)["fused"] == 1
    dbn, qn = _points(B, N, M, False)
    db, q = _t(dbn, dev), _t(qn, dev)
    idx = torch.full((B, M, K), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((B, M), -1, dtype=torch.int32, device=dev)
    dst = torch.full((B, M, K), -1.0, dtype=torch.float32, device=dev)
    filt = torch.full((B, M, K), -1, dtype=torch.int32, device=dev)
    twsb = l.sph3d_graph_transpose_workspace(B, N, M, K, F)
    tws = torch.empty((twsb,), dtype=torch.uint8, device=dev)
    before = l.sph3d_nngrid_launches()
    rc = l.sph3d_build_sphere_graph_ws(B, N, M, K, radius, *KERNEL, 0, _lib.ptr(db), _lib.ptr(q), _lib.ptr(idx), _lib.ptr(cnt),
                                       _lib.ptr(dst), _lib.ptr(filt), _lib.ptr(tws), twsb, None, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and l.sph3d_nngrid_launches() == before
    idx_o, cnt_o, dst_o = oracle.build_sphere_neighbor(dbn, qn, radius, None, K)
    filt_o = oracle.spherical_kernel(dbn, qn, idx_o, cnt_o, dst_o, radius, list(KERNEL))
    np.testing.assert_array_equal(cnt.cpu().numpy(), cnt_o)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_o)
    np.testing.assert_array_equal(dst.cpu().numpy().view(np.int32), dst_o.view(np.int32))
    np.testing.assert_array_equal(filt.cpu().numpy(), filt_o)
    # the segment counts of the transposed graph (common.hpp tg_ws: the counters lead the workspace)
    seg = tws[:B * N * F * 4].view(torch.int32).reshape(B, N * F).cpu().numpy()
    want = np.zeros_like(seg)
    used = np.arange(K)[None, None, :] < cnt_o[:, :, None]
    for b in range(B):
        np.add.at(want[b], (idx_o[b].astype(np.int64) * F + filt_o[b])[used[b]], 1)
    np.testing.assert_array_equal(seg, want)
    assert len(np.unique(filt_o)) > 8 and (cnt_o < K).any()
