"""The scene-level evaluation, measured: device time of the stages of harness/scenemerge.py (csrc/scene.hip) on
synthetic scenes at the size of an S3DIS room, against the host form of the same stage in the same run.

  scene   harness/scenesynth.py: a 9 x 7 x 3 m room of labelled surfaces, F = 3e6 full-resolution points in RANDOM order (the
          worst case for the search kernel, which takes the queries as they come), V ~ 3e5 voxel points (2.2 cm cells), blocks
          cut with the reference's geometry (1.5 m inner squares every 0.75 m, 0.3 m of context)
  votes   random vote sums [rows, 13] in the voter's layout (the stages after the voting do not care where the sums come from)
  device  event pairs around sph3d_scene_merge (all batches of 16 blocks), _finalize, sph3d_nn1 in grid and in brute mode, _lift;
          median of `repeats`
  host    the numpy statement on the sums copied back (the copy is timed with it): merge_update per block, finalize_reference,
          lift_reference; nearest_reference on a SUBSAMPLE of `nn_sub` queries, extrapolated linearly to F and labelled as such
usage: python tools/exp_scene.py [repeats] [full_points] [nn_sub]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import feed, scenemerge as sm, scenesynth

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
FULL = int(sys.argv[2]) if len(sys.argv) > 2 else 3000000
NN_SUB = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
B, C = 16, 13
dev = torch.device("cuda:0"); l = _lib.lib()

full_xyz, full_label, vx, vl = scenesynth.synthetic_scene(0, FULL, extent=(9.0, 7.0, 3.0), voxel=0.022)
blocks, index = scenesynth.split_scene(vx, vl)
V, F = len(vx), len(full_xyz)
pool = feed.BlockPool(blocks, dev, index, [0] * len(blocks))
T = int(pool.rows.shape[0])
rng = np.random.RandomState(1)
votes_host = (rng.randn(T, C) * 5).astype(np.float32)
votes = torch.from_numpy(votes_host).to(dev)
hits_per_row = np.bincount(np.concatenate([i[b[:, 7] == 1] for b, i in zip(blocks, index)]), minlength=V)
print("scene: V = %d voxel points, F = %d full points, %d blocks of %d .. %d rows (%d rows), inner hits per scene row: mean %.2f max %d"
      % (V, F, len(blocks), min(map(len, blocks)), max(map(len, blocks)), T, hits_per_row.mean(), hits_per_row.max()))

vx_dev, full_dev = torch.from_numpy(vx).to(dev), torch.from_numpy(full_xyz).to(dev)
vl_dev, fl_dev = torch.from_numpy(vl).to(dev), torch.from_numpy(full_label).to(dev)
merged = torch.zeros((V, C), dtype=torch.float32, device=dev)
hits = torch.zeros((V,), dtype=torch.int32, device=dev)
counters = torch.zeros((3,), dtype=torch.int64, device=dev)
conf = torch.zeros((2, C * C), dtype=torch.int64, device=dev)
pv = torch.empty((V,), dtype=torch.int32, device=dev)
pf = torch.empty((F,), dtype=torch.int32, device=dev)
idx = torch.empty((F,), dtype=torch.int32, device=dev)
ws = torch.empty((l.sph3d_nn1_workspace(V, F),), dtype=torch.uint8, device=dev)
batches = [np.arange(a, min(len(blocks), a + B), dtype=np.int32) for a in range(0, len(blocks), B)]
batches_dev = [torch.from_numpy(ids).to(dev) for ids in batches]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def dev_merge():
    merged.zero_(); hits.zero_(); counters.zero_()
    for ids, ids_dev in zip(batches, batches_dev):
        base = int(pool.host_offsets[ids[0]])
        nrows = int(pool.host_offsets[ids[-1] + 1]) - base
        # votes: the whole pool's sums in pool-row order; a batch's range starts at its first row, as in the voter's buffer
        _lib.check(l.sph3d_scene_merge(len(ids), C, len(pool), T, _lib.ptr(pool.rows), _lib.ptr(pool.offsets), _lib.ptr(pool.index),
                                       _lib.ptr(ids_dev), base, nrows, votes[base:].data_ptr(), V, _lib.ptr(merged), _lib.ptr(hits),
                                       _lib.ptr(counters), _lib.stream_ptr()))


def dev_finalize():
    _lib.check(l.sph3d_scene_finalize(C, V, _lib.ptr(merged), _lib.ptr(hits), _lib.ptr(vl_dev), _lib.ptr(pv), _lib.ptr(counters[2:]),
                                      _lib.ptr(conf[1]), _lib.stream_ptr()))


def dev_nn1(mode):
    _lib.check(l.sph3d_nn1(V, F, _lib.ptr(vx_dev), _lib.ptr(full_dev), mode, _lib.ptr(idx), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))


def dev_lift():
    _lib.check(l.sph3d_scene_lift(C, V, F, _lib.ptr(pv), _lib.ptr(idx), None, _lib.ptr(fl_dev), _lib.ptr(pf), _lib.ptr(conf[0]),
                                  _lib.stream_ptr()))


stages = [("merge", dev_merge), ("finalize", dev_finalize), ("nn1 grid", lambda: dev_nn1(sm.NN1_GRID)), ("lift", dev_lift)]
for _name, fn in stages:                      # priming
    fn()
torch.cuda.synchronize()
device_ms = {name: float(np.median([timed(fn) for _ in range(REPEATS)])) for name, fn in stages}
idx_grid = idx.cpu().numpy()
device_ms["nn1 brute"] = float(np.median([timed(lambda: dev_nn1(sm.NN1_BRUTE)) for _ in range(max(1, REPEATS // 2))]))
print("grid and brute give the same idx: %s" % bool(np.array_equal(idx_grid, idx.cpu().numpy())))

# ---- the host form ----------------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
h_votes = votes.cpu().numpy()
h_merged, h_hits = np.zeros((V, C), np.float32), np.zeros((V,), np.int32)
for k, (b, i) in enumerate(zip(blocks, index)):
    lo, hi = int(pool.host_offsets[k]), int(pool.host_offsets[k + 1])
    sm.merge_update(h_merged, h_hits, h_votes[lo:hi], b[:, 7], i)
t1 = time.perf_counter()
h_pv, _unseen = sm.finalize_reference(h_merged, h_hits)
sm.voxel_confusion(h_pv, vl, C)
t2 = time.perf_counter()
sub = np.random.RandomState(2).permutation(F)[:NN_SUB]
h_idx_sub = sm.nearest_reference(vx, full_xyz[sub])
t3 = time.perf_counter()
sm.lift_reference(h_pv, idx_grid, full_label, None, C)
t4 = time.perf_counter()
host_ms = {"merge": (t1 - t0) * 1e3, "finalize": (t2 - t1) * 1e3, "nn1 grid": (t3 - t2) * 1e3 * F / NN_SUB, "lift": (t4 - t3) * 1e3}
dev_merge(); dev_finalize()
torch.cuda.synchronize()
print("device equals host: merged %s, pred_voxel %s, idx on the subsample %s"
      % (bool(np.array_equal(merged.cpu().numpy().view(np.int32), h_merged.view(np.int32))), bool(np.array_equal(pv.cpu().numpy(), h_pv)),
         bool(np.array_equal(idx_grid[sub], h_idx_sub))))
for name in ("merge", "finalize", "nn1 grid", "lift"):
    note = " [host: %d queries took %.1f s, EXTRAPOLATED linearly to %d]" % (NN_SUB, t3 - t2, F) if name == "nn1 grid" else ""
    print("%-9s device %10.3f ms   host %12.1f ms   host / device %10.1f%s" % (name, device_ms[name], host_ms[name],
                                                                             host_ms[name] / device_ms[name], note))
print("nn1 brute device %10.3f ms   brute / grid %.1f" % (device_ms["nn1 brute"], device_ms["nn1 brute"] / device_ms["nn1 grid"]))
