"""Scene preparation, measured: device time of the stages of harness/sceneprep.py (csrc/prep.hip) on a synthetic
room at the size of an S3DIS room, against the numpy statement of the same stage in the same run.

  scene   harness/scenesynth.py: a 9 x 7 x 3 m room of labelled surfaces, F = 3e6 full-resolution points in RANDOM order with
          random colours (the shape of tools/exp_scene.py), voxelised at 3 cm
  device  event pairs around the entries of a stage; median of `repeats` after a priming run
            grid      sph3d_prep_voxel_grid (box, table, mark, scan, voxel_of_point)
            reduce    sph3d_prep_voxel_reduce in BOTH forms (64-bit integer atomics | counting sort + per-row sum) + _finalize
            counts    sph3d_prep_normalise and sph3d_prep_rect_count over all candidates (18 per square) in one launch
            fill      sph3d_prep_block_fill into the pool's tensors
            nn1       sph3d_nn1 of the room (voxel cloud as reference, full cloud as queries): the step the whole preparation
                      is to stay below
  host    voxel_reference (grid + reduce together: the statement does not separate them), normalise_reference +
          rect_counts_reference, the fill loop of split_reference
usage: python tools/exp_prep.py [repeats] [full_points]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import sceneprep as sp, scenemerge as sm, scenesynth

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
FULL = int(sys.argv[2]) if len(sys.argv) > 2 else 3000000
H, THRESH = 0.03, 10000
dev = torch.device("cuda:0"); l = _lib.lib()

full_xyz, full_label, _vx, _vl = scenesynth.synthetic_scene(0, FULL, extent=(9.0, 7.0, 3.0))
full_rgb = (np.random.RandomState(1).rand(FULL, 3) * 255).astype(np.float32)
fx, fc = torch.from_numpy(full_xyz).to(dev), torch.from_numpy(full_rgb).to(dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def median(fn):
    fn()                                                       # priming
    torch.cuda.synchronize()
    runs = [timed(fn) for _ in range(REPEATS)]
    return float(np.median([r[0] for r in runs])), runs[-1][1]


# ---- the device stages --------------------------------------------------------------------------------------------------------
# grid: the entry alone (buffers allocated outside the timed region); the header's read is the harness's one synchronisation
vop = torch.empty((FULL,), dtype=torch.int32, device=dev)
header = torch.empty((sp.HEADER_WORDS,), dtype=torch.int32, device=dev)
need = int(l.sph3d_prep_voxel_grid_workspace(FULL, sp.DEFAULT_MAX_CELLS))
ws = torch.empty((need,), dtype=torch.uint8, device=dev)
grid_ms, _ = median(lambda: _lib.check(l.sph3d_prep_voxel_grid(FULL, 3, _lib.ptr(fx), _lib.ptr(fc), H, sp.DEFAULT_MAX_CELLS, _lib.ptr(vop),
                                                               _lib.ptr(header), _lib.ptr(ws), need, _lib.stream_ptr())))
hd = header.cpu().numpy()
V, cells = int(hd[0]), int(hd[12])
del ws
print("scene: F = %d full points, V = %d voxel points, grid %d x %d x %d = %d cells (table of %d)"
      % (FULL, V, hd[3], hd[4], hd[5], cells, sp.DEFAULT_MAX_CELLS))
reduce_ms = {}
for name, mode in (("atomic", sp.REDUCE_ATOMIC), ("sorted", sp.REDUCE_SORTED)):
    reduce_ms[name], (vx, vc, count, box) = median(lambda: sp.voxel_reduce(fx, fc, vop, V, mode))
    if name == "atomic":
        first = [t.cpu().numpy() for t in (vx, vc, count)]
    else:
        print("both reduce forms give the same bits: %s" % all(np.array_equal(a.view(np.int32), t.cpu().numpy().view(np.int32))
                                                             for a, t in zip(first, (vx, vc, count))))
box_h = box.cpu().numpy()
lo, hi = sp.normalised_extrema(box_h)
cand = sp.candidate_rects(lo[0:2], hi[0:2])
both = torch.from_numpy(np.concatenate([sp.rounded_rects(cand).reshape(-1, 4), sp.rounded_rects(cand, 0.3).reshape(-1, 4)])).to(dev)


def dev_counts():
    nx, nc = sp.normalise(vx, vc, box)
    return nx, nc, sp.rect_counts(nx, both)


counts_ms, (nx, nc, _counts) = median(dev_counts)
vl = torch.zeros((V,), dtype=torch.int32, device=dev)
plan = sp.plan_split(nx, lo[0:2], hi[0:2], thresh=THRESH)
T, P = int(plan.sizes.sum()), len(plan.sizes)
rows = torch.empty((T, 8), dtype=torch.float32, device=dev)
index = torch.empty((T,), dtype=torch.int32, device=dev)
offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(plan.sizes))).astype(np.int64)).to(dev)
fill_ms, _ = median(lambda: sp.fill_split(nx, nc, vl, plan, rows, index, offsets))
kinds = np.bincount(np.array([k for k, _r in plan.plan]) + 1, minlength=10)
print("plan: %d squares, %d rectangles counted in one launch, %d blocks (%d kept, %d merged, %d skipped), %d rows"
      % (len(plan.plan), both.shape[0], P, kinds[1], kinds[2:].sum(), kinds[0], T))
idx = torch.empty((FULL,), dtype=torch.int32, device=dev)
nn_need = int(l.sph3d_nn1_workspace(V, FULL))
nn_ws = torch.empty((nn_need,), dtype=torch.uint8, device=dev)
nn1_ms, _ = median(lambda: _lib.check(l.sph3d_nn1(V, FULL, _lib.ptr(vx), _lib.ptr(fx), sm.NN1_GRID, _lib.ptr(idx), _lib.ptr(nn_ws), nn_need,
                                                  _lib.stream_ptr())))

# ---- the host form --------------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
voxel, h_count, h_vop, _dropped = sp.voxel_reference(full_xyz, full_rgb, H)
t1 = time.perf_counter()
h_nx, h_nc, _c = sp.normalise_reference(voxel[:, 0:3], voxel[:, 3:6])
h_counts = sp.rect_counts_reference(h_nx, both.cpu().numpy())
t2 = time.perf_counter()
h_blocks, h_index, h_plan = sp.split_reference(h_nx, h_nc, np.zeros((len(h_nx),), np.int32), thresh=THRESH)
t3 = time.perf_counter()
split_counts_ms = 0.0                                          # (split_reference counts the candidates again: taken off below)
ta = time.perf_counter()
sp.rect_counts_reference(h_nx, sp.rounded_rects(cand).reshape(-1, 4))
split_counts_ms = (time.perf_counter() - ta) * 1e3
same = (np.array_equal(voxel[:, 0:3].view(np.int32), first[0].view(np.int32)) and np.array_equal(voxel[:, 3:6].view(np.int32), first[1].view(np.int32))
        and np.array_equal(h_count, first[2]) and np.array_equal(h_vop, vop.cpu().numpy()))
print("device equals host: voxel cloud %s, counts %s, plan %s, rows %s, index %s"
      % (same, bool(np.array_equal(h_counts, _counts.cpu().numpy())), h_plan == plan.plan,
         bool(np.array_equal(np.concatenate(h_blocks).view(np.int32), rows.cpu().numpy().view(np.int32))),
         bool(np.array_equal(np.concatenate(h_index), index.cpu().numpy()))))
best = min(reduce_ms, key=reduce_ms.get)
host = {"grid + reduce": (t1 - t0) * 1e3, "counts": (t2 - t1) * 1e3, "fill": (t3 - t2) * 1e3 - split_counts_ms}
print("grid            device %10.3f ms" % grid_ms)
for name in ("atomic", "sorted"):
    print("reduce %-8s device %10.3f ms%s" % (name, reduce_ms[name], "   <- the faster form" if name == best else ""))
print("grid + reduce   device %10.3f ms   host %12.1f ms   host / device %8.1f" % (grid_ms + reduce_ms[best], host["grid + reduce"],
                                                                                 host["grid + reduce"] / (grid_ms + reduce_ms[best])))
print("counts          device %10.3f ms   host %12.1f ms   host / device %8.1f" % (counts_ms, host["counts"], host["counts"] / counts_ms))
print("fill            device %10.3f ms   host %12.1f ms   host / device %8.1f" % (fill_ms, host["fill"], host["fill"] / fill_ms))
total = grid_ms + reduce_ms[best] + counts_ms + fill_ms
print("preparation     device %10.3f ms (with the default form, atomic: %.3f ms)   nn1 grid of the room %10.3f ms   preparation / nn1 %.2f"
      % (total, grid_ms + reduce_ms["atomic"] + counts_ms + fill_ms, nn1_ms, total / nn1_ms))
