"""The normal kernels, measured: device time of tf_surface.graph_normals and tf_surface.ball_normals against the
numpy statement of harness/normals.py on the host, and the calls' algorithmic bytes over the achievable HBM rate.

  arms    graph   the level-0 graph of the headline plan: 16 S3DIS-like blocks of 8192 points, radius 0.1, K = 64
          facade  ball_normals at r = 0.1 on a synthetic facade of 400 000 rows (a jittered 12 m x 8 m wall with two ledges)
          room    ball_normals at r = 0.1 on a room of harness/scenesynth.py, about 1 M voxel rows
  device  HIP events around the call, median of 10 launches after one warm-up; every arm is run twice, in turn
  host    the statement: the graph arm in full; the ball arms on a SUBSAMPLE of `sub` queries against all points, extrapolated
          linearly to all rows and labelled as such
  bytes   graph: 4 B M K index words + 12 per gathered row (sum of min(count, K)) + 12 per query + the outputs (12 + 4 + 4);
          ball: 16 per sorted point of the cells a query's walk visits, summed over the 64-query waves' UNION of cells (lanes
          of a wave share what they load), + 16 per query + the outputs (12 + 4 + 4).  Over HBM_GBS = 6290 (the measured copy rate).
usage: python tools/exp_normals.py [sub]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sph3d_gcn_amd import tf_nnquery, tf_surface
from sph3d_gcn_amd.harness import normals as nrm, scenesynth, synth

SUB = int(sys.argv[1]) if len(sys.argv) > 1 else 512
HBM_GBS = 6290.0
dev = torch.device("cuda:0")


def timed(fn, launches=10):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def facade(n, seed=0):
    rng = np.random.RandomState(seed)
    p = np.stack([rng.rand(n) * 12.0, 0.01 * rng.randn(n), rng.rand(n) * 8.0], axis=1)
    ledge = (np.floor(p[:, 2]) % 3 == 2)
    p[ledge, 1] += 0.25
    return p.astype(np.float32)


def ball_bytes(xyz, radius):
    """lower bound of the walk's point traffic: per cell of a radius-sized grid, the points of its 27-cell neighbourhood are
    loaded once per wave of 64 queries that sit in it"""
    c = np.floor((xyz - xyz.min(axis=0)) / radius).astype(np.int64)
    dims = c.max(axis=0) + 3
    key = ((c[:, 0] + 1) * dims[1] + (c[:, 1] + 1)) * dims[2] + (c[:, 2] + 1)
    occ = np.bincount(key, minlength=int(dims.prod()))
    grid = occ.reshape(dims)
    around = np.zeros_like(grid)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                around += np.roll(grid, (dx, dy, dz), axis=(0, 1, 2))
    waves = (grid + 63) // 64
    return int((waves * around).sum()) * 16 + len(xyz) * (16 + 20)


def report(name, ms, host_s, host_note, nbytes, rows):
    med, lo, hi = ms
    print("%-7s %9.3f ms per call (min %.3f max %.3f)  %7.1f M rows/s  host statement %.2f s%s  alg bytes %.1f MB = %.3f of the "
          "time at %.0f GB/s" % (name, med, lo, hi, rows / med / 1e3, host_s, host_note, nbytes / 1e6,
                                 nbytes / 1e9 / HBM_GBS / (med / 1e3), HBM_GBS))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
B, N, K, R = 16, 8192, 64, 0.1
batch = synth.s3dis_batch(0, B, N)[0][:, :, 0:3].astype(np.float32).copy()
pts = torch.from_numpy(batch).to(dev)
idx, cnt, _ = tf_nnquery.build_sphere_neighbor(pts, pts, R, None, K)
toward_b = torch.tensor([[0.0, 0.0, 10.0]] * B, device=dev)
edges = int(torch.clamp(cnt, 0, K).sum())
graph_bytes = 4 * B * N * K + 12 * edges + 12 * B * N + 20 * B * N

fac = facade(400000)
_full, _label, room, _vl = scenesynth.synthetic_scene(0, 4000000, extent=(9.0, 7.0, 3.0), voxel=0.0155)
room = np.ascontiguousarray(room, dtype=np.float32)
print("graph: %d x %d rows, K = %d, %d edges (%.1f per row); facade: %d rows; room: %d rows" % (B, N, K, edges, edges / (B * N), len(fac),
                                                                                           len(room)))
clouds = {"facade": (fac, torch.from_numpy(fac).to(dev)), "room": (room, torch.from_numpy(room).to(dev))}
toward = torch.tensor([0.0, -5.0, 1.5], device=dev)

# ---- host ----------------------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
ref = nrm.graph_normals_reference(batch, batch, idx.cpu().numpy(), cnt.cpu().numpy(), R, toward_b.cpu().numpy(), 3)
host = {"graph": (time.perf_counter() - t0, "")}
for name, (xyz, _d) in clouds.items():
    rows = np.random.RandomState(1).choice(len(xyz), SUB, replace=False)
    t0 = time.perf_counter()
    m = nrm.ball_moments_reference(xyz, R, rows=rows)
    nrm.normals_from_moments_reference(m, xyz[rows], toward.cpu().numpy(), 3)
    host[name] = ((time.perf_counter() - t0) * len(xyz) / SUB, " (from %d queries, x %.0f)" % (SUB, len(xyz) / SUB))
    got = tf_surface.ball_normals(_d, R, toward, 3, want_moments=True)
    assert np.array_equal(got[3][torch.from_numpy(rows).to(dev)].cpu().numpy(), m), name
    print("%s: moments of the %d sampled rows equal the statement's; neighbours per row: mean %.1f max %d; rows without a normal %.4f"
          % (name, SUB, float(got[2].float().mean()), int(got[2].max()), float((got[0] == 0).all(dim=1).float().mean())))
got = tf_surface.graph_normals(pts, pts, idx, cnt, R, toward_b, 3, want_moments=True)
assert np.array_equal(got[3].cpu().numpy(), ref.moments) and int(got[4][0]) == ref.skipped

# ---- device: every arm twice, in turn ------------------------------------------------------------------------------------------
for turn in (1, 2):
    print("turn %d" % turn)
    report("graph", timed(lambda: tf_surface.graph_normals(pts, pts, idx, cnt, R, toward_b, 3)), *host["graph"], graph_bytes, B * N)
    for name, (xyz, d) in clouds.items():
        report(name, timed(lambda: tf_surface.ball_normals(d, R, toward, 3)), *host[name], ball_bytes(xyz, R), len(xyz))
