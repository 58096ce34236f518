"""csrc/scene.hip and harness/scenemerge.py on the device against the numpy statement: merged probabilities as bit patterns,
hits, predictions, counters, confusion matrices and nearest-neighbour indices all EQUAL, no tolerance.  Every launch here is an
ordinary one; out-of-range requests are refused by the entries' own checks and tested through status codes."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import evalvote, feed, scenemerge as sm, scenesynth

pytestmark = pytest.mark.gpu

SIZES = [1500, 1, 2, 3, 30000, 900, 12000, 20000, 64, 2500, 8192, 700, 5000, 1023, 16000, 4096]


class _Toy:
    """a cheap deterministic "network": a fixed [6, C] matrix on the points (the same function in every call)"""

    def __init__(self, C, dev, seed=0):
        import torch
        self.w = torch.from_numpy(np.random.RandomState(seed).randn(6, C).astype(np.float32)).to(dev)

    def __call__(self, points, label, inner):
        return (points.unsqueeze(-1) * self.w).sum(dim=2)


class _Recorder:
    def __init__(self):
        self.index, self.logits = {}, {}

    def __call__(self, batch_index, p, index, logits):
        assert p == len(self.index.setdefault(batch_index, []))
        self.index[batch_index].append(index.cpu().numpy())
        self.logits.setdefault(batch_index, []).append(logits.cpu().numpy())

    def replay(self, i, p, index):
        assert np.array_equal(index, self.index[i][p])
        return self.logits[i][p]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("C", [13, 21])
@pytest.mark.parametrize("b", [16, 7])
def test_merge_and_finalize_equal_the_statement_bit_for_bit(dev, C, b):
    """one batch of b blocks (1, 2, 3 .. 30 000 rows) voted by the toy network; the sums the voter leaves are merged into a scene
    of V rows by the kernels and, copied back, by merge_reference.  A block's rows point at distinct random scene rows below
    35 000 of V = 36 000, so scene rows are hit 0, 1 and >= 4 times; some sums are overwritten with zeros, non-finite and
    overflowing values (skipped rows), and a second scene of 30 000 rows cuts indices off (out_of_scene)."""
    import torch
    from sph3d_gcn_amd import _lib
    N, seed, V = 1024, 3, 36000
    sizes = SIZES[:b]
    rng = np.random.RandomState(C + b)
    blocks, index = [], []
    for n in sizes:
        blk = np.empty((n, 8), dtype=np.float32)
        blk[:, 0:3], blk[:, 3:6] = rng.rand(n, 3) * 2.0, rng.rand(n, 3)
        blk[:, 6], blk[:, 7] = rng.randint(0, C, n), rng.rand(n) < 0.7
        blocks.append(blk)
        index.append(rng.permutation(34000)[:n].astype(np.int32) + (0 if n < 30000 else 1000))
    blocks[0][5:9, 7] = 1                                               # (the rows whose sums are overwritten below are inner)
    pool = feed.BlockPool(blocks, dev, index, [0] * b)
    voter = evalvote.Voter(pool, b, N, C, sum(sizes))
    ids = np.arange(b, dtype=np.int32)
    got = voter.run_batch(_Toy(C, dev), ids, seed, 0)
    assert got.complete
    base, nrows = voter.row_range(ids)
    assert (base, nrows) == (0, sum(sizes))
    voter.votes[5:9] = 0.0
    voter.votes[2000, 3] = float("nan")
    voter.votes[2001, 0] = float("inf")
    voter.votes[2002] = 3.0e19                                           # finite sums whose squares overflow
    host_votes = voter.votes[:nrows].cpu().numpy()
    off = pool.host_offsets
    want = sm.merge_reference([host_votes[off[k]:off[k + 1]] for k in range(b)], [blk[:, 7] for blk in blocks], index, V, C)
    assert want.hits.max() >= 4 and (want.hits == 0).any() and (want.hits == 1).any()
    assert want.skipped_rows > 0 and want.out_of_scene == 0
    voxel_label = rng.randint(-1, C + 1, V).astype(np.int32)
    l = _lib.lib()
    ids_dev = torch.from_numpy(ids).to(dev)
    for scene_rows in (V, 30000):
        merged = torch.zeros((scene_rows, C), dtype=torch.float32, device=dev)
        hits = torch.zeros((scene_rows,), dtype=torch.int32, device=dev)
        counters = torch.zeros((3,), dtype=torch.int64, device=dev)
        conf = torch.zeros((C * C,), dtype=torch.int64, device=dev)
        pred = torch.empty((scene_rows,), dtype=torch.int32, device=dev)
        label_dev = torch.from_numpy(voxel_label[:scene_rows].copy()).to(dev)
        _lib.check(l.sph3d_scene_merge(b, C, len(pool), int(pool.rows.shape[0]), _lib.ptr(pool.rows), _lib.ptr(pool.offsets),
                                       _lib.ptr(pool.index), _lib.ptr(ids_dev), base, nrows, _lib.ptr(voter.votes), scene_rows,
                                       _lib.ptr(merged), _lib.ptr(hits), _lib.ptr(counters), _lib.stream_ptr()))
        _lib.check(l.sph3d_scene_finalize(C, scene_rows, _lib.ptr(merged), _lib.ptr(hits), _lib.ptr(label_dev), _lib.ptr(pred),
                                          _lib.ptr(counters[2:]), _lib.ptr(conf), _lib.stream_ptr()))
        if scene_rows != V:
            want = sm.merge_reference([host_votes[off[k]:off[k + 1]] for k in range(b)], [blk[:, 7] for blk in blocks], index,
                                      scene_rows, C)
            assert want.out_of_scene > 0
        assert _same_bits(merged.cpu().numpy().view(np.int32), want.merged.view(np.int32))
        assert np.array_equal(hits.cpu().numpy(), want.hits) and np.array_equal(pred.cpu().numpy(), want.pred_voxel)
        assert counters.cpu().numpy().tolist() == [want.skipped_rows, want.out_of_scene, want.unseen_rows]
        assert np.array_equal(conf.cpu().numpy().reshape(C, C), sm.voxel_confusion(want.pred_voxel, voxel_label[:scene_rows], C))
    print("C=%d b=%d: hits up to %d, %d unseen, %d skipped" % (C, b, want.hits.max(), want.unseen_rows, want.skipped_rows))


def _both_modes(dev, ref, qry):
    import torch
    r, q = torch.from_numpy(np.ascontiguousarray(ref, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(qry, np.float32)).to(dev)
    return sm.nearest(r, q, sm.NN1_GRID).cpu().numpy(), sm.nearest(r, q, sm.NN1_BRUTE).cpu().numpy()


def _check_nn1(dev, ref, qry, name):
    want = sm.nearest_reference(ref, qry)
    grid, brute = _both_modes(dev, ref, qry)
    assert np.array_equal(brute, want), name + " (brute)"
    assert np.array_equal(grid, want), name + " (grid)"
    return want


def test_nn1_on_a_jittered_lattice(dev):
    """F = 1e5 queries against V = 3e4 points of a 3 cm lattice (a slab of 100 x 100 x 3 cells) jittered by up to 1 cm"""
    rng = np.random.RandomState(0)
    g = np.stack(np.meshgrid(np.arange(100), np.arange(100), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    ref = (g * 0.03 + (rng.rand(len(g), 3) - 0.5) * 0.02).astype(np.float32)[rng.permutation(len(g))]
    qry = (rng.rand(100000, 3) * np.array([3.0, 3.0, 0.09]) - 0.015).astype(np.float32)
    want = _check_nn1(dev, ref, qry, "lattice")
    assert want.min() >= 0 and len(np.unique(want)) > 25000


def test_nn1_ties_duplicates_flat_clouds_and_small_references(dev):
    rng = np.random.RandomState(1)
    # exact duplicates (every point three times, shuffled) and queries ON the points: the lowest of three indices must win
    base = (rng.rand(2000, 3) * 2).astype(np.float32)
    ref = np.concatenate([base, base, base])[rng.permutation(6000)]
    want = _check_nn1(dev, ref, base, "duplicates")
    first = {}
    for i, p in enumerate(map(bytes, ref)):
        first.setdefault(p, i)
    assert want.tolist() == [first[bytes(p)] for p in base]
    # constructed equidistant pairs: lattice points with integer coordinates, queries at the midpoints of its edges and cells
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    ref = g[rng.permutation(len(g))]
    qry = np.concatenate([g[:500] + np.float32(0.5) * np.eye(3, dtype=np.float32)[rng.randint(0, 3, 500)], g[:300] + np.float32(0.5)])
    _check_nn1(dev, ref, qry, "equidistant")
    # a flat cloud (zero z-extent), queries above and below it; a line; all points in one place
    flat = np.concatenate([rng.rand(5000, 2), np.full((5000, 1), 0.25)], axis=1).astype(np.float32)
    _check_nn1(dev, flat, (rng.rand(4000, 3) * 1.2 - 0.1).astype(np.float32), "flat")
    line = np.zeros((3000, 3), np.float32)
    line[:, 1] = rng.rand(3000)
    _check_nn1(dev, line, rng.rand(1000, 3).astype(np.float32), "line")
    _check_nn1(dev, np.ones((500, 3), np.float32), rng.rand(100, 3).astype(np.float32), "one place")
    for V in (1, 2, 63, 64, 65):
        _check_nn1(dev, rng.rand(V, 3).astype(np.float32), rng.rand(777, 3).astype(np.float32), "V=%d" % V)


def test_nn1_far_queries_and_non_finite_points(dev):
    rng = np.random.RandomState(2)
    ref = (rng.rand(20000, 3) * np.array([4.0, 3.0, 2.5])).astype(np.float32)
    far = (rng.randn(300, 3) * 50).astype(np.float32)
    far[:6] = [[1e4, 0, 0], [-1e4, 1, 1], [2, 3e5, 1], [0, 0, -7e3], [1e30, 1, 1], [-1e25, -1e25, 1e25]]
    near = (rng.rand(3000, 3) * np.array([4.4, 3.3, 2.8]) - 0.15).astype(np.float32)
    want = _check_nn1(dev, ref, np.concatenate([far, near]), "far")
    assert want[4] == -1 and want[5] == -1 and (want[6:] >= 0).all()        # d2 overflows: no candidate
    bad = ref.copy()
    bad[::50, 0] = np.nan
    bad[7::50, 1] = np.inf
    bad[9::50, 2] = -np.inf
    qry = near.copy()
    qry[::40, 2] = np.nan
    qry[3::40, 0] = np.inf
    want = _check_nn1(dev, bad, qry, "non-finite")
    finite_ref = np.isfinite(bad).all(axis=1)
    assert (want[::40] == -1).all() and (want[3::40] == -1).all() and finite_ref[want[want >= 0]].all()
    _check_nn1(dev, np.full((100, 3), np.nan, np.float32), near[:50], "no finite reference point")


def test_nn1_at_the_size_of_an_s3dis_room_grid_equals_brute(dev):
    """V = 3e5, F = 1e6 on a synthetic room.  The numpy statement would take hours here (3e11 distances), so the two device
    modes are compared with each other; each is compared with the statement at smaller sizes above."""
    full_xyz, _l, vx, _vl = scenesynth.synthetic_scene(7, 1000000, extent=(9.0, 7.0, 3.0), voxel=0.022)
    vx = vx[:300000]
    assert len(vx) == 300000
    grid, brute = _both_modes(dev, vx, full_xyz)
    assert grid.min() >= 0 and np.array_equal(grid, brute)
    for f in np.random.RandomState(0).permutation(len(full_xyz))[:100]:      # and a float64 spot check
        d = ((vx.astype(np.float64) - full_xyz[f].astype(np.float64)) ** 2).sum(axis=1)
        assert d[grid[f]] <= d.min() * (1 + 1e-5)


def test_entries_refuse_bad_requests_through_status_codes(dev):
    import torch
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    ref = torch.zeros((10, 3), device=dev)
    idx = torch.zeros((10,), dtype=torch.int32, device=dev)
    ws = torch.empty((l.sph3d_nn1_workspace(10, 10),), dtype=torch.uint8, device=dev)
    args = (_lib.ptr(ref), _lib.ptr(ref))
    assert l.sph3d_nn1(10, 10, *args, 0, _lib.ptr(idx), _lib.ptr(ws), ws.numel() - 1, _lib.stream_ptr()) == -1
    assert b"workspace" in l.sph3d_last_error()
    assert l.sph3d_nn1(10, 10, *args, 7, _lib.ptr(idx), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -1
    assert l.sph3d_nn1(10, 1 << 31, *args, 0, _lib.ptr(idx), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -1
    assert l.sph3d_nn1(10, 10, None, _lib.ptr(ref), 0, _lib.ptr(idx), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -1
    assert l.sph3d_scene_lift(13, 10, 10, _lib.ptr(idx), _lib.ptr(idx), None, _lib.ptr(idx), _lib.ptr(idx), None, _lib.stream_ptr()) == -1
    assert b"come together" in l.sph3d_last_error()
    assert l.sph3d_scene_finalize(13, 10, _lib.ptr(ref), _lib.ptr(idx), _lib.ptr(idx), _lib.ptr(idx), _lib.ptr(ws), None,
                                  _lib.stream_ptr()) == -1
    with pytest.raises(ValueError):
        sm.evaluate_scenes(None, feed.BlockPool([np.zeros((4, 8), np.float32)], dev), [sm.Scene(np.zeros((4, 3)))], 2, 16, 0)
    torch.cuda.synchronize()


def _scenes(C, counts=(60000, 3000, 20000)):
    """three synthetic scenes with differing block counts (the second a single block, the third without a full cloud), cut with
    the reference's geometry -> pool pieces and Scene objects"""
    blocks, index, sob, scenes = [], [], [], []
    for s, n in enumerate(counts):
        ext = [(3.0, 2.4, 2.0), (1.2, 1.2, 1.0), (2.4, 1.4, 2.0)][s]
        full_xyz, full_label, vx, vl = scenesynth.synthetic_scene(20 + s, n, extent=ext, num_cls=C)
        rgb = np.random.RandomState(s).rand(len(vx), 3).astype(np.float32)
        blk, idx = scenesynth.split_scene(vx, vl, rgb)
        blocks += blk
        index += idx
        sob += [s] * len(blk)
        scenes.append(sm.Scene(vx, vl, None if s == 2 else full_xyz, None if s == 2 else full_label))
    return blocks, index, sob, scenes


def _compare(got, want):
    assert got.scenes == want.scenes and got.complete == want.complete
    assert got.unseen_rows == want.unseen_rows and got.skipped_rows == want.skipped_rows and got.out_of_scene == want.out_of_scene
    assert np.array_equal(got.confusion_full, want.confusion_full) and np.array_equal(got.confusion_voxel, want.confusion_voxel)
    assert np.array_equal(got.block.confusion, want.block.confusion) and got.block.passes == want.block.passes
    assert got.block.batches == want.block.batches and got.block.nonfinite_rows == want.block.nonfinite_rows
    assert got.full.miou == want.full.miou and got.voxel.miou == want.voxel.miou and got.full.overall_acc == want.full.overall_acc
    for s in want.scenes:
        for key in ("merged", "hits", "pred_voxel", "pred_full", "idx"):
            a, b = got.pred[s][key], want.pred[s][key]
            assert (a is None and b is None) or _same_bits(a, b), (s, key)


def _replay(rec, blocks, index, sob, scenes, bs, N, seed, C, **kw):
    rows = np.concatenate(blocks)
    return sm.evaluate_scenes_reference(rec.replay, [len(b) for b in blocks], rows[:, 6], rows[:, 7], np.concatenate(index), sob,
                                        scenes, bs, N, seed, C, keep_pred=True, **kw)


def test_evaluate_scenes_with_the_toy_network(dev):
    C, N, seed, bs = 13, 1024, 9, 4
    blocks, index, sob, scenes = _scenes(C)
    per_scene = np.bincount(sob)
    assert per_scene[1] == 1 and len(set(per_scene.tolist())) == 3 and (per_scene % bs != 0).any()
    pool = feed.BlockPool(blocks, dev, index, sob)
    label_map = np.arange(C, dtype=np.int32)[::-1] * 3 + 1

    def run(rank=0, world=1, rec=None, label_map=None):
        return sm.evaluate_scenes(_Toy(C, dev), pool, scenes, bs, N, seed, C, rank=rank, world=world, keep_pred=True, on_pass=rec,
                                  label_map=label_map)
    rec = _Recorder()
    a = run(rec=rec)
    assert a.scenes == [0, 1, 2] and all(a.complete) and sum(a.unseen_rows) == 0 and sum(a.out_of_scene) == 0
    assert a.confusion_full.sum() == len(scenes[0].full_xyz) + len(scenes[1].full_xyz)
    assert a.confusion_voxel.sum() == sum(len(s.voxel_xyz) for s in scenes)
    assert a.pred[2]["idx"] is None and a.pred[2]["pred_full"] is None
    assert max(int(a.pred[s]["hits"].max()) for s in a.scenes) >= 4
    _compare(a, _replay(rec, blocks, index, sob, scenes, bs, N, seed, C))
    print("toy: full mIoU %.4f voxel mIoU %.4f block mIoU %.4f" % (a.full.miou, a.voxel.miou, a.block.miou))
    _compare(run(), a)                                                       # identical bytes across two runs
    _compare(sm.SceneResult.merge([run(1, 2), run(0, 2)]), a)                # world = 1 equals merged world = 2
    rec2 = _Recorder()
    m = run(rec=rec2, label_map=label_map)
    _compare(m, _replay(rec2, blocks, index, sob, scenes, bs, N, seed, C, label_map=label_map))
    assert np.array_equal(m.confusion_full, a.confusion_full)
    for s in (0, 1):
        assert np.array_equal(m.pred[s]["pred_full"], label_map[a.pred[s]["pred_full"]])


def test_evaluate_scenes_with_the_real_network(dev):
    """SPH3DS3DIS (reduced plan) in inference mode on the three scenes: every pass's logits replayed through the statement"""
    import torch
    from sph3d_gcn_amd.harness import s3dis_net
    C, N, seed, bs = 13, 1024, 21, 4
    blocks, index, sob, scenes = _scenes(C)
    pool = feed.BlockPool(blocks, dev, index, sob)
    model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(N), device=dev, seed=3)
    rec = _Recorder()
    res = sm.evaluate_scenes(lambda p, l, i: model(p, is_training=False)[0], pool, scenes, bs, N, seed, C, keep_pred=True, on_pass=rec)
    torch.cuda.synchronize()
    print("real net: passes %s full mIoU %.4f overall %.4f" % (res.block.passes, res.full.miou, res.full.overall_acc))
    assert all(res.complete) and res.block.nonfinite_rows == 0 and sum(res.skipped_rows) == 0
    for v in [res.full.miou, res.full.overall_acc, res.voxel.miou] + list(res.full.class_iou):
        assert np.isfinite(v) and 0.0 <= v <= 1.0
    _compare(res, _replay(rec, blocks, index, sob, scenes, bs, N, seed, C))
