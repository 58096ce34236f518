"""csrc/cropfeed.hip on the device against harness/cropfeed.py's numpy statement: index, label, inner, the crop record and the
copied colours bit for bit, untouched xyz bit for bit, rotated and jittered xyz within the bound tests/test_gpu_feed.py holds
feed.assemble to; determinism; CropFeed's two output sets, its crop record and a second stage behind it; one training step fed by
it; and prepare_training_scenes against the host statement.  Every launch here is an ordinary one."""
import numpy as np
import pytest

import _cropfeed_cases as cases
from sph3d_gcn_amd.harness import cropfeed, feed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool(dev):
    p = cropfeed.ScenePool(cases.host_pool(), dev, keep_host=True)
    assert len(p) == 4 and p.sizes.tolist() == list(cases.SIZES) and p.rows.shape == (sum(cases.SIZES), 8)
    return p


def _ids(dev):
    import torch
    return torch.from_numpy(cases.SCENE_IDS).to(dev)


def test_the_case_table_reaches_every_branch():
    reached = set()
    for c in cases.all_cases():
        reached |= cases.branches(*c)
    assert reached == cases.ALL_BRANCHES


@pytest.mark.parametrize("augment", [True, False])
@pytest.mark.parametrize("halves", cases.HALVES)
@pytest.mark.parametrize("num_point", cases.N_POINTS)
def test_kernel_equals_the_numpy_statement(pool, dev, num_point, halves, augment):
    """index / label / inner / crop / colours / untouched xyz bit-equal; rotated and jittered xyz within 1e-5 of the magnitudes of
    the element's terms (|x| + |y| + |z| of the source row, + the 0.02 clip where noise is added) of the float64 evaluation —
    tests/test_gpu_feed.py's bound for feed.assemble, whose transform code the kernel shares.  Without the index output the
    other outputs are the same bits."""
    import torch
    g = cases.geometry_of(halves, num_point)
    worst = {1: 0.0, 2: 0.0}
    for draw in cases.DRAWS:
        ref, (want_pts, want_label, want_inner) = cases.reference(num_point, halves, draw, augment)
        pts, label, inner, index, crop = cropfeed.assemble(pool, _ids(dev), num_point, draw[0], draw[1], augment, want_index=True,
                                                           geometry=g)
        pts2, label2, inner2, crop2 = cropfeed.assemble(pool, _ids(dev), num_point, draw[0], draw[1], augment, geometry=g)
        torch.cuda.synchronize()
        for a, b in ((pts, pts2), (label, label2), (inner, inner2), (crop, crop2)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        pts, label, inner, index, crop = (t.cpu().numpy() for t in (pts, label, inner, index, crop))
        assert np.array_equal(crop, ref.crop)
        assert np.array_equal(index, ref.index)
        assert np.array_equal(label, want_label) and np.array_equal(inner, want_inner)
        assert np.array_equal(pts[:, :, 3:6].view(np.int32), want_pts[:, :, 3:6].astype(np.float32).view(np.int32))
        assert ref.kind.tolist() == ([1, 1, 2, 2, 0, 0, 0] if augment else [0] * 7)
        for b in range(cases.B):
            src = pool.host[int(cases.SCENE_IDS[b])].rows[ref.index[b], 0:3]
            if ref.kind[b] == 0:
                assert np.array_equal(pts[b, :, 0:3].view(np.int32), src.view(np.int32))
                continue
            bound = 1e-5 * (np.abs(src.astype(np.float64)).sum(axis=1, keepdims=True) + (feed.JITTER_CLIP if ref.kind[b] == 2 else 0.0))
            err = np.abs(pts[b, :, 0:3].astype(np.float64) - want_pts[b, :, 0:3])
            worst[int(ref.kind[b])] = max(worst[int(ref.kind[b])], float((err / bound).max()))
            assert (err <= bound).all(), (b, float((err / bound).max()))
            if ref.kind[b] == 2:
                assert np.abs(pts[b, :, 0:3] - src).max() <= feed.JITTER_CLIP + 2.4e-7        # (half an ulp of a coordinate below 4)
    print("N=%d halves=%s: worst error / bound: rotated %.4f, jittered %.4f" % (num_point, halves, worst[1], worst[2]))


def test_default_geometry_is_the_15_21_window_and_outputs_can_be_given(pool, dev):
    import torch
    draw = cases.DRAWS[0]
    ref, _ = cases.reference(256, (15, 21), draw, True)
    out = (torch.empty((7, 256, 6), device=dev), torch.empty((7, 256), dtype=torch.int32, device=dev),
           torch.empty((7, 256), dtype=torch.int32, device=dev), torch.empty((7, 4), dtype=torch.int32, device=dev))
    got = cropfeed.assemble(pool, _ids(dev), 256, draw[0], draw[1], True, out=out, want_index=True)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip((got[0], got[1], got[2], got[4]), out))
    assert np.array_equal(got[3].cpu().numpy(), ref.index) and np.array_equal(got[4].cpu().numpy(), ref.crop)
    with pytest.raises(ValueError):
        cropfeed.assemble(pool, _ids(dev), 256, 1, 1, out=out[:3] + (torch.empty((7, 3), dtype=torch.int32, device=dev),))


def test_scene_ids_outside_the_pool_read_nothing(pool, dev):
    """the kernel checks a scene id against the pool before it forms an address: zeros, index -1, crop -1"""
    import torch
    ids = torch.tensor([0, -1, 4, 3, 1 << 30], dtype=torch.int32, device=dev)
    pts, label, inner, index, crop = cropfeed.assemble(pool, ids, 300, 1, 1, True, want_index=True,
                                                       geometry=cropfeed.Geometry(15, 21, 4, 300))
    for b in (1, 2, 4):
        assert (index[b] == -1).all() and not pts[b].any() and not label[b].any() and not inner[b].any() and (crop[b] == -1).all()
    want = cropfeed.crop_reference(pool.host, [0, 0, 0, 3, 0], 300, 1, 1, True, cropfeed.Geometry(15, 21, 4, 300))
    for b in (0, 3):
        assert np.array_equal(index[b].cpu().numpy(), want.index[b]) and np.array_equal(crop[b].cpu().numpy(), want.crop[b])


def test_entry_refusals(pool, dev):
    import torch
    ids = _ids(dev)
    for g in ((2, 128, 4, 1), (3, 2, 4, 1), (1, 2, 0, 1), (1, 2, 9, 1), (1, 2, 4, 0)):
        with pytest.raises(ValueError):
            cropfeed.assemble(pool, ids, 64, 1, 1, geometry=cropfeed.Geometry(*g))
    from sph3d_gcn_amd import _lib
    l, p = _lib.lib(), _lib.ptr
    out = [torch.empty((7, 64, 6), device=dev)] + [torch.empty((7, 64), dtype=torch.int32, device=dev) for _ in range(3)]
    crop = torch.empty((7, 4), dtype=torch.int32, device=dev)

    def call(B=7, N=64, rows=p(pool.rows), column=p(pool.column), points=p(out[0]), crop_=p(crop), oh=21, attempts=4):
        return l.sph3d_cropfeed_assemble(B, N, 4, int(pool.rows.shape[0]), int(pool.col_start.shape[0]), rows, column, p(pool.col_start),
                                         p(pool.scene_tab), p(ids), 1, 1, 1, 15, oh, attempts, 64, points, p(out[1]), p(out[2]),
                                         p(out[3]), crop_, _lib.stream_ptr())
    assert call() == 0
    for kw, text in ((dict(rows=None), "null input"), (dict(crop_=None), "null output"), (dict(rows=p(pool.rows) + 4), "aligned"),
                     (dict(points=p(out[0]) + 4), "aligned"), (dict(column=p(pool.column) + 2), "aligned"),
                     (dict(B=65535, N=65535), "too large"), (dict(oh=128), "outer_half"), (dict(attempts=0), "attempts"),
                     (dict(attempts=9), "attempts")):
        assert call(**kw) == -1
        assert text in l.sph3d_last_error().decode()
    torch.cuda.synchronize()


def test_same_arguments_give_identical_bits(pool, dev):
    import torch
    g = cases.geometry_of((15, 21), 1024)
    a = cropfeed.assemble(pool, _ids(dev), 1024, 42, 7, True, want_index=True, geometry=g)
    b = cropfeed.assemble(pool, _ids(dev), 1024, 42, 7, True, want_index=True, geometry=g)
    c = cropfeed.assemble(pool, _ids(dev), 1024, 42, 8, True, want_index=True, geometry=g)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(a[3], c[3]) and not torch.equal(a[4], c[4])


def test_crop_feed_epoch_matches_its_plan_alternates_two_sets_and_keeps_the_crop_record(pool, dev):
    """every item equals assemble() of its planned (step, scene ids) and crop_of(ready) the statement's record; two consecutive
    items never share storage, item i + 2 reuses item i's; the last batch is the short one; done(ready) is taken; the second
    epoch continues the step numbers"""
    import torch
    N, bs, seed, E = 256, 4, 6, 10
    f = cropfeed.CropFeed(pool, bs, N, seed=seed, crops_per_epoch=E)
    assert f.stream != torch.cuda.current_stream() and f.geometry == cropfeed.Geometry(15, 21, 4, N)
    assert cropfeed.CropFeed(pool, bs, N, seed=seed).crops_per_epoch == cropfeed.default_crops_per_epoch(sum(cases.SIZES), N) == 14
    for epoch in range(2):
        plan = cropfeed.epoch_scenes(pool.sizes, E, bs, seed, epoch)
        assert len(f) == len(plan) == 3 and [len(i) for _, i in plan] == [4, 4, 2]
        prev, seen = None, []
        for k, (pts, label, inner, ready) in enumerate(f):
            step, ids = plan[k]
            assert step == epoch * 3 + k
            assert pts.shape == (len(ids), N, 6) and label.shape == inner.shape == (len(ids), N)
            if prev is not None:            # both live: no aliasing
                lo, hi = pts.data_ptr(), pts.data_ptr() + pts.numel() * 4
                assert hi <= prev[0].data_ptr() or lo >= prev[0].data_ptr() + prev[0].numel() * 4
                assert label.data_ptr() != prev[1].data_ptr() and inner.data_ptr() != prev[2].data_ptr()
            torch.cuda.current_stream().wait_event(ready)
            want = cropfeed.assemble(pool, torch.from_numpy(ids).to(dev), N, seed, step, True, geometry=f.geometry)
            for g, w in zip((pts, label, inner, f.crop_of(ready)), want):
                assert torch.equal(g.view(torch.int32), w.view(torch.int32))
            ref = cropfeed.crop_reference(pool.host, ids, N, seed, step, True, f.geometry)
            assert np.array_equal(f.crop_of(ready).cpu().numpy(), ref.crop)
            seen.append(pts.data_ptr())
            prev = (pts, label, inner)
            if k % 2 == 0:
                f.done(ready)                # (item 1: no event handed back — the feed waits for the consuming stream instead)
        assert seen[0] == seen[2] and seen[0] != seen[1]
    assert f.epoch == 2
    with pytest.raises(ValueError):
        f.crop_of(torch.cuda.Event())


def test_an_augmentation_stage_runs_behind_the_crop_feed(pool, dev):
    """post=augment.Stage(...): an item equals augment.apply on assemble()'s batch for the same (seed, step)"""
    import torch
    from sph3d_gcn_amd.harness import augment
    N, bs, seed, E = 256, 4, 9, 6
    opts = augment.default_options("s3dis")
    f = cropfeed.CropFeed(pool, bs, N, seed=seed, crops_per_epoch=E, post=augment.Stage(opts, bs, N, 6, dev))
    plan = cropfeed.epoch_scenes(pool.sizes, E, bs, seed, 0)
    changed = False
    for (pts, label, inner, ready), (step, ids) in zip(f, plan):
        torch.cuda.current_stream().wait_event(ready)
        base = cropfeed.assemble(pool, torch.from_numpy(ids).to(dev), N, seed, step, True, geometry=f.geometry)
        changed = changed or not torch.equal(pts, base[0])
        want = augment.apply(base[0].clone(), base[1].clone(), base[2].clone(), seed, step, opts)
        for g, w in zip((pts, label, inner), want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
        f.done(ready)
    assert changed


def test_one_training_step_fed_by_a_crop_feed(dev):
    """one Trainer.train_step on the reduced S3DIS plan, fed by a CropFeed over two synthetic rooms: a finite loss, rows counted"""
    import torch
    from sph3d_gcn_amd.harness import optim, s3dis_net, scenesynth, train
    N, bs, seed = 1024, 3, 21
    scenes = []
    for s in range(2):
        _fx, _fl, vx, vl = scenesynth.synthetic_scene(40 + s, 30000, extent=(3.0, 2.4, 2.0), voxel=0.05)
        scenes.append((vx, np.random.RandomState(s).rand(len(vx), 3).astype(np.float32), vl))
    p = cropfeed.ScenePool.from_arrays(scenes, dev)
    f = cropfeed.CropFeed(p, bs, N, seed=seed, crops_per_epoch=bs)
    prime = cropfeed.assemble(p, torch.zeros((bs,), dtype=torch.int32, device=dev), N, seed, 0)[:3]
    model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(N), device=dev, seed=3)
    tr = train.Trainer(model, model.loss, lambda q: optim.FlatTFAdam(q, lr=1e-3, eps=1e-4), train.Schedule(1e-3, bs), 13,
                       prime=prime, seed=seed, log=lambda s: None)
    before = tr.flat.flat_param.detach().clone()
    items = 0
    for item in f:
        assert int(f.crop_of(item[-1])[:, 3].min()) >= N             # rooms this dense fill every crop
        tr.train_step(item, f)
        items += 1
    r = tr.metrics.read()
    assert items == 1 and tr.global_step == 1 and r.batches == 1 and np.isfinite(r.mean_loss) and r.nonfinite == 0
    assert 0 < r.seen <= bs * N and r.update_nonfinite == 0
    assert torch.isfinite(tr.flat.flat_param).all() and not torch.equal(before, tr.flat.flat_param)


def test_prepare_training_scenes_equals_the_host_statement(dev):
    """one small synthetic room: voxel_reference -> the nearest full point's label -> normalise_reference -> column_sort_reference"""
    from sph3d_gcn_amd.harness import scenemerge, scenesynth, sceneprep
    fx, fl, _vx, _vl = scenesynth.synthetic_scene(33, 8000, extent=(2.4, 1.6, 2.0))
    rgb = (np.random.RandomState(2).rand(len(fx), 3) * 255).astype(np.float32)
    voxel, _count, _vop, _dropped = sceneprep.voxel_reference(fx, rgb, 0.05)
    vx = np.ascontiguousarray(voxel[:, 0:3])
    near = scenemerge.nearest_reference(fx, vx)
    vl = np.where(near >= 0, fl[np.maximum(near, 0)], -1).astype(np.int32)
    nx, nrgb, _c = sceneprep.normalise_reference(vx, voxel[:, 3:6])
    want = cropfeed.sort_scene(nx, nrgb, vl, 0.05)
    got = sceneprep.prepare_training_scenes([(fx, rgb, fl)], h=0.05, cell=0.05, device=dev, keep_host=True)
    assert len(got) == 1 and got.sizes.tolist() == [len(vx)] and (np.diff(want.column) >= 0).all()
    assert np.array_equal(got.rows.cpu().numpy().view(np.int32), want.rows.view(np.int32))
    assert np.array_equal(got.column.cpu().numpy(), want.column) and np.array_equal(got.index.cpu().numpy(), want.index)
    assert np.array_equal(got.col_start.cpu().numpy(), want.col_start)
    assert got.scene_tab.cpu().numpy().tolist() == [[0, 0, want.n_x, want.n_y, len(vx)]]
    assert np.array_equal(got.host[0].rows.view(np.int32), want.rows.view(np.int32))
