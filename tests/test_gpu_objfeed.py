"""csrc/objfeed.hip on the device against harness/objfeed.py's numpy statement: index and label bit for bit, a mask of 0 copies xyz
bit for bit, every other mask within the project's floating-point bound of the float64 evaluation; refusal of bad ids,
determinism, the two output sets of ObjectFeed, and a ShapeNet training step that consumes the feed through `points_ready`.
Every launch here is an ordinary one."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import feed, objfeed

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 500, 2047, 2048, 2049, 3000, 4097]
NUM_PARTS = 6


def _shapes(seed=0, sizes=SIZES):
    """shape_blocks rows: xyz in the unit cube around the origin (the datasets' normalisation), part labels 0..5"""
    rng = np.random.RandomState(seed)
    return [objfeed.shape_blocks((rng.rand(n, 3) * 2.0 - 1.0).astype(np.float32), rng.randint(0, NUM_PARTS, n)) for n in sizes]


@pytest.fixture(scope="module")
def pool(dev):
    shapes = _shapes()
    category = np.arange(len(SIZES), dtype=np.int32) % 4
    return shapes, objfeed.ShapePool(shapes, category, device=dev)


def _batch(B, seed):
    """-> (shape ids [B], recipe [B]): B = 32 has one cloud per mask value 0..31 over shapes on both sides of N; B = 7 the masks
    the two training recipes and the evaluation use, and 0"""
    rng = np.random.RandomState(seed)
    ids = np.concatenate([rng.permutation(len(SIZES)) for _ in range(3)])[:B].astype(np.int32)
    if B == 32:
        return ids, rng.permutation(32).astype(np.int32)
    return ids, np.array([31, 28, 0, objfeed.EVAL_AUGMENT, 15, 16, 4], dtype=np.int32)[:B]


def _bound(src, mask):
    """1e-5 * (1.25 (|x| + |y| + |z|) of the source row + 0.1 if SHIFT + 0.02 if JITTER): the project's bound with the recipe's
    constants (1.25 the largest scale, 0.1 the largest shift, 0.02 the noise's clip)"""
    extra = (objfeed.SHIFT_RANGE if mask & objfeed.SHIFT else 0.0) + (objfeed.JITTER_CLIP if mask & objfeed.JITTER else 0.0)
    return 1e-5 * (1.25 * np.abs(src.astype(np.float64)).sum(axis=1, keepdims=True) + extra)


@pytest.mark.parametrize("B", [32, 7])
@pytest.mark.parametrize("N", [64, 2048])
def test_kernel_equals_the_numpy_statement(pool, dev, B, N):
    """index / label bit-equal; mask-0 xyz bit-equal; otherwise per element |err| <= 1e-5 * (1.25 (|x| + |y| + |z|) of the source
    row + 0.1 if SHIFT + 0.02 if JITTER) against the float64 statement.
    Worst error / bound on the MI355X: not measured yet (the test prints it per case)."""
    import torch
    shapes, p = pool
    worst = 0.0
    for seed, step in ((1, 0), (2, 12345678901), (0xfedcba9876543210, (1 << 33) + 3)):
        ids, recipe = _batch(B, seed & 0xffff)
        n = p.sizes[ids]
        assert (n >= N).any() and (n < N).any()
        ref = objfeed.assemble_reference(p.sizes, ids, N, seed, step, recipe)
        want_pts, want_label = objfeed.apply_reference(shapes, ids, ref)
        pts, label, index = objfeed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, recipe, want_index=True)
        torch.cuda.synchronize()
        pts, label, index = pts.cpu().numpy(), label.cpu().numpy(), index.cpu().numpy()
        assert pts.shape == (B, N, 3) and np.array_equal(index, ref.index) and np.array_equal(label, want_label)
        assert np.array_equal(index, feed.assemble_reference(p.sizes, ids, N, seed, step, False).index)
        for b in range(B):
            src = shapes[ids[b]][ref.index[b], 0:3]
            mask = int(recipe[b])
            if mask == 0:
                assert np.array_equal(pts[b].view(np.int32), src.view(np.int32))
                continue
            bound = _bound(src, mask)
            err = np.abs(pts[b].astype(np.float64) - want_pts[b])
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (b, mask, float((err / bound).max()))
            assert not np.array_equal(pts[b], src)
    print("B=%d N=%d: worst error / bound %.4f" % (B, N, worst))


def test_the_sample_does_not_depend_on_the_recipe(pool, dev):
    """the evaluation's two draws: recipe 0 and EVAL_AUGMENT with the same (seed, step) take the same rows; a device recipe and
    a single mask for all clouds are accepted; masks outside [0, 31] are refused on the host"""
    import torch
    _shapes_, p = pool
    ids = torch.from_numpy(_batch(7, 3)[0]).to(dev)
    a = objfeed.assemble(p.rows, p.offsets, ids, 256, 1 << 40, 1 << 35, 0, want_index=True)
    b = objfeed.assemble(p.rows, p.offsets, ids, 256, 1 << 40, 1 << 35, objfeed.EVAL_AUGMENT, want_index=True)
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], b[0])
    rows = p.rows[(p.offsets[ids.long()].reshape(-1, 1) + a[2].long())]                                  # [B, N, 8]
    assert torch.equal(a[0].view(torch.int32), rows[:, :, 0:3].contiguous().view(torch.int32)) and torch.equal(a[1], rows[:, :, 6].int())
    c = objfeed.assemble(p.rows, p.offsets, ids, 256, 1 << 40, 1 << 35, torch.full((7,), objfeed.EVAL_AUGMENT, dtype=torch.int32, device=dev))
    assert torch.equal(c[0].view(torch.int32), b[0].view(torch.int32)) and len(c) == 2
    for bad in (32, -1, [0, 1, 2, 3, 4, 5, 99]):
        with pytest.raises(ValueError):
            objfeed.assemble(p.rows, p.offsets, ids, 256, 1, 1, bad)


def test_shape_ids_outside_the_pool_read_nothing(pool, dev):
    """the kernel checks a shape id and its offsets against the pool before it forms an address: index -1, zeros"""
    import torch
    _shapes_, p = pool
    ids = torch.tensor([0, -1, len(SIZES), 3], dtype=torch.int32, device=dev)
    pts, label, index = objfeed.assemble(p.rows, p.offsets, ids, 300, 1, 1, 31, want_index=True)
    assert (index[1] == -1).all() and (index[2] == -1).all() and not pts[1:3].any() and not label[1:3].any()
    assert (index[0] == 0).all() and (index[3] >= 0).all() and (index[3] < 64).all()
    # offsets that do not describe rows of the pool: a negative size, and a range past the last row
    off = p.offsets.clone()
    off[4] = off[3] - 1
    off[-1] = p.rows.shape[0] + 1
    ids = torch.tensor([3, 10, 5], dtype=torch.int32, device=dev)
    pts, label, index = objfeed.assemble(p.rows, off, ids, 300, 1, 1, 31, want_index=True)
    assert (index[0] == -1).all() and (index[1] == -1).all() and not pts[0:2].any() and (index[2] >= 0).all()


def test_same_arguments_give_identical_bytes(pool, dev):
    import torch
    _shapes_, p = pool
    ids, recipe = _batch(32, 8)
    ids = torch.from_numpy(ids).to(dev)
    a = objfeed.assemble(p.rows, p.offsets, ids, 2048, (1 << 50) + 42, (1 << 34) + 7, recipe, want_index=True)
    b = objfeed.assemble(p.rows, p.offsets, ids, 2048, (1 << 50) + 42, (1 << 34) + 7, recipe, want_index=True)
    c = objfeed.assemble(p.rows, p.offsets, ids, 2048, (1 << 50) + 42, (1 << 34) + 8, recipe, want_index=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(a[2], c[2])


def test_object_feed_epochs_match_their_plan_and_alternate_two_sets(pool, dev):
    """every item equals the statement of its planned (step, shape ids) under train_recipe of its size; two consecutive items
    never share storage; item i+2 reuses item i's; the last batch is the short one; the second epoch continues the steps"""
    import torch
    shapes, p = pool
    N, B, seed = 64, 4, (1 << 36) + 6
    f = objfeed.ObjectFeed(p, B, N, seed=seed, dataset="shapenet")
    assert f.stream != torch.cuda.current_stream()
    for epoch in range(2):
        plan = feed.epoch_plan(len(p), B, seed, epoch)
        assert len(f) == len(plan) == 3 and [len(i) for _, i in plan] == [4, 4, 3]
        prev, seen = None, []
        for k, (pts, label, category, ready) in enumerate(f):
            step, ids = plan[k]
            assert step == epoch * 3 + k
            assert pts.shape == (len(ids), N, 3) and label.shape == (len(ids), N) and category.shape == (len(ids),)
            if prev is not None:            # both live: no aliasing
                lo, hi = pts.data_ptr(), pts.data_ptr() + pts.numel() * 4
                assert hi <= prev[0].data_ptr() or lo >= prev[0].data_ptr() + prev[0].numel() * 4
                assert label.data_ptr() != prev[1].data_ptr() and category.data_ptr() != prev[2].data_ptr()
            torch.cuda.current_stream().wait_event(ready)
            recipe = objfeed.train_recipe(len(ids), "shapenet")
            ref = objfeed.assemble_reference(p.sizes, ids, N, seed, step, recipe)
            want_pts, want_label = objfeed.apply_reference(shapes, ids, ref)
            got = pts.cpu().numpy()
            assert np.array_equal(label.cpu().numpy(), want_label) and np.array_equal(category.cpu().numpy(), p.category[ids])
            for b in range(len(ids)):
                src = shapes[ids[b]][ref.index[b], 0:3]
                if recipe[b] == 0:
                    assert np.array_equal(got[b].view(np.int32), src.view(np.int32))
                else:
                    assert (np.abs(got[b].astype(np.float64) - want_pts[b]) <= _bound(src, int(recipe[b]))).all()
            want = objfeed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, recipe)
            assert torch.equal(pts.view(torch.int32), want[0].view(torch.int32)) and torch.equal(label, want[1])
            seen.append(pts.data_ptr())
            prev = (pts, label, category)
            if k % 2 == 0:
                f.done(ready)                # (items 1: no event handed back — the feed waits for the consuming stream instead)
        assert seen[0] == seen[2] and seen[0] != seen[1]
    assert f.epoch == 2
    m = objfeed.ObjectFeed(p, B, N, seed=seed, dataset="modelnet")
    pts, label, category, ready = next(iter(m))
    torch.cuda.current_stream().wait_event(ready)
    step, ids = feed.epoch_plan(len(p), B, seed, 0)[0]
    want = objfeed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, objfeed.train_recipe(B, "modelnet"))
    assert torch.equal(pts.view(torch.int32), want[0].view(torch.int32))


def test_a_shapenet_training_step_consumes_the_feed_through_points_ready(dev):
    """one reduced-plan SPH3DShapeNet training step (forward, backward) on an ObjectFeed item handed over as `points_ready`,
    issued without a host synchronisation: the loss and every gradient are finite, and the item is the batch of its plan entry"""
    import torch
    from sph3d_gcn_amd.harness import shapenet_net, synth
    N, B, seed, parts = 512, 3, 21, 4
    rng = np.random.RandomState(2)
    shapes = [objfeed.shape_blocks(synth.modelnet_cloud(40 + k, n), rng.randint(0, parts, n)) for k, n in enumerate((700, 512, 400, 1500))]
    p = objfeed.ShapePool(shapes, [0, 0, 1, 1], device=dev)
    model = shapenet_net.SPH3DShapeNet(parts, shapenet_net.small_config(N), device=dev, seed=3)
    f = objfeed.ObjectFeed(p, B, N, seed=seed, dataset="shapenet")
    pts, label, category, ready = next(iter(f))
    pred, _ = model(pts, is_training=True, points_ready=ready)
    torch.cuda.current_stream().wait_event(ready)          # (the loss reads label on the main stream)
    loss = model.loss(pred, label)
    f.done(ready)
    loss.backward()
    fed = loss.detach().clone()
    torch.cuda.synchronize()
    assert pred.shape == (B, N, parts) and np.isfinite(float(fed))
    grads = [q.grad for q in model.parameters() if q.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    step, ids = feed.epoch_plan(len(p), B, seed, 0)[0]
    pts2, label2 = objfeed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, objfeed.train_recipe(B, "shapenet"))
    torch.cuda.synchronize()
    assert torch.equal(pts2.view(torch.int32), pts.view(torch.int32)) and torch.equal(category.cpu(), torch.tensor(p.category[ids]))
    assert torch.equal(label2, label) and objfeed.train_recipe(B, "shapenet").tolist() == [31, 28, 0]
    print("loss %r" % float(fed))
