"""csrc/feed.hip on the device against harness/feed.py's numpy statement: integer outputs and everything copied bit for bit,
computed coordinates within the project's floating-point bound of the float64 evaluation; determinism, the two output sets of
DeviceFeed, and a training step that consumes the feed through `points_ready`.  Every launch here is an ordinary one."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import feed

pytestmark = pytest.mark.gpu

SIZES = [8192, 8193, 16384, 16385, 30000, 1024, 1025, 1023, 8191, 500, 64, 1, 2, 12000, 6000, 20000, 4096, 4097, 9000, 700] * 2 + [100000, 3]


def _blocks(seed=0, sizes=SIZES, extent=(2.1, 2.1, 3.0)):
    """blockio.parse_block-shaped blocks: xyz in an S3DIS-like slab, rgb in [0, 1], label 0..12, inner 0/1"""
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        b = np.empty((n, 8), dtype=np.float32)
        b[:, 0:3] = rng.rand(n, 3) * np.array(extent)
        b[:, 3:6] = rng.rand(n, 3)
        b[:, 6] = rng.randint(0, 13, n)
        b[:, 7] = rng.randint(0, 2, n)
        out.append(b)
    return out


@pytest.fixture(scope="module")
def pool(dev):
    blocks = _blocks()
    assert len(blocks) >= 40
    return blocks, feed.BlockPool.from_blocks(blocks, dev)


def _ids(B, seed):
    """block ids of a batch: a random draw from the pool that has blocks on both sides of N at every third of the batch"""
    return np.random.RandomState(seed).permutation(len(SIZES))[:B].astype(np.int32)


@pytest.mark.parametrize("B", [16, 7])
@pytest.mark.parametrize("N", [8192, 1024])
def test_kernel_equals_the_numpy_statement(pool, dev, B, N):
    """index / label / inner / colours / untouched xyz bit-equal; rotated and jittered xyz within 1e-5 of the magnitudes of the
    element's terms (|x| + |y| + |z| of the source row, + the 0.02 clip where noise is added) of the float64 evaluation.
    Worst error / bound measured on the MI355X over the four cases: rotated 0.027, jittered 0.0057."""
    import torch
    blocks, p = pool
    worst = {1: 0.0, 2: 0.0}
    for seed, step in ((1, 0), (2, 12345678901), (0xfedcba9876543210, 3)):
        ids = _ids(B, seed & 0xffff)
        n = p.sizes[ids]
        assert (n >= N).any() and (n < N).any()
        ref = feed.assemble_reference(p.sizes, ids, N, seed, step, True)
        want_pts, want_label, want_inner = feed.apply_reference(blocks, ids, ref)
        pts, label, inner, index = feed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, True, want_index=True)
        torch.cuda.synchronize()
        pts, label, inner, index = pts.cpu().numpy(), label.cpu().numpy(), inner.cpu().numpy(), index.cpu().numpy()
        assert np.array_equal(index, ref.index)
        assert np.array_equal(label, want_label) and np.array_equal(inner, want_inner)
        assert np.array_equal(pts[:, :, 3:6].view(np.int32), want_pts[:, :, 3:6].astype(np.float32).view(np.int32))
        assert ref.kind.tolist() == [1] * (B // 3) + [2] * (B // 3) + [0] * (B - 2 * (B // 3))
        for b in range(B):
            src = blocks[ids[b]][ref.index[b], 0:3]
            if ref.kind[b] == 0:
                assert np.array_equal(pts[b, :, 0:3].view(np.int32), src.view(np.int32))
                continue
            bound = 1e-5 * (np.abs(src.astype(np.float64)).sum(axis=1, keepdims=True) + (feed.JITTER_CLIP if ref.kind[b] == 2 else 0.0))
            err = np.abs(pts[b, :, 0:3].astype(np.float64) - want_pts[b, :, 0:3])
            worst[int(ref.kind[b])] = max(worst[int(ref.kind[b])], float((err / bound).max()))
            assert (err <= bound).all(), (b, float((err / bound).max()))
            if ref.kind[b] == 2:
                assert np.abs(pts[b, :, 0:3] - src).max() <= feed.JITTER_CLIP + 2.4e-7        # (half an ulp of a coordinate below 4)
    print("B=%d N=%d: worst error / bound: rotated %.4f, jittered %.4f" % (B, N, worst[1], worst[2]))


def test_without_augmentation_the_batch_is_the_gathered_rows(pool, dev):
    import torch
    blocks, p = pool
    ids = _ids(16, 5)
    pts, label, inner, index = feed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), 2048, 9, 4, False, want_index=True)
    rows = p.rows[(p.offsets[torch.from_numpy(ids).long().to(dev)].reshape(-1, 1) + index.long())]          # [B, N, 8]
    assert torch.equal(pts.view(torch.int32), rows[:, :, 0:6].contiguous().view(torch.int32))
    assert torch.equal(label, rows[:, :, 6].int()) and torch.equal(inner, rows[:, :, 7].int())
    ref = feed.assemble_reference(p.sizes, ids, 2048, 9, 4, False)
    assert np.array_equal(index.cpu().numpy(), ref.index)
    # and without the index output
    pts2, label2, inner2 = feed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), 2048, 9, 4, False)
    assert torch.equal(pts2.view(torch.int32), pts.view(torch.int32)) and torch.equal(label2, label) and torch.equal(inner2, inner)


def test_block_ids_outside_the_pool_read_nothing(pool, dev):
    """the kernel checks a block id and its offsets against the pool before it forms an address: index -1, zeros"""
    import torch
    _blocks_, p = pool
    ids = torch.tensor([0, -1, len(SIZES), 3], dtype=torch.int32, device=dev)
    pts, label, inner, index = feed.assemble(p.rows, p.offsets, ids, 256, 1, 1, True, want_index=True)
    assert (index[1] == -1).all() and (index[2] == -1).all() and not pts[1:3].any() and not label[1:3].any()
    assert (index[0] >= 0).all() and (index[3] >= 0).all()


def test_same_seed_and_step_give_identical_bytes(pool, dev):
    import torch
    _blocks_, p = pool
    ids = torch.from_numpy(_ids(16, 8)).to(dev)
    a = feed.assemble(p.rows, p.offsets, ids, 8192, 42, 7, True, want_index=True)
    b = feed.assemble(p.rows, p.offsets, ids, 8192, 42, 7, True, want_index=True)
    c = feed.assemble(p.rows, p.offsets, ids, 8192, 42, 8, True, want_index=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(a[3], c[3])


def test_both_assemble_kernels_share_the_pool_lookup_and_the_sample(dev):
    """feed.hip and objfeed.hip take a cloud's rows and a slot's row from the same helpers (csrc/feed_draws.hpp): on one pool,
    without augmentation, index, label and xyz of the two are the same bytes.  Blocks of 1 and 40 rows are sampled with
    replacement, 64 is n == N, and 64 / 65 / 257 / 1025 put the Feistel width on both sides of a power of two, odd and even;
    an id of -1 reads nothing in both."""
    import torch
    from sph3d_gcn_amd.harness import objfeed
    rng = np.random.RandomState(11)
    blocks = [objfeed.shape_blocks(rng.rand(n, 3).astype(np.float32), rng.randint(0, 13, n)) for n in (1, 40, 64, 65, 257, 1025)]
    p = feed.BlockPool.from_blocks(blocks, dev)
    N, seed, step = 64, 0x1234567890abcdef, 77
    for ids in ([0, 1, 2, 3, 4, 5], [5, -1, 3, 2, 1, 0]):
        ids_dev = torch.tensor(ids, dtype=torch.int32, device=dev)
        pts, label, inner, index = feed.assemble(p.rows, p.offsets, ids_dev, N, seed, step, augment=False, want_index=True)
        opts, olabel, oindex = objfeed.assemble(p.rows, p.offsets, ids_dev, N, seed, step, 0, want_index=True)
        assert torch.equal(index, oindex) and torch.equal(label, olabel)
        assert torch.equal(pts[..., :3].contiguous().view(torch.int32), opts.view(torch.int32))
        want = feed.assemble_reference(p.sizes, [i for i in ids if i >= 0], N, seed, step, False).index
        for b, i in enumerate(ids):
            if i < 0:
                assert (index[b] == -1).all() and (oindex[b] == -1).all() and not pts[b].any() and not opts[b].any()
            else:
                assert (index[b] >= 0).all() and (index[b] < len(blocks[i])).all() and bool(inner[b].all())
        if -1 not in ids:
            assert np.array_equal(index.cpu().numpy(), want)


def test_device_feed_epoch_matches_its_plan_and_alternates_two_sets(pool, dev):
    """every item equals assemble() of its planned (step, block ids); two consecutive items never share storage; item i+2 reuses
    item i's; the last batch is the short one; the second epoch has another order and continues the step numbers"""
    import torch
    blocks, p = pool
    f = feed.DeviceFeed(p, 16, 1024, seed=6, augment=True)
    assert f.stream != torch.cuda.current_stream()
    for epoch in range(2):
        plan = feed.epoch_plan(len(p), 16, 6, epoch)
        assert len(f) == len(plan) == 3 and [len(i) for _, i in plan] == [16, 16, len(SIZES) - 32]
        prev, seen = None, []
        for k, (pts, label, inner, ready) in enumerate(f):
            step, ids = plan[k]
            assert pts.shape == (len(ids), 1024, 6) and label.shape == inner.shape == (len(ids), 1024)
            if prev is not None:            # both live: no aliasing
                lo, hi = pts.data_ptr(), pts.data_ptr() + pts.numel() * 4
                assert hi <= prev[0].data_ptr() or lo >= prev[0].data_ptr() + prev[0].numel() * 4
                assert label.data_ptr() != prev[1].data_ptr() and inner.data_ptr() != prev[2].data_ptr()
            torch.cuda.current_stream().wait_event(ready)
            want = feed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), 1024, 6, step, True)
            for g, w in zip((pts, label, inner), want):
                assert torch.equal(g.view(torch.int32), w.view(torch.int32))
            seen.append(pts.data_ptr())
            prev = (pts, label, inner)
            if k % 2 == 0:
                f.done(ready)                # (items 1: no event handed back — the feed waits for the consuming stream instead)
        assert seen[0] == seen[2] and seen[0] != seen[1]
    assert f.epoch == 2


def test_training_steps_consume_the_feed_through_points_ready(dev):
    """three reduced-plan training steps (forward, backward, Adam) fed by DeviceFeed through `points_ready`, issued without a
    host synchronisation in between; each step's loss equals, bit for bit, the loss of the same parameters on a synchronised
    clone of the same batch (assembled again from its plan entry: the forward pass is order-fixed), and is finite"""
    import torch
    from sph3d_gcn_amd.harness import s3dis_net, synth
    from sph3d_gcn_amd.harness import optim as hoptim
    from sph3d_gcn_amd.harness import dist as hdist
    N, seed = 1024, 21
    blocks = _blocks(3, [1500, 1024, 900, 2000, 3000, 1100, 5000, 1300, 700, 2500, 1800, 1024], extent=(1.0, 1.0, 1.5))
    p = feed.BlockPool.from_blocks(blocks, dev)
    model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(N), device=dev, seed=3)
    # the variables are created by the first forward: one pass on a synthetic batch, then the flat buffers and Adam
    xyz, label0, inner0 = synth.s3dis_batch(0, 4, N, extent=(1.0, 1.0, 1.5))
    prime = torch.from_numpy(np.concatenate([xyz, np.zeros_like(xyz)], axis=2)).to(dev)
    model.loss(model(prime, is_training=True)[0], torch.from_numpy(label0).to(dev), torch.from_numpy(inner0).to(dev)).backward()
    flat = hdist.FlatGradAllReduce(model.parameters())
    opt = hoptim.FlatAdam(flat.flat_param, lr=1e-3, eps=1e-4)
    torch.cuda.synchronize()

    plan = feed.epoch_plan(len(p), 4, seed, 0)
    params_before, fed = [], []
    for pts, label, inner, ready in feed.DeviceFeed(p, 4, N, seed=seed, augment=True):
        params_before.append(flat.flat_param.detach().clone())
        pred, _ = model(pts, is_training=True, points_ready=ready)
        loss = model.loss(pred, label, inner)
        flat.backward(loss)
        flat.all_reduce()
        opt.step()
        fed.append(loss.detach())
    torch.cuda.synchronize()
    fed = [float(l) for l in fed]
    assert len(fed) == len(plan) == 3 and all(np.isfinite(fed))
    assert not torch.equal(params_before[0], params_before[2])            # the steps did step

    final = flat.flat_param.detach().clone()
    want = []
    for (step, ids), before in zip(plan, params_before):
        pts, label, inner = feed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, True)
        pts, label, inner = pts.clone(), label.clone(), inner.clone()
        with torch.no_grad():
            flat.flat_param.copy_(before)
        torch.cuda.synchronize()                                           # resident, nothing in flight
        with torch.no_grad():
            want.append(float(model.loss(model(pts, is_training=True)[0], label, inner)))
    with torch.no_grad():
        flat.flat_param.copy_(final)
    print("losses fed: %s resident: %s" % (fed, want))
    assert fed == want
