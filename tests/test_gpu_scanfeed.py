"""csrc/scanfeed.hip on the device against harness/scannet.py's numpy statement: index, label, inner and rgb bit for bit in every
view and equal to feed.assemble(augment=False); a mask of 0 copies the previous view bit for bit; a one-view launch equals
objfeed.assemble bit for bit; every view within the project's floating-point bound of the float64 transform of the kernel's own
previous view, and the chain within three times that of the float64 chain; refusals; and ScanNetFeed's epochs.
Every launch here is an ordinary one."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import feed, objfeed, scannet

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 63, 64, 65, 300, 1000, 257]          # N in {1, 64, 257}: with and without replacement, and n == N
TOL = 1e-5                                           # the project's bound, rtol = atol


def _blocks(seed=0, sizes=SIZES, rgb=True):
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        blk = np.zeros((n, 8), dtype=np.float32)
        blk[:, 0:3] = rng.rand(n, 3) * 2.0 - 0.5
        if rgb:
            blk[:, 3:6] = rng.rand(n, 3)
        blk[:, 6], blk[:, 7] = rng.randint(0, 21, n), rng.rand(n) < 0.6
        out.append(blk)
    return out


@pytest.fixture(scope="module")
def pool(dev):
    blocks = _blocks()
    return blocks, feed.BlockPool(blocks, dev)


def _batch(B, V, seed):
    """-> (block ids [B], recipes [V, B]): random masks with a zero in every view where B allows it"""
    rng = np.random.RandomState(seed)
    ids = np.concatenate([rng.permutation(len(SIZES)) for _ in range(2)])[:B].astype(np.int32)
    recipes = rng.randint(1, 32, (V, B)).astype(np.int32)
    for v in range(V):
        if B > 1:
            recipes[v, (v + seed) % B] = 0
    return ids, recipes


def _within(got, want, factor=1.0):
    err = np.abs(got.astype(np.float64) - want)
    bound = factor * (TOL + TOL * np.abs(want))
    assert (err <= bound).all(), float((err / bound).max())
    return float((err / bound).max())


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("B", [1, 3, 7])
@pytest.mark.parametrize("N", [1, 64, 257])
def test_kernel_equals_the_numpy_statement(pool, dev, N, B, V):
    """index / label / inner / rgb bit-equal; a mask-0 view bit-equal to the view before it; otherwise per element
    |err| <= 1e-5 + 1e-5 |want| against the float64 transform of the kernel's own previous view, and 3 x that against the float64
    chain from the pool row.  Worst error / bound on the MI355X over the 18 cases: 0.074 per view, 0.029 of the 3 x bound over the
    chain (N = 257, B = 7, three views); the test prints it per case."""
    import torch
    blocks, p = pool
    worst = chain = 0.0
    for seed, step in ((1, 0), (0xfedcba9876543210, (1 << 33) + 3)):
        ids, recipes = _batch(B, V, (seed + N + B) & 0xffff)
        ids_dev = torch.from_numpy(ids).to(dev)
        ref = scannet.assemble_reference(p.sizes, ids, N, seed, step, recipes)
        pts, label, inner, index = scannet.assemble(p.rows, p.offsets, ids_dev, N, seed, step, recipes, want_index=True)
        plain = feed.assemble(p.rows, p.offsets, ids_dev, N, seed, step, augment=False, want_index=True)
        torch.cuda.synchronize()
        assert pts.shape == (V, B, N, 6)
        for got, same in zip((label, inner, index), plain[1:]):
            assert torch.equal(got, same)
        pts, label, inner, index = pts.cpu().numpy(), label.cpu().numpy(), inner.cpu().numpy(), index.cpu().numpy()
        want_chain, want_label, want_inner = scannet.apply_reference(blocks, ids, ref)
        want_step, _l, _i = scannet.apply_reference(blocks, ids, ref, base=pts)
        assert np.array_equal(index, ref.index) and np.array_equal(label, want_label) and np.array_equal(inner, want_inner)
        for b in range(B):
            src = blocks[ids[b]][ref.index[b]]
            prev = src[:, 0:3]
            for v in range(V):
                assert np.array_equal(pts[v, b, :, 3:6].view(np.int32), src[:, 3:6].view(np.int32))           # rgb, every view
                if recipes[v, b] == 0:
                    assert np.array_equal(pts[v, b, :, 0:3].view(np.int32), prev.view(np.int32)), (v, b)
                else:
                    worst = max(worst, _within(pts[v, b, :, 0:3], want_step[v, b, :, 0:3]))
                    assert not np.array_equal(pts[v, b, :, 0:3], prev)
                chain = max(chain, _within(pts[v, b, :, 0:3], want_chain[v, b, :, 0:3], 3.0))
                prev = pts[v, b, :, 0:3]
    print("N=%d B=%d V=%d: worst error / bound %.4f per view, %.4f of 3x over the chain" % (N, B, V, worst, chain))


def test_every_mask_as_a_single_view(pool, dev):
    """B = 32: one cloud per mask 0..31, as a one-view launch with a 1-D recipe, over blocks on both sides of N = 64"""
    import torch
    blocks, p = pool
    N, seed, step = 64, 77, 1 << 21
    ids = (np.arange(32) % len(SIZES)).astype(np.int32)
    recipe = np.arange(32, dtype=np.int32)
    ref = scannet.assemble_reference(p.sizes, ids, N, seed, step, recipe)
    pts, label, inner = scannet.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, recipe)
    torch.cuda.synchronize()
    assert pts.shape == (32, N, 6)                                        # a 1-D recipe means one view
    want, want_label, want_inner = scannet.apply_reference(blocks, ids, ref)
    pts = pts.cpu().numpy()
    assert np.array_equal(label.cpu().numpy(), want_label) and np.array_equal(inner.cpu().numpy(), want_inner)
    assert np.array_equal(pts[0].view(np.int32), blocks[ids[0]][ref.index[0], 0:6].view(np.int32))
    worst = max(_within(pts[b, :, 0:3], want[0, b, :, 0:3]) for b in range(1, 32))
    for b in range(1, 32):
        assert not np.array_equal(pts[b, :, 0:3], blocks[ids[b]][ref.index[b], 0:3])
    print("masks 1..31: worst error / bound %.4f" % worst)


def test_all_zero_recipes_copy_the_pool_rows_into_every_view(pool, dev):
    import torch
    blocks, p = pool
    ids = np.array([6, 0, 3, 7, 2], dtype=np.int32)
    pts, label, inner, index = scannet.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), 257, 5, 9,
                                                np.zeros((4, 5), np.int32), want_index=True)
    torch.cuda.synchronize()
    pts, index = pts.cpu().numpy(), index.cpu().numpy()
    assert pts.shape == (4, 5, 257, 6)
    for b in range(5):
        src = blocks[ids[b]][index[b]]
        for v in range(4):
            assert np.array_equal(pts[v, b].view(np.int32), src[:, 0:6].view(np.int32))
        assert np.array_equal(label[b].cpu().numpy(), src[:, 6].astype(np.int32)) and np.array_equal(inner[b].cpu().numpy(), src[:, 7].astype(np.int32))


def test_one_view_equals_objfeed_bit_for_bit(dev):
    """on a pool whose rgb columns are zero (what objfeed's shapes are) the one-view launch writes objfeed.assemble's xyz: the draws
    are the same; and view 0 of a three-view launch is that launch too"""
    import torch
    blocks = _blocks(seed=4, rgb=False)
    for blk in blocks:
        blk[:, 7] = 1
    p = feed.BlockPool(blocks, dev)
    for N in (64, 257):
        ids, recipes = _batch(7, 3, N)
        recipes[0] = [31, 30, 0, 1, 2, 28, 16]
        ids_dev = torch.from_numpy(ids).to(dev)
        seed, step = (1 << 50) + 42, (1 << 34) + 7
        one = scannet.assemble(p.rows, p.offsets, ids_dev, N, seed, step, recipes[0], want_index=True)
        three = scannet.assemble(p.rows, p.offsets, ids_dev, N, seed, step, recipes)
        obj = objfeed.assemble(p.rows, p.offsets, ids_dev, N, seed, step, recipes[0], want_index=True)
        torch.cuda.synchronize()
        assert torch.equal(one[0][:, :, 0:3].contiguous().view(torch.int32), obj[0].view(torch.int32))
        assert not one[0][:, :, 3:6].any() and torch.equal(one[1], obj[1]) and torch.equal(one[3], obj[2])
        assert torch.equal(three[0][0].view(torch.int32), one[0].view(torch.int32))
        again = scannet.assemble(p.rows, p.offsets, ids_dev, N, seed, step, torch.from_numpy(recipes).to(dev))      # a device recipe
        assert torch.equal(again[0].view(torch.int32), three[0].view(torch.int32)) and len(again) == 3


def test_block_ids_outside_the_pool_read_nothing(pool, dev):
    """the kernel checks a block id and its offsets against the pool before it forms an address: zeros in every view, index -1"""
    import torch
    _blocks_, p = pool
    ids = torch.tensor([0, -1, len(SIZES), 5], dtype=torch.int32, device=dev)
    recipes = scannet.eval_recipes(scannet.EVAL_VIEWS, 4)
    pts, label, inner, index = scannet.assemble(p.rows, p.offsets, ids, 300, 1, 1, recipes, want_index=True)
    assert (index[1] == -1).all() and (index[2] == -1).all() and not pts[:, 1:3].any()
    assert not label[1:3].any() and not inner[1:3].any()
    assert (index[0] == 0).all() and (index[3] >= 0).all() and (index[3] < 300).all() and pts[:, 3].any()
    off = p.offsets.clone()
    off[4] = off[3] - 1                                                    # a negative size, and a range past the last row
    off[-1] = p.rows.shape[0] + 1
    ids = torch.tensor([3, 7, 5], dtype=torch.int32, device=dev)
    pts, label, inner, index = scannet.assemble(p.rows, off, ids, 300, 1, 1, recipes[:, :3].copy(), want_index=True)
    assert (index[0] == -1).all() and (index[1] == -1).all() and not pts[:, 0:2].any() and (index[2] >= 0).all()
    # without an index the other outputs are the same
    a = scannet.assemble(p.rows, p.offsets, ids, 300, 1, 1, recipes[:, :3].copy())
    b = scannet.assemble(p.rows, p.offsets, ids, 300, 1, 1, recipes[:, :3].copy(), want_index=True)
    assert len(a) == 3 and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b[:3]))


def test_the_entry_refuses_bad_requests(pool, dev):
    import torch
    from sph3d_gcn_amd import _lib
    _blocks_, p = pool
    B, N = 2, 64
    ids = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    recipe = torch.zeros((4, B), dtype=torch.int32, device=dev)
    pts = torch.zeros((4, B, N, 6), device=dev)
    lab = torch.zeros((B, N), dtype=torch.int32, device=dev)
    call = lambda views, rec: _lib.lib().sph3d_blockfeed_assemble(
        B, N, len(p), int(p.rows.shape[0]), _lib.ptr(p.rows), _lib.ptr(p.offsets), _lib.ptr(ids), 1, 1, views, rec, _lib.ptr(pts),
        _lib.ptr(lab), _lib.ptr(lab), None, _lib.stream_ptr())
    assert call(0, _lib.ptr(recipe)) == -1 and b"views" in _lib.lib().sph3d_last_error()
    assert call(5, _lib.ptr(recipe)) == -1 and b"views" in _lib.lib().sph3d_last_error()
    assert call(3, None) == -1 and b"null input" in _lib.lib().sph3d_last_error()
    assert call(4, _lib.ptr(recipe)) == 0
    torch.cuda.synchronize()
    for bad in ([[0, 32]], np.zeros((5, 2), np.int32)):
        with pytest.raises(ValueError):
            scannet.assemble(p.rows, p.offsets, ids, N, 1, 1, bad)
    with pytest.raises(ValueError):
        scannet.assemble(p.rows, p.offsets, ids, N, 1, 1, np.zeros((3, 2), np.int32), out=(pts, lab, lab))     # four views' storage


def test_scannet_feed_epochs_reproduce_direct_assembly(pool, dev):
    """two epochs on the feed's own stream with done(ready) handed back: every item equals scannet.assemble at its planned
    (step, block ids) under train_recipe of its size; augment=False gives masks 0"""
    import torch
    _blocks_, p = pool
    N, B, seed = 64, 3, (1 << 36) + 6
    f = scannet.ScanNetFeed(p, B, N, seed=seed)
    assert f.stream != torch.cuda.current_stream() and f.recipe(7).tolist() == scannet.train_recipe(7).tolist()
    for epoch in range(2):
        plan = feed.epoch_plan(len(p), B, seed, epoch)
        assert len(f) == len(plan) == 3 and [len(i) for _, i in plan] == [3, 3, 2]
        for k, (pts, label, inner, ready) in enumerate(f):
            step, ids = plan[k]
            assert step == epoch * 3 + k and pts.shape == (len(ids), N, 6)
            torch.cuda.current_stream().wait_event(ready)
            want = scannet.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, scannet.train_recipe(len(ids)))
            assert torch.equal(pts.view(torch.int32), want[0].view(torch.int32))
            assert torch.equal(label, want[1]) and torch.equal(inner, want[2])
            f.done(ready)
    assert f.epoch == 2
    plain = scannet.ScanNetFeed(p, B, N, seed=seed, augment=False)
    pts, label, inner, ready = next(iter(plain))
    torch.cuda.current_stream().wait_event(ready)
    step, ids = feed.epoch_plan(len(p), B, seed, 0)[0]
    want = feed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, augment=False)
    assert torch.equal(pts.view(torch.int32), want[0].view(torch.int32)) and torch.equal(label, want[1])


def test_rank_shares_are_disjoint_and_give_the_one_rank_epoch(pool, dev):
    import torch
    _blocks_, p = pool
    N, B, seed = 64, 3, 12

    def epoch(rank, world):
        out = []
        f = scannet.ScanNetFeed(p, B, N, seed=seed, rank=rank, world=world)
        for pts, label, inner, ready in f:
            torch.cuda.current_stream().wait_event(ready)
            out.append((pts.clone(), label.clone(), inner.clone()))
            f.done(ready)
        return out
    one, r0, r1 = epoch(0, 1), epoch(0, 2), epoch(1, 2)
    assert len(one) == 3 and len(r0) == 2 and len(r1) == 1
    for got, want in zip((r0[0], r1[0], r0[1]), one):
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(got, want))
    assert not torch.equal(one[0][0], one[1][0])
