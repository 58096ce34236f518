"""csrc/facadefeed.hip on the device against harness/facadefeed.py's numpy statement: index and label bit for bit, rgb always and
every untouched channel copied bit for bit, rotated xyz and normals within the floating-point bound of the float64 evaluation;
refusal of bad ids and misaligned normals, determinism, and the two output sets of FacadeFeed over an epoch that visits every
facade `repeat` times.  Every launch here is an ordinary one."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import facadefeed, feed
from test_gpu_objfeed import _bound

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 500, 2047, 2048, 2049, 3000, 4097]
ROT = facadefeed.TURN | facadefeed.TILT


def _facades(seed=0, sizes=SIZES):
    """facade_blocks pairs: xyz in a facade-like slab (xy about the origin, z from 0), unit normals, rgb in [-1, 1], 7 labels"""
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        normal = rng.randn(n, 3)
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        xyz = (rng.rand(n, 3) - [0.5, 0.5, 0.0]) * [2.0, 1.0, 1.5]
        out.append(facadefeed.facade_blocks(xyz.astype(np.float32), normal.astype(np.float32),
                                            (rng.rand(n, 3) * 2 - 1).astype(np.float32), rng.randint(0, 7, n)))
    return [o[0] for o in out], [o[1] for o in out]


@pytest.fixture(scope="module")
def pool(dev):
    blocks, normals = _facades()
    return blocks, normals, facadefeed.FacadePool(blocks, normals, device=dev)


def _batch(B, seed):
    """-> (ids [B], recipe [B]): B = 32 has one cloud per mask value 0..31 over facades on both sides of N; B = 7 the masks of
    the training recipe and the evaluation, and others"""
    rng = np.random.RandomState(seed)
    ids = np.concatenate([rng.permutation(len(SIZES)) for _ in range(3)])[:B].astype(np.int32)
    if B == 32:
        return ids, rng.permutation(32).astype(np.int32)
    return ids, np.array([31, 28, 0, 3, 15, 16, 4], dtype=np.int32)[:B]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("B", [32, 7])
@pytest.mark.parametrize("N", [64, 2048])
def test_kernel_equals_the_numpy_statement(pool, dev, B, N):
    """index / label bit-equal; rgb the source's bit patterns always; mask 0 copies all nine channels and a mask without TURN and
    TILT the normal, bit for bit; otherwise xyz within test_gpu_objfeed._bound of the float64 statement and the normal within
    1e-5 * (|nx| + |ny| + |nz|) of the source row (two rotations of at most five roundings each with entries of magnitude at
    most 1: about 1e-6 of that sum; the bound leaves ten times that).
    Worst error / bound on the MI355X (the test prints it per case): xyz 0.030, normal 0.037 (B = 32, N = 2048)."""
    import torch
    blocks, normals, p = pool
    worst_xyz = worst_n = 0.0
    for seed, step in ((1, 0), (2, 12345678901), (0xfedcba9876543210, (1 << 33) + 3)):
        ids, recipe = _batch(B, seed & 0xffff)
        n = p.sizes[ids]
        assert (n >= N).any() and (n < N).any()
        ref = facadefeed.assemble_reference(p.sizes, ids, N, seed, step, recipe)
        want_pts, want_label = facadefeed.apply_reference(blocks, normals, ids, ref)
        pts, label, index = facadefeed.assemble(p.rows, p.normals, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, recipe,
                                                want_index=True)
        torch.cuda.synchronize()
        pts, label, index = pts.cpu().numpy(), label.cpu().numpy(), index.cpu().numpy()
        assert pts.shape == (B, N, 9) and np.array_equal(index, ref.index) and np.array_equal(label, want_label)
        assert np.array_equal(index, feed.assemble_reference(p.sizes, ids, N, seed, step, False).index)
        for b in range(B):
            src = blocks[ids[b]][ref.index[b]]
            nrm = normals[ids[b]][ref.index[b], 0:3]
            mask = int(recipe[b])
            assert np.array_equal(_bits(pts[b, :, 6:9]), _bits(src[:, 3:6]))
            if mask & ROT:
                bound = 1e-5 * np.abs(nrm.astype(np.float64)).sum(axis=1, keepdims=True)
                err = np.abs(pts[b, :, 3:6].astype(np.float64) - want_pts[b, :, 3:6])
                worst_n = max(worst_n, float((err / bound).max()))
                assert (err <= bound).all(), (b, mask, float((err / bound).max()))
                assert not np.array_equal(pts[b, :, 3:6], nrm)
            else:
                assert np.array_equal(_bits(pts[b, :, 3:6]), _bits(nrm))
            if mask == 0:
                assert np.array_equal(_bits(pts[b, :, 0:3]), _bits(src[:, 0:3]))
                continue
            bound = _bound(src[:, 0:3], mask)
            err = np.abs(pts[b, :, 0:3].astype(np.float64) - want_pts[b, :, 0:3])
            worst_xyz = max(worst_xyz, float((err / bound).max()))
            assert (err <= bound).all(), (b, mask, float((err / bound).max()))
            assert not np.array_equal(pts[b, :, 0:3], src[:, 0:3])
    print("B=%d N=%d: worst error / bound xyz %.4f normal %.4f" % (B, N, worst_xyz, worst_n))


def test_device_recipe_equals_host_recipe_and_bad_masks_are_refused(pool, dev):
    """recipe 0 and EVAL_AUGMENT with the same (seed, step) take the same rows; a device recipe and a single mask for all clouds
    are accepted; masks outside [0, 31] are refused on the host"""
    import torch
    _b, _n, p = pool
    ids = torch.from_numpy(_batch(7, 3)[0]).to(dev)
    args = (p.rows, p.normals, p.offsets, ids, 256, 1 << 40, 1 << 35)
    a = facadefeed.assemble(*args, 0, want_index=True)
    b = facadefeed.assemble(*args, facadefeed.EVAL_AUGMENT, want_index=True)
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]) and not torch.equal(a[0][:, :, 0:6], b[0][:, :, 0:6])
    at = (p.offsets[ids.long()].reshape(-1, 1) + a[2].long())
    rows, nrm = p.rows[at], p.normals[at]                                                                # [B, N, 8], [B, N, 4]
    plain = torch.cat((rows[:, :, 0:3], nrm[:, :, 0:3], rows[:, :, 3:6]), dim=2).contiguous()
    assert torch.equal(a[0].view(torch.int32), plain.view(torch.int32)) and torch.equal(a[1], rows[:, :, 6].int())
    assert torch.equal(b[0][:, :, 6:9].contiguous().view(torch.int32), plain[:, :, 6:9].contiguous().view(torch.int32))
    c = facadefeed.assemble(*args, torch.full((7,), facadefeed.EVAL_AUGMENT, dtype=torch.int32, device=dev))
    assert torch.equal(c[0].view(torch.int32), b[0].view(torch.int32)) and len(c) == 2
    host = np.array([31, 28, 0, 3, 15, 16, 4], dtype=np.int32)
    d = facadefeed.assemble(*args, host)
    e = facadefeed.assemble(*args, torch.from_numpy(host).to(dev))
    assert torch.equal(d[0].view(torch.int32), e[0].view(torch.int32)) and torch.equal(d[1], e[1])
    for bad in (32, -1, [0, 1, 2, 3, 4, 5, 99]):
        with pytest.raises(ValueError):
            facadefeed.assemble(*args, bad)


def test_ids_outside_the_pool_read_nothing(pool, dev):
    """the kernel checks an id and its offsets against the pool before it forms an address: index -1, zeros in all nine
    channels, label 0"""
    import torch
    _b, _n, p = pool
    ids = torch.tensor([0, -1, len(SIZES), 3], dtype=torch.int32, device=dev)
    pts, label, index = facadefeed.assemble(p.rows, p.normals, p.offsets, ids, 300, 1, 1, 31, want_index=True)
    assert (index[1] == -1).all() and (index[2] == -1).all() and not pts[1:3].any() and not label[1:3].any()
    assert (index[0] == 0).all() and (index[3] >= 0).all() and (index[3] < 64).all()
    # offsets that do not describe rows of the pool: a negative size, and a range past the last row
    off = p.offsets.clone()
    off[4] = off[3] - 1
    off[-1] = p.rows.shape[0] + 1
    ids = torch.tensor([3, 10, 5], dtype=torch.int32, device=dev)
    pts, label, index = facadefeed.assemble(p.rows, p.normals, off, ids, 300, 1, 1, 31, want_index=True)
    assert (index[0] == -1).all() and (index[1] == -1).all() and not pts[0:2].any() and not label[0:2].any()
    assert (index[2] >= 0).all() and pts[2].any()


def test_misaligned_normals_are_refused_by_the_entry(pool, dev):
    """a contiguous [T, 4] view that starts 4 bytes into an allocation passes the host's shape checks; the C entry refuses it
    before it launches"""
    import torch
    from sph3d_gcn_amd import _lib
    _b, _n, p = pool
    T = int(p.rows.shape[0])
    buf = torch.zeros((4 * T + 4,), dtype=torch.float32, device=dev)
    shifted = buf[1:1 + 4 * T].view(T, 4)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    ids = torch.tensor([5, 6], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError) as e:                   # (SPH3D_EINVAL, as the reference's errors::InvalidArgument)
        facadefeed.assemble(p.rows, shifted, p.offsets, ids, 64, 1, 1, 3)
    assert "normals must be 16-byte aligned" in str(e.value)
    assert b"normals must be 16-byte aligned" in _lib.lib().sph3d_last_error()
    with pytest.raises(ValueError) as e:
        facadefeed.assemble(p.rows, p.normals[:-1], p.offsets, ids, 64, 1, 1, 3)
    assert "[T, 4]" in str(e.value)


def test_same_arguments_give_identical_bytes(pool, dev):
    import torch
    _b, _n, p = pool
    ids, recipe = _batch(32, 8)
    ids = torch.from_numpy(ids).to(dev)
    args = (p.rows, p.normals, p.offsets, ids, 2048, (1 << 50) + 42)
    a = facadefeed.assemble(*args, (1 << 34) + 7, recipe, want_index=True)
    b = facadefeed.assemble(*args, (1 << 34) + 7, recipe, want_index=True)
    c = facadefeed.assemble(*args, (1 << 34) + 8, recipe, want_index=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(a[2], c[2])


def test_facade_feed_epochs_match_their_plan_and_alternate_two_sets(pool, dev):
    """repeat = 3 on the 11-facade pool: every item equals the kernel's and the statement's batch of its planned (step, ids) under
    train_recipe of its size; two consecutive items never share storage; item i+2 reuses item i's; the last batch is the short
    one; the second epoch continues the steps; done() with and without an event"""
    import torch
    blocks, normals, p = pool
    N, B, seed, repeat = 64, 4, (1 << 36) + 6, 3
    f = facadefeed.FacadeFeed(p, B, N, seed=seed, repeat=repeat)
    assert f.stream != torch.cuda.current_stream()
    for epoch in range(2):
        plan = facadefeed.epoch_plan(len(p), B, seed, epoch, repeat=repeat)
        assert len(f) == len(plan) == 9 and [len(i) for _, i in plan] == [4] * 8 + [1]
        prev, seen, visits = None, [], np.zeros(len(p), np.int64)
        for k, (pts, label, ready) in enumerate(f):
            step, ids = plan[k]
            assert step == epoch * 9 + k
            assert pts.shape == (len(ids), N, 9) and label.shape == (len(ids), N)
            if prev is not None:            # both live: no aliasing
                lo, hi = pts.data_ptr(), pts.data_ptr() + pts.numel() * 4
                assert hi <= prev[0].data_ptr() or lo >= prev[0].data_ptr() + prev[0].numel() * 4
                assert label.data_ptr() != prev[1].data_ptr()
            torch.cuda.current_stream().wait_event(ready)
            recipe = facadefeed.train_recipe(len(ids))
            ref = facadefeed.assemble_reference(p.sizes, ids, N, seed, step, recipe)
            want_pts, want_label = facadefeed.apply_reference(blocks, normals, ids, ref)
            got = pts.cpu().numpy()
            assert np.array_equal(label.cpu().numpy(), want_label)
            for b in range(len(ids)):
                src = blocks[ids[b]][ref.index[b]]
                if recipe[b] == 0:
                    assert np.array_equal(_bits(got[b]), _bits(np.concatenate((src[:, 0:3], normals[ids[b]][ref.index[b], 0:3],
                                                                               src[:, 3:6]), axis=1)))
                else:
                    assert (np.abs(got[b, :, 0:3].astype(np.float64) - want_pts[b, :, 0:3]) <= _bound(src[:, 0:3], int(recipe[b]))).all()
            want = facadefeed.assemble(p.rows, p.normals, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, recipe)
            assert torch.equal(pts.view(torch.int32), want[0].view(torch.int32)) and torch.equal(label, want[1])
            seen.append(pts.data_ptr())
            visits += np.bincount(ids, minlength=len(p))
            prev = (pts, label)
            if k % 2 == 0:
                f.done(ready)                # (odd items: no event handed back — the feed waits for the consuming stream instead)
            elif k == 3:
                ev = torch.cuda.Event()
                ev.record()
                f.done(ready, ev)
        assert seen[0] == seen[2] == seen[8] and seen[0] != seen[1] and seen[1] == seen[3]
        assert (visits == repeat).all()
    assert f.epoch == 2
    with pytest.raises(ValueError):
        f.done(torch.cuda.Event())
    # a mask for every cloud instead of the training recipe
    plain = facadefeed.FacadeFeed(p, B, N, seed=seed, repeat=1, recipe=0)
    pts, label, ready = next(iter(plain))
    torch.cuda.current_stream().wait_event(ready)
    step, ids = facadefeed.epoch_plan(len(p), B, seed, 0, repeat=1)[0]
    want = facadefeed.assemble(p.rows, p.normals, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, 0)
    assert torch.equal(pts.view(torch.int32), want[0].view(torch.int32))
