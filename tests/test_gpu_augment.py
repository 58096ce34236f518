"""csrc/augment.hip on the device against harness/augment.py's numpy statement: labels, inner, the gate masks, which slot came
from which cloud and the counters bit for bit; floats within the per-element bound tests/_augment_ref.py derives (an element no
transform computes has a bound of zero: it is compared bit for bit).  tests/test_augment.py checks on the CPU that the statement
decides every elastic skip of these cases with a whole node to spare.  Worst error / bound measured on the MI355X over all cases:
0.95 (an element with a single rounding on its path reaches its bound by nature); the largest bound of any element is 7.6e-5."""
import numpy as np
import pytest

import _augment_cases as cases
import _augment_ref as aref
from sph3d_gcn_amd.harness import augment, feed

pytestmark = pytest.mark.gpu


def _device_run(dev, batch, seed, step, opts):
    """-> points, label, inner (numpy), gates int32 [B], counters [3]"""
    import torch
    p, label, inner = batch
    B, N, _C = p.shape
    tp, tl = torch.from_numpy(p).to(dev), torch.from_numpy(label).to(dev)
    ti = None if inner is None else torch.from_numpy(inner).to(dev)
    ws = torch.empty((augment.workspace_bytes(B, N, opts.max_nodes),), dtype=torch.uint8, device=dev)
    status = torch.zeros((3,), dtype=torch.int64, device=dev)
    got = augment.apply(tp, tl, ti, seed, step, opts, ws, status)
    assert got[0] is tp and got[1] is tl and got[2] is ti
    torch.cuda.synchronize()
    return (tp.cpu().numpy(), tl.cpu().numpy(), None if ti is None else ti.cpu().numpy(), augment.read_gates(ws, B),
            status.cpu().tolist())


def _tracer(batch):
    """inner replaced by the element's own number b * N + slot: what came from where is then an integer output"""
    p, label, inner = batch
    if inner is None:
        return batch
    return p, label, np.arange(label.size, dtype=np.int32).reshape(label.shape)


@pytest.mark.parametrize("name", ["a", "a_skip", "b", "c", "d", "e", "xyz"])
def test_kernels_equal_the_numpy_statement(dev, name):
    batch, opts, keys = cases.CASES[name]
    batch = _tracer(batch)
    worst = 0.0
    for seed, step in keys:
        V, E, lab, inn, rep, _want = aref.evaluate(*batch, seed, step, opts)
        pts, label, inner, gates, counters = _device_run(dev, batch, seed, step, opts)
        assert np.array_equal(gates, rep.gates)
        assert np.array_equal(label, lab)
        assert (inner is None and inn is None) or np.array_equal(inner, inn)
        assert counters == [rep.elastic_skipped[0], rep.elastic_skipped[1], rep.mixed_pairs]
        err = np.abs(pts.astype(np.float64) - V)
        exact = E == 0
        assert (pts[exact] == V[exact].astype(np.float32)).all()
        ratio = float((err[~exact] / E[~exact]).max()) if (~exact).any() else 0.0
        worst = max(worst, ratio)
        print("%s seed=%d step=%d gates=%s skipped=%s mixed=%d: worst error / bound %.4f, largest bound %.3g"
              % (name, seed, step, gates.tolist(), rep.elastic_skipped, rep.mixed_pairs, ratio, float(E.max())))
        assert (err <= E).all(), (name, seed, step, ratio)
        for b in np.nonzero(rep.gates == 0)[0]:
            assert np.array_equal(pts[b].view(np.int32), batch[0][b].view(np.int32))
    if name == "a_skip":
        assert counters[:2] == [2, 2]                      # exactly the last two clouds, in both passes


def test_a_colour_bit_on_xyz_only_clouds_is_refused(dev):
    import torch
    p, label, inner = (torch.from_numpy(t).to(dev) for t in cases.small(2, 16, 3, 0))
    before = p.clone()
    with pytest.raises(ValueError, match="colour"):
        augment.apply(p, label, inner, 1, 1, augment.default_options("object")._replace(enable=augment.FLIPX | augment.CDROP))
    assert torch.equal(p, before)


def test_cpu_tensors_are_refused():
    import torch
    from sph3d_gcn_amd import _lib
    p, label, inner = (torch.from_numpy(t) for t in cases.small(2, 16, 6, 0))
    with pytest.raises(_lib.Sph3dError):
        augment.apply(p, label, inner, 1, 1, augment.default_options("s3dis"))


def test_all_gates_off_copies_the_batch_bit_for_bit(dev):
    batch, opts, _ = cases.CASES["a"]
    for o in (opts._replace(enable=0), opts._replace(prob=(0.0,) * 9)):
        pts, label, inner, gates, counters = _device_run(dev, batch, 3, 4, o)
        assert np.array_equal(pts.view(np.int32), batch[0].view(np.int32))
        assert np.array_equal(label, batch[1]) and np.array_equal(inner, batch[2]) and counters == [0, 0, 0]


def test_same_seed_and_step_give_identical_bits(dev):
    batch, opts, _ = cases.CASES["a"]
    a = _device_run(dev, batch, 42, 7, opts)
    b = _device_run(dev, batch, 42, 7, opts)
    c = _device_run(dev, batch, 42, 8, opts)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3]) and a[4] == b[4]
    assert not np.array_equal(a[0].view(np.int32), c[0].view(np.int32))


def _pool(dev):
    rng = np.random.RandomState(5)
    blocks = []
    for n in (600, 256, 900, 300, 1200, 257, 512, 700, 100, 2000):
        b = np.empty((n, 8), dtype=np.float32)
        b[:, 0:3] = rng.rand(n, 3) * np.array([1.5, 1.5, 3.0])
        b[:, 3:6] = rng.rand(n, 3) * 2 - 1
        b[:, 6] = rng.randint(0, 13, n)
        b[:, 7] = rng.randint(0, 2, n)
        blocks.append(b)
    return feed.BlockPool.from_blocks(blocks, dev)


def test_device_feed_with_and_without_a_stage(dev):
    """with a Stage an item is apply(assemble(...)) of its step bit for bit, and the counters add up over the epoch; without one
    the feed yields what assemble() yields, as before"""
    import torch
    p = _pool(dev)
    B, N, seed = 4, 256, 6
    opts = cases.options("s3dis")
    stage = augment.Stage(opts, B, N, 6, dev)
    plain = feed.DeviceFeed(p, B, N, seed=seed)
    staged = feed.DeviceFeed(p, B, N, seed=seed, post=stage)
    assert plain.post is None and staged.post is stage
    plan = feed.epoch_plan(len(p), B, seed, 0)
    status = torch.zeros((3,), dtype=torch.int64, device=dev)
    for (step, ids), a, b in zip(plan, plain, staged):
        for item in (a, b):
            torch.cuda.current_stream().wait_event(item[3])
        want = feed.assemble(p.rows, p.offsets, torch.from_numpy(ids).to(dev), N, seed, step, True)
        for g, w in zip(a[:3], want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
        augment.apply(*want, seed, step, opts, status=status)
        for g, w in zip(b[:3], want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
        assert not torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        plain.done(a[3])
        staged.done(b[3])
    got = stage.read()
    assert [got.elastic_skipped[0], got.elastic_skipped[1], got.mixed_pairs] == status.cpu().tolist()
    assert got.mixed_pairs > 0


def test_the_other_feeds_carry_a_stage(dev):
    """ScanNetFeed (6 channels with inner) and ObjectFeed (xyz only, a category instead of inner): an item of the feed with a
    Stage is apply() of the same feed's item without one"""
    import torch
    from sph3d_gcn_amd.harness import objfeed, scannet
    p = _pool(dev)
    B, N, seed = 4, 128, 3
    made = ((lambda post: scannet.ScanNetFeed(p, B, N, seed=seed, post=post), "scannet", 6, True),
            (lambda post: objfeed.ObjectFeed(_shapes(dev), B, N, seed=seed, dataset="shapenet", post=post), "object", 3, False))
    for make, layout, C, has_inner in made:
        opts = cases.options(layout, mix=1.0)
        plain, staged = make(None), make(augment.Stage(opts, B, N, C, dev))
        step0 = 0
        for k, (a, b) in enumerate(zip(plain, staged)):
            torch.cuda.current_stream().wait_event(a[-1])
            torch.cuda.current_stream().wait_event(b[-1])
            pts, label = a[0].clone(), a[1].clone()
            inner = a[2].clone() if has_inner else None
            augment.apply(pts, label, inner, seed, step0 + k, opts)
            assert torch.equal(b[0].view(torch.int32), pts.view(torch.int32)) and torch.equal(b[1], label)
            if has_inner:
                assert torch.equal(b[2], inner)
            else:
                assert torch.equal(b[2], a[2])                          # the category is not exchanged
            plain.done(a[-1])
            staged.done(b[-1])
        assert staged.post.read().mixed_pairs > 0


def _shapes(dev):
    from sph3d_gcn_amd.harness import objfeed
    rng = np.random.RandomState(2)
    shapes = [rng.rand(n, 3).astype(np.float32) * 2 - 1 for n in (300, 128, 500, 200, 129, 400, 250, 640)]
    labels = [rng.randint(0, 4, s.shape[0]) for s in shapes]
    return objfeed.ShapePool.from_arrays(shapes, labels, [0, 1, 2, 3, 0, 1, 2, 3], device=dev)
