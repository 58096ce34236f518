"""csrc/clseval.hip on the device against harness/clseval.py's numpy statement: the whole-shape batch (index and the mask-0
coordinates bit for bit, every other mask within the bound tests/test_gpu_objfeed.py uses for the same arithmetic), the float64
vote sums as bit patterns with predictions and counters, the loop of `evaluate` against the replay of its recorded logits, the
absence of host reads inside the loop, and one real model.  Every launch here is an ordinary one."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import clseval, objfeed

from _clseval_cases import KINDS, same_f64, same_result, vote_logits

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 700]


@pytest.fixture(scope="module")
def pool(dev):
    rng = np.random.RandomState(0)
    shapes = [objfeed.shape_blocks((rng.rand(n, 3) * 2.0 - 1.0).astype(np.float32), k) for k, n in enumerate(SIZES)]
    return np.concatenate(shapes)[:, 0:3].copy(), objfeed.ShapePool(shapes, np.arange(len(SIZES)), device=dev)


def _bound(src, mask):
    """tests/test_gpu_objfeed.py's bound without its jitter term: 1e-5 * (1.25 (|x| + |y| + |z|) of the source row + 0.1 if SHIFT)"""
    return 1e-5 * (1.25 * np.abs(src.astype(np.float64)).sum(axis=1, keepdims=True) + (objfeed.SHIFT_RANGE if mask & objfeed.SHIFT else 0.0))


# ---------------------------------------------------------------------------------------------------------------
# the feed
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_feed_equals_the_numpy_statement(pool, dev, N):
    """B = 3: a shape, the id -1 and the id P, in rotating positions; both orders, both swaps, masks 0, 1, 2, 4, 8, 15"""
    import torch
    rows_xyz, p = pool
    P, worst, seed = len(p), 0.0, (1 << 41) + 5
    for s in range(P):
        ids = np.roll(np.array([s, -1, P], dtype=np.int32), s)
        ids_dev = torch.from_numpy(ids).to(dev)
        for order in (0, 1):
            for swap in (0, 1):
                for mask in (0, 1, 2, 4, 8, 15):
                    step = (s << 20) | mask
                    ref = clseval.assemble_reference(p.sizes, rows_xyz, ids, N, seed, step, mask, order, swap)
                    pts, index = clseval.assemble(p.rows, p.offsets, ids_dev, N, seed, step, mask, order, bool(swap), want_index=True)
                    pts, index = pts.cpu().numpy(), index.cpu().numpy()
                    assert pts.shape == (3, N, 3) and np.array_equal(index, ref.index), (s, order, swap, mask)
                    took = index >= 0
                    assert not pts[~took].any() and not took[ids != s].any()
                    if order == 1:          # stored order: rows 0..n-1, zeros and index -1 past row n
                        n = min(SIZES[s], N)
                        assert index[ids == s][0].tolist() == list(range(n)) + [-1] * (N - n)
                    if mask == 0:
                        assert np.array_equal(pts.view(np.int32), ref.source.view(np.int32))
                        assert np.array_equal(pts.astype(np.float64), ref.points)
                        continue
                    bound = _bound(ref.source[took], mask)
                    err = np.abs(pts[took].astype(np.float64) - ref.points[took])
                    worst = max(worst, float((err / bound).max()))
                    assert (err <= bound).all(), (s, order, swap, mask, float((err / bound).max()))
                    assert not np.array_equal(pts[took], ref.source[took])
    print("N=%d: worst error / bound %.4f" % (N, worst))


def test_feed_swap_is_the_references_column_exchange(pool, dev):
    """mask 0, stored order, swap_yz: `xyz[:, [0, 2, 1]]` bit for bit; and the sample of order 0 is objfeed's"""
    import torch
    rows_xyz, p = pool
    ids = torch.tensor([4, 3, 2], dtype=torch.int32, device=dev)
    pts = clseval.assemble(p.rows, p.offsets, ids, 256, 1, 2, 0, 1, True).cpu().numpy()
    off = p.host_offsets
    for b, s in enumerate((4, 3, 2)):
        assert np.array_equal(pts[b].view(np.int32), rows_xyz[off[s]:off[s] + 256][:, [0, 2, 1]].view(np.int32))
    _pts, index = clseval.assemble(p.rows, p.offsets, ids, 256, 1, 2, 15, 0, True, want_index=True)
    _o, _l, want = objfeed.assemble(p.rows, p.offsets, ids, 256, 1, 2, 15, want_index=True)
    assert torch.equal(index, want)


def test_feed_refuses_jitter(pool, dev):
    import torch
    from sph3d_gcn_amd import _lib
    _rows, p = pool
    ids = torch.tensor([4, 3, 2], dtype=torch.int32, device=dev)
    for bad in (16, 31, [0, 16, 0]):
        with pytest.raises(_lib.Sph3dError):
            clseval.assemble(p.rows, p.offsets, ids, 8, 1, 1, bad)
    for bad in (-1, 32, [0, 1]):
        with pytest.raises(ValueError):
            clseval.assemble(p.rows, p.offsets, ids, 8, 1, 1, bad)
    with pytest.raises(ValueError):
        clseval.assemble(p.rows, p.offsets, ids, 8, 1, 1, 0, order=2)
    with pytest.raises(ValueError):                                    # stored order needs num_point rows in every shape
        clseval.ClassVoter(p, 2, 8, 5, 1)
    assert clseval.ClassVoter(p, 2, 1, 5, 1).batches == [0, 1, 2] and clseval.ClassVoter(p, 2, 8, 5, 1, order=0).V == 1


# ---------------------------------------------------------------------------------------------------------------
# the vote
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 12])
@pytest.mark.parametrize("C", [1, 2, 40, 64])
@pytest.mark.parametrize("B", [1, 3, 32])
def test_vote_kernels_equal_the_numpy_statement(dev, B, C, V):
    """sums as float64 bit patterns, pred, the four counters, class_seen, class_correct and votes_out, with a label outside [0, C)
    and a shape id outside the pool among the clouds"""
    import torch
    from sph3d_gcn_amd import _lib
    l, P = _lib.lib(), B + 3
    for shift in range(KINDS):
        rng = np.random.RandomState(1000 * B + 10 * C + V + shift)
        logits = vote_logits(B, C, V, 7 * B + C + V, shift)
        ids = rng.permutation(P)[:B].astype(np.int32)
        category = rng.randint(0, C, P).astype(np.int32)
        out_at, bad_at = (1, 2) if B >= 3 else (0, 0)
        if B >= 3 or shift % 3 == 1:
            ids[out_at] = -1 if shift % 2 else P
        if B >= 3 or shift % 3 == 2:
            category[ids[bad_at]] = C if shift % 2 else -1
        inside = (ids >= 0) & (ids < P)

        every = clseval.vote_reference(logits, np.zeros((B,), np.int32), C)                  # the sums and arg-max of all clouds
        want = clseval.vote_reference(logits[:, inside], category[ids[inside]], C)          # the counts of those in the pool
        want_pred = np.full((P,), -1, np.int32)
        want_pred[ids[inside]] = every.pred[inside]
        want_votes = np.zeros((P, V, C), np.float32)
        want_votes[ids[inside]] = logits[:, inside].transpose(1, 0, 2)

        ids_dev, cat_dev = torch.from_numpy(ids).to(dev), torch.from_numpy(category).to(dev)
        sums = torch.full((B, C), 123.0, dtype=torch.float64, device=dev)                   # (vote 0 overwrites what is there)
        state = torch.zeros((P + 4 + 2 * C,), dtype=torch.int32, device=dev)
        state[:P] = -1
        votes_out = torch.zeros((P, V, C), dtype=torch.float32, device=dev)
        for v in range(V):
            lg = torch.from_numpy(logits[v]).to(dev)
            _lib.check(l.sph3d_cls_vote_accumulate(B, C, _lib.ptr(lg), v, V, _lib.ptr(sums), _lib.ptr(ids_dev), _lib.ptr(votes_out),
                                                   P, _lib.stream_ptr()))
        _lib.check(l.sph3d_cls_vote_finalize(B, C, _lib.ptr(sums), _lib.ptr(ids_dev), _lib.ptr(cat_dev), P, _lib.ptr(state),
                                             _lib.ptr(state[P:]), _lib.ptr(state[P + 4:]), _lib.ptr(state[P + 4 + C:]),
                                             _lib.stream_ptr()))
        got, got_sums, got_votes = state.cpu().numpy(), sums.cpu().numpy(), votes_out.cpu().numpy()
        assert same_f64(got_sums, every.sums), (shift, got_sums, every.sums)
        assert np.array_equal(got[:P], want_pred), (shift, got[:P], want_pred)
        assert got[P:P + 4].tolist() == [want.seen, want.correct, want.nonfinite, want.bad_label], shift
        assert np.array_equal(got[P + 4:P + 4 + C], want.class_seen) and np.array_equal(got[P + 4 + C:], want.class_correct)
        assert np.array_equal(got_votes.view(np.int32), want_votes.view(np.int32))
        assert want.bad_label == int(B >= 3 or shift % 3 == 2) and int((~inside).sum()) == int(B >= 3 or shift % 3 == 1)


def test_vote_entries_validate_on_the_host(dev):
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    for rc in (l.sph3d_cls_vote_accumulate(1, 65, None, 0, 1, None, None, None, 1, None),
               l.sph3d_cls_vote_accumulate(1, 4, None, 2, 2, None, None, None, 1, None),
               l.sph3d_cls_vote_finalize(1, 0, None, None, None, 1, None, None, None, None, None),
               l.sph3d_clsfeed_assemble(1, 4, 1, 8, None, None, None, 0, 0, None, 2, 0, None, None, None)):
        with pytest.raises(ValueError):
            _lib.check(rc)


# ---------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------
def _small_pool(dev, C):
    rng = np.random.RandomState(3)
    xyz = [(rng.rand(256, 3) * 2.0 - 1.0).astype(np.float32) for _ in range(7)]
    category = np.array([0, 1, 2, 3, 4, C, 1], dtype=np.int32)                              # (one class outside [0, C))
    return objfeed.ShapePool.from_arrays(xyz, list(category), category, device=dev)


def _matrix_model(dev, C, record=None):
    import torch
    W = torch.from_numpy(np.random.RandomState(4).randn(3, C).astype(np.float32)).to(dev)

    def model_fn(points):
        logits = points.mean(dim=1) @ W
        if record is not None:
            record.append(logits.clone())
        return logits
    return model_fn


def test_evaluate_equals_the_replay_of_its_logits(dev):
    """7 shapes of 256 rows, batch 3 (a last batch of 1), 3 votes: every field of ClsResult; world 2 merged equals world 1"""
    C, B, V = 5, 3, 3
    p = _small_pool(dev, C)
    record = []
    res = clseval.evaluate(_matrix_model(dev, C, record), p, B, 256, seed=9, num_cls=C, num_votes=V, swap_yz=True, keep_votes=True)
    assert len(record) == 3 * V and [tuple(r.shape) for r in record] == [(3, C)] * 6 + [(1, C)] * 3
    host = [r.cpu().numpy() for r in record]
    want = clseval.evaluate_reference(lambda i, v: host[i * V + v], p.category, B, C, V, keep_votes=True)
    same_result(res, want)
    assert res.seen == 6 and res.bad_label == 1 and res.nonfinite == 0 and res.shapes.tolist() == list(range(7))
    assert not np.array_equal(host[0], host[1]) and not np.array_equal(host[1], host[2])           # the votes are augmented
    shares = [clseval.evaluate(_matrix_model(dev, C), p, B, 256, seed=9, num_cls=C, num_votes=V, rank=r, world=2, swap_yz=True,
                               keep_votes=True) for r in range(2)]
    assert shares[0].batches == [0, 2] and shares[1].batches == [1] and (shares[1].pred >= 0).sum() == 3
    same_result(clseval.ClsResult.merge(shares), res)
    plain = clseval.evaluate(_matrix_model(dev, C), p, B, 256, seed=9, num_cls=C, num_votes=1)
    assert plain.votes is None and plain.seen == 6


def test_no_host_read_inside_the_loop(dev):
    """torch's synchronisation trap around every run_batch: nothing raises; the trap is first shown to work in this build"""
    import torch
    C, B, V = 5, 3, 3
    p = _small_pool(dev, C)
    model_fn = _matrix_model(dev, C)
    voter = clseval.ClassVoter(p, B, 256, C, V, swap_yz=True, keep_votes=True, seed=9)
    one = torch.ones((1,), device=dev)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):
            one.item()
        for i in voter.batches:
            voter.run_batch(model_fn, i)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    res = voter.result()
    same_result(res, clseval.evaluate(model_fn, p, B, 256, seed=9, num_cls=C, num_votes=V, swap_yz=True, keep_votes=True))
    with pytest.raises(ValueError):
        voter.run_batch(model_fn, 0)                                   # a batch is evaluated once


def test_one_real_model(dev):
    """SPH3DModelNet on the reduced 1024-point plan, 4 shapes, batch 2, 2 votes: pred is the arg-max of the float64 sums of the
    logits the same calls returned"""
    from sph3d_gcn_amd.harness import modelnet_net, synth
    cfg = modelnet_net.small_config(1024)
    model = modelnet_net.SPH3DModelNet(cfg, device=dev, seed=3)
    p = objfeed.ShapePool.from_arrays([synth.modelnet_cloud(60 + k, 1024) for k in range(4)], [3, 17, 39, 0], [3, 17, 39, 0], device=dev)
    record = []

    def model_fn(points):
        logits = model(points, is_training=False)[0]
        record.append(logits.clone())
        return logits
    res = clseval.evaluate(model_fn, p, 2, 1024, seed=1, num_cls=cfg.num_cls, num_votes=2)
    assert res.seen == 4 and res.nonfinite == 0 and res.bad_label == 0 and len(record) == 4
    host = [r.cpu().numpy().astype(np.float64) for r in record]
    sums = np.concatenate([host[0] + host[1], host[2] + host[3]])
    assert np.array_equal(res.pred, np.argmax(sums, 1)) and res.correct == int((res.pred == p.category).sum())
    print("accuracy %.2f, logits range [%.3g, %.3g]" % (res.accuracy, sums.min(), sums.max()))
