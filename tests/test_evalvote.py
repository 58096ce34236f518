"""harness/evalvote.py without a GPU: the numpy statement of the overlap-voting evaluation (the duplicate rule against numpy's own
fancy-index `+=`, the coverage loop, max_passes, metrics, merging ranks) and the C entries' host-side validation."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest

from sph3d_gcn_amd.harness import evalvote, feed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1500, 1024, 900, 2000, 3000, 1100, 5000, 700]


def _pool(sizes, seed=0, num_cls=13, inner_of=None):
    rng = np.random.RandomState(seed)
    T = int(np.sum(sizes))
    label = rng.randint(0, num_cls, T).astype(np.float32)
    inner = rng.randint(0, 2, T).astype(np.float32)
    if inner_of is not None:
        off = np.concatenate(([0], np.cumsum(sizes)))
        for k, v in inner_of.items():
            inner[off[k]:off[k + 1]] = v
    return label, inner


def _logits(C):
    def fn(p, index):
        b, N = index.shape
        return np.random.RandomState(1000 + p).randn(b, N, C).astype(np.float32)
    return fn


def test_last_slot_wins_written_out_by_hand():
    """5 rows, 8 slots: row 1 is drawn by slots 0, 1, 3 -> slot 3 votes; row 4 by slots 4, 6 -> slot 6; row 2 by 2, 7 -> 7; row 3 by
    nobody; slot j carries (j + 1) * [1, 10]"""
    index = np.array([1, 1, 2, 1, 4, 0, 4, 2], dtype=np.int32)
    logits = (np.arange(1, 9, dtype=np.float32).reshape(8, 1) * np.array([1, 10], dtype=np.float32))
    votes, count = np.zeros((5, 2), np.float32), np.zeros((5,), np.int32)
    rows = evalvote.vote_update(votes, count, index, logits)
    assert rows.tolist() == [0, 1, 2, 4]
    assert votes.tolist() == [[6, 60], [4, 40], [8, 80], [0, 0], [7, 70]]
    assert count.tolist() == [1, 1, 1, 0, 1]
    # a second pass adds once more; slots outside the block (-1, 5) vote nothing
    evalvote.vote_update(votes, count, np.array([3, -1, 5, 3, 0, 0, -1, 1]), logits)
    assert votes.tolist() == [[12, 120], [12, 120], [8, 80], [4, 40], [7, 70]]
    assert count.tolist() == [2, 2, 1, 1, 1]


def test_a_five_row_block_sampled_with_replacement():
    """vote_reference on one block of 5 rows at N = 8: the expected sums from a dict that a later slot overwrites"""
    C, N = 3, 8
    label, inner = np.array([0, 1, 2, 1, 0], np.float32), np.array([1, 1, 0, 1, 1], np.float32)
    seen = []

    def val(p):
        return np.arange(N * C, dtype=np.float32).reshape(1, N, C) + 100 * p

    def fn(p, index):
        seen.append(index.copy())
        return val(p)
    out = evalvote.vote_reference([5], label, inner, [0], N, seed=4, batch_index=2, logits_of_pass=fn, num_cls=C)
    assert out.complete and out.passes == len(seen) >= 1 and out.inner_size.tolist() == [4] == out.covered.tolist()
    want, cnt = np.zeros((5, C), np.float32), np.zeros(5, np.int32)
    for p, index in enumerate(seen):
        assert np.array_equal(index, feed.assemble_reference([5], [0], N, 4, (2 << 20) | p, False).index)
        assert index.min() >= 0 and index.max() < 5
        latest = {}
        for j, r in enumerate(index[0]):
            latest[int(r)] = j
        for r, j in latest.items():
            want[r] = want[r] + val(p)[0, j]
            cnt[r] += 1
    assert np.array_equal(out.votes[0].view(np.int32), want.view(np.int32)) and np.array_equal(out.count[0], cnt)
    assert np.array_equal(out.pred[0], np.argmax(want, axis=1))
    assert out.confusion.sum() == 4


@pytest.mark.parametrize("n,N", [(5, 8), (300, 1024), (1024, 1024), (2000, 512)])
def test_the_update_equals_numpys_fancy_index_add_bit_for_bit(n, N):
    rng = np.random.RandomState(n + N)
    a = rng.randn(n, 13).astype(np.float32)
    c = rng.randint(0, 5, n).astype(np.int32)
    votes, count = a.copy(), c.copy()
    for _ in range(3):
        idx = rng.randint(0, n, N) if n < N else rng.permutation(n)[:N]
        v = (rng.randn(N, 13) * 10 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
        a[idx] += v
        c[idx] += 1
        evalvote.vote_update(votes, count, idx, v)
        assert np.array_equal(votes.view(np.int32), a.view(np.int32)) and np.array_equal(count, c)


def _recount(indices, sizes, ids, inner, min_votes, upto):
    """covered per block after the first `upto` recorded passes, from the indices alone"""
    off = np.concatenate(([0], np.cumsum(sizes)))
    cov = []
    for k, i in enumerate(ids):
        cnt = np.zeros(sizes[i], np.int64)
        for index in indices[:upto]:
            cnt[np.unique(index[k])] += 1
        cov.append(int(((cnt >= min_votes) & (inner[off[i]:off[i + 1]] == 1)).sum()))
    return np.array(cov)


def test_coverage_decides_the_number_of_passes():
    C, N = 13, 1024
    label, inner = _pool(SIZES, 1)
    ids = np.arange(len(SIZES))
    passes = {}
    for mv in (1, 2):
        rec = []

        def fn(p, index):
            rec.append(index.copy())
            return _logits(C)(p, index)
        out = evalvote.vote_reference(SIZES, label, inner, ids, N, 3, 0, fn, C, min_votes=mv)
        assert out.complete and out.passes == len(rec)
        # the loop stops at the FIRST pass after which every inner row has min_votes counts
        assert (_recount(rec, SIZES, ids, inner, mv, out.passes) == out.inner_size).all()
        assert (_recount(rec, SIZES, ids, inner, mv, out.passes - 1) < out.inner_size).any()
        assert np.array_equal(out.covered, out.inner_size)
        # every block of the batch got the same number of passes: a drawn row is counted once per pass
        for k, n in enumerate(SIZES):
            per_pass = [len(np.unique(index[k])) for index in rec]
            assert out.count[k].sum() == sum(per_pass) and out.count[k].max() <= out.passes
            if n >= N:
                assert per_pass == [N] * out.passes
        assert out.confusion.sum() == int(inner.sum()) == out.inner_size.sum()
        passes[mv] = out.passes
    assert passes[2] >= passes[1] > 1


def test_a_block_without_inner_rows_does_not_prolong_the_batch():
    C, N = 5, 256
    sizes = [300, 40000, 200]
    label, inner = _pool(sizes, 2, C, inner_of={1: 0.0})
    both = evalvote.vote_reference(sizes, label, inner, [0, 1, 2], N, 1, 0, _logits(C), C)
    assert both.inner_size[1] == 0 and both.complete
    # 40000 rows at 256 per pass would need hundreds of passes; the small blocks' coverage ends the batch
    assert both.passes < 60 and both.count[1].sum() == both.passes * N
    # alone, that block needs no pass at all and contributes nothing
    alone = evalvote.vote_reference(sizes, label, inner, [1], N, 1, 0, _logits(C), C)
    assert alone.passes == 0 and alone.complete and alone.confusion.sum() == 0 and not alone.votes[0].any()


def test_max_passes_ends_an_uncovered_batch():
    C, N = 13, 1024
    label, inner = _pool(SIZES, 1)
    out = evalvote.vote_reference(SIZES, label, inner, np.arange(8), N, 3, 0, _logits(C), C, max_passes=2)
    assert out.passes == 2 and not out.complete
    assert (out.covered <= out.inner_size).all() and (out.covered < out.inner_size).any()
    for k in range(8):
        assert out.covered[k] == (out.count[k][inner[sum(SIZES[:k]):sum(SIZES[:k + 1])] == 1] >= 1).sum()
    # the confusion matrix still counts every inner row (rows never drawn predict class 0)
    assert out.confusion.sum() == int(inner.sum())
    for bad in (0, 1 << 20):
        with pytest.raises(ValueError):
            evalvote.vote_reference(SIZES, label, inner, np.arange(8), N, 3, 0, _logits(C), C, max_passes=bad)
    with pytest.raises(ValueError):
        evalvote.vote_reference(SIZES, label, inner, [1, 1], N, 3, 0, _logits(C), C)


def test_block_ids_outside_the_pool_vote_nothing():
    C, N = 4, 128
    sizes = [100, 200, 300]
    label, inner = _pool(sizes, 5, C)
    out = evalvote.vote_reference(sizes, label, inner, [2, -1, 3, 0], N, 1, 7, _logits(C), C)
    assert out.complete and out.inner_size[1] == out.inner_size[2] == 0 and out.votes[1].shape == (0, C)
    index = evalvote.draw_index(sizes, [2, -1, 3, 0], N, 1, evalvote.pass_step(7, 0))
    assert (index[1] == -1).all() and (index[2] == -1).all()
    # cloud k's draws use its position in the batch
    assert np.array_equal(index[3], feed.assemble_reference(sizes, [2, 2, 2, 0], N, 1, (7 << 20), False).index[3])


def test_metrics_on_a_hand_written_matrix():
    cm = np.array([[5, 1, 0],
                   [2, 2, 0],
                   [0, 0, 0]])                  # class 2 is absent and never predicted
    m = evalvote.metrics(cm)
    eps = np.finfo(float).eps
    assert m.overall_acc == 7 / 10
    assert np.array_equal(m.class_acc, np.array([5 / (6 + eps), 2 / (4 + eps), 0.0]))
    assert np.array_equal(m.class_iou, np.array([5 / (8 + eps), 2 / (5 + eps), 0.0]))
    assert m.miou == np.mean([5 / (8 + eps), 2 / (5 + eps), 0.0]) and m.mean_class_acc == np.mean(m.class_acc)
    assert abs(m.miou - (0.625 + 0.4) / 3) < 1e-15
    with pytest.raises(ValueError):
        evalvote.metrics(np.zeros((2, 3)))


def test_merged_ranks_equal_one_rank():
    C, N = 6, 256
    sizes = [300, 256, 100, 700, 257, 90, 400, 1000, 64, 500, 255]
    label, inner = _pool(sizes, 8, C)

    def fn(i, p, index):
        return np.random.RandomState(i * 4096 + p).randn(index.shape[0], N, C).astype(np.float32)
    one = evalvote.evaluate_reference(fn, sizes, label, inner, 3, N, 5, C, keep_votes=True)
    assert one.batches == [0, 1, 2, 3] and one.complete and one.confusion.sum() == int(inner.sum())
    assert [len(c) for c in one.covered] == [3, 3, 3, 2]                 # the last batch is the short one
    parts = [evalvote.evaluate_reference(fn, sizes, label, inner, 3, N, 5, C, rank=r, world=3, keep_votes=True) for r in range(3)]
    assert [p.batches for p in parts] == [[0, 3], [1], [2]]
    merged = evalvote.EvalResult.merge(parts[::-1])
    assert np.array_equal(merged.confusion, one.confusion) and merged.batches == one.batches and merged.passes == one.passes
    assert merged.miou == one.miou and merged.overall_acc == one.overall_acc and merged.complete
    assert np.array_equal(merged.class_iou, one.class_iou) and np.array_equal(merged.class_acc, one.class_acc)
    for i in one.batches:
        for a, b in zip(merged.votes[i].votes, one.votes[i].votes):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    with pytest.raises(ValueError):
        evalvote.EvalResult.merge([parts[0], parts[0]])


def test_vote_entries_are_declared_exported_and_bound():
    from sph3d_gcn_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sph3d.h")).read(), flags=re.S)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sph3d_vote_workspace", "sph3d_vote_begin", "sph3d_vote_accumulate", "sph3d_vote_finalize"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(l, name) and name in _lib.SIGNATURES
    assert "evaluate_s3dis_with_overlap.py" in open(os.path.join(ROOT, "include", "sph3d.h")).read()
    src = open(os.path.join(ROOT, "sph3d_gcn_amd", "csrc", "vote.hip")).read()
    assert "hipMalloc" not in src and "stream_scratch" not in src             # every buffer is the caller's
    assert not re.search(r"atomicAdd\(\s*&?\s*votes", src) and "unsafeAtomicAdd" not in src


def test_vote_entries_validate_on_the_host():
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    assert l.sph3d_abi_version() == 2
    assert l.sph3d_vote_workspace(1000) == 8000 and l.sph3d_vote_workspace(0) == 0
    one = ctypes.create_string_buffer(64)
    p = ctypes.cast(one, ctypes.c_void_p).value          # a non-null host address: validation fails before any use of it

    def accumulate(B=2, N=8, C=13, P=4, T=100, base=0, nrows=50, ps=0, mv=1, ptr=p, ws=p, ws_bytes=400):
        return l.sph3d_vote_accumulate(B, N, C, P, T, ptr, ptr, ptr, base, nrows, ps, ptr, ptr, mv, ptr, ptr, ptr, ptr, ptr, ws, ws_bytes, None)
    for kw, msg in ((dict(B=0), b"B<="), (dict(C=0), b"classes"), (dict(C=65), b"classes"), (dict(N=0), b"num_point>0"),
                    (dict(mv=0), b"min_votes>=1"), (dict(ps=1 << 20), b"pass in"), (dict(ps=-1), b"pass in"),
                    (dict(ptr=None), b"null"), (dict(ws=None), b"workspace"), (dict(ws_bytes=399), b"workspace"),
                    (dict(T=0), b"empty pool"), (dict(base=60), b"not a range"), (dict(nrows=0), b"not a range")):
        rc = accumulate(**kw)
        assert rc == -1 and msg in l.sph3d_last_error(), (kw, l.sph3d_last_error())
    rc = l.sph3d_vote_begin(2, 65, 4, 100, p, p, p, 0, 50, p, p, p, p, p, p, 400, None)
    assert rc == -1 and b"classes" in l.sph3d_last_error()
    rc = l.sph3d_vote_begin(2, 13, 4, 100, p, p, p, 0, 50, p, None, p, p, p, p, 400, None)
    assert rc == -1 and b"null output" in l.sph3d_last_error()
    rc = l.sph3d_vote_finalize(2, 0, 4, 100, p, p, p, 0, 50, p, p, p, p, None)
    assert rc == -1 and b"classes" in l.sph3d_last_error()
    rc = l.sph3d_vote_finalize(2, 13, 4, 100, p, p, p, 0, 50, p, p, None, p, None)
    assert rc == -1 and b"null output" in l.sph3d_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_python_side_argument_checks():
    for kw in (dict(num_cls=65), dict(min_votes=0), dict(max_passes=1 << 20), dict(world=0), dict(rank=2, world=2), dict(batch_size=0)):
        args = dict(batch_size=2, num_point=8, seed=0, num_cls=3, min_votes=1, max_passes=4, rank=0, world=1)
        args.update(kw)
        with pytest.raises(ValueError):
            evalvote.evaluate(lambda p, l, i: None, None, **args)


def test_merge_order_sorts_interleaved_ranks_and_refuses_a_repeated_key():
    """the helper behind EvalResult / ShapeResult / SceneResult.merge: rank r of 3 evaluated batches r, r + 3, ...; the merged
    order is ascending by key whatever order the results come in, the kept dicts are joined only when all have one"""
    Res = collections.namedtuple("Res", "batches passes votes")
    ranks = [Res([r, r + 3, r + 6][:3 - (r == 2)], ["p%d" % k for k in [r, r + 3, r + 6][:3 - (r == 2)]], {r: "v%d" % r}) for r in range(3)]
    for order in ([0, 1, 2], [2, 0, 1]):
        results, pick, votes = evalvote.merge_order([ranks[r] for r in order])
        assert [res.batches for res in results] == [ranks[r].batches for r in order]
        assert pick("batches") == list(range(8)) and pick("passes") == ["p%d" % k for k in range(8)]
        assert votes == {0: "v0", 1: "v1", 2: "v2"}
    _, _, votes = evalvote.merge_order([ranks[0], ranks[1]._replace(votes=None)])
    assert votes is None
    with pytest.raises(ValueError, match="a batch occurs in two results"):
        evalvote.merge_order([ranks[0], ranks[1], Res([7, 3], ["x", "y"], None)])
    Scenes = collections.namedtuple("Scenes", "scenes pred")
    with pytest.raises(ValueError, match="a scene occurs in two results"):
        evalvote.merge_order([Scenes([0, 2], None), Scenes([2], None)], "scenes", "scene", "pred")
    with pytest.raises(ValueError, match="no results"):
        evalvote.merge_order([])


def test_check_share_refuses_what_is_no_share():
    evalvote.check_share(1, 0, 1, "evaluate")
    evalvote.check_share(16, 3, 4, "evaluate")
    for batch_size, rank, world in ((16, 0, 0), (16, 4, 4), (0, 0, 1), (16, -1, 4)):
        with pytest.raises(ValueError, match="evaluate_scenes: bad batch_size / rank / world"):
            evalvote.check_share(batch_size, rank, world, "evaluate_scenes")
