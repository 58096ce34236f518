"""harness/scannet.py without a GPU: the recipes, the numpy statement of a batch of chained views against the reference's own
functions through their recorded inputs, random numbers and outputs (tests/golden/scannet_ref.npz, written by
tests/golden/make_scannet_golden.py), the view keys, the three-view vote loop, the sub-20 figures and `merge`; and the assertion
that every evaluation the GPU tests run (tests/_scannet_cases.py) completes inside its cap in the statement."""
import os

import numpy as np
import pytest

import _scannet_cases as cases
from sph3d_gcn_amd.harness import evalvote, feed, objfeed, scannet, scenemerge

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scannet_ref.npz")
T, L, S, H, J = objfeed.TURN, objfeed.TILT, objfeed.SCALE, objfeed.SHIFT, objfeed.JITTER
SIZES = [1, 5, 63, 64, 65, 300, 1000]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------------------------
# recipes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,third", [(1, 0), (2, 0), (3, 1), (7, 2), (16, 5)])
def test_the_training_recipe(B, third):
    r = scannet.train_recipe(B)
    assert r.dtype == np.int32 and r.tolist() == [T | L | S | H | J] * third + [L | S | H | J] * third + [0] * (B - 2 * third)
    assert third == B // 3 and r[2 * third:].tolist() == [0] * (B - 2 * third)


def test_the_evaluation_views_and_the_constants():
    assert scannet.EVAL_VIEWS == (0, L | S | H | J, T | L | S | H | J) == (0, 30, 31)
    assert scannet.TRAIN_FULL == 31 and scannet.TRAIN_LIGHT == 30
    assert len(scannet.CLASS_NAMES) == 21 and scannet.CLASS_NAMES[0] == "other20" and scannet.CLASS_NAMES[20] == "otherfurniture"
    assert scannet.SUB20 == tuple(range(1, 20)) and scannet.BENCHMARK20 == tuple(range(1, 21))
    assert len(scannet.LABELID_SET) == 21 and scannet.LABELID_SET[0] == 40 and scannet.LABELID_SET[13] == 14
    assert list(scannet.LABELID_SET[1:13]) == list(range(1, 13)) and scannet.LABELID_SET[-1] == 39
    with pytest.raises(ValueError):
        scannet.train_recipe(0)


def test_masks_outside_the_five_bits_and_bad_view_counts_are_refused():
    for bad in ([[0, 32]], [[-1, 0]], [[0, 1], [2, 64]]):
        with pytest.raises(ValueError):
            scannet.check_recipes(bad, 2)
        with pytest.raises(ValueError):
            scannet.assemble_reference(SIZES, [0, 1], 16, 1, 1, bad)
    with pytest.raises(ValueError):
        scannet.check_recipes(np.zeros((5, 2), np.int32), 2)                 # five views
    with pytest.raises(ValueError):
        scannet.check_recipes(np.zeros((0, 2), np.int32), 2)
    with pytest.raises(ValueError):
        scannet.check_recipes(np.zeros((2, 3), np.int32), 2)                 # not B masks per view
    with pytest.raises(ValueError):
        scannet.check_recipes([[1.0, 2.0]], 2)
    assert scannet.check_recipes([3, 4], 2).tolist() == [[3, 4]]             # [B]: one view
    assert scannet.eval_recipes(scannet.EVAL_VIEWS, 5).tolist() == [[0] * 5, [30] * 5, [31] * 5]
    with pytest.raises(ValueError):
        scannet.check_recipes(scannet.EVAL_VIEWS, 5)                         # (one mask per view: eval_recipes)
    assert scannet.eval_recipes((0, 31), 2).tolist() == [[0, 0], [31, 31]]
    with pytest.raises(ValueError):
        scannet.eval_recipes((0, 32), 2)


def test_the_entry_validates_on_the_host():
    """sph3d_blockfeed_assemble refuses requests that describe no launch before touching a device"""
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    n = [None] * 3
    for views in (0, 5, -1):
        assert l.sph3d_blockfeed_assemble(2, 64, 1, 8, *n, 1, 1, views, None, None, None, None, None, None) == -1
        assert b"views" in l.sph3d_last_error()
    assert l.sph3d_blockfeed_assemble(0, 64, 1, 8, *n, 1, 1, 3, None, None, None, None, None, None) == -1
    assert b"B<=65535" in l.sph3d_last_error()
    assert l.sph3d_blockfeed_assemble(70000, 64, 1, 8, *n, 1, 1, 3, None, None, None, None, None, None) == -1
    assert l.sph3d_blockfeed_assemble(2, 0, 1, 8, *n, 1, 1, 3, None, None, None, None, None, None) == -1
    assert b"num_point>0" in l.sph3d_last_error()
    assert l.sph3d_blockfeed_assemble(2, 64, 1, 8, *n, 1, 1, 3, None, None, None, None, None, None) == -1
    assert b"null input" in l.sph3d_last_error()


# ---------------------------------------------------------------------------------------------------------------
# the golden: the statement's arithmetic against the reference's own functions
# ---------------------------------------------------------------------------------------------------------------
class _Take:
    def __init__(self, a):
        self.a, self.at = np.asarray(a), 0

    def __call__(self, *shape):
        n = int(np.prod(shape))
        v = self.a[self.at:self.at + n].reshape(shape)
        self.at += n
        return v

    def done(self):
        return self.at == self.a.shape[0]


def _recorded_view(take, mask, clouds, B, N):
    """an objfeed.Reference of one view whose numbers are the recorded ones, consumed in the order utils/data_util.py asks for
    them, for the clouds `clouds` (the others: mask 0)"""
    recipe = np.zeros((B,), np.int32)
    theta, tilt = np.zeros((B,)), np.zeros((B, 3))
    scale, shift, noise = np.ones((B,)), np.zeros((B, 3)), np.zeros((B, N, 3))
    c = len(clouds)
    recipe[clouds] = mask
    if mask & T:
        theta[clouds] = take(c) * 2 * np.pi
    tilt[clouds] = np.clip(objfeed.ANGLE_SIGMA * take(c, 3), -objfeed.ANGLE_CLIP, objfeed.ANGLE_CLIP)
    scale[clouds] = take(c)
    shift[clouds] = take(c, 3)
    noise[clouds] = np.clip(objfeed.JITTER_SIGMA * take(c, N, 3), -objfeed.JITTER_CLIP, objfeed.JITTER_CLIP)
    return [recipe, theta, tilt, scale, shift, noise]


def _merge(a, b):
    """two recorded views over disjoint clouds -> one"""
    out = [a[0] + b[0]]
    for x, y, ident in zip(a[1:], b[1:], (0.0, 0.0, 1.0, 0.0, 0.0)):
        out.append(np.where(x == ident, y, x))
    return out


def _terms(xyz, r, b):
    """per row the largest magnitude sum of the terms of any element at any stage of the view's transform: what one fp32
    rounding is relative to (tests/test_objfeed.py: _close), and the float64 value after the view"""
    cur = np.asarray(xyz, dtype=np.float64)
    big = np.zeros((cur.shape[0], 1))
    m = int(r[0][b])
    stages = []
    if m & T:
        stages.append(("mat", objfeed.turn_matrix(r[1][b])))
    if m & L:
        stages.append(("mat", objfeed.tilt_matrix(*r[2][b])))
    if m & S:
        stages.append(("mul", r[3][b]))
    if m & H:
        stages.append(("add", r[4][b]))
    if m & J:
        stages.append(("add", r[5][b]))
    for kind, v in stages:
        if kind == "mat":
            t, cur = np.dot(np.abs(cur), np.abs(v)), np.dot(cur, v)
        elif kind == "mul":
            t, cur = np.abs(cur) * v, cur * v
        else:
            t, cur = np.abs(cur) + np.abs(v), cur + v
        big = np.maximum(big, t.max(axis=1, keepdims=True))
    return big, cur, len(stages)


def _check_chain(got, want, src, views, b):
    """|got - want| <= (number of chained transforms) * 2^-23 * terms: tests/test_objfeed.py's bound for one transform — the
    reference rounds a matrix entry and the result of every transform to float32, 2^-24 of the terms each — times the length of
    the chain.  -> worst error / bound"""
    big, cur, k = np.zeros((src.shape[0], 1)), src, 0
    for r in views:
        t, cur, n = _terms(cur, r, b)
        big, k = np.maximum(big, t), k + n
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    if k == 0:
        assert (err == 0).all()
        return 0.0
    bound = k * 2.0 ** -23 * big
    assert (err <= bound).all(), (b, float((err / bound).max()))
    return float((err / bound).max())


def _as_blocks(inp, label, inner):
    return [np.concatenate([inp[b], label[b][:, None].astype(np.float32), inner[b][:, None].astype(np.float32)], axis=1)
            for b in range(inp.shape[0])]


def test_the_statement_reproduces_the_references_training_recipe(golden):
    """train_scannet.py's augment_fn, run from its AST by the generator: with its two shuffles applied to the input and its random
    numbers substituted for the draws, apply_reference under train_recipe(6) gives what it gave — five chained transforms on
    clouds 0:2, four on clouds 2:4, clouds 4:6 copied unchanged"""
    B, N = 6, 16
    inp = golden["input"]
    assert inp.shape == (B, N, 6) and inp.dtype == np.float32
    pb, pp = golden["train_shuffle"][:B], golden["train_shuffle"][B:]
    assert sorted(pb.tolist()) == list(range(B)) and sorted(pp.tolist()) == list(range(N))
    x, lab, inn = inp[pb][:, pp], golden["label"][pb][:, pp], golden["inner"][pb][:, pp]
    take = _Take(golden["train_random"])
    full = _recorded_view(take, scannet.TRAIN_FULL, [0, 1], B, N)
    light = _recorded_view(take, scannet.TRAIN_LIGHT, [2, 3], B, N)
    assert take.done()
    view = _merge(full, light)
    assert view[0].tolist() == scannet.train_recipe(B).tolist()
    index = np.tile(np.arange(N, dtype=np.int32), (B, 1))
    ref = scannet.ScanReference(index, view[0][None], [objfeed.Reference(index, *view)])
    pts, label, inner = scannet.apply_reference(_as_blocks(x, lab, inn), np.arange(B), ref)
    want = golden["train_out_input"]
    assert pts.shape == (1, B, N, 6) and want.dtype == np.float32
    assert np.array_equal(label, golden["train_out_label"]) and np.array_equal(inner, golden["train_out_inner"])
    assert np.array_equal(pts[0, :, :, 3:6], want[:, :, 3:6].astype(np.float64))                  # rgb: copied
    worst = max(_check_chain(pts[0, b, :, 0:3], want[b, :, 0:3], x[b, :, 0:3], [view], b) for b in range(4))
    for b in (4, 5):                                                                               # the last third: unchanged
        assert np.array_equal(pts[0, b], x[b].astype(np.float64)) and np.array_equal(want[b], x[b])
    for b in range(4):
        assert not np.array_equal(want[b, :, 0:3], x[b, :, 0:3])
    print("training recipe: worst error / bound %.3f" % worst)


def test_the_statement_reproduces_the_references_evaluation_chain(golden):
    """evaluate_scannet_withoverlap.py's augment_fn1 on the plain batch, then augment_fn2 on what it left: views 1 and 2 of
    EVAL_VIEWS, each computed from the view before it; view 0 is the plain batch"""
    B, N = 6, 16
    inp = golden["input"]
    t1, t2 = _Take(golden["eval1_random"]), _Take(golden["eval2_random"])
    plain = _recorded_view(_Take(np.zeros(0)), 0, [], B, N)
    v1 = _recorded_view(t1, scannet.EVAL_VIEWS[1], list(range(B)), B, N)
    v2 = _recorded_view(t2, scannet.EVAL_VIEWS[2], list(range(B)), B, N)
    assert t1.done() and t2.done()
    index = np.tile(np.arange(N, dtype=np.int32), (B, 1))
    views = [plain, v1, v2]
    ref = scannet.ScanReference(index, np.stack([v[0] for v in views]), [objfeed.Reference(index, *v) for v in views])
    assert ref.recipes.tolist() == scannet.eval_recipes(scannet.EVAL_VIEWS, B).tolist()
    blocks = _as_blocks(inp, golden["label"], golden["inner"])
    pts, label, inner = scannet.apply_reference(blocks, np.arange(B), ref)
    assert pts.shape == (3, B, N, 6) and np.array_equal(pts[0], inp.astype(np.float64))
    assert np.array_equal(label, golden["label"]) and np.array_equal(inner, golden["inner"])
    worst1 = max(_check_chain(pts[1, b, :, 0:3], golden["eval1_out"][b, :, 0:3], inp[b, :, 0:3], [v1], b) for b in range(B))
    worst2 = max(_check_chain(pts[2, b, :, 0:3], golden["eval2_out"][b, :, 0:3], inp[b, :, 0:3], [v1, v2], b) for b in range(B))
    for v in range(3):
        assert np.array_equal(pts[v, :, :, 3:6], inp[:, :, 3:6].astype(np.float64))
    # view 2 sits ON TOP of view 1: from the reference's own view 1 (base=) one view's bound suffices, and fn2 applied to the
    # plain batch would be far off
    base = np.stack([inp, golden["eval1_out"], golden["eval2_out"]])
    step, _l, _i = scannet.apply_reference(blocks, np.arange(B), ref, base=base)
    for b in range(B):
        _check_chain(step[2, b, :, 0:3], golden["eval2_out"][b, :, 0:3], golden["eval1_out"][b, :, 0:3], [v2], b)
    alone = scannet.ScanReference(index, v2[0][None], [objfeed.Reference(index, *v2)])
    off = scannet.apply_reference(blocks, np.arange(B), alone)[0][0]
    assert np.abs(off[:, :, 0:3] - golden["eval2_out"][:, :, 0:3]).max() > 1e-2
    print("evaluation chain: worst error / bound %.3f (view 1), %.3f (view 2)" % (worst1, worst2))


# ---------------------------------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------------------------------
def test_the_view_keys():
    for seed, step, b in ((1, 0, 0), (0xfedcba9876543210, (1 << 40) + 3, 6)):
        ck = feed.cloud_key(seed, step, b)
        assert scannet.view_key(ck, 0) == ck
        keys = [int(scannet.view_key(ck, v)) for v in range(4)]
        assert len(set(keys)) == 4
        for v in (1, 2, 3):
            z = (int(ck) + v + 0x9e3779b97f4a7c15) & 0xffffffffffffffff
            z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & 0xffffffffffffffff
            z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & 0xffffffffffffffff
            assert keys[v] == z ^ (z >> 31)
    with pytest.raises(ValueError):
        scannet.view_key(1, -1)


def test_one_view_draws_what_objfeed_draws_and_the_index_does_not_depend_on_the_recipes():
    ids = np.array([6, 0, 3, 5, 1, 2, 4], dtype=np.int32)
    recipe = np.array([0, 31, 30, 3, 16, 12, 5], dtype=np.int32)
    for N in (1, 64, 257):
        for seed, step in ((1, 0), (0xfedcba9876543210, (1 << 40) + 3)):
            one = scannet.assemble_reference(SIZES, ids, N, seed, step, recipe)
            obj = objfeed.assemble_reference(SIZES, ids, N, seed, step, recipe)
            assert len(one.views) == 1 and one.recipes.tolist() == [recipe.tolist()]
            for x, y in zip(one.views[0], obj):
                assert np.array_equal(x, y)
            want = feed.assemble_reference(SIZES, ids, N, seed, step, False).index
            assert one.index.dtype == np.int32 and np.array_equal(one.index, want)
            three = scannet.assemble_reference(SIZES, ids, N, seed, step, np.stack([recipe, recipe[::-1], recipe]))
            assert np.array_equal(three.index, want) and all(np.array_equal(v.index, want) for v in three.views)
            # view 0 of many is the one-view launch; a later view with the same masks draws other numbers
            for x, y in zip(three.views[0], one.views[0]):
                assert np.array_equal(x, y)
            assert three.views[2].theta[1] != three.views[0].theta[1] and three.views[2].scale[1] != three.views[0].scale[1]
            assert not np.array_equal(three.views[2].noise[1], three.views[0].noise[1])
            again = scannet.assemble_reference(SIZES, ids, N, seed, step, np.stack([recipe, recipe[::-1], recipe]))
            for a, b in zip(three.views, again.views):
                assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_apply_reference_chains_the_views():
    rng = np.random.RandomState(0)
    blocks = [np.concatenate([rng.rand(n, 6), rng.randint(0, 21, (n, 1)), rng.randint(0, 2, (n, 1))], axis=1).astype(np.float32)
              for n in (5, 40)]
    ref = scannet.assemble_reference([5, 40], [1, 0], 16, 2, 3, [[0, S], [S, 0], [H, S]])
    pts, label, inner = scannet.apply_reference(blocks, [1, 0], ref)
    src = [blocks[1][ref.index[0]], blocks[0][ref.index[1]]]
    assert np.array_equal(pts[0, 0, :, 0:3], src[0][:, 0:3].astype(np.float64))
    assert np.array_equal(pts[1, 0, :, 0:3], pts[0, 0, :, 0:3] * ref.views[1].scale[0])
    assert np.array_equal(pts[2, 0, :, 0:3], pts[1, 0, :, 0:3] + ref.views[2].shift[0])
    assert np.array_equal(pts[1, 1], pts[0, 1])                                        # mask 0: the previous view
    assert np.array_equal(pts[2, 1, :, 0:3], pts[1, 1, :, 0:3] * ref.views[2].scale[1])
    for v in range(3):
        assert np.array_equal(pts[v, 0, :, 3:6], src[0][:, 3:6].astype(np.float64))
    assert np.array_equal(label[1], src[1][:, 6].astype(np.int32)) and np.array_equal(inner[0], src[0][:, 7].astype(np.int32))
    base = rng.rand(3, 2, 16, 6).astype(np.float32)
    stepwise = scannet.apply_reference(blocks, [1, 0], ref, base=base)[0]
    assert np.array_equal(stepwise[0], pts[0])
    assert np.array_equal(stepwise[1, 0, :, 0:3], base[0, 0, :, 0:3].astype(np.float64) * ref.views[1].scale[0])
    assert np.array_equal(stepwise[2, 1, :, 0:3], base[1, 1, :, 0:3].astype(np.float64) * ref.views[2].scale[1])


# ---------------------------------------------------------------------------------------------------------------
# the vote loop
# ---------------------------------------------------------------------------------------------------------------
def _pool_columns(blocks):
    rows = np.concatenate(blocks)
    return [len(b) for b in blocks], rows[:, 6].copy(), rows[:, 7].copy(), np.concatenate(([0], np.cumsum([len(b) for b in blocks])))


def test_three_identical_views_are_the_plain_vote_with_two_votes():
    """with the same small-integer logits in all three views the fp32 sums are exact: counts / 3, coverage, passes and
    predictions equal evalvote.vote_reference(min_votes=2), the sums are three times its sums"""
    sizes, label, inner, offsets = _pool_columns(cases.blocks())
    ids = np.array([2, 0, 3, 5], dtype=np.int32)
    base = offsets[ids][:, None]
    fn = lambda _q, index: cases.toy_logits(base + index, 0)
    three = scannet.scan_vote_reference(sizes, label, inner, ids, cases.NUM_POINT, 4, 2, fn, cases.C, max_passes=cases.MAX_PASSES)
    plain = evalvote.vote_reference(sizes, label, inner, ids, cases.NUM_POINT, 4, 2, fn, cases.C, min_votes=2,
                                    max_passes=cases.MAX_PASSES)
    assert three.complete and plain.complete and three.passes == plain.passes < cases.MAX_PASSES
    assert np.array_equal(three.covered, plain.covered) and np.array_equal(three.inner_size, plain.inner_size)
    for k in range(len(ids)):
        assert (three.count[k] % 3 == 0).all() and np.array_equal(three.count[k] // 3, plain.count[k])
        assert np.array_equal(three.votes[k], plain.votes[k] * np.float32(3.0))
        assert np.array_equal(three.pred[k], plain.pred[k])
    assert np.array_equal(three.confusion, plain.confusion)


def test_the_loop_is_the_references_loop():
    """a literal transcription of evaluate_scannet_withoverlap.py:263-302,314 around this project's draws: one sample per draw,
    `count[sample_index] += 1`, coverage `count > 1` over the inner rows, three `pred_sum[sample_index] += pred_val`"""
    sizes, label, inner, offsets = _pool_columns(cases.blocks())
    ids = np.array([1, 4, 2], dtype=np.int32)
    N, seed, batch_index = cases.NUM_POINT, 9, 5
    base = offsets[ids][:, None]
    fn = lambda q, index: cases.toy_logits(base + index, q % 3) + np.float32(q // 3 % 2)
    got = scannet.scan_vote_reference(sizes, label, inner, ids, N, seed, batch_index, fn, cases.C, max_passes=cases.MAX_PASSES)
    bsize = len(ids)
    pred_sum = [np.zeros((sizes[i], cases.C), dtype=np.float32) for i in ids]
    sample_count = [np.zeros((sizes[i],), dtype=np.int32) for i in ids]
    inner_label = [inner[offsets[i]:offsets[i + 1]] for i in ids]
    inner_size = np.array([(m == 1).sum() for m in inner_label])
    inner_covered = np.zeros((bsize,), np.int32)
    draws = 0
    while any(inner_covered < inner_size):
        sample_index = evalvote.draw_index(sizes, ids, N, seed, evalvote.pass_step(batch_index, draws))
        for b in range(bsize):
            sample_count[b][sample_index[b]] += 1
            inner_covered[b] = np.sum(sample_count[b][inner_label[b] == 1] > 1)
        for a in range(3):
            pred_val = fn(3 * draws + a, sample_index)
            for b in range(bsize):
                pred_sum[b][sample_index[b]] += pred_val[b, ...]
        draws += 1
    assert got.complete and got.passes == draws < cases.MAX_PASSES
    for b in range(bsize):
        assert np.array_equal(got.votes[b].view(np.int32), pred_sum[b].view(np.int32))
        assert np.array_equal(got.count[b], 3 * sample_count[b])
        assert np.array_equal(got.pred[b], np.argmax(pred_sum[b], 1))
    assert np.array_equal(got.covered, inner_covered)


def test_the_loop_refuses_what_does_not_fit_the_pass_number():
    sizes, label, inner, _o = _pool_columns(cases.blocks())
    fn = lambda q, index: np.zeros(index.shape + (cases.C,), np.float32)
    for kw in (dict(views=0), dict(views=5), dict(min_draws=0), dict(max_passes=0), dict(max_passes=(1 << 20) // 3 + 1)):
        with pytest.raises(ValueError):
            scannet.scan_vote_reference(sizes, label, inner, [0], cases.NUM_POINT, 1, 0, fn, cases.C, **kw)
    capped = scannet.scan_vote_reference(sizes, label, inner, [2], cases.NUM_POINT, 1, 0, fn, cases.C, max_passes=3)
    assert capped.passes == 3 and not capped.complete and (capped.count[0] % 3 == 0).all()


def test_every_evaluation_of_the_gpu_tests_completes_inside_its_cap():
    """the exact pools, seeds and max_passes of tests/test_gpu_scaneval.py in the statement: complete, with passes to spare"""
    blocks = cases.blocks()
    sizes, label, inner, offsets = _pool_columns(blocks)
    fn = cases.logits_fn(offsets, cases.pool_batch_ids)
    res = scannet.evaluate_reference(fn, sizes, label, inner, cases.BATCH, cases.NUM_POINT, cases.SEED, cases.C,
                                     max_passes=cases.MAX_PASSES, keep_votes=True)
    assert res.batches == [0, 1] and res.complete and all(2 <= p < cases.MAX_PASSES for p in res.passes)
    assert len(res.votes[1].votes) == 2                                                # the last batch is the smaller one
    empty = scannet.scan_vote_reference(sizes, label, inner, cases.EMPTY_IDS, cases.NUM_POINT, cases.SEED, cases.EMPTY_BATCH_INDEX,
                                        lambda q, index: fn(cases.EMPTY_BATCH_INDEX, q, index), cases.C, max_passes=cases.MAX_PASSES)
    assert empty.complete and 2 <= empty.passes < cases.MAX_PASSES and empty.inner_size[1] == 0 and empty.votes[1].shape == (0, cases.C)
    zeros = lambda q, index: np.zeros(index.shape + (cases.C,), np.float32)            # (coverage does not depend on the logits)
    views = scannet.scan_vote_reference(sizes, label, inner, cases.VIEW_IDS, cases.NUM_POINT, cases.SEED, cases.VIEW_BATCH_INDEX, zeros,
                                        cases.C, max_passes=cases.MAX_PASSES)
    assert views.complete and 2 <= views.passes < cases.MAX_PASSES
    two = scannet.scan_vote_reference(sizes, label, inner, [2], cases.NUM_POINT, cases.SEED, 1, zeros, cases.C, max_passes=2)
    assert not two.complete and two.count[0].max() == 6                                # (the capped run the GPU test makes on purpose)
    sblocks, index, sob, scenes = cases.scenes()
    assert len(scenes) == 2 and max(len(b) for b in sblocks) <= 400 and len(sblocks) >= 3
    ssizes, slabel, sinner, soffsets = _pool_columns(sblocks)
    table = cases.scene_batch_ids(sob)
    res = scannet.evaluate_scenes_reference(cases.logits_fn(soffsets, lambda i: table[i]), ssizes, slabel, sinner, np.concatenate(index),
                                            sob, scenes, cases.SCENE_BATCH, cases.NUM_POINT, cases.SCENE_SEED, cases.C,
                                            max_passes=cases.MAX_PASSES)
    assert all(res.complete) and res.block.complete and all(2 <= p < cases.MAX_PASSES for p in res.block.passes)
    assert sum(res.unseen_rows) == 0
    # .. and the plain two-vote loop scenemerge.evaluate_scenes runs on the same scenes by default
    plain = scenemerge.evaluate_scenes_reference(lambda i, p, idx: zeros(p, idx), ssizes, slabel, sinner, np.concatenate(index), sob,
                                                 scenes, cases.SCENE_BATCH, cases.NUM_POINT, cases.SCENE_SEED, cases.C, min_votes=2,
                                                 max_passes=cases.MAX_PASSES)
    assert all(plain.complete) and all(p < cases.MAX_PASSES for p in plain.block.passes)


def test_merged_ranks_equal_one_rank():
    sizes, label, inner, offsets = _pool_columns(cases.blocks())
    fn = cases.logits_fn(offsets, lambda i: evalvote.batch_blocks(len(sizes), 2, i))
    run = lambda rank, world: scannet.evaluate_reference(fn, sizes, label, inner, 2, cases.NUM_POINT, cases.SEED, cases.C,
                                                         max_passes=cases.MAX_PASSES, rank=rank, world=world, keep_votes=True)
    one = run(0, 1)
    assert one.batches == [0, 1, 2] and one.complete
    for world in (2, 3):
        merged = evalvote.EvalResult.merge([run(r, world) for r in reversed(range(world))])
        assert merged.batches == one.batches and merged.passes == one.passes and merged.complete
        assert np.array_equal(merged.confusion, one.confusion) and merged.nonfinite_rows == one.nonfinite_rows
        for c, s, c1, s1 in zip(merged.covered, merged.inner_size, one.covered, one.inner_size):
            assert np.array_equal(c, c1) and np.array_equal(s, s1)
        for i in one.batches:
            for a, b in zip(merged.votes[i].votes, one.votes[i].votes):
                assert np.array_equal(a.view(np.int32), b.view(np.int32))
        m, o = scannet.scannet_metrics(merged.confusion), scannet.scannet_metrics(one.confusion)
        assert m.miou == o.miou and m.overall_acc == o.overall_acc and m.mean_class_acc == o.mean_class_acc


# ---------------------------------------------------------------------------------------------------------------
# the figures
# ---------------------------------------------------------------------------------------------------------------
def test_the_sub20_figures_on_a_hand_counted_matrix():
    cm = np.zeros((21, 21), np.int64)
    cm[1, 1], cm[1, 0], cm[0, 1] = 5, 2, 3            # wall: 7 seen, 9 predicted (3 of them labelled other20), union 11
    cm[2, 2], cm[2, 1] = 4, 1                         # floor: 5 seen, 6 predicted, union 7
    cm[19, 19] = 1                                    # bathtub: 1 / 1
    cm[20, 20], cm[20, 2] = 6, 2                      # otherfurniture: 8 seen, 6 predicted, union 8
    cm[0, 0] = 7
    m = scannet.scannet_metrics(cm)
    assert m.classes == scannet.SUB20 and m.class_iou.shape == (21,) and m.class_acc.shape == (21,)
    close = lambda a, b: abs(a - b) < 1e-12
    assert close(m.class_iou[1], 5 / 11) and close(m.class_acc[1], 5 / 7)         # class 0's row and column are in the union
    assert close(m.class_iou[2], 4 / 7) and close(m.class_acc[2], 4 / 5)
    assert close(m.class_iou[19], 1.0) and close(m.class_iou[20], 6 / 8) and m.class_iou[3] == 0.0
    assert close(m.miou, (5 / 11 + 4 / 7 + 1) / 19) and close(m.mean_class_acc, (5 / 7 + 4 / 5 + 1) / 19)
    assert m.overall_acc == 10 / 13                                                 # (5 + 4 + 1) / (7 + 5 + 1)
    # class 0 does not enter the means or the overall accuracy: its diagonal and its seen count may be anything
    cm2 = cm.copy()
    cm2[0, 0] = 1000
    m2 = scannet.scannet_metrics(cm2)
    assert m2.miou == m.miou and m2.mean_class_acc == m.mean_class_acc and m2.overall_acc == m.overall_acc
    # but its row and column are in the other classes' unions
    cm3 = cm.copy()
    cm3[0, 1] = 0
    assert close(scannet.scannet_metrics(cm3).class_iou[1], 5 / 8)
    bench = scannet.scannet_metrics(cm, scannet.BENCHMARK20)
    assert close(bench.miou, (5 / 11 + 4 / 7 + 1 + 6 / 8) / 20) and bench.overall_acc == 16 / 21
    assert close(bench.mean_class_acc, (5 / 7 + 4 / 5 + 1 + 6 / 8) / 20)
    # evalvote.metrics averages over all 21 classes: not these figures
    assert not close(evalvote.metrics(cm).miou, m.miou)
    assert np.isnan(scannet.scannet_metrics(np.zeros((21, 21)), (3,)).overall_acc)
    for bad in ((), (21,), (1, 1), (-1,)):
        with pytest.raises(ValueError):
            scannet.scannet_metrics(cm, bad)


def test_predictions_round_trip_through_their_files(tmp_path):
    pred = {0: dict(pred_full=np.array([40, 1, 39, -1, 14], np.int32)), 2: dict(pred_full=None), 1: dict(pred_full=np.array([2], np.int32))}
    res = scenemerge.SceneResult(np.zeros((21, 21)), np.zeros((21, 21)), None, [0, 1, 2], [0] * 3, [0] * 3, [0] * 3, [True] * 3, pred)
    paths = scannet.write_predictions(str(tmp_path / "out"), ["scene0000_00", "scene0001_00", "scene0002_00"], res)
    assert [os.path.basename(p) for p in paths] == ["scene0000_00.txt", "scene0001_00.txt"]
    assert open(paths[0]).read() == "40\n1\n39\n-1\n14\n"
    assert np.array_equal(scannet.read_predictions(paths[0]), pred[0]["pred_full"])
    assert np.array_equal(scannet.read_predictions(paths[1]), pred[1]["pred_full"])
    res.pred = None
    with pytest.raises(ValueError):
        scannet.write_predictions(str(tmp_path / "out"), ["a", "b", "c"], res)
