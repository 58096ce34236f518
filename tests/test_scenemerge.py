"""harness/scenemerge.py without a GPU: the numpy statement of the scene-level evaluation against the reference's formulas in
float64 (post-merging/s3dis_merge.m), the pool's scene index and its validation, and the independence of the world size.

The bound on the probabilities is the project's parity bound for activations, 1e-5 absolute (README "Parity"); on a merged
scene row it is that bound times the row's hit count (one fp32 add per hit, each term within the bound)."""
import os

import numpy as np
import pytest

from sph3d_gcn_amd.harness import blockio, evalvote, feed, scenemerge as sm, scenesynth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-5


def _softmax64(v):
    v = np.asarray(v, dtype=np.float64)
    u = v / np.sqrt((v * v).sum(axis=1, keepdims=True))
    e = np.exp(u)
    return e / e.sum(axis=1, keepdims=True)


def test_parse_block_index_round_trips():
    rng = np.random.RandomState(0)
    n = 37
    xyz, rgb = rng.rand(n, 3).astype(np.float32), rng.rand(n, 3).astype(np.float32)
    seg, inner = rng.randint(0, 13, n), rng.randint(0, 2, n)
    index = rng.permutation(1000)[:n].astype(np.int32)
    rec = blockio.encode_block(xyz, rgb, seg, inner, index_label=index, scene_idx=7)
    got, scene = blockio.parse_block_index(rec)
    assert got.dtype == np.int32 and np.array_equal(got, index) and scene == 7
    assert blockio.parse_block(rec).shape == (n, 8)
    bad = blockio.encode_block(xyz, rgb, seg, inner, index_label=index[:-1], scene_idx=7)
    with pytest.raises(ValueError):
        blockio.parse_block_index(bad)


def _two_blocks():
    a = np.zeros((4, 8), np.float32)
    a[:, 7] = [1, 1, 0, 0]
    return [a, a.copy(), a.copy()]


def test_pool_validation_refuses_what_the_merge_cannot_state():
    blocks = _two_blocks()
    good = [np.array([0, 1, 1, 1]), np.array([2, 3, 0, 0]), np.array([4, 5, 6, 7])]
    index, scene = feed.check_scene_index(blocks, good, [0, 0, 1])          # outer rows may repeat
    assert index.dtype == np.int32 and index.tolist() == [0, 1, 1, 1, 2, 3, 0, 0, 4, 5, 6, 7] and scene.tolist() == [0, 0, 1]
    cases = {"duplicate inner": ([np.array([1, 1, 2, 3]), good[1], good[2]], [0, 0, 1]),
             "not consecutive": (good, [0, 1, 0]),
             "negative": ([np.array([0, 1, -1, 2]), good[1], good[2]], [0, 0, 1]),
             "length": ([np.array([0, 1, 2]), good[1], good[2]], [0, 0, 1])}
    for name, (idx, sob) in cases.items():
        with pytest.raises(ValueError):
            feed.check_scene_index(blocks, idx, sob)
        with pytest.raises(ValueError):                                      # the pool refuses before it touches a device
            feed.BlockPool(blocks, "cpu", idx, sob)
    with pytest.raises(ValueError):
        feed.BlockPool(blocks, "cpu", index=good)
    pool = feed.BlockPool(blocks, "cpu", good, [0, 0, 1])
    assert pool.index.tolist() == index.tolist() and pool.scene_of_block.tolist() == [0, 0, 1]
    plain = feed.BlockPool(blocks, "cpu")
    assert plain.index is None and plain.scene_of_block is None


def test_pool_from_records_numbers_scenes_by_file(tmp_path):
    rng = np.random.RandomState(1)
    paths, want = [], []
    for s, sizes in enumerate([[5, 7], [3]]):
        recs = []
        for n in sizes:
            index = rng.permutation(50)[:n]
            want.append(index)
            recs.append(blockio.encode_block(rng.rand(n, 3), rng.rand(n, 3), rng.randint(0, 13, n), rng.randint(0, 2, n),
                                             index_label=index, scene_idx=99))
        paths.append(str(tmp_path / ("scene%d.tfrecord" % s)))
        blockio.write_records(paths[-1], recs)
    pool = feed.BlockPool.from_records(paths, "cpu", with_index=True)
    assert pool.scene_of_block.tolist() == [0, 0, 1] and pool.index.tolist() == np.concatenate(want).tolist()
    assert feed.BlockPool.from_records(paths, "cpu").index is None


def test_exp32_coefficients_come_from_the_header():
    c = sm.exp32_coefficients()
    assert c.dtype == np.float32 and c.shape == (11,) and c[0] == 1 and c[2] == 0.5
    u = np.linspace(-1, 1, 20001).astype(np.float32)
    rel = np.abs(sm.exp32(u).astype(np.float64) / np.exp(u.astype(np.float64)) - 1).max()
    print("exp32 max relative error on [-1, 1]: %.3g" % rel)
    assert rel < 1e-6


def test_normalise_reference_holds_the_parity_bound_against_float64():
    rng = np.random.RandomState(2)
    worst = 0.0
    for C in (13, 21):
        sums = rng.randn(4000, C).astype(np.float32) * rng.randint(1, 30, (4000, 1)).astype(np.float32)
        dominant = rng.randn(2000, C).astype(np.float32)
        dominant[np.arange(2000), rng.randint(0, C, 2000)] += 50
        for v in (sums, dominant, sums * np.float32(1e-3), sums * np.float32(1e3)):
            p = sm.normalise_reference(v)
            assert p.dtype == np.float32 and p.shape == v.shape
            err = np.abs(p.astype(np.float64) - _softmax64(v)).max()
            worst = max(worst, err)
            assert err <= BOUND, err
    print("normalise_reference: max |p - float64| = %.3g" % worst)


def test_normalise_reference_skips_zero_and_non_finite_rows():
    v = np.ones((6, 5), np.float32)
    v[1] = 0
    v[2, 3] = np.nan
    v[3, 0] = np.inf
    v[4, 1] = -np.inf
    p, skipped = sm.normalise_reference(v, return_skipped=True)
    assert skipped.tolist() == [False, True, True, True, True, False]
    assert not p[skipped].any() and np.isfinite(p).all() and np.array_equal(p[0], p[5])
    merged, hits = np.zeros((6, 5), np.float32), np.zeros((6,), np.int32)
    a, o = sm.merge_update(merged, hits, v, [1, 1, 1, 0, 1, 1], [0, 1, 2, 3, 4, 9])
    assert (a, o) == (3, 1) and hits.tolist() == [1, 0, 0, 0, 0, 0]          # row 3 is not inner, row 5 lies outside the scene


def _scene_blocks(seed, C, full_points=30000):
    """a synthetic scene cut with the reference's geometry, and random vote sums for every block"""
    full_xyz, full_label, vx, vl = scenesynth.synthetic_scene(seed, full_points, extent=(3.0, 3.0, 2.0), num_cls=C)
    blocks, index = scenesynth.split_scene(vx, vl)
    rng = np.random.RandomState(seed + 100)
    votes = [(rng.randn(len(b), C) * rng.randint(1, 9)).astype(np.float32) for b in blocks]
    return full_xyz, full_label, vx, vl, blocks, index, votes


def test_merge_reference_against_the_matlab_loop_in_float64():
    C = 13
    _f, _fl, vx, _vl, blocks, index, votes = _scene_blocks(3, C)
    V = len(vx) + 5                                                          # five scene rows no block reaches
    votes[1][::7] = 0                                                        # skipped rows
    inner = [b[:, 7] for b in blocks]
    got = sm.merge_reference(votes, inner, index, V, C)
    # s3dis_merge.m:42-60, literally, in float64 (rows the statement skips would be NaN there: left out)
    predictions, hits = np.zeros((V, C)), np.zeros((V,), np.int64)
    skipped = 0
    for v, m, i in zip(votes, inner, index):
        in_index = (m == 1) & (np.abs(v).sum(axis=1) > 0)
        skipped += int(((m == 1) & ~in_index).sum())
        predictions[i[in_index]] = predictions[i[in_index]] + _softmax64(v[in_index])
        hits[i[in_index]] += 1
    assert hits.max() >= 3 and (hits == 0).sum() >= 5
    assert np.array_equal(got.hits, hits) and got.skipped_rows == skipped > 0 and got.out_of_scene == 0
    assert got.unseen_rows == int((hits == 0).sum())
    err = np.abs(got.merged.astype(np.float64) - predictions)
    print("merge_reference: max |merged - float64| = %.3g at up to %d hits" % (err.max(), hits.max()))
    assert (err <= BOUND * np.maximum(hits, 1)[:, None]).all()
    assert not got.merged[hits == 0].any() and (got.pred_voxel[hits == 0] == 0).all()
    clear = np.sort(predictions, axis=1)
    clear = (clear[:, -1] - clear[:, -2] > 1e-4) & (hits > 0)
    assert clear.sum() > 0.9 * (hits > 0).sum()
    assert np.array_equal(got.pred_voxel[clear], np.argmax(predictions, axis=1)[clear])
    # an index beyond the scene is counted and ignored
    cut = sm.merge_reference(votes, inner, index, len(vx) - 100, C)
    assert cut.out_of_scene > 0 and np.array_equal(cut.merged, got.merged[:len(vx) - 100])


def test_nearest_reference_equals_float64_brute_force_and_resolves_ties():
    rng = np.random.RandomState(4)
    ref, qry = rng.rand(700, 3).astype(np.float32), rng.rand(900, 3).astype(np.float32) * 1.4 - 0.2
    d = ((qry[:, None, :].astype(np.float64) - ref[None].astype(np.float64)) ** 2).sum(axis=2)
    two = np.sort(d, axis=1)[:, :2]
    assert ((two[:, 1] - two[:, 0]) > 1e-6 * two[:, 1]).all()                # no near-ties in this input
    assert np.array_equal(sm.nearest_reference(ref, qry, chunk_elements=5000), np.argmin(d, axis=1))
    # hand-made ties: exact duplicates and points at equal distance on both sides of a query
    ref = np.array([[5, 5, 5], [1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, 2, 0], [0, -2, 0], [5, 5, 5]], np.float32)
    qry = np.array([[0, 0, 0], [5, 5, 5], [0, 0.5, 0], [0, 8, 0]], np.float32)
    assert sm.nearest_reference(ref, qry).tolist() == [1, 0, 1, 4]
    # non-finite points: such a query gets -1, such a reference point is never chosen
    ref[1, 1] = np.nan
    ref[3, 0] = np.inf
    qry[3, 2] = np.nan
    assert sm.nearest_reference(ref, qry).tolist() == [2, 0, 2, -1]
    assert sm.nearest_reference(np.zeros((0, 3)), qry).tolist() == [-1] * 4
    assert sm.nearest_reference(np.full((3, 3), np.nan), qry).tolist() == [-1] * 4
    assert sm.nearest_reference(ref, np.zeros((0, 3))).shape == (0,)


def test_lift_reference_maps_labels_and_counts_the_full_cloud():
    pred_voxel = np.array([2, 0, 1, 2], np.int32)
    idx = np.array([0, 3, -1, 1, 2, 2], np.int32)
    label = np.array([2, 1, 0, 0, 7, 1], np.int32)
    full, conf = sm.lift_reference(pred_voxel, idx, label, num_cls=3)
    assert full.tolist() == [2, 2, -1, 0, 1, 1]
    want = np.zeros((3, 3), np.int64)
    want[2, 2] = want[1, 2] = want[0, 0] = want[1, 1] = 1                    # idx -1 and label 7 are not counted
    assert np.array_equal(conf, want)
    mapped, conf2 = sm.lift_reference(pred_voxel, idx, label, label_map=[40, 1, 2], num_cls=3)
    assert mapped.tolist() == [2, 2, -1, 40, 1, 1] and np.array_equal(conf2, want)
    assert sm.lift_reference(pred_voxel, idx, num_cls=3).tolist() == full.tolist()


def _pool_of_scenes(C, counts=(30000, 2500, 9000)):
    """three scenes with differing block counts, the second a single block -> host pool pieces and Scene objects"""
    blocks, index, sob, scenes = [], [], [], []
    for s, n in enumerate(counts):
        ext = [(3.0, 2.4, 2.0), (1.2, 1.2, 1.0), (2.4, 1.4, 2.0)][s]
        full_xyz, full_label, vx, vl = scenesynth.synthetic_scene(10 + s, n, extent=ext, num_cls=C)
        b, i = scenesynth.split_scene(vx, vl)
        blocks += b
        index += i
        sob += [s] * len(b)
        scenes.append(sm.Scene(vx, vl, None if s == 2 else full_xyz, None if s == 2 else full_label))
    return blocks, index, sob, scenes


def test_evaluate_scenes_reference_does_not_depend_on_the_world_size():
    C, N, seed, bs = 13, 256, 5, 4
    blocks, index, sob, scenes = _pool_of_scenes(C)
    per_scene = np.bincount(sob)
    assert per_scene[1] == 1 and len(set(per_scene.tolist())) == 3
    sizes = [len(b) for b in blocks]
    rows = np.concatenate(blocks)
    w = np.random.RandomState(0).randn(6, C).astype(np.float32)

    first_block, first_batch = sm.scene_plan(sob, len(scenes), bs)
    batch_ids = {int(first_batch[s]) + j: ids for s in range(len(scenes)) for j, ids in enumerate(sm.scene_batches(first_block, s, bs))}

    def logits_fn(i, p, idx):
        out = np.zeros(idx.shape + (C,), np.float32)
        for k, b in enumerate(batch_ids[i]):
            out[k] = blocks[b][idx[k], 0:6] @ w + np.float32(np.cos(0.3 * i + p))
        return out
    args = (logits_fn, sizes, rows[:, 6], rows[:, 7], np.concatenate(index), sob, scenes, bs, N, seed, C)
    one = sm.evaluate_scenes_reference(*args, keep_pred=True)
    assert one.scenes == [0, 1, 2] and all(one.complete) and one.block.batches == list(range(int(first_batch[-1])))
    assert one.confusion_full.sum() == len(scenes[0].full_xyz) + len(scenes[1].full_xyz)
    assert one.confusion_voxel.sum() == sum(len(s.voxel_xyz) for s in scenes)
    assert one.pred[2]["idx"] is None and one.pred[2]["pred_full"] is None and sum(one.unseen_rows) == 0
    assert 0 <= one.full.miou <= 1 and one.block.confusion.sum() == int((rows[:, 7] == 1).sum())
    for world in (2, 3):
        parts = [sm.evaluate_scenes_reference(*args, rank=r, world=world, keep_pred=True) for r in range(world)]
        got = sm.SceneResult.merge(parts[::-1])
        assert got.scenes == one.scenes and got.complete == one.complete
        assert np.array_equal(got.confusion_full, one.confusion_full) and np.array_equal(got.confusion_voxel, one.confusion_voxel)
        assert np.array_equal(got.block.confusion, one.block.confusion) and got.block.passes == one.block.passes
        assert got.block.batches == one.block.batches and got.full.miou == one.full.miou
        assert got.unseen_rows == one.unseen_rows and got.skipped_rows == one.skipped_rows and got.out_of_scene == one.out_of_scene
        for s in one.scenes:
            for key in ("merged", "hits", "pred_voxel", "pred_full", "idx"):
                a, b = one.pred[s][key], got.pred[s][key]
                assert (a is None and b is None) or a.tobytes() == b.tobytes(), (s, key)
    with pytest.raises(ValueError):
        sm.SceneResult.merge([one, one])


def test_scene_entries_are_declared_exported_and_bound():
    import ctypes
    import re
    from sph3d_gcn_amd import _lib
    header = open(os.path.join(ROOT, "include", "sph3d.h")).read()
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sph3d_scene_merge", "sph3d_scene_finalize", "sph3d_scene_lift", "sph3d_nn1", "sph3d_nn1_workspace"):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(l, name) and name in _lib.SIGNATURES
    src = open(os.path.join(ROOT, "sph3d_gcn_amd", "csrc", "scene.hip")).read()
    assert not re.search(r"atomicAdd\(\s*&?\s*(merged|dst)", src) and "unsafeAtomicAdd" not in src and "hipMalloc" not in src
    lib = _lib.lib()
    # host-side validation answers without a device; workspace: header + cell ends + 16 B per reference point
    assert lib.sph3d_nn1_workspace(0, 5) == 0 and lib.sph3d_nn1_workspace(300000, 10 ** 6) >= 300000 * 16 + 150000 * 4
    assert lib.sph3d_nn1(0, 5, None, None, 0, None, None, 0, None) == -1 and b"0<V,F" in lib.sph3d_last_error()
    assert lib.sph3d_nn1(5, 5, None, None, 2, None, None, 0, None) == -1 and b"mode" in lib.sph3d_last_error()
    assert lib.sph3d_scene_merge(1, 65, 1, 1, None, None, None, None, 0, 1, None, 1, None, None, None, None) == -1
    assert b"classes" in lib.sph3d_last_error()
    assert lib.sph3d_scene_merge(1, 13, 1, 10, None, None, None, None, 5, 6, None, 1, None, None, None, None) == -1
    assert b"not a range" in lib.sph3d_last_error()
    assert lib.sph3d_scene_finalize(13, 0, None, None, None, None, None, None, None) == -1
    assert lib.sph3d_scene_lift(13, 4, 0, None, None, None, None, None, None, None) == -1
