"""harness/facadefeed.py without a GPU: the record of a facade split, the numpy statement of its batches — the draws are
objfeed's, the normal turns with the cloud — against the reference's own with-normal functions through their recorded inputs,
random numbers and outputs (tests/golden/facade_ref.npz, written by tests/golden/make_facade_golden.py), the recipes, and the
epoch plan that visits every facade `repeat` times."""
import os

import numpy as np
import pytest

from sph3d_gcn_amd.harness import facadefeed, feed, objfeed

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "facade_ref.npz")
SIZES = [1, 2, 63, 64, 65, 500, 2047, 2048, 2049, 3000, 4097]
T, L = facadefeed.TURN, facadefeed.TILT


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _close(got, want, terms):
    """tests/test_objfeed.py's tolerance for objfeed_ref.npz: |got - want| <= 2^-23 * (sum of the magnitudes of the element's
    terms) — the reference keeps the z rotation's matrix and the results in float32"""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    bound = 2.0 ** -23 * terms
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    return float((err / np.maximum(bound, 1e-300)).max())


def test_the_float64_transform_reproduces_the_references_with_normal_functions(golden):
    """given the random numbers numpy handed out, facadefeed.transform gives what utils/data_util.py:64-105 gave, for xyz and
    for the normal"""
    src = golden["xyz_normal"]
    assert src.shape == (4, 16, 6) and src.dtype == np.float32
    a = np.abs(src.astype(np.float64))
    worst = {}
    u = golden["rotate_point_cloud_with_normal_random"]
    assert u.shape == (4,)
    want = golden["rotate_point_cloud_with_normal"]
    for b in range(4):
        theta = u[b] * 2 * np.pi
        xyz, nrm = facadefeed.transform(src[b, :, 0:3], src[b, :, 3:6], T, theta=theta)
        m = np.abs(objfeed.turn_matrix(theta))
        worst["turn xyz"] = max(worst.get("turn xyz", 0.0), _close(xyz, want[b, :, 0:3], np.dot(a[b, :, 0:3], m)))
        worst["turn normal"] = max(worst.get("turn normal", 0.0), _close(nrm, want[b, :, 3:6], np.dot(a[b, :, 3:6], m)))
        assert not np.array_equal(nrm, src[b, :, 3:6].astype(np.float64))
    z = golden["rotate_perturbation_point_cloud_with_normal_random"].reshape(4, 3)
    want = golden["rotate_perturbation_point_cloud_with_normal"]
    for b in range(4):
        angles = np.clip(objfeed.ANGLE_SIGMA * z[b], -objfeed.ANGLE_CLIP, objfeed.ANGLE_CLIP)
        xyz, nrm = facadefeed.transform(src[b, :, 0:3], src[b, :, 3:6], L, tilt=angles)
        m = np.abs(objfeed.tilt_matrix(*angles))
        worst["tilt xyz"] = max(worst.get("tilt xyz", 0.0), _close(xyz, want[b, :, 0:3], np.dot(a[b, :, 0:3], m)))
        worst["tilt normal"] = max(worst.get("tilt normal", 0.0), _close(nrm, want[b, :, 3:6], np.dot(a[b, :, 3:6], m)))
    print("worst error / bound per function:", worst)


def test_scale_shift_and_jitter_leave_the_normal_alone(golden):
    src = golden["xyz_normal"][0]
    kw = dict(theta=0.7, tilt=(0.1, -0.05, 0.18), scale=1.1, shift=(0.05, -0.1, 0.0), noise=np.full((16, 3), 0.01))
    n64 = src[:, 3:6].astype(np.float64)
    for mask in (0, 4, 8, 16, 28):
        xyz, nrm = facadefeed.transform(src[:, 0:3], src[:, 3:6], mask, **kw)
        assert np.array_equal(nrm, n64) and np.array_equal(xyz, objfeed.transform(src[:, 0:3], mask, **kw))
    xyz, nrm = facadefeed.transform(src[:, 0:3], src[:, 3:6], 31, **kw)
    assert np.array_equal(xyz, objfeed.transform(src[:, 0:3], 31, **kw))
    assert np.array_equal(nrm, np.dot(np.dot(n64, objfeed.turn_matrix(0.7)), objfeed.tilt_matrix(0.1, -0.05, 0.18)))
    # a rotation keeps the length
    assert np.abs(np.linalg.norm(nrm, axis=1) - np.linalg.norm(n64, axis=1)).max() < 1e-12


def _facade(seed, n):
    rng = np.random.RandomState(seed)
    normal = rng.randn(n, 3)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    return ((rng.rand(n, 3) * [6.0, 2.0, 9.0]).astype(np.float32), normal.astype(np.float32),
            (rng.rand(n, 3) * 2 - 1).astype(np.float32), rng.randint(0, 7, n).astype(np.int32))


def test_a_record_round_trips_bit_for_bit(tmp_path):
    facades = [_facade(1, 37), _facade(2, 1)]
    for f in facades:
        back = facadefeed.parse_facade(facadefeed.encode_facade(*f))
        for x, y in zip(f, back):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    path = str(tmp_path / "train_1.tfrecord")
    facadefeed.write_facade_records(path, facades)
    read = facadefeed.read_facade_records(path)
    assert len(read) == 2
    for f, g in zip(facades, read):
        for x, y in zip(f, g):
            assert x.tobytes() == y.tobytes()
    # the feature names are the record writer's
    from sph3d_gcn_amd.harness import blockio
    assert sorted(blockio.decode_example(facadefeed.encode_facade(*facades[0]))) == ["normal_raw", "rgb_raw", "seg_label", "xyz_raw"]
    with pytest.raises(ValueError):
        facadefeed.encode_facade(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), [])
    with pytest.raises(ValueError):
        facadefeed.encode_facade(np.zeros((4, 3)), np.zeros((3, 3)), np.zeros((4, 3)), np.zeros(4))


def test_facade_from_columns_centres_and_normalises_as_the_record_writer(tmp_path):
    rng = np.random.RandomState(5)
    n = 1000
    data = np.zeros((n, 10), dtype=np.float32)
    data[:, 0:3] = rng.rand(n, 3) * [12.0, 3.0, 9.0] + [100.0, -40.0, 7.0]
    data[:, 3:6] = rng.randint(0, 256, (n, 3))
    data[0, 3:6], data[1, 3:6] = 0, 255
    data[:, 6:9] = rng.randn(n, 3)
    data[:, 9] = rng.randint(0, 7, n)
    xyz, normal, rgb, label = facadefeed.facade_from_columns(data)
    assert xyz.dtype == normal.dtype == rgb.dtype == np.float32 and label.dtype == np.int32
    # the mean is formed and subtracted in fp32: what is left is the roundings of numpy's pairwise fp32 sum (at most
    # log2(n) = 10 of them on a path), of the division and of the subtraction, 2^-24 of the coordinates' magnitude each:
    # 12 * 2^-24 < 2^-20
    scale = np.abs(data[:, 0:2]).max()
    assert np.abs(xyz[:, 0:2].astype(np.float64).mean(axis=0)).max() <= 2.0 ** -20 * scale
    assert xyz[:, 2].min() == 0.0
    assert (rgb[0] == -1.0).all() and (rgb[1] == 1.0).all() and rgb.min() >= -1.0 and rgb.max() <= 1.0
    assert np.array_equal(normal, data[:, 6:9]) and np.array_equal(label, data[:, 9].astype(np.int32))
    # the reference's own expressions, in its order
    ref_xyz = data[:, 0:3].copy()
    center = np.mean(ref_xyz, axis=0)
    center[2] = np.amin(ref_xyz[:, 2], axis=0)
    ref_xyz -= center
    assert np.array_equal(xyz, ref_xyz) and np.array_equal(rgb, 2 * data[:, 3:6] / 255.0 - 1)
    # the text file: 10 comma-separated columns
    path = str(tmp_path / "split.txt")
    np.savetxt(path, data[:20], delimiter=",", fmt="%.9g")
    for x, y in zip(facadefeed.read_facade_txt(path), facadefeed.facade_from_columns(data[:20])):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        facadefeed.facade_from_columns(data[:, :9])


def test_facade_blocks_and_the_refusals():
    xyz, normal, rgb, label = _facade(3, 50)
    rows, nrm = facadefeed.facade_blocks(xyz, normal, rgb, label)
    assert rows.shape == (50, 8) and nrm.shape == (50, 4) and rows.dtype == nrm.dtype == np.float32
    assert np.array_equal(rows[:, 0:3], xyz) and np.array_equal(rows[:, 3:6], rgb) and np.array_equal(rows[:, 6], label)
    assert (rows[:, 7] == 1).all() and np.array_equal(nrm[:, 0:3], normal) and not nrm[:, 3].any()
    with pytest.raises(ValueError):
        facadefeed.facade_blocks(xyz[:0], normal[:0], rgb[:0], label[:0])
    with pytest.raises(ValueError):
        facadefeed.facade_blocks(xyz, normal[:, :2], rgb, label)
    bad = normal.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError):
        facadefeed.facade_blocks(xyz, bad, rgb, label)


def test_the_recipes():
    assert facadefeed.train_recipe(7).tolist() == [31, 31, 28, 28, 0, 0, 0]
    for B in (1, 2, 3, 16):
        third = B // 3
        assert facadefeed.train_recipe(B).tolist() == [31] * third + [28] * third + [0] * (B - 2 * third)
    assert facadefeed.EVAL_AUGMENT == T | L == 3 and facadefeed.train_recipe(3).dtype == np.int32


def test_the_index_does_not_depend_on_the_recipe_and_apply_reference_copies():
    ids = np.array([10, 0, 3, 9, 5, 1, 7], dtype=np.int32)
    blocks, normals = zip(*[facadefeed.facade_blocks(*_facade(40 + k, n)) for k, n in enumerate(SIZES)])
    for N in (64, 2048):
        for seed, step in ((1, 0), (0xfedcba9876543210, (1 << 40) + 3)):
            want = feed.assemble_reference(SIZES, ids, N, seed, step, False).index
            for recipe in (0, 31, facadefeed.EVAL_AUGMENT, [31, 28, 0, 3, 15, 16, 4]):
                ref = facadefeed.assemble_reference(SIZES, ids, N, seed, step, recipe)
                assert ref.index.dtype == np.int32 and np.array_equal(ref.index, want)
    ref = facadefeed.assemble_reference(SIZES, ids, 64, 3, 4, [31, 28, 0, 3, 15, 16, 4])
    pts, label = facadefeed.apply_reference(blocks, normals, ids, ref)
    assert pts.shape == (7, 64, 9) and pts.dtype == np.float64 and label.dtype == np.int32
    for b, mask in enumerate(ref.recipe):
        rows, nrm = blocks[ids[b]][ref.index[b]], normals[ids[b]][ref.index[b], 0:3]
        assert np.array_equal(pts[b, :, 6:9], rows[:, 3:6]) and np.array_equal(label[b], rows[:, 6].astype(np.int32))
        assert np.array_equal(pts[b, :, 0:3], objfeed.transform(rows[:, 0:3], int(mask), ref.theta[b], ref.tilt[b], ref.scale[b],
                                                                ref.shift[b], ref.noise[b]))
        if mask & 3:
            assert not np.array_equal(pts[b, :, 3:6], nrm)
            assert np.abs(np.linalg.norm(pts[b, :, 3:6], axis=1) - np.linalg.norm(nrm.astype(np.float64), axis=1)).max() < 1e-12
        else:
            assert np.array_equal(pts[b, :, 3:6], nrm)
        if mask == 0:
            assert np.array_equal(pts[b, :, 0:3], rows[:, 0:3])


def test_an_epoch_visits_every_facade_repeat_times():
    P, B, seed, repeat = 11, 4, (1 << 36) + 6, 3
    per = feed.batches_per_epoch(P * repeat, B)
    assert per == 9
    for epoch in range(2):
        whole = facadefeed.epoch_plan(P, B, seed, epoch, repeat=repeat)
        assert [s for s, _ in whole] == list(range(epoch * per, (epoch + 1) * per))          # steps continue across epochs
        assert [len(i) for _, i in whole] == [4] * 8 + [1]
        ids = np.concatenate([i for _, i in whole])
        assert ids.dtype == np.int32 and np.array_equal(np.bincount(ids, minlength=P), np.full(P, repeat))
        # it is the feed's plan over P * repeat virtual ids, v -> v % P
        virtual = feed.epoch_plan(P * repeat, B, seed, epoch)
        for (s, i), (sv, v) in zip(whole, virtual):
            assert s == sv and np.array_equal(i, v % P)
        # ranks partition the batches of one and the same plan
        for world in (2, 3):
            parts = [facadefeed.epoch_plan(P, B, seed, epoch, r, world, repeat) for r in range(world)]
            merged = sorted((s, tuple(i)) for part in parts for s, i in part)
            assert merged == [(s, tuple(i)) for s, i in whole]
            for r, part in enumerate(parts):
                assert [s % per for s, _ in part] == list(range(r, per, world))
    assert not np.array_equal(np.concatenate([i for _, i in facadefeed.epoch_plan(P, B, seed, 0, repeat=repeat)]),
                              np.concatenate([i for _, i in facadefeed.epoch_plan(P, B, seed, 1, repeat=repeat)]))
    assert len(facadefeed.epoch_plan(30, 16, 1, 0)) == feed.batches_per_epoch(30 * 100, 16)          # repeat = 100 by default
    with pytest.raises(ValueError):
        facadefeed.epoch_plan(P, B, seed, 0, repeat=0)


def test_the_feeds_hooks_leave_the_other_feeds_plan_alone():
    """TwoSetFeed's defaults: an epoch permutes one id per block and the table goes up as it is"""
    class Pool:
        def __len__(self):
            return 11
    f = feed.TwoSetFeed.__new__(feed.TwoSetFeed)
    f.pool, f.batch_size, f.rank, f.world = Pool(), 4, 0, 1
    table = np.arange(12, dtype=np.int32).reshape(3, 4)
    assert f._epoch_ids() == 11 and f._map_ids(table) is table and len(f) == 3
    g = facadefeed.FacadeFeed.__new__(facadefeed.FacadeFeed)
    g.pool, g.batch_size, g.rank, g.world, g.repeat = Pool(), 4, 1, 2, 3
    assert g._epoch_ids() == 33 and len(g) == 4 and g._map_ids(table + 20).tolist() == ((table + 20) % 11).tolist()
    assert g._map_ids(table).dtype == np.int32


def test_the_entry_validates_on_the_host():
    """sph3d_facadefeed_assemble refuses requests that describe no launch before touching a device"""
    import ctypes
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    none = [None] * 4
    assert l.sph3d_facadefeed_assemble(0, 64, 1, 8, None, None, None, None, 1, 1, *none, None) == -1
    assert b"B<=65535" in l.sph3d_last_error()
    assert l.sph3d_facadefeed_assemble(70000, 64, 1, 8, None, None, None, None, 1, 1, *none, None) == -1
    assert l.sph3d_facadefeed_assemble(2, 0, 1, 8, None, None, None, None, 1, 1, *none, None) == -1
    assert b"num_point>0" in l.sph3d_last_error()
    assert l.sph3d_facadefeed_assemble(2, 64, 0, 0, None, None, None, None, 1, 1, *none, None) == -1
    assert b"empty pool" in l.sph3d_last_error()
    assert l.sph3d_facadefeed_assemble(2, 64, 1, 8, None, None, None, None, 1, 1, *none, None) == -1
    assert b"null input" in l.sph3d_last_error()
    # host buffers stand in for device ones: every refusal comes before the launch
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p
    assert l.sph3d_facadefeed_assemble(2, 64, 1, 8, p(base), p(base), p(base), p(base), 1, 1, p(base), None, None, None, None) == -1
    assert b"null output" in l.sph3d_last_error()
    assert l.sph3d_facadefeed_assemble(2, 64, 1, 8, p(base + 4), p(base), p(base), p(base), 1, 1, p(base), p(base), p(base), None, None) == -1
    assert b"rows must be 16-byte aligned" in l.sph3d_last_error()
    assert l.sph3d_facadefeed_assemble(2, 64, 1, 8, p(base), p(base + 4), p(base), p(base), 1, 1, p(base), p(base), p(base), None, None) == -1
    assert b"normals must be 16-byte aligned" in l.sph3d_last_error()
    assert l.sph3d_facadefeed_assemble(65535, 1 << 20, 1, 8, p(base), p(base), p(base), p(base), 1, 1, p(base), p(base), p(base), None, None) == -1
    assert b"too large" in l.sph3d_last_error()
