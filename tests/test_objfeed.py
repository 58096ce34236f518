"""harness/objfeed.py without a GPU: the numpy statement of the object datasets' batches — its draws (the feed's sample, whatever
the recipe), the two datasets' recipes, the ranges of scale and shift, and its float64 arithmetic against the reference's own
functions through their recorded inputs, random numbers and outputs (tests/golden/objfeed_ref.npz, written by
tests/golden/make_objfeed_golden.py)."""
import os

import numpy as np
import pytest

from sph3d_gcn_amd.harness import feed, objfeed

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objfeed_ref.npz")
SIZES = [1, 2, 63, 64, 65, 500, 2047, 2048, 2049, 3000, 4097]
T, L, S, H, J = objfeed.TURN, objfeed.TILT, objfeed.SCALE, objfeed.SHIFT, objfeed.JITTER


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_assemble_reference_is_a_pure_function_and_its_index_is_the_feeds():
    ids = np.array([10, 0, 3, 9, 5, 1, 7], dtype=np.int32)
    for N in (64, 2048):
        for seed, step in ((1, 0), (0xfedcba9876543210, (1 << 40) + 3)):
            recipe = np.array([0, 31, 28, 3, 16, 12, 5], dtype=np.int32)
            a = objfeed.assemble_reference(SIZES, ids, N, seed, step, recipe)
            b = objfeed.assemble_reference(SIZES, ids, N, seed, step, recipe)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
            want = feed.assemble_reference(SIZES, ids, N, seed, step, False).index
            assert a.index.dtype == np.int32 and np.array_equal(a.index, want)
            for other in (0, 31, objfeed.EVAL_AUGMENT, recipe[::-1].copy()):
                assert np.array_equal(objfeed.assemble_reference(SIZES, ids, N, seed, step, other).index, want)
            # a transform's draw does not depend on the other bits of the mask either
            full = objfeed.assemble_reference(SIZES, ids, N, seed, step, 31)
            for k, m in enumerate(recipe):
                assert a.theta[k] == (full.theta[k] if m & T else 0.0)
                assert np.array_equal(a.tilt[k], full.tilt[k] if m & L else np.zeros(3))
                assert a.scale[k] == (full.scale[k] if m & S else 1.0)
                assert np.array_equal(a.shift[k], full.shift[k] if m & H else np.zeros(3))
                assert np.array_equal(a.noise[k], full.noise[k] if m & J else np.zeros((N, 3)))
            assert not np.array_equal(a.index, objfeed.assemble_reference(SIZES, ids, N, seed, step + 1, recipe).index)


def test_the_angles_and_the_noise_are_the_feeds_draws():
    """TURN, TILT and JITTER are feed.py's purposes 3, 4, 5: cloud b of a feed batch whose kind asks for them has the same numbers"""
    ids = np.arange(9, dtype=np.int32)
    f = feed.assemble_reference(SIZES, ids, 64, 7, 11, True)
    o = objfeed.assemble_reference(SIZES, ids, 64, 7, 11, 31)
    assert f.kind.tolist() == [1, 1, 1, 2, 2, 2, 0, 0, 0]
    assert np.array_equal(o.theta[:3], f.theta[:3]) and np.array_equal(o.tilt[:3], f.tilt[:3])
    assert np.array_equal(o.noise[3:6], f.noise[3:6])


@pytest.mark.parametrize("B", [1, 2, 3, 7, 16, 32])
def test_the_recipes_of_both_datasets(B):
    s = objfeed.train_recipe(B, "shapenet")
    third = B // 3
    assert s.dtype == np.int32 and s.tolist() == [T | L | S | H | J] * third + [S | H | J] * third + [0] * (B - 2 * third)
    m = objfeed.train_recipe(B, "modelnet")
    half = int(0.5 * B)
    assert m.dtype == np.int32 and m.tolist() == [T | L | S | H] * half + [0] * (B - half)
    assert objfeed.EVAL_AUGMENT == L | S | H | J == 30
    with pytest.raises(ValueError):
        objfeed.train_recipe(B, "s3dis")


def test_masks_outside_the_five_bits_are_refused():
    for bad in (-1, 32, [0, 64], [3, -2]):
        with pytest.raises(ValueError):
            objfeed.check_recipe(bad, 2)
        with pytest.raises(ValueError):
            objfeed.assemble_reference(SIZES, [0, 1], 16, 1, 1, bad)
    with pytest.raises(ValueError):
        objfeed.check_recipe([1, 2, 3], 2)
    with pytest.raises(ValueError):
        objfeed.check_recipe([1.0, 2.0], 2)
    assert objfeed.check_recipe(5, 3).tolist() == [5, 5, 5]


def test_scale_and_shift_stay_in_their_ranges():
    """s = 0.8 + 0.45 u in [0.8, 1.25), shift = -0.1 + 0.2 u in [-0.1, 0.1) with u = k 2^-24, k < 2^24: over many clouds, and at
    the two ends of u"""
    b = np.arange(4096)
    ck = feed.cloud_key(3, 1 << 33, b)
    scale = np.array([objfeed.scale_factor(k) for k in ck])
    shift = np.stack([objfeed.shift_vector(k) for k in ck])
    assert scale.min() >= 0.8 and scale.max() < 1.25 and scale.max() - scale.min() > 0.4
    assert shift.min() >= -0.1 and shift.max() < 0.1 and shift.max() - shift.min() > 0.19
    assert abs(scale.mean() - 1.025) < 0.01 and np.abs(shift.mean(axis=0)).max() < 0.005
    top = float(feed.uniform(np.uint32(0xffffffff)))
    assert top < 1.0 and 0.8 + 0.45 * top < 1.25 and -0.1 + 0.2 * top < 0.1 and float(feed.uniform(np.uint32(0))) == 0.0
    # in fp32, as the kernel evaluates them, the largest u may round onto the upper end (as numpy's own uniform(low, high) may):
    # never past it
    assert np.float32(0.8) + np.float32(0.45) * np.float32(top) <= np.float32(1.25)
    assert np.float32(-0.1) + np.float32(0.2) * np.float32(top) <= np.float32(0.1)
    # the three shifts of a cloud are three draws, and scale is not one of them
    assert len(set(shift[0].tolist())) == 3


def _close(got, want, terms):
    """|got - want| <= 2^-23 * (sum of the magnitudes of the element's terms): the reference keeps the z rotation's matrix and
    most results in float32 (one rounding of a matrix entry and one of the result, 2^-24 of the terms each)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    bound = 2.0 ** -23 * terms
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    return float((err / np.maximum(bound, 1e-300)).max())


def test_the_float64_transform_reproduces_the_references_functions(golden):
    """given the random numbers numpy handed out, objfeed.transform gives what utils/data_util.py gave, per function"""
    xyz = golden["xyz"]
    assert xyz.shape == (4, 16, 3) and xyz.dtype == np.float32
    ax = np.abs(xyz.astype(np.float64))
    worst = {}
    # rotate_point_cloud: one uniform per cloud, angle = u * 2 pi
    u = golden["rotate_point_cloud_random"]
    assert u.shape == (4,)
    for b in range(4):
        theta = u[b] * 2 * np.pi
        got = objfeed.transform(xyz[b], T, theta=theta)
        terms = np.dot(ax[b], np.abs(objfeed.turn_matrix(theta)))
        worst["turn"] = max(worst.get("turn", 0.0), _close(got, golden["rotate_point_cloud"][b], terms))
    # rotate_perturbation_point_cloud: three normals per cloud, angles = clip(0.06 z, -0.18, 0.18)
    z = golden["rotate_perturbation_point_cloud_random"].reshape(4, 3)
    for b in range(4):
        angles = np.clip(objfeed.ANGLE_SIGMA * z[b], -objfeed.ANGLE_CLIP, objfeed.ANGLE_CLIP)
        got = objfeed.transform(xyz[b], L, tilt=angles)
        terms = np.dot(ax[b], np.abs(objfeed.tilt_matrix(*angles)))
        worst["tilt"] = max(worst.get("tilt", 0.0), _close(got, golden["rotate_perturbation_point_cloud"][b], terms))
    # random_scale_point_cloud: uniform(0.8, 1.25) per cloud
    s = golden["random_scale_point_cloud_random"]
    assert s.shape == (4,) and s.min() >= 0.8 and s.max() < 1.25
    for b in range(4):
        got = objfeed.transform(xyz[b], S, scale=s[b])
        worst["scale"] = max(worst.get("scale", 0.0), _close(got, golden["random_scale_point_cloud"][b], ax[b] * s[b]))
    # shift_point_cloud: uniform(-0.1, 0.1) per cloud and axis
    h = golden["shift_point_cloud_random"].reshape(4, 3)
    assert h.min() >= -0.1 and h.max() < 0.1
    for b in range(4):
        got = objfeed.transform(xyz[b], H, shift=h[b])
        worst["shift"] = max(worst.get("shift", 0.0), _close(got, golden["shift_point_cloud"][b], ax[b] + np.abs(h[b])))
    # jitter_point_cloud: one normal per coordinate, noise = clip(0.01 z, -0.02, 0.02)
    n = np.clip(objfeed.JITTER_SIGMA * golden["jitter_point_cloud_random"].reshape(4, 16, 3), -objfeed.JITTER_CLIP, objfeed.JITTER_CLIP)
    for b in range(4):
        got = objfeed.transform(xyz[b], J, noise=n[b])
        worst["jitter"] = max(worst.get("jitter", 0.0), _close(got, golden["jitter_point_cloud"][b], ax[b] + np.abs(n[b])))
    print("worst error / bound per function:", worst)


def test_the_transforms_compose_in_the_references_order(golden):
    """mask 31 is turn, tilt, scale, shift, jitter one after the other; mask 0 is the identity on the bits"""
    xyz = golden["xyz"][0]
    kw = dict(theta=0.7, tilt=(0.1, -0.05, 0.18), scale=1.1, shift=(0.05, -0.1, 0.0), noise=np.full((16, 3), 0.01))
    step = xyz
    for bit in (T, L, S, H, J):
        step = objfeed.transform(step, bit, **kw)
    assert np.array_equal(objfeed.transform(xyz, 31, **kw), step)
    assert np.array_equal(objfeed.transform(xyz, 0, **kw), xyz.astype(np.float64))
    assert np.array_equal(objfeed.transform(xyz, S | J, **kw), xyz.astype(np.float64) * 1.1 + 0.01)


def test_shape_blocks_and_apply_reference():
    rng = np.random.RandomState(0)
    xyz = [rng.rand(n, 3).astype(np.float32) for n in (5, 40)]
    lab = [rng.randint(0, 4, 5), 7]
    blocks = [objfeed.shape_blocks(x, l) for x, l in zip(xyz, lab)]
    for blk, x in zip(blocks, xyz):
        assert blk.shape == (x.shape[0], 8) and blk.dtype == np.float32
        assert np.array_equal(blk[:, 0:3], x) and not blk[:, 3:6].any() and (blk[:, 7] == 1).all()
    assert np.array_equal(blocks[0][:, 6], lab[0]) and (blocks[1][:, 6] == 7).all()
    with pytest.raises(ValueError):
        objfeed.shape_blocks(np.zeros((0, 3)), [])
    with pytest.raises(ValueError):
        objfeed.shape_blocks(xyz[0], [1, 2])
    ref = objfeed.assemble_reference([5, 40], [1, 0], 16, 2, 3, [0, S])
    pts, label = objfeed.apply_reference(blocks, [1, 0], ref)
    assert np.array_equal(pts[0], xyz[1][ref.index[0]].astype(np.float64)) and (label[0] == 7).all()
    assert np.array_equal(pts[1], xyz[0][ref.index[1]].astype(np.float64) * ref.scale[1])
    assert np.array_equal(label[1], lab[0][ref.index[1]])


def test_the_entries_validate_on_the_host():
    """sph3d_objfeed_assemble and sph3d_shape_iou refuse requests that describe no launch before touching a device"""
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    assert l.sph3d_objfeed_assemble(0, 64, 1, 8, None, None, None, 1, 1, None, None, None, None, None) == -1
    assert b"B<=65535" in l.sph3d_last_error()
    assert l.sph3d_objfeed_assemble(70000, 64, 1, 8, None, None, None, 1, 1, None, None, None, None, None) == -1
    assert l.sph3d_objfeed_assemble(2, 0, 1, 8, None, None, None, 1, 1, None, None, None, None, None) == -1
    assert b"num_point>0" in l.sph3d_last_error()
    assert l.sph3d_objfeed_assemble(2, 64, 1, 8, None, None, None, 1, 1, None, None, None, None, None) == -1
    assert b"null input" in l.sph3d_last_error()
    none = [None] * 6
    assert l.sph3d_shape_iou(2, 65, 1, 8, None, None, None, 0, 8, None, None, None, *none, None) == -1
    assert b"classes" in l.sph3d_last_error()
    assert l.sph3d_shape_iou(2, 6, 1, 8, None, None, None, 4, 8, None, None, None, *none, None) == -1
    assert b"not a range" in l.sph3d_last_error()
    assert l.sph3d_shape_iou(2, 6, 1, 8, None, None, None, 0, 8, None, None, None, *none, None) == -1
    assert b"null input" in l.sph3d_last_error()
