"""harness/sceneprep.py, the statement (numpy, no GPU): the voxel means against an exact mean within the derived bound,
order-independence, dropped points, degenerate clouds and cell faces, the block plan against a plain transcription of the
reference writer's loop on a cloud that takes every branch, the record round trip, validation."""
import collections
import math

import numpy as np
import pytest

from sph3d_gcn_amd.harness import feed, sceneprep as sp, scenesynth

F32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.dtype, a.shape, a.tobytes()


def _cloud(seed, n, A=3, extent=(2.0, 1.5, 1.0)):
    rng = np.random.RandomState(seed)
    xyz = (rng.rand(n, 3) * np.array(extent) + np.array([-0.7, 3.0, 0.1])).astype(F32)
    attr = (rng.rand(n, A) * 255).astype(F32)
    return xyz, attr


def test_voxel_means_within_the_derived_bound_of_the_exact_mean():
    """|mean - exact mean of the fp32 values| <= 2^-21 (half a unit of q = rint(v 2^20), averaged) + half an fp32 ulp of the
    result (the final cast); the exact mean: math.fsum per cell (exact sum, one float64 division: 2^-53 relative, allowed for
    by the 1e-12 below).  Cell membership is recomputed here from the stated formula."""
    xyz, attr = _cloud(0, 20000)
    h = 0.05
    voxel, count, vop, dropped = sp.voxel_reference(xyz, attr, h)
    assert dropped == 0 and vop.min() == 0 and vop.max() == len(voxel) - 1 and count.sum() == len(xyz) and count.max() >= 4
    lo = xyz.min(axis=0)
    i = np.floor(((xyz - lo).astype(F32) / F32(h)).astype(F32)).astype(np.int64)
    n = i.max(axis=0) + 1
    key = (i[:, 0] * n[1] + i[:, 1]) * n[2] + i[:, 2]
    keys, inv = np.unique(key, return_inverse=True)
    assert np.array_equal(inv.reshape(-1), vop) and np.array_equal(np.bincount(vop), count)
    vals = np.concatenate([xyz, attr], axis=1).astype(np.float64)
    members = collections.defaultdict(list)
    for p, r in enumerate(vop):
        members[int(r)].append(p)
    worst = 0.0
    for r in range(len(voxel)):
        for c in range(6):
            exact = math.fsum(vals[members[r], c]) / len(members[r])
            err = abs(float(voxel[r, c]) - exact)
            bound = 2.0 ** -21 + 0.5 * float(np.spacing(np.abs(voxel[r, c]))) + 1e-12
            assert err <= bound, (r, c, err, bound)
            worst = max(worst, err / bound)
    print("worst error / bound: %.3f" % worst)


def test_voxel_result_does_not_depend_on_the_order_of_the_points():
    xyz, attr = _cloud(1, 30000)
    a = sp.voxel_reference(xyz, attr, 0.03)
    perm = np.random.RandomState(2).permutation(len(xyz))
    b = sp.voxel_reference(xyz[perm], attr[perm], 0.03)
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1]) and np.array_equal(a[2][perm], b[2])


def test_dropped_points():
    xyz, attr = _cloud(3, 500)
    xyz[3, 0] = np.nan
    xyz[10, 2] = np.inf
    attr[20, 1] = -np.inf
    attr[30, 0] = np.nan
    xyz[40, 1] = F32(2.0 ** 17) * F32(1.0001)               # out of range
    attr[50, 2] = -F32(2.0 ** 18)
    xyz[60, 0] = F32(2.0 ** 17)                               # exactly 2^17: kept
    bad = [3, 10, 20, 30, 40, 50]
    voxel, count, vop, dropped = sp.voxel_reference(xyz, attr, 0.5, max_cells=1 << 30)
    assert dropped == 6 and (vop[bad] == -1).all() and (np.delete(vop, bad) >= 0).all() and vop[60] >= 0
    assert count.sum() == 494 and np.isfinite(voxel).all()
    good = np.delete(np.arange(500), bad)
    again = sp.voxel_reference(xyz[good], attr[good], 0.5, max_cells=1 << 30)
    assert _bits(again[0]) == _bits(voxel) and np.array_equal(again[2], vop[good])
    with pytest.raises(ValueError):
        sp.voxel_reference(np.full((4, 3), np.nan, F32), None, 0.1)


def test_single_point_single_cell_and_cell_faces():
    one = sp.voxel_reference(np.array([[1.25, -2.5, 3.0]], F32), np.array([[7.0]], F32), 0.03)
    assert one[0].tolist() == [[1.25, -2.5, 3.0, 7.0]] and one[1].tolist() == [1] and one[2].tolist() == [0] and one[3] == 0
    xyz, attr = _cloud(4, 300, extent=(0.02, 0.02, 0.02))
    voxel, count, vop, _ = sp.voxel_reference(xyz, attr, 0.03)
    assert len(voxel) == 1 and count.tolist() == [300] and (vop == 0).all()
    # points exactly on lo, on hi and on cell faces (h = 0.25 and lattice coordinates k / 4 are exact in fp32): a face belongs to
    # the cell above it, and hi opens the last cell
    g = np.stack(np.meshgrid(np.arange(5), np.arange(3), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3)
    xyz = (g * 0.25 + np.array([1.0, -1.0, 0.5])).astype(F32)
    voxel, count, vop, _ = sp.voxel_reference(xyz, None, 0.25)
    assert len(voxel) == 30 and (count == 1).all() and np.array_equal(vop, np.arange(30)) and _bits(voxel) == _bits(xyz)
    inside = np.concatenate([xyz, xyz + F32(0.125)]).astype(F32)            # a second point inside every cell: means 1/16 up
    voxel, count, vop, _ = sp.voxel_reference(inside, None, 0.25)
    assert (sp.grid_shape(inside.min(0), inside.max(0), F32(0.25), 1 << 20) == (5, 3, 2)) and (count == 2).all()
    assert _bits(voxel) == _bits((xyz + F32(0.0625)).astype(F32)) and np.array_equal(vop, np.tile(np.arange(30), 2))


def test_grid_too_large_and_an_axis_of_one_cell():
    xyz, attr = _cloud(5, 1000)
    with pytest.raises(sp.GridTooLarge):
        sp.voxel_reference(xyz, attr, 0.03, max_cells=1000)
    with pytest.raises(sp.GridTooLarge):
        sp.voxel_reference(xyz, attr, 1e-30)
    flat = xyz.copy()
    flat[:, 2] = 0.25
    voxel, count, vop, _ = sp.voxel_reference(flat, attr, 0.1)
    assert sp.grid_shape(flat.min(0), flat.max(0), F32(0.1), 1 << 20)[2] == 1 and (voxel[:, 2] == F32(0.25)).all()


def test_normalise_is_the_writers_arithmetic_in_fp32():
    xyz, rgb = _cloud(6, 4000)
    nx, nc, c = sp.normalise_reference(xyz, rgb)
    lo, hi = xyz.min(0), xyz.max(0)
    assert c[2] == lo[2] and nx[:, 2].min() == 0 and nx.dtype == F32 and nc.dtype == F32
    assert np.abs(nx.astype(np.float64) - (xyz.astype(np.float64) - [(lo[0] + hi[0]) / 2.0, (lo[1] + hi[1]) / 2.0, lo[2]])).max() < 1e-6
    assert np.abs(nc.astype(np.float64) - (2 * rgb.astype(np.float64) / 255.0 - 1)).max() < 2e-7 and np.abs(nc).max() <= 1
    # the extrema of xyz' follow from those of xyz (what the device path relies on)
    box = np.concatenate([lo, hi]).view(np.uint32)
    ordered = np.where(box & np.uint32(0x80000000), ~box, box | np.uint32(0x80000000)).astype(np.uint32).view(np.int32)
    lo2, hi2 = sp.normalised_extrema(ordered)
    assert _bits(lo2) == _bits(nx.min(0)) and _bits(hi2) == _bits(nx.max(0))


def _writer_loop(xyz, block, stride, context, thresh):
    """the reference writer's loop, step for step, with the fp32 predicate: -> [(kind, (x_lo, x_hi, y_lo, y_hi) | None)]"""
    x32, y32 = xyz[:, 0], xyz[:, 1]
    lo, hi = xyz.min(axis=0).astype(np.float64), xyz.max(axis=0).astype(np.float64)

    def count(x0, x1, y0, y1):
        return int(((x32 >= F32(x0)) & (x32 <= F32(x1)) & (y32 >= F32(y0)) & (y32 <= F32(y1))).sum())
    if stride >= block:
        stride = block
    left = np.arange(lo[0], hi[0] - block, stride)
    back = np.arange(lo[1], hi[1] - block, stride)
    if not left.size:
        left = np.append(left, lo[0])
    if not back.size:
        back = np.append(back, lo[1])
    if left[-1] < hi[0] - block:
        left = np.append(left, hi[0] - block)
    if back[-1] < hi[1] - block:
        back = np.append(back, hi[1] - block)
    out = []
    for x in left:
        for y in back:
            if count(x, x + block, y, y + block) >= thresh:
                out.append((0, (x, x + block, y, y + block)))
                continue
            around = [(x - block, x + block, y, y + block), (x, x + 2 * block, y, y + block),
                      (x, x + block, y - block, y + block), (x, x + block, y, y + 2 * block),
                      (x - block, x + block, y - block, y + block), (x - block, x + block, y, y + 2 * block),
                      (x, x + 2 * block, y - block, y + block), (x, x + 2 * block, y, y + 2 * block)]
            for k, r in enumerate(around):
                if count(*r) >= thresh:
                    out.append((k + 1, r))
                    break
            else:
                out.append((-1, None))
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_block_plan_takes_every_branch_and_equals_the_writers_loop(seed):
    xyz = scenesynth.coverage_cloud(seed)
    assert xyz.shape == (2602, 3)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    plan = sp.block_plan(lo[0:2], hi[0:2], lambda r: sp.rect_counts_reference(xyz, r), thresh=500)
    kinds = collections.Counter(k for k, _r in plan)
    written = [r for k, r in plan if k >= 0]
    # the coverage this cloud exists for, as a condition before the comparison
    assert len(plan) == 81 and set(kinds) == set(range(-1, 9)), sorted(kinds.items())
    assert len(set(written)) < len(written), "no two squares merged into the same rectangle"
    want = _writer_loop(xyz, 1.5, 0.75, 0.3, 500)
    assert [k for k, _r in plan] == [k for k, _r in want]
    for (_k, a), (_k2, b) in zip(plan, want):
        assert a == (None if b is None else tuple(float(v) for v in b))
    # the blocks: rows within the context of the rectangle in ascending voxel index, inner on the rectangle itself
    rgb = np.random.RandomState(seed).rand(len(xyz), 3).astype(F32)
    label = np.random.RandomState(seed + 1).randint(0, 13, len(xyz)).astype(np.int32)
    blocks, index, plan2 = sp.split_reference(xyz, rgb, label, thresh=500)
    assert plan2 == plan and len(blocks) == len(written)
    dup = [k for k in range(1, len(written)) if written[k] in written[:k]]
    assert dup and all(_bits(blocks[k]) == _bits(blocks[written.index(written[k])]) for k in dup)        # duplicates are kept
    for blk, idx, r in zip(blocks, index, written):
        pad = [F32(r[0] - 0.3), F32(r[1] + 0.3), F32(r[2] - 0.3), F32(r[3] + 0.3)]
        take = (xyz[:, 0] >= pad[0]) & (xyz[:, 0] <= pad[1]) & (xyz[:, 1] >= pad[2]) & (xyz[:, 1] <= pad[3])
        assert np.array_equal(idx, np.nonzero(take)[0]) and idx.dtype == np.int32 and blk.dtype == F32 and blk.shape == (len(idx), 8)
        assert _bits(blk[:, 0:3]) == _bits(xyz[idx]) and _bits(blk[:, 3:6]) == _bits(rgb[idx]) and np.array_equal(blk[:, 6], label[idx])
        inner = (xyz[idx, 0] >= F32(r[0])) & (xyz[idx, 0] <= F32(r[1])) & (xyz[idx, 1] >= F32(r[2])) & (xyz[idx, 1] <= F32(r[3]))
        assert np.array_equal(blk[:, 7], inner.astype(F32)) and inner.sum() >= 500


def test_start_lists_and_forced_stride():
    assert sp.block_starts(0.0, 1.0, 1.5, 0.75).tolist() == [0.0]                       # a room smaller than a block
    assert sp.block_starts(0.0, 3.0, 1.5, 0.75).tolist() == [0.0, 0.75, 1.5]            # arange ends below hi - block: appended
    assert sp.block_starts(0.0, 3.2, 1.5, 0.75).tolist() == [0.0, 0.75, 1.5, float(F32(3.2)) - 1.5]
    a = sp.candidate_rects([0, 0], [6, 6], 1.5, 2.0)                                     # stride >= block: stride = block
    b = sp.candidate_rects([0, 0], [6, 6], 1.5, 1.5)
    assert np.array_equal(a, b) and a.shape == (16, 9, 4)


def test_records_round_trip_into_the_same_pool(tmp_path):
    blocks, index, sob = [], [], []
    paths = []
    for s in range(2):
        xyz = scenesynth.coverage_cloud(s)
        nx, nc, _c = sp.normalise_reference(xyz, np.random.RandomState(s).rand(len(xyz), 3).astype(F32) * 255)
        label = np.random.RandomState(s + 5).randint(0, 13, len(xyz)).astype(np.int32)
        b, i, _plan = sp.split_reference(nx, nc, label, thresh=500)
        path = str(tmp_path / ("scene%d.tfrecord" % s))
        sp.write_scene_records(path, b, i, scene_idx=s)
        paths.append(path)
        blocks += b
        index += i
        sob += [s] * len(b)
    got = feed.BlockPool.from_records(paths, device="cpu", with_index=True)
    want = feed.BlockPool(blocks, "cpu", index, sob)
    assert _bits(got.rows.numpy()) == _bits(want.rows.numpy()) and _bits(got.index.numpy()) == _bits(want.index.numpy())
    assert np.array_equal(got.host_offsets, want.host_offsets) and np.array_equal(got.scene_of_block, want.scene_of_block)
    assert np.array_equal(got.sizes, want.sizes) and len(got) == len(blocks)


def test_validation_errors():
    xyz, attr = _cloud(7, 100)
    for bad in (dict(h=0.0), dict(h=-1.0), dict(h=float("nan")), dict(max_cells=0), dict(max_cells=(1 << 30) + 1)):
        with pytest.raises(ValueError):
            sp.voxel_reference(xyz, attr, **dict(dict(h=0.1), **bad))
    with pytest.raises(ValueError):
        sp.voxel_reference(xyz[:, :2], attr, 0.1)
    with pytest.raises(ValueError):
        sp.voxel_reference(xyz, attr[:50], 0.1)
    with pytest.raises(ValueError):
        sp.voxel_reference(np.zeros((0, 3), F32), None, 0.1)
    with pytest.raises(ValueError):
        sp.voxel_reference(xyz, np.zeros((100, 14), F32), 0.1)
    count = lambda r: sp.rect_counts_reference(xyz, r)
    for bad in (dict(thresh=0), dict(block=0.0), dict(stride=-1.0), dict(context=-0.1)):
        with pytest.raises(ValueError):
            sp.block_plan([0, 0], [1, 1], count, **bad)
    with pytest.raises(ValueError):
        sp.split_reference(xyz, attr[:, :3], np.zeros(99, np.int32))
    with pytest.raises(ValueError):
        sp.normalise_reference(xyz, attr[:50, :3])
    with pytest.raises(ValueError):
        sp.write_scene_records("unused", [np.zeros((3, 8), F32)], [np.zeros(2, np.int32)])
    with pytest.raises(ValueError):
        sp.write_scene_records("unused", [], [])


def test_from_device_refuses_host_tensors_and_wrong_shapes():
    import torch
    rows, index = torch.zeros((5, 8)), torch.zeros((5,), dtype=torch.int32)
    with pytest.raises(ValueError):
        feed.BlockPool.from_device(rows, torch.tensor([0, 2, 5]), [2, 3], index, [0, 0])
