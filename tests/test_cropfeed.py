"""harness/cropfeed.py without a GPU: the column sort, a crop's strips against brute-force membership, the attempt and inner rules
against a restatement, the epoch's id -> scene map, and the refusals."""
import numpy as np
import pytest

import _cropfeed_cases as cases
from sph3d_gcn_amd.harness import cropfeed, feed, sceneprep


def _scene(cells, n_x, n_y, seed=0, cell=0.05):
    """a scene with one point per entry of `cells` [(ix, iy)], placed at a random position inside its cell of an n_x x n_y grid
    whose corner cells (0, 0) and (n_x - 1, n_y - 1) are occupied (they fix lo and the grid's shape)"""
    rng = np.random.RandomState(seed)
    cells = np.array([(0, 0), (n_x - 1, n_y - 1)] + list(cells), dtype=np.float64)
    xy = (cells + 0.25 + 0.5 * rng.rand(len(cells), 2)) * cell
    xy[0] = 0.0                                             # lo = (0, 0): cell k is [k c, (k + 1) c)
    xyz = np.concatenate([xy, rng.rand(len(cells), 1)], axis=1).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    return xyz, cropfeed.sort_scene(xyz, rng.rand(len(xyz), 3), rng.randint(0, 13, len(xyz)))


def test_column_sort_is_a_stable_sort_by_column_and_col_start_brackets_every_column():
    rng = np.random.RandomState(1)
    xyz = (rng.rand(5000, 3) * np.array([1.3, 0.7, 2.0]) + np.array([-3.0, 11.0, 0.0])).astype(np.float32)
    xyz[100:200] = xyz[0]                                   # many rows in one cell: the tie rule
    cs = cropfeed.column_sort_reference(xyz, 0.05)
    assert np.array_equal(np.sort(cs.order), np.arange(5000))                       # a permutation of the scene
    assert (np.diff(cs.column) >= 0).all()                                          # column ascending
    same = np.diff(cs.column) == 0
    assert same.any() and (np.diff(cs.order)[same] > 0).all()                       # ties in original order
    # the columns restated from the definition, cast by cast
    lo = xyz[:, 0:2].min(axis=0)
    ix = np.floor(((xyz[:, 0] - lo[0]).astype(np.float32) / np.float32(0.05)).astype(np.float32)).astype(np.int64)
    iy = np.floor(((xyz[:, 1] - lo[1]).astype(np.float32) / np.float32(0.05)).astype(np.float32)).astype(np.int64)
    assert (cs.n_x, cs.n_y) == (ix.max() + 1, iy.max() + 1)
    col = ix * cs.n_y + iy
    assert np.array_equal(cs.column, col[cs.order])
    assert cs.col_start.shape == (cs.n_x * cs.n_y + 1,) and cs.col_start[0] == 0 and cs.col_start[-1] == 5000
    for c in range(cs.n_x * cs.n_y):
        a, e = cs.col_start[c], cs.col_start[c + 1]
        assert (cs.column[a:e] == c).all() and e - a == (col == c).sum()
    s = cropfeed.sort_scene(xyz, xyz, np.arange(5000))
    assert np.array_equal(s.rows[:, 0:3], xyz[cs.order]) and np.array_equal(s.index, cs.order) and not s.rows[:, 7].any()
    assert np.array_equal(s.rows[:, 6].astype(np.int64), cs.order)


@pytest.mark.parametrize("n_x,n_y,outer_half", [(12, 9, 3), (12, 9, 0), (9, 1, 2), (1, 7, 2), (5, 4, 127), (1, 1, 0)])
def test_strips_equal_brute_force_membership_for_every_window_shape(n_x, n_y, outer_half):
    """centres in every cell of the grid: all four corners, all four edges and the interior; a grid with n_y = 1 and one with
    n_x = 1; outer_half = 0 (the window is one cell) and a window larger than the scene"""
    rng = np.random.RandomState(n_x * 100 + n_y)
    # 0 .. 3 points per cell (empty columns included), at least one in the border cells and in cell (1, 1)
    must = lambda x, y: x in (0, n_x - 1) or y in (0, n_y - 1) or (x, y) == (1, 1)
    occupied = [(x, y) for x in range(n_x) for y in range(n_y) for _ in range(max(rng.randint(0, 4), int(must(x, y))))]
    _xyz, scene = _scene(occupied, n_x, n_y, seed=3)
    assert (scene.n_x, scene.n_y) == (n_x, n_y)
    seen = set()
    for centre in range(scene.column.shape[0]):
        win = cropfeed.window(scene, centre, outer_half)
        want, (cx, cy) = cases.brute_members(scene, centre, outer_half)
        got = cropfeed.members(scene, win)
        assert np.array_equal(got, want) and centre in got
        first, end = cropfeed.strips(scene, win)
        assert len(first) == win[3] - win[2] + 1 <= 2 * outer_half + 1 and int((end - first).sum()) == len(want)
        seen.add((cx == 0, cx == n_x - 1, cy == 0, cy == n_y - 1))
    assert len(seen) == min(n_x, 3) * min(n_y, 3)          # every corner / edge / interior position of the grid was a centre


def test_the_case_table_reaches_every_branch():
    """told from the brute-force restatement alone: T on both sides of N, attempt 0 accepted, a later attempt accepted, no attempt
    accepted (with and without a tie for the best), a window clipped on each of the four sides, a one-row scene"""
    reached = set()
    for c in cases.all_cases():
        reached |= cases.branches(*c)
    assert reached == cases.ALL_BRANCHES
    later = [c for c in cases.all_cases() if "later" in cases.branches(*c)]
    assert later and all(c[0] == 1024 for c in later)


@pytest.mark.parametrize("num_point,halves,draw", cases.all_cases())
def test_crop_reference_equals_the_brute_force_restatement(num_point, halves, draw):
    """T, the attempt rule, the members' order, the inner rule; distinct rows when T >= N; rows of the crop only"""
    pool, g = cases.host_pool(), cases.geometry_of(halves, num_point)
    ref, (points, label, inner) = cases.reference(num_point, halves, draw, True)
    assert ref.kind.tolist() == [1, 1, 2, 2, 0, 0, 0]
    for b, sid in enumerate(cases.SCENE_IDS):
        scene, ck = pool[int(sid)], feed.cloud_key(draw[0], draw[1], b)
        a, centre, T, _tags = cases.brute_choice(scene, ck, g)
        assert ref.crop[b].tolist() == [sid, centre, a, T]
        mem, (cx, cy) = cases.brute_members(scene, centre, g.outer_half)
        assert T == len(mem) >= 1
        t = feed.sample_without_replacement(ck, T, num_point) if T >= num_point else feed.sample_with_replacement(ck, T, num_point)
        assert np.array_equal(ref.index[b], mem[t])
        if T >= num_point:
            assert np.unique(ref.index[b]).shape[0] == num_point
        ix, iy = np.divmod(scene.column[ref.index[b]].astype(np.int64), scene.n_y)
        assert np.array_equal(inner[b], ((np.abs(ix - cx) <= g.inner_half) & (np.abs(iy - cy) <= g.inner_half)).astype(np.int32))
        assert np.array_equal(label[b], scene.rows[ref.index[b], 6].astype(np.int32))
        assert np.array_equal(points[b, :, 3:6], scene.rows[ref.index[b], 3:6].astype(np.float64))
        if ref.kind[b] == 0:
            assert np.array_equal(points[b, :, 0:3], scene.rows[ref.index[b], 0:3].astype(np.float64))
    # the centre's own cell is inner, and (0, 0) makes exactly that cell inner
    if halves == (0, 0):
        assert inner.all()
    plain, _ = cases.reference(num_point, halves, draw, False)
    assert np.array_equal(plain.index, ref.index) and np.array_equal(plain.crop, ref.crop) and not plain.kind.any()


def test_geometry_is_formed_in_float64_from_the_fp32_cell_edge():
    assert cropfeed.crop_geometry(8192) == cropfeed.Geometry(15, 21, 4, 8192)
    assert cropfeed.crop_geometry(4096, cell=0.1, block=2.0, context=0.5, attempts=8, min_points=100) == cropfeed.Geometry(10, 15, 8, 100)
    assert cropfeed.crop_geometry(1, block=0.0, context=0.0) == cropfeed.Geometry(0, 0, 4, 1)
    assert cropfeed.crop_geometry(1, cell=0.05, block=12.0, context=0.35)[:2] == (120, 127)


def test_the_id_to_scene_map_visits_every_scene_in_proportion_to_its_size():
    for sizes, E in (((3000, 700, 5, 1), 3706), ((3000, 700, 5, 1), 37), ((10, 10, 10), 3), ((1000, 1), 1000), ((5, 2000, 7), 64)):
        m = cropfeed.scene_of_crop(sizes, E)
        T = float(sum(sizes))
        got = np.bincount(m, minlength=len(sizes))
        assert m.shape == (E,) and (np.diff(m) >= 0).all() and got.sum() == E
        assert (np.abs(got - np.array(sizes) * E / T) <= 1.0).all(), (sizes, E, got)
        if E >= T:
            assert (got >= 1).all()
    assert (np.bincount(cropfeed.scene_of_crop((3000, 700, 5, 1), 3706), minlength=4) >= 1).all()          # every scene is visited
    assert cropfeed.default_crops_per_epoch(3706, 256) == 14 and cropfeed.default_crops_per_epoch(10, 8192) == 1


def test_an_epochs_items_do_not_depend_on_world():
    sizes, E, bs, seed = (3000, 700, 5, 1), 29, 4, 11
    for epoch in (0, 1):
        one = cropfeed.epoch_scenes(sizes, E, bs, seed, epoch)
        assert len(one) == 8 and [len(i) for _s, i in one] == [4] * 7 + [1]
        assert [s for s, _ in one] == list(range(epoch * 8, epoch * 8 + 8))
        for world in (2, 3):
            parts = [cropfeed.epoch_scenes(sizes, E, bs, seed, epoch, r, world) for r in range(world)]
            merged = sorted((item for p in parts for item in p), key=lambda it: it[0])
            assert len(merged) == len(one)
            for (s0, i0), (s1, i1) in zip(one, merged):
                assert s0 == s1 and np.array_equal(i0, i1)
        assert np.array_equal(np.sort(np.concatenate([i for _s, i in one])), cropfeed.scene_of_crop(sizes, E))
    assert not all(np.array_equal(a[1], b[1]) for a, b in zip(cropfeed.epoch_scenes(sizes, E, bs, seed, 0),
                                                                cropfeed.epoch_scenes(sizes, E, bs, seed, 1)))


def test_refusals():
    ok = np.random.RandomState(0).rand(10, 3).astype(np.float32)
    with pytest.raises(ValueError, match="empty scene"):
        cropfeed.column_sort_reference(np.zeros((0, 3), np.float32))
    for bad in (np.nan, np.inf, -np.inf):
        x = ok.copy()
        x[3, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            cropfeed.column_sort_reference(x)
    with pytest.raises(ValueError, match="max_columns"):
        cropfeed.column_sort_reference(ok, 0.05, max_columns=50)                   # about 20 x 20 cells
    with pytest.raises(ValueError, match="max_columns"):
        cropfeed.column_sort_reference(ok * np.float32(1e30), 0.05)                # an overflowing quotient
    far = ok.copy()
    far[0, 0] = 1e6                                                                # 2e7 cells along x
    with pytest.raises(ValueError, match="max_columns"):
        cropfeed.column_sort_reference(far, 0.05)
    assert cropfeed.column_sort_reference(ok, 0.05, max_columns=400).n_x <= 20

    class _Huge:                                                                   # n >= 2^31 without the memory
        ndim, shape, dtype = 2, (1 << 31, 3), np.dtype(np.float32)
    import unittest.mock
    with unittest.mock.patch.object(np, "ascontiguousarray", lambda a, dtype=None: a):
        with pytest.raises(ValueError, match="2\\^31"):
            cropfeed.column_sort_reference(_Huge())
    with pytest.raises(ValueError):
        cropfeed.sort_scene(ok, ok[:5], np.zeros(10))
    for g in ((3, 2, 4, 1), (-1, 2, 4, 1), (0, 128, 4, 1), (1, 2, 0, 1), (1, 2, 9, 1), (1, 2, 4, 0)):
        with pytest.raises(ValueError, match="geometry"):
            cropfeed.check_geometry(g)
    assert cropfeed.check_geometry((2, 127, 8, 1)) == cropfeed.Geometry(2, 127, 8, 1)
    pool = cases.host_pool()
    g = cases.geometry_of((15, 21), 64)
    for ids in ([0, 4], [-1]):
        with pytest.raises(ValueError, match="outside the pool"):
            cropfeed.crop_reference(pool, ids, 64, 1, 1, True, g)
    with pytest.raises(ValueError):
        cropfeed.crop_reference(pool, [0], 0, 1, 1, True, g)
    with pytest.raises(ValueError):
        cropfeed.scene_of_crop((3, 0), 4)
    with pytest.raises(ValueError):
        cropfeed.scene_of_crop((3, 1), 0)
    assert cropfeed.CROP == 40 and cropfeed.CROP not in (feed.PERM, feed.REPL, feed.TURN, feed.TILT, feed.JITTER) + tuple(range(32, 39))
