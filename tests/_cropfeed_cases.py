"""What tests/test_cropfeed.py (no GPU) and tests/test_gpu_cropfeed.py share: one pool of four scenes, the table of batch cases,
a brute-force restatement of a crop that uses neither col_start nor the strips, and the branches a case takes — told from the
statement alone, so both files can assert that the table reaches every one of them."""
import functools

import numpy as np

from sph3d_gcn_amd.harness import cropfeed, feed

SIZES = (3000, 700, 5, 1)
B = 7                                                      # thirds 2 / 2 / 3
SCENE_IDS = np.array([0, 1, 0, 2, 0, 3, 1], dtype=np.int32)
N_POINTS = (256, 1024)
HALVES = ((15, 21), (0, 0), (2, 127))                      # (inner_half, outer_half)
DRAWS = ((1, 0), (0xfedcba9876543210, 12345678901))        # (seed, step)
ALL_BRANCHES = {"T>=N", "T<N", "first", "later", "none", "tie", "clip x0", "clip x1", "clip y0", "clip y1", "one row"}


@functools.lru_cache(maxsize=None)
def host_pool():
    """scenes of 3000, 700, 5 and 1 rows.  The first is a 3 m x 2 m room (60 x 40 cells of 0.05 m) with two thirds of its rows in
    one 0.9 m patch, so a 43-cell window holds between a few hundred and over two thousand rows depending on its centre; the
    second a 1.2 m x 1 m one"""
    rng = np.random.RandomState(7)
    scenes = []
    for k, n in enumerate(SIZES):
        ext = np.array([(3.0, 2.0, 2.5), (1.2, 1.0, 2.5), (0.5, 0.3, 1.0), (1.0, 1.0, 1.0)][k])
        xyz = rng.rand(n, 3) * ext
        if k == 0:
            xyz[:2000] = np.array([2.0, 1.0, 0.0]) + rng.rand(2000, 3) * np.array([0.9, 0.9, 2.5])
            xyz = xyz[rng.permutation(n)]
        scenes.append(cropfeed.sort_scene(xyz.astype(np.float32), rng.rand(n, 3).astype(np.float32), rng.randint(0, 13, n)))
    return tuple(scenes)


def geometry_of(halves, num_point):
    return cropfeed.Geometry(halves[0], halves[1], 4, num_point)


@functools.lru_cache(maxsize=None)
def reference(num_point, halves, draw, augment):
    """crop_reference and apply_reference of a case, computed once and shared (read-only)"""
    g = geometry_of(halves, num_point)
    ref = cropfeed.crop_reference(host_pool(), SCENE_IDS, num_point, draw[0], draw[1], augment, g)
    return ref, cropfeed.apply_reference(host_pool(), ref, g)


def brute_members(scene, centre, outer_half):
    """the crop around stored row `centre` without col_start: every stored row whose cell is within outer_half of the centre's on
    both axes, in stored order (ascending column, then original order: the strips' order)"""
    ix, iy = np.divmod(scene.column.astype(np.int64), scene.n_y)
    cx, cy = divmod(int(scene.column[centre]), scene.n_y)
    return np.nonzero((np.abs(ix - cx) <= outer_half) & (np.abs(iy - cy) <= outer_half))[0], (cx, cy)


def brute_choice(scene, ck, g):
    """the attempt rule restated -> (attempt, centre, T, tags)"""
    n = scene.column.shape[0]
    centres = [int((int(feed.draw(ck, cropfeed.CROP, a)) >> 32) * n >> 32) for a in range(g.attempts)]
    Ts = [len(brute_members(scene, c, g.outer_half)[0]) for c in centres]
    ok = [a for a in range(g.attempts) if Ts[a] >= g.min_points]
    tags = set()
    if ok:
        a = ok[0]
        tags.add("first" if a == 0 else "later")
    else:
        a = int(np.argmax(Ts))                             # (the first maximum)
        tags.add("none")
        if Ts.count(max(Ts)) > 1:
            tags.add("tie")
    return a, centres[a], Ts[a], tags


def branches(num_point, halves, draw):
    """the branches the case's B clouds take"""
    g, tags = geometry_of(halves, num_point), set()
    for b, sid in enumerate(SCENE_IDS):
        scene = host_pool()[int(sid)]
        _a, centre, T, t = brute_choice(scene, feed.cloud_key(draw[0], draw[1], b), g)
        tags |= t
        tags.add("T>=N" if T >= num_point else "T<N")
        cx, cy = divmod(int(scene.column[centre]), scene.n_y)
        if cx - g.outer_half < 0: tags.add("clip x0")
        if cx + g.outer_half > scene.n_x - 1: tags.add("clip x1")
        if cy - g.outer_half < 0: tags.add("clip y0")
        if cy + g.outer_half > scene.n_y - 1: tags.add("clip y1")
        if scene.column.shape[0] == 1: tags.add("one row")
    return tags


def all_cases():
    return [(n, h, d) for n in N_POINTS for h in HALVES for d in DRAWS]
