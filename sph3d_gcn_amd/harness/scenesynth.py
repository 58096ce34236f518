"""Synthetic scenes for the scene-level evaluation (harness/scenemerge.py): a room of labelled surfaces sampled at full
resolution, its voxel cloud, and a splitter that cuts the voxel cloud into overlapping blocks with the reference's geometry
(1.5 m inner squares every 0.75 m, context padding around them — io/make_tfrecord_s3dis.py:150-221, :250-251).  For tests and
tools/exp_scene.py; it is NOT the reference's record writer: it does not merge sparse blocks into a neighbour, and an empty
square gives no block."""
import numpy as np


def synthetic_scene(seed, full_points, extent=(6.0, 5.0, 3.0), voxel=0.03, num_cls=13, furniture=6):
    """-> full_xyz [F, 3] fp32, full_label [F] i32, voxel_xyz [V, 3] fp32, voxel_label [V] i32: points on the floor, the ceiling,
    the four walls and the faces of a few boxes, in random order; the voxel cloud keeps the first point of every `voxel` cell"""
    rng = np.random.RandomState(seed)
    ex = np.asarray(extent, dtype=np.float64)
    # every surface: origin, two edge vectors, label
    faces = [((0, 0, 0), (ex[0], 0, 0), (0, ex[1], 0), 1), ((0, 0, ex[2]), (ex[0], 0, 0), (0, ex[1], 0), 0),
             ((0, 0, 0), (ex[0], 0, 0), (0, 0, ex[2]), 2), ((0, ex[1], 0), (ex[0], 0, 0), (0, 0, ex[2]), 2),
             ((0, 0, 0), (0, ex[1], 0), (0, 0, ex[2]), 2), ((ex[0], 0, 0), (0, ex[1], 0), (0, 0, ex[2]), 2)]
    for k in range(furniture):
        size = 0.3 + rng.rand(3) * np.array([1.2, 1.2, 0.9])
        org = np.append(rng.rand(2) * (ex[:2] - size[:2]), 0.0)
        lab = 3 + k % max(1, num_cls - 3)
        for a in range(3):
            u, v = np.zeros(3), np.zeros(3)
            u[(a + 1) % 3], v[(a + 2) % 3] = size[(a + 1) % 3], size[(a + 2) % 3]
            far = org.copy()
            far[a] += size[a]
            faces += [(org, u, v, lab), (far, u, v, lab)]
    area = np.array([np.linalg.norm(np.cross(u, v)) for _o, u, v, _l in faces])
    which = rng.choice(len(faces), int(full_points), p=area / area.sum())
    org = np.array([f[0] for f in faces], dtype=np.float64)[which]
    eu = np.array([f[1] for f in faces], dtype=np.float64)[which]
    ev = np.array([f[2] for f in faces], dtype=np.float64)[which]
    full_xyz = (org + rng.rand(len(which), 1) * eu + rng.rand(len(which), 1) * ev).astype(np.float32)
    full_label = (np.array([f[3] for f in faces], dtype=np.int32) % num_cls)[which]
    cells = np.floor(full_xyz.astype(np.float64) / voxel).astype(np.int64)
    _, first = np.unique(cells, axis=0, return_index=True)
    first.sort()
    return full_xyz, full_label, full_xyz[first].copy(), full_label[first].copy()


def split_scene(voxel_xyz, voxel_label, rgb=None, block=1.5, stride=0.75, context=0.3):
    """-> (blocks, index): per block the rows [n, 8] fp32 (xyz, rgb, label, inner) of blockio.parse_block and the rows'
    positions int32 [n] in voxel_xyz; a block is the points within `context` of a `block` x `block` square, inner = inside it"""
    xyz = np.asarray(voxel_xyz, dtype=np.float32)
    label = np.asarray(voxel_label).reshape(-1)
    rgb = np.zeros_like(xyz) if rgb is None else np.asarray(rgb, dtype=np.float32)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)

    def starts(a):
        s = list(np.arange(lo[a], hi[a] - block, stride))
        if not s:
            s = [lo[a]]
        if s[-1] < hi[a] - block:
            s.append(hi[a] - block)
        return s
    blocks, index = [], []
    for x in starts(0):
        for y in starts(1):
            inside = (xyz[:, 0] >= x) & (xyz[:, 0] <= x + block) & (xyz[:, 1] >= y) & (xyz[:, 1] <= y + block)
            if not inside.any():
                continue
            take = ((xyz[:, 0] >= x - context) & (xyz[:, 0] <= x + block + context) &
                    (xyz[:, 1] >= y - context) & (xyz[:, 1] <= y + block + context))
            at = np.nonzero(take)[0].astype(np.int32)
            rows = np.concatenate([xyz[at], rgb[at], label[at].reshape(-1, 1).astype(np.float32),
                                   inside[at].reshape(-1, 1).astype(np.float32)], axis=1)
            blocks.append(rows)
            index.append(at)
    return blocks, index


def coverage_cloud(seed, thresh=500):
    """-> xyz [2602, 3] fp32 for the block writer's branches (harness/sceneprep.py: block_plan with thresh = 500): 2000 uniform
    points in a 7.5 x 7.5 x 2 box (81 squares of 1.5 m every 0.75 m, about 80 points each: all sparse), 600 points in the
    0.6 x 0.6 patch at (3.45, 3.45) (the squares over it are kept, the ones beside it merge into each of the eight neighbour
    rectangles, some of them into the same one, the far ones are skipped), and the two corners of the box; shuffled"""
    rng = np.random.RandomState(seed)
    box = rng.rand(2000, 3) * np.array([7.5, 7.5, 2.0])
    patch = np.array([3.45, 3.45, 0.0]) + rng.rand(600, 3) * np.array([0.6, 0.6, 2.0])
    xyz = np.concatenate([box, patch, [[0.0, 0.0, 0.0], [7.5, 7.5, 2.0]]]).astype(np.float32)
    return xyz[rng.permutation(len(xyz))]
