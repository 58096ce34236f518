"""Scene preparation: from a full-resolution cloud to the pool of blocks the segmentation networks are evaluated on — what the
reference does offline in two stages, MATLAB `pcdownsample(..., 'gridAverage', 0.03)` (preprocesing/s3dis_prepare_data.m:35-37,
scannet_prepare_data.m:101-107) and the block writer (io/make_tfrecord_s3dis.py:113-242, make_tfrecord_scannet.py:98-180):

    full cloud -> voxel cloud -> blocks (a BlockPool with a scene index) -> [evalvote, scenemerge: votes -> merge -> lift]

  * ``voxel_reference`` / ``normalise_reference`` / ``block_plan`` / ``split_reference``: the SPECIFICATION in numpy, no GPU,
    every cast written out.  csrc/prep.hip (sph3d_prep_*) equals it bit for bit, the fp32 means included
    (tests/test_gpu_sceneprep.py);
  * ``write_scene_records``: the statement's blocks as a record file BlockPool.from_records(..., with_index=True) reads back;
  * ``voxelize`` / ``voxel_labels`` / ``voxelize_objects`` / ``normalise`` / ``rect_counts`` / ``split`` / ``prepare_scenes``:
    the same on the device, resident in HBM.

The voxel mean is ORDER-FREE BY CONSTRUCTION: a value is turned into the integer q = rint(v * 2^20) (float64 product, exact;
ties to even), a cell's S = sum of q is an int64 sum, and mean = f32(f64(S) / f64(count) * 2^-20).  Integer addition commutes,
so any order of the points and any order of the device's atomics give the same bits.  |q| <= 2^37 (a kept value is at most
2^17 in magnitude), so S is exact for a cell of up to 2^26 points; beyond that both sides wrap modulo 2^64 alike.  The mean
differs from the exact mean of the fp32 values by at most 2^-21 (4.8e-7 m: half a unit of q) plus half an fp32 ulp of the result.

What differs from MATLAB, which cannot be run here, on purpose: the voxel rows come in ascending cell key (x slowest, z fastest),
and colour means are not rounded back to uint8 (the network sees 2c/255 - 1: a difference of at most 0.004).  The statement is
the contract, not MATLAB's bits.

THE PREDICATE of the block writer.  A bound (x, x + block, x - context, ...) is computed in float64, rounded to fp32 ONCE, and
compared with the fp32 coordinate by inclusive >= / <=.  That is what the numpy of the reference's time did with a float32 array
and a Python scalar (the scalar took the array's type); newer numpy compares such a pair in float64, and the two differ only for
a coordinate within an ulp of a bound.  The fp32 comparison is chosen: it is the one the records of the paper were written with,
and the one a device kernel evaluates without double precision.
"""
import numpy as np

_F32 = np.float32
_F64 = np.float64
QSCALE = 2.0 ** 20                    # csrc/prep.hip: kPrepQScale
MAX_VALUE = 2.0 ** 17                 # a kept value's magnitude is at most this
DEFAULT_MAX_CELLS = 1 << 26           # the dense cell table of the device: 4 bytes per cell
MAX_CELLS_LIMIT = 1 << 30             # cell keys are int32 on the device
# the nine candidate rectangles of a square (x, y) of edge b, as multiples of b added to x (lo, hi) and to y (lo, hi):
# the square itself, then the eight neighbour rectangles in the order of make_tfrecord_s3dis.py:179-186
_CAND = np.array([[0, 1, 0, 1],
                  [-1, 1, 0, 1], [0, 2, 0, 1], [0, 1, -1, 1], [0, 1, 0, 2],
                  [-1, 1, -1, 1], [-1, 1, 0, 2], [0, 2, -1, 1], [0, 2, 0, 2]], dtype=_F64)


class GridTooLarge(ValueError):
    """the voxel grid of this cloud and cell edge has more cells than max_cells"""


# ---------------------------------------------------------------------------------------------------------------
# the statement (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
def _check_cloud(xyz, attr, h, max_cells):
    xyz = np.ascontiguousarray(xyz, dtype=_F32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz [F, 3] expected")
    F = xyz.shape[0]
    attr = np.zeros((F, 0), dtype=_F32) if attr is None else np.ascontiguousarray(attr, dtype=_F32)
    if attr.ndim != 2 or attr.shape[0] != F:
        raise ValueError("attr [F, A] expected, one row per point")
    if not 0 < F < 1 << 31:
        raise ValueError("0 < F < 2^31 points required, got %d" % F)
    if attr.shape[1] > 13:
        raise ValueError("at most 13 attribute columns, got %d" % attr.shape[1])
    h32 = _F32(h)
    if not (h32 > 0 and np.isfinite(h32)):
        raise ValueError("cell edge h > 0 required, got %r" % (h,))
    if not 1 <= int(max_cells) <= MAX_CELLS_LIMIT:
        raise ValueError("1 <= max_cells <= 2^30 required, got %r" % (max_cells,))
    return xyz, attr, h32, int(max_cells)


def cell_coordinate(v, lo, h32):
    """floor(f32(f32(v - lo) / h)) as float32: the subtraction and the division are each rounded to fp32 once"""
    d = np.subtract(np.asarray(v, dtype=_F32), np.asarray(lo, dtype=_F32), dtype=_F32)
    return np.floor(np.divide(d, _F32(h32), dtype=_F32))


def grid_shape(lo, hi, h32, max_cells):
    """-> (n_x, n_y, n_z), n_a = i_a(hi_a) + 1; GridTooLarge when an axis or the product exceeds max_cells"""
    top = cell_coordinate(hi, lo, h32)
    if not (top < _F32(max_cells)).all():                         # (also an overflowing or NaN quotient)
        raise GridTooLarge("voxel grid: an axis needs %s cells, max_cells = %d" % (top.max(), max_cells))
    n = [int(t) + 1 for t in top]
    if n[0] * n[1] > max_cells or n[0] * n[1] * n[2] > max_cells:
        raise GridTooLarge("voxel grid of %d x %d x %d cells, max_cells = %d" % (n[0], n[1], n[2], max_cells))
    return tuple(n)


def voxel_reference(xyz, attr, h, max_cells=DEFAULT_MAX_CELLS):
    """xyz [F, 3] f32, attr [F, A] f32 (None: A = 0), cell edge h -> voxel [V, 3+A] f32, count [V] i32,
    voxel_of_point [F] i32, dropped.

    A point is KEPT when all its 3+A values are finite and at most 2^17 in magnitude; the others get voxel_of_point = -1 and are
    counted in `dropped`.  lo, hi: per-axis fp32 extrema of the kept points; i_a = int(floor(f32(f32(v_a - lo_a) / h)));
    n_a = i_a(hi_a) + 1; key = (i_x n_y + i_y) n_z + i_z; the voxel rows are the occupied cells in ascending key; a column's
    mean over a cell is f32(f64(sum of rint(f64(v) 2^20)) / f64(count) * 2^-20) (see the module's head).
    ValueError without a kept point; GridTooLarge for a grid of more than max_cells cells."""
    xyz, attr, h32, max_cells = _check_cloud(xyz, attr, h, max_cells)
    F = xyz.shape[0]
    vals = np.concatenate([xyz, attr], axis=1)
    with np.errstate(all="ignore"):
        kept = (np.abs(vals) <= _F32(MAX_VALUE)).all(axis=1)       # (a NaN or an infinity fails the comparison)
    dropped = int(F - kept.sum())
    if dropped == F:
        raise ValueError("voxel grid: no point of the cloud is kept (all non-finite or above 2^17)")
    kx = xyz[kept]
    lo, hi = kx.min(axis=0), kx.max(axis=0)
    nx, ny, nz = grid_shape(lo, hi, h32, max_cells)
    i = cell_coordinate(kx, lo, h32).astype(np.int64)
    key = (i[:, 0] * np.int64(ny) + i[:, 1]) * np.int64(nz) + i[:, 2]
    _keys, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    V = int(_keys.shape[0])
    voxel_of_point = np.full((F,), -1, dtype=np.int32)
    voxel_of_point[kept] = inv.astype(np.int32)
    q = np.rint(vals[kept].astype(_F64) * _F64(QSCALE)).astype(np.int64)
    order = np.argsort(inv, kind="stable")
    count = np.bincount(inv, minlength=V).astype(np.int64)
    first = np.concatenate(([0], np.cumsum(count)[:-1])).astype(np.int64)
    with np.errstate(over="ignore"):
        S = np.add.reduceat(q[order], first, axis=0, dtype=np.int64)
    mean = (S.astype(_F64) / count.astype(_F64)[:, None] * _F64(1.0 / QSCALE)).astype(_F32)
    return mean, count.astype(np.int32), voxel_of_point, dropped


def normalise_reference(voxel_xyz, voxel_rgb):
    """make_tfrecord_s3dis.py:114-122 in fp32, every operation rounded separately: c = (lo + hi) / 2 with c_z = lo_z,
    xyz' = xyz - c (the room's bottom centre becomes the origin), rgb' = (2 rgb) / 255 - 1 -> xyz' [V, 3], rgb' [V, 3], c [3]"""
    xyz = np.ascontiguousarray(voxel_xyz, dtype=_F32).reshape(-1, 3)
    rgb = np.ascontiguousarray(voxel_rgb, dtype=_F32).reshape(-1, 3)
    if xyz.shape[0] == 0 or rgb.shape[0] != xyz.shape[0]:
        raise ValueError("normalise: a non-empty [V, 3] cloud and as many colours expected")
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    c = np.divide(np.add(lo, hi, dtype=_F32), _F32(2), dtype=_F32)
    c[2] = lo[2]
    out_xyz = np.subtract(xyz, c[None, :], dtype=_F32)
    out_rgb = np.subtract(np.divide(np.multiply(rgb, _F32(2), dtype=_F32), _F32(255), dtype=_F32), _F32(1), dtype=_F32)
    return out_xyz, out_rgb, c


def block_starts(lo, hi, block, stride):
    """the start list along one axis (make_tfrecord_s3dis.py:150-165), float64 from the fp32 extrema: arange(lo, hi - block,
    stride); lo alone when that is empty; hi - block appended when the last start lies below it"""
    lo, hi = float(_F32(lo)), float(_F32(hi))
    s = np.arange(lo, hi - block, stride, dtype=_F64)
    if s.size == 0:
        s = np.append(s, lo)
    if s[-1] < hi - block:
        s = np.append(s, hi - block)
    return s


def _check_split_args(block, stride, context, thresh):
    block, stride, context = float(block), float(stride), float(context)
    if not (block > 0 and stride > 0 and context >= 0 and np.isfinite(block + stride + context)):
        raise ValueError("block > 0, stride > 0 and context >= 0 required")
    if int(thresh) < 1:
        raise ValueError("thresh >= 1 required, got %r" % (thresh,))
    if stride >= block:
        stride = block                                             # (:143-147: no gaps between the squares)
    return block, stride, context, int(thresh)


def candidate_rects(lo_xy, hi_xy, block=1.5, stride=0.75, context=0.3):
    """-> rects float64 [S, 9, 4] (x_lo, x_hi, y_lo, y_hi): per square, x outer and y inner, the square and its eight neighbour
    rectangles, unrounded"""
    block, stride, context, _ = _check_split_args(block, stride, context, 1)
    xs, ys = block_starts(lo_xy[0], hi_xy[0], block, stride), block_starts(lo_xy[1], hi_xy[1], block, stride)
    org = np.stack(np.meshgrid(xs, ys, indexing="ij"), axis=-1).reshape(-1, 2)
    rects = np.empty((org.shape[0], 9, 4), dtype=_F64)
    rects[:, :, 0:2] = org[:, None, 0:1] + _CAND[None, :, 0:2] * block
    rects[:, :, 2:4] = org[:, None, 1:2] + _CAND[None, :, 2:4] * block
    return rects


def rounded_rects(rects, context=0.0):
    """float64 rectangles widened by `context` in float64, then rounded to fp32 once -> [..., 4] f32"""
    pad = np.array([-context, context, -context, context], dtype=_F64)
    return (np.asarray(rects, dtype=_F64) + pad).astype(_F32)


def rect_counts_reference(xyz, rects, chunk=1 << 22):
    """-> int32 [R]: the points of xyz [V, >=2] f32 inside each of rects [R, 4] f32, bounds inclusive, compared in fp32"""
    xy = np.ascontiguousarray(np.asarray(xyz, dtype=_F32)[:, 0:2])
    r = np.ascontiguousarray(rects, dtype=_F32).reshape(-1, 4)
    out = np.zeros((r.shape[0],), dtype=np.int32)
    step = max(1, chunk // max(1, xy.shape[0]))
    x, y = xy[:, 0][None, :], xy[:, 1][None, :]
    for a in range(0, r.shape[0], step):
        t = r[a:a + step]
        inside = (x >= t[:, 0:1]) & (x <= t[:, 1:2]) & (y >= t[:, 2:3]) & (y <= t[:, 3:4])
        out[a:a + step] = inside.sum(axis=1)
    return out


def plan_from_counts(rects, counts, thresh):
    """rects float64 [S, 9, 4], counts [S, 9] of the rounded rectangles -> [(kind, rect)] per square: kind 0 the square itself
    (>= thresh points), 1 .. 8 the first neighbour rectangle with >= thresh points, -1 (rect None) a skipped square"""
    plan = []
    enough = np.asarray(counts).reshape(-1, 9) >= int(thresh)
    for s in range(enough.shape[0]):
        k = int(np.argmax(enough[s])) if enough[s].any() else -1
        plan.append((k, tuple(float(v) for v in rects[s, k]) if k >= 0 else None))
    return plan


def block_plan(lo_xy, hi_xy, count_fn, block=1.5, stride=0.75, context=0.3, thresh=10000):
    """make_tfrecord_s3dis.py:143-202 -> [(kind, rect)], one entry per square in the writer's order (x outer, y inner).
    count_fn(rects [R, 4] f32) -> counts [R]: the points inside each ROUNDED rectangle (see the module's head for the
    predicate); it is asked once, for all candidates.  A square with >= thresh points stays (kind 0); otherwise it becomes the
    first of its eight neighbour rectangles with >= thresh points (kind 1 .. 8); otherwise it is skipped (kind -1, rect None).
    Two squares that merge into the same rectangle give two identical blocks, as the reference writes them.  `rect` is the
    unrounded float64 (x_lo, x_hi, y_lo, y_hi); `context` only takes part in validation here."""
    block, stride, context, thresh = _check_split_args(block, stride, context, thresh)
    rects = candidate_rects(lo_xy, hi_xy, block, stride, context)
    counts = np.asarray(count_fn(rounded_rects(rects).reshape(-1, 4))).reshape(-1, 9)
    return plan_from_counts(rects, counts, thresh)


def _check_voxel_cloud(voxel_xyz, voxel_rgb, voxel_label):
    xyz = np.ascontiguousarray(voxel_xyz, dtype=_F32)
    rgb = np.ascontiguousarray(voxel_rgb, dtype=_F32)
    label = np.ascontiguousarray(voxel_label, dtype=np.int32).reshape(-1)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.shape[0] == 0 or rgb.shape != xyz.shape or label.shape[0] != xyz.shape[0]:
        raise ValueError("split: xyz [V, 3], rgb [V, 3] and label [V] of a non-empty cloud expected")
    return xyz, rgb, label


def split_reference(voxel_xyz, voxel_rgb, voxel_label, block=1.5, stride=0.75, context=0.3, thresh=10000):
    """the block writer on a NORMALISED voxel cloud (normalise_reference's xyz', rgb') -> (blocks, index, plan):
    per written block the rows [n, 8] f32 of blockio.parse_block (xyz', rgb', label, inner) — the points within `context` of the
    block's rectangle in ascending voxel index, inner = the same predicate on the rectangle itself — and index int32 [n], the
    rows' positions in the voxel cloud; plan: block_plan's list (skipped squares included)"""
    xyz, rgb, label = _check_voxel_cloud(voxel_xyz, voxel_rgb, voxel_label)
    block, stride, context, thresh = _check_split_args(block, stride, context, thresh)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    plan = block_plan(lo[0:2], hi[0:2], lambda r: rect_counts_reference(xyz, r), block, stride, context, thresh)
    blocks, index = [], []
    x, y = xyz[:, 0], xyz[:, 1]
    for kind, rect in plan:
        if kind < 0:
            continue
        p, t = rounded_rects(rect, context), rounded_rects(rect)
        at = np.nonzero((x >= p[0]) & (x <= p[1]) & (y >= p[2]) & (y <= p[3]))[0].astype(np.int32)
        inner = (x[at] >= t[0]) & (x[at] <= t[1]) & (y[at] >= t[2]) & (y[at] <= t[3])
        blocks.append(np.concatenate([xyz[at], rgb[at], label[at].astype(_F32)[:, None], inner.astype(_F32)[:, None]], axis=1))
        index.append(at)
    return blocks, index, plan


def write_scene_records(path, blocks, index, scene_idx=0):
    """one record file = one scene: the blocks through blockio.encode_block / write_records, `index` as index_label.
    BlockPool.from_records([path, ...], with_index=True) reads the same pool back"""
    from . import blockio
    if len(blocks) != len(index) or not blocks:
        raise ValueError("write_scene_records: one index array per block of a non-empty list")
    payloads = []
    for b, i in zip(blocks, index):
        b = np.ascontiguousarray(b, dtype=_F32)
        i = np.ascontiguousarray(i, dtype=np.int32).reshape(-1)
        if b.ndim != 2 or b.shape[1] != 8 or i.shape[0] != b.shape[0]:
            raise ValueError("write_scene_records: a block is [n, 8] with n index values")
        payloads.append(blockio.encode_block(b[:, 0:3], b[:, 3:6], b[:, 6].astype(np.int32), b[:, 7].astype(np.int32),
                                             index_label=i, scene_idx=int(scene_idx)))
    blockio.write_records(path, payloads)


def prepare_scene_reference(full_xyz, full_rgb, full_label, h=0.03, block=1.5, stride=0.75, context=0.3, thresh=10000,
                            max_cells=DEFAULT_MAX_CELLS):
    """one scene on the host, stage by stage as prepare_scenes does it -> (blocks, index, voxel_xyz, voxel_label):
    voxel_reference, the label of the nearest full point (scenemerge.nearest_reference), normalise_reference, split_reference;
    voxel_xyz stays in the ORIGINAL frame (what scenemerge.Scene takes), the blocks hold the normalised one"""
    from . import scenemerge
    voxel, _count, _vop, _dropped = voxel_reference(full_xyz, full_rgb, h, max_cells)
    vx = np.ascontiguousarray(voxel[:, 0:3])
    near = scenemerge.nearest_reference(full_xyz, vx)
    label = np.asarray(full_label, dtype=np.int32).reshape(-1)
    vl = np.where(near >= 0, label[np.maximum(near, 0)], -1).astype(np.int32)
    nx, nrgb, _c = normalise_reference(vx, voxel[:, 3:6])
    blocks, index, _plan = split_reference(nx, nrgb, vl, block, stride, context, thresh)
    return blocks, index, vx, vl


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
HEADER_WORDS = 16                     # include/sph3d.h: the header of sph3d_prep_voxel_grid
BOX_WORDS = 8                         # include/sph3d.h: the box of sph3d_prep_box
REDUCE_ATOMIC, REDUCE_SORTED = 0, 1   # include/sph3d.h: SPH3D_PREP_REDUCE_ATOMIC, SPH3D_PREP_REDUCE_SORTED


def to_host(*tensors):
    """device tensors -> numpy arrays with ONE host synchronisation: copies into pinned memory queued on the current stream,
    then one wait for the stream"""
    import torch
    out = [torch.empty(t.shape, dtype=t.dtype, device="cpu", pin_memory=True) for t in tensors]
    for o, t in zip(out, tensors):
        o.copy_(t, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return [o.numpy() for o in out]


def _ord_to_f32(words):
    """the ordered-integer form of the kernels' atomicMin / Max back to float32 (csrc/prep.hip: ord2f)"""
    o = np.asarray(words).astype(np.uint32)
    bits = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7fffffff), ~o)
    return bits.astype(np.uint32).view(_F32)


def voxel_grid(full_xyz, full_attr, h=0.03, max_cells=DEFAULT_MAX_CELLS):
    """sph3d_prep_voxel_grid and the read of its header (ONE host synchronisation) -> (V, dropped, (n_x, n_y, n_z), lo, hi,
    voxel_of_point [F] i32 on the device).  GridTooLarge / ValueError as voxel_reference"""
    import torch
    from .. import _lib
    _lib.require_device(full_xyz, full_attr)
    xyz, attr = _lib.f32(full_xyz), _lib.f32(full_attr)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or attr.dim() != 2 or attr.shape[0] != xyz.shape[0]:
        raise ValueError("voxelize: xyz [F, 3] and attr [F, A] expected")
    F, A = int(xyz.shape[0]), int(attr.shape[1])
    h32 = _F32(h)
    if not (h32 > 0 and np.isfinite(h32)):
        raise ValueError("cell edge h > 0 required, got %r" % (h,))
    l = _lib.lib()
    vop = torch.empty((F,), dtype=torch.int32, device=xyz.device)
    header = torch.empty((HEADER_WORDS,), dtype=torch.int32, device=xyz.device)
    need = int(l.sph3d_prep_voxel_grid_workspace(F, int(max_cells)))
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=xyz.device)
    _lib.check(l.sph3d_prep_voxel_grid(F, A, _lib.ptr(xyz), _lib.ptr(attr) if A else None, float(h32), int(max_cells), _lib.ptr(vop),
                                       _lib.ptr(header), _lib.ptr(ws), need, _lib.stream_ptr()))
    (hd,) = to_host(header)
    V, dropped, flag = int(hd[0]), int(hd[1]), int(hd[2])
    if flag == 2:
        raise ValueError("voxel grid: no point of the cloud is kept (all non-finite or above 2^17)")
    if flag != 0:
        raise GridTooLarge("voxel grid: more than max_cells = %d cells (%d x %d x %d, 0: not representable)"
                           % (max_cells, hd[3], hd[4], hd[5]))
    box = hd[6:12].view(_F32)
    return V, dropped, (int(hd[3]), int(hd[4]), int(hd[5])), box[0:3].copy(), box[3:6].copy(), vop


def voxel_reduce(full_xyz, full_attr, voxel_of_point, V, mode=REDUCE_ATOMIC):
    """sph3d_prep_voxel_reduce + _finalize -> voxel_xyz [V, 3], voxel_attr [V, A] f32, count [V] i32, box [8] i32 (the ordered
    integer extrema of voxel_xyz, for `normalise`), all on the device, no host synchronisation"""
    import torch
    from .. import _lib
    xyz, attr = _lib.f32(full_xyz), _lib.f32(full_attr)
    F, A, dev, l = int(xyz.shape[0]), int(attr.shape[1]), xyz.device, _lib.lib()
    sums = torch.empty((V, 3 + A), dtype=torch.int64, device=dev)
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    need = int(l.sph3d_prep_voxel_reduce_workspace(F, V, int(mode)))
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    _lib.check(l.sph3d_prep_voxel_reduce(F, A, V, _lib.ptr(xyz), _lib.ptr(attr) if A else None, _lib.ptr(voxel_of_point), int(mode),
                                         _lib.ptr(sums), _lib.ptr(count), _lib.ptr(ws), need, _lib.stream_ptr()))
    vx = torch.empty((V, 3), dtype=torch.float32, device=dev)
    va = torch.empty((V, A), dtype=torch.float32, device=dev)
    box = torch.empty((BOX_WORDS,), dtype=torch.int32, device=dev)
    _lib.check(l.sph3d_prep_voxel_finalize(V, A, _lib.ptr(sums), _lib.ptr(count), _lib.ptr(vx), _lib.ptr(va) if A else None,
                                           _lib.ptr(box), _lib.stream_ptr()))
    return vx, va, count, box


def voxelize(full_xyz, full_attr, h=0.03, max_cells=DEFAULT_MAX_CELLS, mode=REDUCE_ATOMIC, want_box=False):
    """full_xyz [F, 3], full_attr [F, A] fp32 on the device -> voxel_xyz [V, 3], voxel_attr [V, A], count [V] i32,
    voxel_of_point [F] i32 (-1 for a dropped point), all on the device and equal to voxel_reference bit for bit.
    One host synchronisation (the header, before the [V, ...] outputs are allocated).  max_cells sizes the dense cell table
    (4 bytes per cell); a cloud whose grid needs more raises GridTooLarge."""
    V, _dropped, _n, _lo, _hi, vop = voxel_grid(full_xyz, full_attr, h, max_cells)
    vx, va, count, box = voxel_reduce(full_xyz, full_attr, vop, V, mode)
    return (vx, va, count, vop, box) if want_box else (vx, va, count, vop)


def voxel_labels(full_xyz, full_label, voxel_xyz):
    """the label of the full point nearest to every voxel point (scannet_prepare_data.m:106-107), through scenemerge.nearest
    (ties to the lowest index) -> [V] i32 on the device"""
    import torch
    from . import scenemerge
    from .. import _lib
    near = scenemerge.nearest(full_xyz, voxel_xyz)
    label = _lib.i32(full_label).reshape(-1)
    return torch.where(near >= 0, label[near.clamp(min=0).long()], torch.full_like(near, -1))


def voxelize_objects(objects, h=0.03, max_cells=DEFAULT_MAX_CELLS):
    """S3DIS voxelises every annotated object on its own (s3dis_prepare_data.m:26-38), so a voxel point's label is its
    object's: objects = [(xyz [F_k, 3], rgb [F_k, 3], label), ...] on the device -> voxel_xyz, voxel_rgb, voxel_label [V] i32,
    the objects' voxel clouds back to back.  One host synchronisation per object"""
    import torch
    xs, cs, ls = [], [], []
    for xyz, rgb, label in objects:
        vx, vc, _count, _vop = voxelize(xyz, rgb, h, max_cells)
        xs.append(vx); cs.append(vc)
        ls.append(torch.full((vx.shape[0],), int(label), dtype=torch.int32, device=vx.device))
    if not xs:
        raise ValueError("voxelize_objects: no objects")
    return torch.cat(xs), torch.cat(cs), torch.cat(ls)


def voxel_box(voxel_xyz):
    """the ordered-integer extrema of a device cloud [V, 3] -> box [8] i32 on the device (what voxel_reduce returns with a
    cloud it averaged itself)"""
    import torch
    from .. import _lib
    xyz = _lib.f32(voxel_xyz)
    box = torch.empty((BOX_WORDS,), dtype=torch.int32, device=xyz.device)
    _lib.check(_lib.lib().sph3d_prep_box(int(xyz.shape[0]), _lib.ptr(xyz), _lib.ptr(box), _lib.stream_ptr()))
    return box


def normalise(voxel_xyz, voxel_rgb, box=None):
    """sph3d_prep_normalise -> xyz' [V, 3], rgb' [V, 3] on the device, equal to normalise_reference; no synchronisation"""
    import torch
    from .. import _lib
    _lib.require_device(voxel_xyz, voxel_rgb)
    xyz, rgb = _lib.f32(voxel_xyz), _lib.f32(voxel_rgb)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape or xyz.shape[0] == 0:
        raise ValueError("normalise: a non-empty [V, 3] cloud and as many colours expected")
    box = voxel_box(xyz) if box is None else box
    out_xyz, out_rgb = torch.empty_like(xyz), torch.empty_like(rgb)
    _lib.check(_lib.lib().sph3d_prep_normalise(int(xyz.shape[0]), _lib.ptr(xyz), _lib.ptr(rgb), _lib.ptr(box), _lib.ptr(out_xyz),
                                               _lib.ptr(out_rgb), _lib.stream_ptr()))
    return out_xyz, out_rgb


def normalised_extrema(box_host):
    """from the extrema of a voxel cloud (host copy of `box`) those of normalise's xyz' -> lo' [3], hi' [3] f32: rounding is
    monotone, so min(f32(x - c)) = f32(min(x) - c)"""
    b = _ord_to_f32(box_host)
    lo, hi = b[0:3], b[3:6]
    c = np.divide(np.add(lo, hi, dtype=_F32), _F32(2), dtype=_F32)
    c[2] = lo[2]
    return np.subtract(lo, c, dtype=_F32), np.subtract(hi, c, dtype=_F32)


def rect_counts(xyz, rects):
    """sph3d_prep_rect_count: xyz [V, 3] f32 on the device, rects [R, 4] f32 (host array or device tensor) -> counts [R] i32 on
    the device; all rectangles in one call, no synchronisation"""
    import torch
    from .. import _lib
    _lib.require_device(xyz)
    xyz = _lib.f32(xyz)
    if not torch.is_tensor(rects):
        rects = torch.from_numpy(np.ascontiguousarray(rects, dtype=_F32).reshape(-1, 4)).to(xyz.device)
    rects = _lib.f32(rects)
    R = int(rects.shape[0])
    counts = torch.empty((R,), dtype=torch.int32, device=xyz.device)
    _lib.check(_lib.lib().sph3d_prep_rect_count(int(xyz.shape[0]), R, _lib.ptr(xyz), _lib.ptr(rects), _lib.ptr(counts),
                                                _lib.stream_ptr()))
    return counts


class SplitPlan:
    """what `plan_split` leaves for `fill_split`: plan (block_plan's list), rects [P, 8] f32 on the host (the padded and the
    plain rectangle of every written block), sizes [P] int64 (rows per block)"""

    def __init__(self, plan, rects, sizes):
        self.plan, self.rects, self.sizes = plan, rects, sizes


def plan_split(voxel_xyz, lo_xy, hi_xy, block=1.5, stride=0.75, context=0.3, thresh=10000):
    """the plan of a normalised device cloud whose xy extrema the host knows: the candidates of all squares, plain and padded
    (18 per square), are counted in ONE launch, and one host read gives the plan and every block's size -> SplitPlan"""
    block, stride, context, thresh = _check_split_args(block, stride, context, thresh)
    cand = candidate_rects(lo_xy, hi_xy, block, stride, context)
    S = cand.shape[0]
    both = np.concatenate([rounded_rects(cand).reshape(-1, 4), rounded_rects(cand, context).reshape(-1, 4)])
    (counts,) = to_host(rect_counts(voxel_xyz, both))
    plan = plan_from_counts(cand, counts[:S * 9].reshape(S, 9), thresh)
    padded = counts[S * 9:].reshape(S, 9)
    rects, sizes = [], []
    for s, (kind, rect) in enumerate(plan):
        if kind >= 0:
            rects.append(np.concatenate([rounded_rects(rect, context), rounded_rects(rect)]))
            sizes.append(int(padded[s, kind]))
    if not rects:
        raise ValueError("split: no square or neighbour rectangle holds thresh = %d points" % thresh)
    return SplitPlan(plan, np.stack(rects).astype(_F32), np.array(sizes, dtype=np.int64))


def fill_split(voxel_xyz, voxel_rgb, voxel_label, sp, rows=None, index=None, offsets=None):
    """sph3d_prep_block_fill: writes the blocks of `sp` into rows [T, 8] / index [T] (views of a pool's tensors, or new ones) at
    offsets [P+1] int64 (relative to rows[0]; on the device) -> rows, index, offsets, mismatch [1] i32 on the device (blocks
    whose fill did not meet their size: 0 unless the cloud changed since plan_split); no synchronisation"""
    import torch
    from .. import _lib
    xyz, rgb, label = _lib.f32(voxel_xyz), _lib.f32(voxel_rgb), _lib.i32(voxel_label)
    dev, l = xyz.device, _lib.lib()
    V, P, T = int(xyz.shape[0]), int(sp.sizes.shape[0]), int(sp.sizes.sum())
    if rgb.shape != xyz.shape or label.dim() != 1 or label.shape[0] != V:
        raise ValueError("split: xyz [V, 3], rgb [V, 3] and label [V] expected")
    if rows is None:
        rows = torch.empty((T, 8), dtype=torch.float32, device=dev)
        index = torch.empty((T,), dtype=torch.int32, device=dev)
        offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(sp.sizes))).astype(np.int64)).to(dev)
    if tuple(rows.shape) != (T, 8) or tuple(index.shape) != (T,) or not (rows.is_contiguous() and index.is_contiguous()):
        raise ValueError("split: rows [T, 8] and index [T] of the plan's size expected")
    rects = torch.from_numpy(sp.rects).to(dev)
    mismatch = torch.zeros((1,), dtype=torch.int32, device=dev)
    need = int(l.sph3d_prep_block_fill_workspace(V, P))
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    _lib.check(l.sph3d_prep_block_fill(V, P, T, _lib.ptr(xyz), _lib.ptr(rgb), _lib.ptr(label), _lib.ptr(rects), _lib.ptr(offsets),
                                       _lib.ptr(rows), _lib.ptr(index), _lib.ptr(mismatch), _lib.ptr(ws), need, _lib.stream_ptr()))
    return rows, index, offsets, mismatch


def split(voxel_xyz, voxel_rgb, voxel_label, block=1.5, stride=0.75, context=0.3, thresh=10000, want_plan=False):
    """the block writer on a NORMALISED voxel cloud on the device (normalise's xyz', rgb'; label [V] i32) -> rows [T, 8] f32,
    offsets [P+1] int64, index [T] i32 on the device and sizes [P] int64 on the host, equal to split_reference's blocks back to
    back (and the SplitPlan with want_plan).  Two host synchronisations: the cloud's extrema, the rectangle counts"""
    from .. import _lib
    _lib.require_device(voxel_xyz, voxel_rgb, voxel_label)
    xyz = _lib.f32(voxel_xyz)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] == 0:
        raise ValueError("split: xyz [V, 3], rgb [V, 3] and label [V] of a non-empty cloud expected")
    _check_split_args(block, stride, context, thresh)
    (box,) = to_host(voxel_box(xyz))
    b = _ord_to_f32(box)
    sp = plan_split(xyz, b[0:2], b[3:5], block, stride, context, thresh)
    rows, index, offsets, _mismatch = fill_split(xyz, voxel_rgb, voxel_label, sp)
    return (rows, offsets, sp.sizes, index, sp) if want_plan else (rows, offsets, sp.sizes, index)


def prepare_scenes(raw_scenes, h=0.03, block=1.5, stride=0.75, context=0.3, thresh=10000, max_cells=DEFAULT_MAX_CELLS, device=None):
    """From scanned rooms to what scenemerge.evaluate_scenes takes -> (feed.BlockPool, [scenemerge.Scene]).

        pool, scenes = sceneprep.prepare_scenes([(full_xyz, full_rgb, full_label), ...])
        res = scenemerge.evaluate_scenes(lambda p, l, i: model(p, is_training=False)[0], pool, scenes, 16, 8192, seed=0)

    raw_scenes: per scene (full_xyz [F, 3], full_rgb [F, 3] in 0 .. 255, full_label [F]) as host arrays or device tensors.
    Per scene: voxelize (cell edge h), the label of the nearest full point, normalise, the plan; then the pool's tensors are
    allocated once and every scene's blocks are written into them by sph3d_prep_block_fill — no block row passes through the
    host.  A Scene keeps the voxel cloud in the ORIGINAL frame (so the nearest-neighbour lift against the full cloud stays
    valid); the blocks hold the normalised frame.  THREE host synchronisations per scene: the grid's header (V), the voxel
    cloud's extrema together with the Scene's host copy of the voxel cloud and labels, the rectangle counts."""
    import torch
    from . import feed, scenemerge
    if not raw_scenes:
        raise ValueError("prepare_scenes: no scenes")
    dev = torch.device(device if device is not None else "cuda:0")
    up = lambda a, dt: a.to(dev) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    kept, scenes = [], []
    for full_xyz, full_rgb, full_label in raw_scenes:
        fx, fc, fl = up(full_xyz, _F32), up(full_rgb, _F32), up(full_label, np.int32)
        vx, vc, _count, _vop, box = voxelize(fx, fc, h, max_cells, want_box=True)                 # synchronisation 1
        vl = voxel_labels(fx, fl, vx)
        nx, nc = normalise(vx, vc, box)
        box_h, vx_h, vl_h = to_host(box, vx, vl)                                                  # synchronisation 2
        lo, hi = normalised_extrema(box_h)
        sp = plan_split(nx, lo[0:2], hi[0:2], block, stride, context, thresh)                     # synchronisation 3
        kept.append((nx, nc, vl, sp))
        as_host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else a
        scenes.append(scenemerge.Scene(vx_h, vl_h, as_host(full_xyz), as_host(full_label)))
    sizes = np.concatenate([sp.sizes for _x, _c, _l, sp in kept])
    host_offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    T = int(host_offsets[-1])
    rows = torch.empty((T, 8), dtype=torch.float32, device=dev)
    index = torch.empty((T,), dtype=torch.int32, device=dev)
    offsets = torch.from_numpy(host_offsets).to(dev)
    scene_of_block, p0 = [], 0
    for s, (nx, nc, vl, sp) in enumerate(kept):
        P = int(sp.sizes.shape[0])
        t0, t1 = int(host_offsets[p0]), int(host_offsets[p0 + P])
        rel = offsets[p0:p0 + P + 1] - t0
        fill_split(nx, nc, vl, sp, rows[t0:t1], index[t0:t1], rel)
        scene_of_block += [s] * P
        p0 += P
    return feed.BlockPool.from_device(rows, offsets, sizes, index, scene_of_block), scenes


def prepare_training_scenes(raw_scenes, h=0.03, cell=0.05, max_cells=DEFAULT_MAX_CELLS, max_columns=None, device=None,
                            keep_host=False):
    """From scanned rooms to the pool harness/cropfeed.py's CropFeed draws training crops from -> cropfeed.ScenePool.

        pool = sceneprep.prepare_training_scenes([(full_xyz, full_rgb, full_label), ...])
        feed = cropfeed.CropFeed(pool, 16, 8192, seed=1)

    raw_scenes: as prepare_scenes takes them.  Per scene: voxelize (cell edge h), the label of the nearest full point and
    normalise, all on the device as in prepare_scenes — without the block split; the normalised voxel cloud is then copied to
    the host ONCE and put into stored order by cropfeed.column_sort_reference (cell edge `cell`).  A scene equals
    voxel_reference -> nearest_reference labels -> normalise_reference -> column_sort_reference bit for bit.  Two host
    synchronisations per scene: the grid's header, the copy."""
    import torch
    from . import cropfeed
    if not raw_scenes:
        raise ValueError("prepare_training_scenes: no scenes")
    dev = torch.device(device if device is not None else "cuda:0")
    up = lambda a, dt: a.to(dev) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    scenes = []
    for full_xyz, full_rgb, full_label in raw_scenes:
        fx, fc, fl = up(full_xyz, _F32), up(full_rgb, _F32), up(full_label, np.int32)
        vx, vc, _count, _vop, box = voxelize(fx, fc, h, max_cells, want_box=True)                 # synchronisation 1
        vl = voxel_labels(fx, fl, vx)
        nx, nc = normalise(vx, vc, box)
        nx_h, nc_h, vl_h = to_host(nx, nc, vl)                                                    # synchronisation 2
        scenes.append(cropfeed.sort_scene(nx_h, nc_h, vl_h, cell,
                                          cropfeed.DEFAULT_MAX_COLUMNS if max_columns is None else max_columns))
    return cropfeed.ScenePool(scenes, dev, cell, keep_host)
