"""Training crops drawn from whole scenes on the device: a pool of column-sorted scenes resident in HBM and a feed that cuts a
batch of crops out of it in one launch (csrc/cropfeed.hip, include/sph3d.h: sph3d_cropfeed_assemble) — what later
indoor-segmentation recipes do per step (keep the room, crop around a random point) in place of the offline block writer, whose
fixed 1.5 m squares on a 0.75 m grid are all that `sceneprep.split` / `DeviceFeed` ever show the network.

  * ``column_sort_reference``: the SPECIFICATION of a scene's stored order, in numpy, no GPU.  The xy plane is cut into cells of
    edge c; a row's column is col = ix n_y + iy; the rows are sorted by (col, original row).  The rows of cells (ix, y0 .. y1) are
    then ONE contiguous range — a strip — and a square window of cells is at most 2 outer_half + 1 strips;
  * ``ScenePool``: the sorted scenes back to back on the device, built once on the host by the statement itself;
  * ``crop_geometry`` / ``window`` / ``strips`` / ``members``: a crop as integers.  Only integers reach the kernel: the cell counts
    inner_half and outer_half are formed once on the host in float64;
  * ``crop_reference`` / ``apply_reference``: the SPECIFICATION of a batch.  Every draw is a pure function of (seed, step, cloud)
    like every draw of harness/feed.py, whose sample, angle and noise functions are used unchanged; the new purpose is CROP = 40,
    counter = the attempt.  The kernel's integer outputs (index, label, inner, crop) and everything it copies equal the statement
    bit for bit; rotated and jittered xyz are held to feed.py's bound against the float64 evaluation;
  * ``assemble``: the C entry;  ``CropFeed``: one epoch of crops under ``feed.TwoSetFeed``'s protocol, in ``feed.DeviceFeed``'s
    item format, so ``train.s3dis_line``, ``train.LINES["scannet"]``, ``train.Trainer`` and ``augment.Stage`` take it unchanged.

A crop stays in the scene's coordinates: the models' `normalize_xyz` centres xy per block.  `inner` marks the rows within
inner_half cells of the centre's cell on both axes — the crop's counterpart of the block writer's inner square.  Evaluation
keeps using block pools (harness/evalvote.py, scenemerge.py).
"""
import collections

import numpy as np

from . import feed, sceneprep

_F32 = np.float32
CROP = 40                             # the `purpose` of the centre draws (csrc/feed_draws.hpp: kFeedCrop); counter = the attempt
DEFAULT_CELL = 0.05
DEFAULT_MAX_COLUMNS = 1 << 24
MAX_WINDOW = 256                      # csrc/cropfeed.hip: kCropThreads — strips per window
MAX_ATTEMPTS = 8                      # csrc/cropfeed.hip: kCropMaxAttempts


# ---------------------------------------------------------------------------------------------------------------
# the stored order of a scene (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
ColumnSort = collections.namedtuple("ColumnSort", "order column col_start n_x n_y")


def column_sort_reference(xyz, cell=DEFAULT_CELL, max_columns=DEFAULT_MAX_COLUMNS):
    """xyz [n, 3] f32 -> ColumnSort(order int64 [n] — stored row k is original row order[k]; column int32 [n] — the stored rows'
    columns, ascending; col_start int32 [n_x n_y + 1] — the first stored row of every column, then n; n_x, n_y).

    lo = the fp32 minima of x and of y; ix, iy = sceneprep.cell_coordinate(v, lo, c) = floor(f32(f32(v - lo) / c)), c = f32(cell);
    n_x, n_y = their maxima + 1; col = ix n_y + iy; the rows are sorted by (col, original row).
    ValueError: an empty scene, n >= 2^31, a non-finite coordinate, a grid of more than max_columns columns."""
    xyz = np.ascontiguousarray(xyz, dtype=_F32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("column sort: xyz [n, 3] expected")
    n = xyz.shape[0]
    if n == 0:
        raise ValueError("column sort: empty scene")
    if n >= 1 << 31:
        raise ValueError("column sort: scene with 2^31 rows or more")
    if not np.isfinite(xyz).all():
        raise ValueError("column sort: non-finite coordinate")
    c = _F32(cell)
    if not (c > 0 and np.isfinite(c)):
        raise ValueError("column sort: cell edge > 0 required, got %r" % (cell,))
    max_columns = int(max_columns)
    if not 1 <= max_columns < 1 << 31:
        raise ValueError("column sort: 1 <= max_columns < 2^31 required")
    xy = xyz[:, 0:2]
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    with np.errstate(over="ignore"):
        top = sceneprep.cell_coordinate(hi, lo, c)
    if not (top < _F32(max_columns)).all():                    # (also an overflowing quotient)
        raise ValueError("column sort: an axis needs more than max_columns = %d cells" % max_columns)
    n_x, n_y = int(top[0]) + 1, int(top[1]) + 1
    if n_x * n_y > max_columns:
        raise ValueError("column sort: a grid of %d x %d columns, max_columns = %d" % (n_x, n_y, max_columns))
    i = sceneprep.cell_coordinate(xy, lo, c).astype(np.int64)
    col = i[:, 0] * np.int64(n_y) + i[:, 1]
    order = np.argsort(col, kind="stable").astype(np.int64)
    column = col[order].astype(np.int32)
    col_start = np.searchsorted(column, np.arange(n_x * n_y + 1), side="left").astype(np.int32)
    return ColumnSort(order, column, col_start, n_x, n_y)


HostScene = collections.namedtuple("HostScene", "rows column index col_start n_x n_y")


def sort_scene(xyz, rgb, label, cell=DEFAULT_CELL, max_columns=DEFAULT_MAX_COLUMNS):
    """one scene in stored order -> HostScene(rows [n, 8] f32: xyz, rgb, label, 0; column [n] i32; index [n] i32 — the stored
    rows' original positions; col_start; n_x; n_y)"""
    xyz = np.ascontiguousarray(xyz, dtype=_F32)
    cs = column_sort_reference(xyz, cell, max_columns)
    rgb = np.ascontiguousarray(rgb, dtype=_F32)
    label = np.ascontiguousarray(label, dtype=np.int32).reshape(-1)
    if rgb.shape != xyz.shape or label.shape[0] != xyz.shape[0]:
        raise ValueError("a scene is xyz [n, 3], rgb [n, 3] and label [n]")
    rows = np.zeros((xyz.shape[0], 8), dtype=_F32)
    rows[:, 0:3], rows[:, 3:6], rows[:, 6] = xyz[cs.order], rgb[cs.order], label[cs.order].astype(_F32)
    return HostScene(rows, cs.column, cs.order.astype(np.int32), cs.col_start, cs.n_x, cs.n_y)


def scene_table(scenes):
    """-> scene_tab int64 [S, 5] of HostScenes stored back to back: row offset, col_start offset, n_x, n_y, n"""
    tab = np.zeros((len(scenes), 5), dtype=np.int64)
    r = c = 0
    for s, sc in enumerate(scenes):
        tab[s] = (r, c, sc.n_x, sc.n_y, sc.column.shape[0])
        r += sc.column.shape[0]
        c += sc.col_start.shape[0]
    return tab


# ---------------------------------------------------------------------------------------------------------------
# a crop, in integers (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
Geometry = collections.namedtuple("Geometry", "inner_half outer_half attempts min_points")


def crop_geometry(num_point=None, cell=DEFAULT_CELL, block=1.5, context=0.3, attempts=4, min_points=None):
    """the integers of a crop, formed once in float64 from the fp32 cell edge: inner_half = round(block / (2 c)) cells on either
    side of the centre's cell are inner, outer_half = round((block / 2 + context) / c) are in the window (round: to the nearest
    integer, ties to even); 15 and 21 at the defaults.  min_points: None = num_point"""
    c = float(_F32(cell))
    block, context = float(block), float(context)
    if not (c > 0 and block >= 0 and context >= 0 and np.isfinite(block + context + c)):
        raise ValueError("geometry: cell > 0, block >= 0 and context >= 0 required")
    g = Geometry(int(round(block / (2.0 * c))), int(round((block / 2.0 + context) / c)), int(attempts),
                 int(num_point if min_points is None else min_points))
    return check_geometry(g)


def check_geometry(g):
    g = Geometry(*(int(v) for v in g))
    if not 0 <= g.inner_half <= g.outer_half:
        raise ValueError("geometry: 0 <= inner_half <= outer_half required, got %d, %d" % (g.inner_half, g.outer_half))
    if 2 * g.outer_half + 1 > MAX_WINDOW:
        raise ValueError("geometry: a window of 2 * %d + 1 cells, at most %d" % (g.outer_half, MAX_WINDOW))
    if not 1 <= g.attempts <= MAX_ATTEMPTS:
        raise ValueError("geometry: 1 <= attempts <= %d required, got %d" % (MAX_ATTEMPTS, g.attempts))
    if g.min_points < 1:
        raise ValueError("geometry: min_points >= 1 required, got %d" % g.min_points)
    return g


def window(scene, centre_row, outer_half):
    """-> (cx, cy, x0, x1, y0, y1): the cell of stored row `centre_row` and the clipped window of cells around it, bounds inclusive"""
    cx, cy = divmod(int(scene.column[int(centre_row)]), scene.n_y)
    return (cx, cy, max(0, cx - outer_half), min(scene.n_x - 1, cx + outer_half), max(0, cy - outer_half),
            min(scene.n_y - 1, cy + outer_half))


def strips(scene, win):
    """-> (first, end) int64 [x1 - x0 + 1]: strip ix of the window is the stored rows [first, end)"""
    _cx, _cy, x0, x1, y0, y1 = win
    at = np.arange(x0, x1 + 1, dtype=np.int64) * scene.n_y
    return scene.col_start[at + y0].astype(np.int64), scene.col_start[at + y1 + 1].astype(np.int64)


def members(scene, win):
    """-> int64 [T]: the crop's stored rows, the strips in ascending ix and each in stored order; member t is element t"""
    first, end = strips(scene, win)
    return np.concatenate([np.arange(f, e, dtype=np.int64) for f, e in zip(first, end)] + [np.zeros((0,), dtype=np.int64)])


def centre_row(ck, attempt, n):
    """mulhi(hi32(draw(ck, CROP, attempt)), n)"""
    return int((int(feed._hi(feed.draw(ck, CROP, attempt))) * int(n)) >> 32)


def choose(scene, ck, g):
    """the attempt rule -> (attempt, centre row, window, T): the first attempt whose window holds >= min_points rows, else the
    one that holds the most (the lowest attempt on a tie)"""
    n = scene.column.shape[0]
    best = None
    for a in range(g.attempts):
        r = centre_row(ck, a, n)
        win = window(scene, r, g.outer_half)
        first, end = strips(scene, win)
        T = int((end - first).sum())
        if best is None or T > best[3]:
            best = (a, r, win, T)
        if T >= g.min_points:
            break
    return best


def inner_of(scene, rows, win, inner_half):
    """-> int32 [len(rows)]: 1 where the stored row's cell is within inner_half of the window's centre cell on both axes"""
    ix, iy = np.divmod(scene.column[rows].astype(np.int64), scene.n_y)
    return ((np.abs(ix - win[0]) <= inner_half) & (np.abs(iy - win[1]) <= inner_half)).astype(np.int32)


CropReference = collections.namedtuple("CropReference", "index crop kind theta tilt noise")


def crop_reference(pool_host, scene_ids, num_point, seed, step, augment, geometry):
    """The draws of one batch.  pool_host: the HostScenes of the pool; scene_ids [B]; geometry: a Geometry.
    -> CropReference(index [B, N] int32 — the stored row of its scene each output point takes;
                     crop [B, 4] int32 — scene id, centre row, attempt used, T;
                     kind, theta, tilt, noise — as feed.assemble_reference)
    A pure function of its arguments."""
    g = check_geometry(geometry)
    scene_ids = np.asarray(scene_ids, dtype=np.int64).reshape(-1)
    B, N = scene_ids.shape[0], int(num_point)
    if B <= 0 or N <= 0:
        raise ValueError("crop_reference: B>0 and num_point>0 required")
    if scene_ids.min() < 0 or scene_ids.max() >= len(pool_host):
        raise ValueError("scene id outside the pool")
    index = np.zeros((B, N), dtype=np.int32)
    crop = np.zeros((B, 4), dtype=np.int32)
    kind = np.zeros((B,), dtype=np.int32)
    theta = np.zeros((B,), dtype=np.float64)
    tilts = np.zeros((B, 3), dtype=np.float64)
    noise = np.zeros((B, N, 3), dtype=np.float64)
    third = B // 3
    for b in range(B):
        scene = pool_host[int(scene_ids[b])]
        ck = feed.cloud_key(seed, step, b)
        a, r, win, T = choose(scene, ck, g)
        t = feed.sample_without_replacement(ck, T, N) if T >= N else feed.sample_with_replacement(ck, T, N)
        index[b] = members(scene, win)[t]
        crop[b] = (scene_ids[b], r, a, T)
        if augment and b < third:
            kind[b], theta[b], tilts[b] = 1, feed.turn_angle(ck), feed.tilt_angles(ck)
        elif augment and b < 2 * third:
            kind[b], noise[b] = 2, feed.jitter_noise(ck, N)
    return CropReference(index, crop, kind, theta, tilts, noise)


def apply_reference(pool_host, ref, geometry):
    """the batch `ref` describes: -> points [B, N, 6] float64, label, inner [B, N] int32"""
    g = check_geometry(geometry)
    B, N = ref.index.shape
    points = np.zeros((B, N, 6), dtype=np.float64)
    label = np.zeros((B, N), dtype=np.int32)
    inner = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        scene = pool_host[int(ref.crop[b, 0])]
        rows = scene.rows[ref.index[b]]
        xyz = rows[:, 0:3].astype(np.float64)
        if ref.kind[b] == 1:
            xyz = feed.tilt(feed.turn(xyz, ref.theta[b]), ref.tilt[b])
        elif ref.kind[b] == 2:
            xyz = feed.jitter(xyz, ref.noise[b])
        points[b, :, 0:3], points[b, :, 3:6] = xyz, rows[:, 3:6]
        label[b] = rows[:, 6].astype(np.int32)
        inner[b] = inner_of(scene, ref.index[b], window(scene, ref.crop[b, 1], g.outer_half), g.inner_half)
    return points, label, inner


# ---------------------------------------------------------------------------------------------------------------
# the epoch plan (host, no device)
# ---------------------------------------------------------------------------------------------------------------
def default_crops_per_epoch(total_rows, num_point):
    return max(1, int(round(int(total_rows) / float(num_point))))


def scene_of_crop(sizes, crops_per_epoch):
    """-> int32 [E]: crop id e of an epoch goes to the scene that holds global row ((2 e + 1) T) // (2 E) of the pool — the
    midpoints of E equal shares of the T rows, so a scene of n rows gets n E / T crops to within one"""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    E, T = int(crops_per_epoch), int(sizes.sum())
    if E <= 0 or sizes.shape[0] == 0 or (sizes <= 0).any():
        raise ValueError("scene_of_crop: crops_per_epoch > 0 and non-empty scenes required")
    if (2 * E + 1) * T >= 1 << 63:
        raise ValueError("scene_of_crop: crops_per_epoch * rows too large")
    g = ((2 * np.arange(E, dtype=np.int64) + 1) * T) // (2 * E)
    return (np.searchsorted(np.cumsum(sizes), g, side="right")).astype(np.int32)


def epoch_scenes(sizes, crops_per_epoch, batch_size, seed, epoch, rank=0, world=1):
    """-> [(step, scene_ids int32 [b])] of rank `rank`: feed.epoch_plan over the epoch's crop ids, mapped by scene_of_crop"""
    table = scene_of_crop(sizes, crops_per_epoch)
    return [(step, table[ids]) for step, ids in feed.epoch_plan(int(crops_per_epoch), batch_size, seed, epoch, rank, world)]


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
class ScenePool:
    """Whole scenes in stored order, resident on the device, uploaded once: rows [T, 8] fp32 (xyz, rgb, label, 0), column [T]
    int32, index [T] int32 (a row's original position in its scene), col_start int32 (n_x n_y + 1 words per scene) and scene_tab
    int64 [S, 5] (row offset, col_start offset, n_x, n_y, n).  `sizes` [S] and `host_tab` stay on the host; `host` are the
    HostScenes (what crop_reference takes) when the pool was built with keep_host, else None."""

    def __init__(self, scenes, device=None, cell=DEFAULT_CELL, keep_host=False):
        import torch
        scenes = list(scenes)
        if not scenes:
            raise ValueError("empty pool")
        self.cell = float(_F32(cell))
        self.sizes = np.array([s.column.shape[0] for s in scenes], dtype=np.int64)
        self.host_tab = scene_table(scenes)
        self.device = torch.device(device if device is not None else "cuda:0")
        up = lambda parts: torch.from_numpy(np.ascontiguousarray(np.concatenate(parts, axis=0))).to(self.device)
        self.rows = up([s.rows for s in scenes])
        self.column = up([s.column for s in scenes])
        self.index = up([s.index for s in scenes])
        self.col_start = up([s.col_start for s in scenes])
        self.scene_tab = torch.from_numpy(self.host_tab).to(self.device)
        self.host = scenes if keep_host else None

    @classmethod
    def from_arrays(cls, scenes, device=None, cell=DEFAULT_CELL, max_columns=DEFAULT_MAX_COLUMNS, keep_host=False):
        """scenes: per scene (xyz [n, 3], rgb [n, 3], label [n]) as host arrays or device tensors (copied to the host once: the
        column sort is column_sort_reference itself)"""
        host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        return cls([sort_scene(host(x), host(c), host(l), cell, max_columns) for x, c, l in scenes], device, cell, keep_host)

    def __len__(self):
        return int(self.sizes.shape[0])


def assemble(pool, scene_ids, num_point, seed, step, augment=True, out=None, want_index=False, geometry=None):
    """sph3d_cropfeed_assemble on torch's current stream.  pool: a ScenePool; scene_ids [B] int32 on the device; geometry: a
    Geometry (default: crop_geometry(num_point, pool.cell)).  out: (points [B, N, 6] fp32, label, inner [B, N] i32, crop [B, 4] i32) to
    write into, else new tensors.  -> points, label, inner, crop (points, label, inner, index [B, N] i32, crop with want_index)"""
    import torch
    from .. import _lib
    g = check_geometry(geometry) if geometry is not None else crop_geometry(num_point, pool.cell)
    crop = None
    if out is not None:
        out, crop = tuple(out[:3]), out[3]
    B, N, (points, label, inner), index = feed.assemble_args(_lib, pool.rows, pool.scene_tab, scene_ids, "scene_ids", num_point, out,
                                                             feed._FEED_OUT, want_index)
    if crop is None:
        crop = torch.empty((B, 4), dtype=torch.int32, device=pool.rows.device)
    if crop.shape != (B, 4) or crop.dtype != torch.int32 or not crop.is_contiguous() or crop.device != pool.rows.device:
        raise ValueError("assemble: crop must be a contiguous int32 [B, 4] on the pool's device")
    _lib.check(_lib.lib().sph3d_cropfeed_assemble(
        B, N, len(pool), int(pool.rows.shape[0]), int(pool.col_start.shape[0]), _lib.ptr(pool.rows), _lib.ptr(pool.column),
        _lib.ptr(pool.col_start), _lib.ptr(pool.scene_tab), _lib.ptr(scene_ids), seed & 0xffffffffffffffff,
        step & 0xffffffffffffffff, 1 if augment else 0, g.inner_half, g.outer_half, g.attempts, g.min_points, _lib.ptr(points),
        _lib.ptr(label), _lib.ptr(inner), _lib.ptr(index), _lib.ptr(crop), _lib.stream_ptr()))
    return (points, label, inner, index, crop) if want_index else (points, label, inner, crop)


class CropFeed(feed.TwoSetFeed):
    """One epoch of training crops per iteration, cut out of a ScenePool on the device (feed.TwoSetFeed states the protocol and who
    owns an item's tensors).  An item is feed.DeviceFeed's: (points [b, N, 6], label, inner, ready).

        pool = sceneprep.prepare_training_scenes([(full_xyz, full_rgb, full_label), ...])
        feed = CropFeed(pool, 16, 8192, seed=1)
        trainer.train_one_epoch(feed)                            # train.Trainer with line=train.s3dis_line, unchanged

    An epoch is `crops_per_epoch` crops (default: max(1, round(T / num_point)), so an epoch shows about as many points as the
    pool holds); crop id e goes to the scene scene_of_crop names, so scenes are visited in proportion to their size, and the
    epoch's permutation of the ids is feed.epoch_plan's.  `crop_of(ready)` is the batch's crop record [b, 4] on the device."""

    def __init__(self, pool, batch_size, num_point, seed, crops_per_epoch=None, augment=True, block=1.5, context=0.3, attempts=4,
                 min_points=None, rank=0, world=1, stream=None, post=None):
        self.augment = bool(augment)
        self.geometry = crop_geometry(num_point, pool.cell, block, context, attempts, min_points)
        self.crops_per_epoch = int(crops_per_epoch) if crops_per_epoch is not None else \
            default_crops_per_epoch(pool.sizes.sum(), num_point)
        self._scene_of_crop = scene_of_crop(pool.sizes, self.crops_per_epoch)
        self._crop = {}                                   # points' address of a set -> [its crop tensor, the live batch's size]
        super().__init__(pool, batch_size, num_point, seed, rank, world, stream, post)

    def _new_set(self, dev):
        import torch
        out = (torch.empty((self.batch_size, self.num_point, 6), dtype=torch.float32, device=dev),
               torch.empty((self.batch_size, self.num_point), dtype=torch.int32, device=dev),
               torch.empty((self.batch_size, self.num_point), dtype=torch.int32, device=dev))
        self._crop[out[0].data_ptr()] = [torch.empty((self.batch_size, 4), dtype=torch.int32, device=dev), 0]
        return out

    def _epoch_ids(self):
        return self.crops_per_epoch

    def _map_ids(self, table):
        return self._scene_of_crop[table]

    def _launch(self, step, ids_dev, out):
        slot = self._crop[out[0].data_ptr()]
        slot[1] = int(ids_dev.shape[0])
        assemble(self.pool, ids_dev, self.num_point, self.seed, step, self.augment, out=out + (slot[0][:slot[1]],),
                 geometry=self.geometry)

    def crop_of(self, ready):
        """the crop record [b, 4] int32 (scene id, centre row, attempt, T) of the live item whose event is `ready`; a view of the
        item's output set, overwritten with it"""
        for s in self._sets:
            if s["ready"] is ready:
                crop, b = self._crop[s["out"][0].data_ptr()]
                return crop[:b]
        raise ValueError("crop_of(): not the ready event of a live item")
