"""Batches of the RueMonge2014 facade line assembled on the device: what ruemonge2014_seg/train_ruemonge2014.py:98-138 does per
step on the host and the augmented passes of ruemonge2014_seg/evaluate_ruemonge2014.py:180-305, as one kernel over a pool of
facade splits that lives in HBM (csrc/facadefeed.hip, include/sph3d.h: sph3d_facadefeed_assemble).

  * ``facade_from_columns`` / ``read_facade_txt`` / ``encode_facade`` / ``parse_facade`` / ``write_facade_records`` /
    ``read_facade_records``: the record of io/make_tfrecord_ruemonge2014.py:45-57 — ONE record is one whole facade split with
    `xyz_raw`, `normal_raw`, `rgb_raw` (fp32 [n, 3]) and `seg_label` (int32 [n]); xy centred on the mean, z on its minimum,
    rgb = 2 rgb / 255 - 1.  There is no inner / outer distinction: every row counts;
  * ``FacadePool``: the facades as blocks of a ``feed.BlockPool`` — rows [n, 8] with xyz, rgb, the label and inner == 1, so the
    vote kernels read the pool unchanged — plus `normals` [T, 4] (nx, ny, nz, 0: one aligned 16-byte row per point);
  * ``assemble_reference`` / ``apply_reference``: the SPECIFICATION in numpy, no GPU.  The draws are ``objfeed``'s, unchanged:
    the same sample (`index` does not depend on the recipe), the same five bits with the same purposes and counters.  What is
    new is that TURN and TILT multiply the NORMAL by the same matrices as xyz (utils/data_util.py:64-105); SCALE, SHIFT and
    JITTER touch xyz only; rgb and the label are copied.  The kernel's integer outputs and every channel it copies equal this
    statement bit for bit; what it computes in fp32 is held to the project's 1e-5 bound against the float64 evaluation;
  * ``train_recipe`` / ``EVAL_AUGMENT``: the reference's recipes as per-cloud bit masks;
  * ``assemble``: the C entry;  ``FacadeFeed``: one epoch of batches on the feed's own stream (``feed.TwoSetFeed``).

The network input is [B, N, 9] with the channels in the reference's order xyz, normal, rgb (train_ruemonge2014.py:159).

What differs from the reference's loop, on purpose — as in feed.py and objfeed.py: the facades of a batch arrive in random
order from the epoch plan and the sample is in random order already, so its two shuffles are not separate steps; the random
numbers are this project's counter-based ones.  The arithmetic is the reference's, checked against its recorded results
(tests/test_facadefeed.py, tests/golden/facade_ref.npz).
"""
import numpy as np

from . import blockio, feed, objfeed
from .objfeed import ALL, JITTER, SCALE, SHIFT, TILT, TURN, check_recipe  # noqa: F401

EVAL_AUGMENT = TURN | TILT                               # evaluate_ruemonge2014.py: every pass is turned and tilted
REPEAT = 100                                             # train_ruemonge2014.py: np.tile(trainlist, 100)
CHANNELS = 9


# ---------------------------------------------------------------------------------------------------------------
# the record (io/make_tfrecord_ruemonge2014.py:45-57)
# ---------------------------------------------------------------------------------------------------------------
def facade_from_columns(data):
    """data [n, 10]: xyz, rgb (0..255), normal, label — the columns of a split's text file
    -> (xyz, normal, rgb fp32 [n, 3], seg_label int32 [n]) as the record writer forms them, in fp32: xy minus its mean, z minus
    its minimum, rgb = 2 rgb / 255 - 1"""
    data = np.array(data, dtype=np.float32)
    if data.ndim != 2 or data.shape[1] != 10 or data.shape[0] == 0:
        raise ValueError("facade_from_columns: [n, 10] with n > 0 expected (xyz, rgb, normal, label)")
    xyz = data[:, 0:3]
    center = np.mean(xyz, axis=0)
    center[2] = np.amin(xyz[:, 2], axis=0)
    xyz = xyz - center
    rgb = 2 * data[:, 3:6] / 255.0 - 1
    return xyz, data[:, 6:9].copy(), rgb, np.int32(data[:, 9])


def read_facade_txt(path):
    """a split's text file (10 comma-separated columns) -> facade_from_columns of it"""
    return facade_from_columns(np.loadtxt(path, dtype=np.float32, delimiter=",", ndmin=2))


def _checked(xyz, normal, rgb, seg_label, what):
    xyz, normal, rgb = (np.ascontiguousarray(a, dtype="<f4") for a in (xyz, normal, rgb))
    seg_label = np.ascontiguousarray(np.asarray(seg_label).reshape(-1), dtype="<i4")
    n = xyz.shape[0]
    if xyz.ndim != 2 or n == 0 or not (xyz.shape == normal.shape == rgb.shape == (n, 3)) or seg_label.shape != (n,):
        raise ValueError("%s: xyz, normal, rgb [n, 3] and seg_label [n] with n > 0 expected" % what)
    return xyz, normal, rgb, seg_label


def encode_facade(xyz, normal, rgb, seg_label):
    """one facade record with the feature names and raw layouts of io/make_tfrecord_ruemonge2014.py:70-78"""
    xyz, normal, rgb, seg_label = _checked(xyz, normal, rgb, seg_label, "encode_facade")
    return blockio.encode_example({"xyz_raw": xyz.tobytes(), "normal_raw": normal.tobytes(), "rgb_raw": rgb.tobytes(),
                                   "seg_label": seg_label.tobytes()})


def parse_facade(record):
    """-> (xyz, normal, rgb fp32 [n, 3], seg_label int32 [n])"""
    ex = blockio.decode_example(record)
    xyz, normal, rgb = (np.frombuffer(ex[k], dtype="<f4").reshape(-1, 3) for k in ("xyz_raw", "normal_raw", "rgb_raw"))
    seg = np.frombuffer(ex["seg_label"], dtype="<i4")
    if not (len(xyz) == len(normal) == len(rgb) == len(seg)):
        raise ValueError("facade record with inconsistent array lengths")
    return xyz, normal, rgb, seg


def write_facade_records(path, facades):
    """facades: (xyz, normal, rgb, seg_label) per record (the reference writes one per file)"""
    blockio.write_records(path, [encode_facade(*f) for f in facades])


def read_facade_records(path, verify=True):
    return [parse_facade(r) for r in blockio.read_records(path, verify=verify)]


# ---------------------------------------------------------------------------------------------------------------
# the pool
# ---------------------------------------------------------------------------------------------------------------
def facade_blocks(xyz, normal, rgb, seg_label):
    """a facade as a block of a feed.BlockPool and its normals: -> (rows [n, 8] fp32: xyz, rgb, label, inner == 1;
    normals [n, 4] fp32: nx, ny, nz, 0).  n == 0, wrong shapes and non-finite normals are refused"""
    xyz, normal, rgb, seg_label = _checked(xyz, normal, rgb, seg_label, "facade_blocks")
    if not np.isfinite(normal).all():
        raise ValueError("facade_blocks: non-finite normal")
    n = xyz.shape[0]
    rows, normals = np.zeros((n, 8), dtype=np.float32), np.zeros((n, 4), dtype=np.float32)
    rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7] = xyz, rgb, seg_label, 1.0
    normals[:, 0:3] = normal
    return rows, normals


class FacadePool:
    """The facade splits of a dataset resident on the device: `pool`, a feed.BlockPool of facade_blocks rows (inner == 1
    everywhere: every row is voted on), and `normals` [T, 4] fp32 in the same row order.  It has the BlockPool's face (rows,
    offsets, sizes, host_offsets, device, len), so it stands where the vote kernels and the evaluation take a pool."""

    def __init__(self, blocks, normals, device=None):
        import torch
        blocks, normals = [np.asarray(b) for b in blocks], [np.ascontiguousarray(m, dtype=np.float32) for m in normals]
        if len(blocks) != len(normals):
            raise ValueError("FacadePool: one normals array per facade expected")
        for b, m in zip(blocks, normals):
            if b.ndim != 2 or b.shape[1] != 8 or b.shape[0] == 0 or not (b[:, 7] == 1).all():
                raise ValueError("FacadePool: a facade is facade_blocks' [n, 8] with n > 0 and column 7 equal to 1")
            if m.shape != (b.shape[0], 4) or m[:, 3].any() or not np.isfinite(m).all():
                raise ValueError("FacadePool: normals are facade_blocks' [n, 4]: finite, column 3 zero")
        self.pool = feed.BlockPool(blocks, device)
        self.normals = torch.from_numpy(np.concatenate(normals, axis=0)).to(self.pool.device)

    @classmethod
    def from_arrays(cls, xyz, normal, rgb, label, device=None):
        """per facade: xyz, normal, rgb [n, 3] and label [n]"""
        pairs = [facade_blocks(*f) for f in zip(xyz, normal, rgb, label)]
        return cls([p[0] for p in pairs], [p[1] for p in pairs], device)

    @classmethod
    def from_arrays_estimated(cls, xyz, rgb, label, radius, toward=None, device=None):
        """per facade: xyz, rgb [n, 3] and label [n], no normals: they are estimated on the device, per facade, from all points
        within `radius` (harness/normals.py: estimate_pool; toward: None or the [3] point the normals face)"""
        from . import normals as _normals
        self = cls.from_arrays(xyz, [np.zeros(np.shape(x), dtype=np.float32) for x in xyz], rgb, label, device)
        self.normals = _normals.estimate_pool(self.pool, radius, toward)
        return self

    @classmethod
    def from_records(cls, paths, device=None, verify=True):
        """every record of every file is one facade, in path order"""
        pairs = [facade_blocks(*f) for p in paths for f in read_facade_records(p, verify=verify)]
        return cls([p[0] for p in pairs], [p[1] for p in pairs], device)

    rows = property(lambda self: self.pool.rows)
    offsets = property(lambda self: self.pool.offsets)
    sizes = property(lambda self: self.pool.sizes)
    host_offsets = property(lambda self: self.pool.host_offsets)
    device = property(lambda self: self.pool.device)

    def __len__(self):
        return len(self.pool)


# ---------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------
def train_recipe(B):
    """-> recipe [B] int32 of a training batch (train_ruemonge2014.py:98-138, third = B // 3): the first third is turned and
    tilted — normals included — then scaled, shifted and jittered (31); the second third is scaled, shifted and jittered (28);
    the rest is untouched (0)"""
    return objfeed.train_recipe(B, "shapenet")


def assemble_reference(sizes, ids, num_point, seed, step, recipe):
    """The draws of one batch: objfeed.assemble_reference, unchanged — index [B, N] int32 (feed.assemble_reference's, whatever
    the recipe), recipe [B], theta [B], tilt [B, 3], scale [B], shift [B, 3], noise [B, N, 3]"""
    return objfeed.assemble_reference(sizes, ids, num_point, seed, step, recipe)


def transform(xyz, normal, mask, theta=0.0, tilt=(0.0, 0.0, 0.0), scale=1.0, shift=(0.0, 0.0, 0.0), noise=0.0):
    """one cloud's transform in float64: xyz, normal [N, 3] -> (xyz, normal).  xyz: objfeed.transform; the normal takes the
    turn and the tilt with the same matrices (utils/data_util.py:64-105) and nothing else"""
    return (objfeed.transform(xyz, mask, theta, tilt, scale, shift, noise),
            objfeed.transform(normal, mask & (TURN | TILT), theta, tilt))


def apply_reference(blocks, normals, ids, ref):
    """the batch `ref` describes, from host facades (facade_blocks' rows [n, 8] and normals [n, 4]):
    -> points [B, N, 9] float64 (xyz, normal, rgb), label [B, N] int32"""
    B, N = ref.index.shape
    points = np.zeros((B, N, CHANNELS), dtype=np.float64)
    label = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        rows = np.asarray(blocks[int(ids[b])])[ref.index[b]]
        nrm = np.asarray(normals[int(ids[b])])[ref.index[b], 0:3]
        points[b, :, 0:3], points[b, :, 3:6] = transform(rows[:, 0:3], nrm, int(ref.recipe[b]), ref.theta[b], ref.tilt[b],
                                                         ref.scale[b], ref.shift[b], ref.noise[b])
        points[b, :, 6:9] = rows[:, 3:6]
        label[b] = rows[:, 6].astype(np.int32)
    return points, label


def epoch_plan(num_facades, batch_size, seed, epoch, rank=0, world=1, repeat=REPEAT):
    """-> [(step, facade ids int32 [b])] of rank `rank`: feed.epoch_plan over num_facades * repeat virtual ids — one permutation
    per epoch, the same on every rank — where virtual id v is facade v % num_facades, so that every facade occurs `repeat` times
    per epoch (np.tile(trainlist, 100)).  A batch may hold the same facade twice: its clouds still differ, the cloud key
    depends on the position in the batch"""
    if num_facades <= 0 or repeat <= 0 or num_facades * repeat >= 1 << 31:
        raise ValueError("epoch_plan: num_facades>0, repeat>0 and num_facades*repeat<2^31 required")
    return [(step, (v % num_facades).astype(np.int32))
            for step, v in feed.epoch_plan(num_facades * repeat, batch_size, seed, epoch, rank, world)]


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
def assemble(rows, normals, offsets, ids, num_point, seed, step, recipe, out=None, want_index=False):
    """sph3d_facadefeed_assemble on torch's current stream.  rows [T, 8] fp32, normals [T, 4] fp32, offsets [P+1] int64,
    ids [B] int32, all on the device.  recipe: a host array of B masks or one mask for all (checked here: masks outside [0, 31]
    are refused, then uploaded), or an int32 device tensor [B] that check_recipe has seen before its upload.
    out: (points [B, N, 9] fp32, label [B, N] i32) to write into, else new tensors.
    -> points, label (and index [B, N] i32 with want_index)"""
    import torch
    from .. import _lib
    B, N, (points, label), index = feed.assemble_args(_lib, rows, offsets, ids, "ids", num_point, out, _FACADE_OUT, want_index)
    _lib.require_device(normals)
    if (normals.dtype != torch.float32 or tuple(normals.shape) != (int(rows.shape[0]), 4) or not normals.is_contiguous()
            or normals.device != rows.device):
        raise ValueError("assemble: normals must be a contiguous fp32 [T, 4] on the rows' device")
    if torch.is_tensor(recipe):
        _lib.require_device(recipe)
        if recipe.dtype != torch.int32 or tuple(recipe.shape) != (B,) or not recipe.is_contiguous():
            raise ValueError("assemble: a device recipe is a contiguous int32 [B]")
    else:
        recipe = torch.from_numpy(check_recipe(recipe, B)).to(rows.device)
    _lib.check(_lib.lib().sph3d_facadefeed_assemble(B, N, int(offsets.shape[0]) - 1, int(rows.shape[0]), _lib.ptr(rows),
                                                    _lib.ptr(normals), _lib.ptr(offsets), _lib.ptr(ids),
                                                    seed & 0xffffffffffffffff, step & 0xffffffffffffffff, _lib.ptr(recipe),
                                                    _lib.ptr(points), _lib.ptr(label), _lib.ptr(index), _lib.stream_ptr()))
    return (points, label, index) if want_index else (points, label)


_FACADE_OUT = ((CHANNELS,), ())     # the shapes after [B, N] of points (fp32) and label (int32)


class FacadeFeed(feed.TwoSetFeed):
    """One epoch of RueMonge2014 training batches per iteration, assembled on the device (feed.TwoSetFeed states the protocol
    and who owns an item's tensors).

        feed = FacadeFeed(pool, 16, 8192, seed=1)
        for points, label, ready in feed:                        # epoch 0; the next `for` is epoch 1
            pred, _ = model(points, is_training=True, points_ready=ready)
            torch.cuda.current_stream().wait_event(ready)        # (the loss reads label on the main stream)
            loss = model.loss(pred, label)
            feed.done(ready)
            ...

    An epoch visits every facade `repeat` times (epoch_plan above).  The last, smaller batch gets train_recipe of its own size.
    `recipe`: a mask for every cloud instead of the training recipe (0: no augmentation)."""

    def __init__(self, pool, batch_size, num_point, seed, repeat=REPEAT, recipe=None, rank=0, world=1, stream=None, post=None):
        self.repeat = int(repeat)
        if self.repeat <= 0 or len(pool) * self.repeat >= 1 << 31:
            raise ValueError("FacadeFeed: repeat>0 and len(pool)*repeat<2^31 required")
        super().__init__(pool, batch_size, num_point, seed, rank, world, stream, post)
        self._recipe = train_recipe if recipe is None else (lambda b: check_recipe(int(recipe), b))
        self._recipe(self.batch_size)                       # (a bad mask fails here, not in the first epoch)
        self._recipes = {}

    def _epoch_ids(self):
        return len(self.pool) * self.repeat

    def _map_ids(self, table):
        return table % np.int32(len(self.pool))

    def _new_set(self, dev):
        import torch
        return (torch.empty((self.batch_size, self.num_point, CHANNELS), dtype=torch.float32, device=dev),
                torch.empty((self.batch_size, self.num_point), dtype=torch.int32, device=dev))

    def _begin_epoch(self, plan):
        import torch
        for b in set(len(ids) for _step, ids in plan) - set(self._recipes):
            self._recipes[b] = torch.from_numpy(self._recipe(b)).to(self.pool.device)

    def _launch(self, step, ids_dev, out):
        assemble(self.pool.rows, self.pool.normals, self.pool.offsets, ids_dev, self.num_point, self.seed, step,
                 self._recipes[int(ids_dev.shape[0])], out=out)
