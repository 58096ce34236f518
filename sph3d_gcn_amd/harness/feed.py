"""Training batches assembled on the device: the per-step half of the input side (blockio.sample_points / augment_batch) as one
kernel over a pool of parsed blocks that lives in HBM (csrc/feed.hip, include/sph3d.h: sph3d_feed_assemble).

  * ``assemble_reference``: the SPECIFICATION of the draws, in numpy, no GPU.  Every draw is a pure function of
    (seed, step, cloud, slot, purpose), so a batch is reproduced from two integers on any rank.  The kernel's integer outputs
    (index, label, inner) and everything it copies equal this statement bit for bit; what it computes in fp32 (angles, noise,
    rotated / jittered xyz) is held to the project's 1e-5 bound against the float64 evaluation given here;
  * ``BlockPool``: the parsed blocks [n, 8] of a dataset back to back on the device, uploaded once;
  * ``DeviceFeed``: one epoch of batches, assembled on the feed's own stream into two alternating output sets, each item with
    the event a GraphPlan takes as ``points_ready``;
  * ``assemble``: the C entry for callers who bring their own block ids.

What differs from the reference's loop, on purpose: its two shuffles (the blocks of a batch, the point order) are not separate
steps — the block ids arrive in random order and the sample is in random order already — and the random numbers are this
module's counter-based ones, not numpy's Mersenne twister.  The arithmetic (rotation about z, then Rz Ry Rx of three clipped
normal angles, on the first third; clipped normal noise on the second third; third = B // 3) is the reference's, checked against
its recorded results (tests/test_feed.py, tests/golden/blockio_ref.npz).
"""
import collections

import numpy as np

_U64 = np.uint64
_GOLD = _U64(0x9e3779b97f4a7c15)
ROUNDS = 6
PERM, REPL, TURN, TILT, JITTER = 1, 2, 3, 4, 5          # the `purpose` of a draw
IDS = 8                                                 # .. of the keyed inverse-density sampler: IDS + level (harness/idsample.py)

ANGLE_SIGMA, ANGLE_CLIP = 0.06, 0.18                    # utils/data_util.py:140
JITTER_SIGMA, JITTER_CLIP = 0.01, 0.02                  # utils/data_util.py:166


# ---------------------------------------------------------------------------------------------------------------
# the draws (csrc/feed.hip computes the same integers)
# ---------------------------------------------------------------------------------------------------------------
def _mix(z):
    """the splitmix64 finaliser on uint64 arrays (arithmetic modulo 2^64)"""
    z = np.asarray(z, dtype=_U64)
    z = (z ^ (z >> _U64(30))) * _U64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> _U64(27))) * _U64(0x94d049bb133111eb)
    return z ^ (z >> _U64(31))


def cloud_key(seed, step, b):
    with np.errstate(over="ignore"):
        k = _mix(_U64(seed & 0xffffffffffffffff) + _GOLD)
        k = _mix(k + _U64(step & 0xffffffffffffffff) + _GOLD)
        return _mix(k + np.asarray(b, dtype=_U64) + _GOLD)


def draw(ck, purpose, counter):
    """-> uint64 words w(purpose, counter) of the cloud with key ck; `counter` < 2^32 may be an array"""
    with np.errstate(over="ignore"):
        return _mix(_U64(ck) ^ (_U64(purpose << 56) | np.asarray(counter, dtype=_U64)))


def _hi(w):
    return (w >> _U64(32)).astype(np.uint32)


def _fmix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85ebca6b)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xc2b2ae35)
    return x ^ (x >> np.uint32(16))


def feistel_bits(n):
    """half the width of the permutation's domain: 2^k >= n > 2^(k-1), half = ceil(k / 2); the domain 2^(2 half) is < 4 n"""
    k = int(n - 1).bit_length()
    return (k + 1) >> 1


def sample_without_replacement(ck, n, num_point):
    """slot j -> pi(j), cycle-walked into [0, n): num_point distinct rows of n >= num_point, in an exchangeable order"""
    half = feistel_bits(n)
    mask = np.uint32((1 << half) - 1)
    sh = np.uint32(half)
    rk = _hi(draw(ck, PERM, np.arange(ROUNDS)))
    r = np.arange(num_point, dtype=np.uint32)
    todo = np.arange(num_point)
    with np.errstate(over="ignore"):
        while todo.size:
            v = r[todo]
            L, R = v >> sh, v & mask
            for t in range(ROUNDS):
                L, R = R, L ^ (_fmix32(R ^ rk[t]) & mask)
            v = (L << sh) | R
            r[todo] = v
            todo = todo[v >= np.uint32(n)]
    return r.astype(np.int32)


def sample_with_replacement(ck, n, num_point):
    """slot j -> floor(u n), u from 32 random bits (multiply-high)"""
    bits = _hi(draw(ck, REPL, np.arange(num_point))).astype(_U64)
    return ((bits * _U64(n)) >> _U64(32)).astype(np.int32)


def uniform(bits32):
    """(bits >> 8) * 2^-24 in [0, 1) — exact in fp32 and in float64"""
    return (np.asarray(bits32, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def normal_pair(w):
    """Box-Muller on one 64-bit draw: u1 = ((hi >> 8) + 1) 2^-24 in (0, 1], u2 from the low word -> two N(0,1), float64 (the
    kernel evaluates the same expression in fp32)"""
    w = np.asarray(w, dtype=_U64)
    u1 = ((_hi(w) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = uniform((w & _U64(0xffffffff)).astype(np.uint32))
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def turn_angle(ck):
    return 2.0 * np.pi * float(uniform(_hi(draw(ck, TURN, 0))))


def tilt_angles(ck):
    ax, ay = normal_pair(draw(ck, TILT, 0))
    az, _ = normal_pair(draw(ck, TILT, 1))
    return np.clip(ANGLE_SIGMA * np.array([ax, ay, az], dtype=np.float64), -ANGLE_CLIP, ANGLE_CLIP)


def jitter_noise(ck, num_point):
    j = np.arange(num_point, dtype=np.int64)
    z0, z1 = normal_pair(draw(ck, JITTER, 2 * j))
    z2, _ = normal_pair(draw(ck, JITTER, 2 * j + 1))
    return np.clip(JITTER_SIGMA * np.stack([z0, z1, z2], axis=1), -JITTER_CLIP, JITTER_CLIP)


# ---------------------------------------------------------------------------------------------------------------
# the transform, in float64 (row vectors times matrices, as utils/data_util.py:47-61,140-176 write it)
# ---------------------------------------------------------------------------------------------------------------
def turn_matrix(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def tilt_matrix(ax, ay, az):
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return np.dot(rz, np.dot(ry, rx))


def turn(xyz, theta):
    return np.dot(np.asarray(xyz, dtype=np.float64), turn_matrix(theta))


def tilt(xyz, angles):
    return np.dot(np.asarray(xyz, dtype=np.float64), tilt_matrix(*angles))


def jitter(xyz, noise):
    return np.asarray(xyz, dtype=np.float64) + noise


Reference = collections.namedtuple("Reference", "index kind theta tilt noise")


def assemble_reference(sizes, block_ids, num_point, seed, step, augment):
    """The draws of one batch.  sizes: rows per block of the pool; block_ids [B]: the blocks of the batch in batch order.
    -> Reference(index [B, N] int32 — the row of its block each output point takes;
                 kind [B] — 1 rotated, 2 jittered, 0 passed through;
                 theta [B], tilt [B, 3] — float64 angles of the rotated clouds (0 elsewhere);
                 noise [B, N, 3] — float64 noise of the jittered clouds (0 elsewhere))
    A pure function of its arguments."""
    sizes = np.asarray(sizes, dtype=np.int64)
    block_ids = np.asarray(block_ids, dtype=np.int64).reshape(-1)
    B, N = block_ids.shape[0], int(num_point)
    if B <= 0 or N <= 0:
        raise ValueError("assemble_reference: B>0 and num_point>0 required")
    if block_ids.min() < 0 or block_ids.max() >= sizes.shape[0]:
        raise ValueError("block id outside the pool")
    index = np.zeros((B, N), dtype=np.int32)
    kind = np.zeros((B,), dtype=np.int32)
    theta = np.zeros((B,), dtype=np.float64)
    tilts = np.zeros((B, 3), dtype=np.float64)
    noise = np.zeros((B, N, 3), dtype=np.float64)
    third = B // 3
    for b in range(B):
        n = int(sizes[block_ids[b]])
        if n <= 0:
            raise ValueError("empty block")
        if n >= 1 << 31:
            raise ValueError("block with 2^31 rows or more")
        ck = cloud_key(seed, step, b)
        index[b] = sample_without_replacement(ck, n, N) if n >= N else sample_with_replacement(ck, n, N)
        if augment and b < third:
            kind[b], theta[b], tilts[b] = 1, turn_angle(ck), tilt_angles(ck)
        elif augment and b < 2 * third:
            kind[b], noise[b] = 2, jitter_noise(ck, N)
    return Reference(index, kind, theta, tilts, noise)


def apply_reference(blocks, block_ids, ref):
    """the batch `ref` describes, from host blocks [n, 8]: -> points [B, N, 6] float64, label, inner [B, N] int32"""
    B, N = ref.index.shape
    points = np.zeros((B, N, 6), dtype=np.float64)
    label = np.zeros((B, N), dtype=np.int32)
    inner = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        rows = np.asarray(blocks[int(block_ids[b])])[ref.index[b]]
        xyz = rows[:, 0:3].astype(np.float64)
        if ref.kind[b] == 1:
            xyz = tilt(turn(xyz, ref.theta[b]), ref.tilt[b])
        elif ref.kind[b] == 2:
            xyz = jitter(xyz, ref.noise[b])
        points[b, :, 0:3], points[b, :, 3:6] = xyz, rows[:, 3:6]
        label[b], inner[b] = rows[:, 6].astype(np.int32), rows[:, 7].astype(np.int32)
    return points, label, inner


# ---------------------------------------------------------------------------------------------------------------
# the epoch plan (host, no device)
# ---------------------------------------------------------------------------------------------------------------
def batches_per_epoch(num_blocks, batch_size):
    return (num_blocks + batch_size - 1) // batch_size


def epoch_order(num_blocks, seed, epoch):
    """the epoch's block order: one permutation from (seed, epoch), the same on every rank"""
    key = np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff, epoch & 0xffffffff], dtype=np.uint32)
    return np.random.RandomState(key).permutation(num_blocks).astype(np.int32)


def epoch_plan(num_blocks, batch_size, seed, epoch, rank=0, world=1):
    """-> [(step, block_ids int32 [b])] of rank `rank`: the epoch's order cut into batches of batch_size (the last one may be
    smaller, like blockio.training_batches'), of which rank r takes r, r + world, ...; `step` is the batch's number counted
    over all ranks and epochs — the `step` of its draws, so a batch does not depend on how many ranks share the epoch"""
    if num_blocks <= 0 or batch_size <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError("epoch_plan: bad num_blocks / batch_size / rank / world")
    order = epoch_order(num_blocks, seed, epoch)
    per = batches_per_epoch(num_blocks, batch_size)
    return [(epoch * per + i, order[i * batch_size:(i + 1) * batch_size]) for i in range(rank, per, world)]


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
def assemble_args(_lib, rows, offsets, ids, ids_name, num_point, out, channels, want_index):
    """what feed.assemble and objfeed.assemble do before they launch: the checks of the pool's tensors and the ids, and the
    outputs.  channels: per output its shape after [B, N]; the first output is fp32, the others int32.  `out` is checked
    against that, or allocated where it is None; index is a new int32 [B, N] with want_index, else None.
    -> B, N, out, index.  (`_lib` is the caller's: importing it here again would cost every call 0.8 us on the host, as much
    as all the checks together.)"""
    import torch
    _lib.require_device(rows, offsets, ids)
    if rows.dtype != torch.float32 or offsets.dtype != torch.int64 or ids.dtype != torch.int32:
        raise TypeError("assemble: rows fp32, offsets int64, %s int32" % ids_name)
    if rows.dim() != 2 or rows.shape[1] != 8 or not (rows.is_contiguous() and offsets.is_contiguous() and ids.is_contiguous()):
        raise ValueError("assemble: rows must be a contiguous [T, 8], offsets and %s contiguous" % ids_name)
    B, N, dev = int(ids.shape[0]), int(num_point), rows.device
    if out is None:
        out = tuple(torch.empty((B, N) + c, dtype=torch.int32 if k else torch.float32, device=dev) for k, c in enumerate(channels))
    bn, dt = (B, N), torch.float32
    for t, c in zip(out, channels):                   # (an `out` of another length fails where the caller unpacks it)
        if t.shape != bn + c or t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError("assemble: output of the wrong shape, type, layout or device")
        dt = torch.int32
    return B, N, out, torch.empty((B, N), dtype=torch.int32, device=dev) if want_index else None


def assemble(rows, offsets, block_ids, num_point, seed, step, augment=True, out=None, want_index=False):
    """sph3d_feed_assemble on torch's current stream.  rows [T, 8] fp32, offsets [P+1] int64, block_ids [B] int32, all on the
    device.  out: (points [B, N, 6] fp32, label [B, N] i32, inner [B, N] i32) to write into, else new tensors.
    -> points, label, inner (and index [B, N] i32 with want_index)"""
    from .. import _lib
    B, N, (points, label, inner), index = assemble_args(_lib, rows, offsets, block_ids, "block_ids", num_point, out, _FEED_OUT,
                                                        want_index)
    _lib.check(_lib.lib().sph3d_feed_assemble(B, N, int(offsets.shape[0]) - 1, int(rows.shape[0]), _lib.ptr(rows), _lib.ptr(offsets),
                                              _lib.ptr(block_ids), seed & 0xffffffffffffffff, step & 0xffffffffffffffff,
                                              1 if augment else 0, _lib.ptr(points), _lib.ptr(label), _lib.ptr(inner),
                                              _lib.ptr(index), _lib.stream_ptr()))
    return (points, label, inner, index) if want_index else (points, label, inner)


_FEED_OUT = ((6,), (), ())          # the shapes after [B, N] of points (fp32), label and inner (int32)


def check_scene_index(blocks, index, scene_of_block):
    """what a pool with a scene index must satisfy (host, no device) -> (index int32 [T], scene_of_block int64 [P]):
    one index array per block, as long as the block, values >= 0; the blocks of a scene consecutive; and the index values of a
    block's INNER rows distinct — the reference's `predictions(idx,:) = predictions(idx,:) + p` would silently keep the last of
    duplicates; its record writer produces none, and they are refused here rather than reproduced"""
    index = [np.ascontiguousarray(np.asarray(i).reshape(-1), dtype=np.int32) for i in index]
    scene_of_block = np.ascontiguousarray(np.asarray(scene_of_block).reshape(-1), dtype=np.int64)
    if len(index) != len(blocks) or scene_of_block.shape[0] != len(blocks):
        raise ValueError("index and scene_of_block have one entry per block")
    seen = set()
    for k, (b, i) in enumerate(zip(blocks, index)):
        if i.shape[0] != b.shape[0]:
            raise ValueError("block %d: %d index values for %d rows" % (k, i.shape[0], b.shape[0]))
        if i.size and i.min() < 0:
            raise ValueError("block %d: negative index value" % k)
        inner = i[b[:, 7] == 1]
        if np.unique(inner).shape[0] != inner.shape[0]:
            raise ValueError("block %d: two inner rows share an index value" % k)
        s = int(scene_of_block[k])
        if s < 0:
            raise ValueError("block %d: negative scene number" % k)
        if k and s != int(scene_of_block[k - 1]) and s in seen:
            raise ValueError("the blocks of scene %d are not consecutive" % s)
        seen.add(s)
    return np.concatenate(index), scene_of_block


class BlockPool:
    """The parsed blocks of a dataset, resident on the device: rows [T, 8] fp32 (blockio.parse_block's layout) back to back and
    offsets [P+1] int64, uploaded once; `sizes` stays on the host.  With `index` (per block: int32 [n], the rows' positions in
    their scene's voxel cloud) and `scene_of_block` [P] the pool also knows its scenes (harness/scenemerge.py): `index` [T]
    int32 on the device, `scene_of_block` on the host, checked by check_scene_index.  Without them both are None."""

    def __init__(self, blocks, device=None, index=None, scene_of_block=None):
        import torch
        blocks = [np.ascontiguousarray(b, dtype=np.float32) for b in blocks]
        if not blocks:
            raise ValueError("empty pool")
        for b in blocks:
            if b.ndim != 2 or b.shape[1] != 8:
                raise ValueError("a block is [n, 8]: xyz, rgb, label, inner")
            if b.shape[0] == 0:
                raise ValueError("empty block")
        if (index is None) != (scene_of_block is None):
            raise ValueError("index and scene_of_block come together")
        host_index = None
        if index is not None:
            host_index, scene_of_block = check_scene_index(blocks, index, scene_of_block)
        self.sizes = np.array([b.shape[0] for b in blocks], dtype=np.int64)
        self.host_offsets = np.concatenate(([0], np.cumsum(self.sizes))).astype(np.int64)
        self.device = torch.device(device if device is not None else "cuda:0")
        self.rows = torch.from_numpy(np.concatenate(blocks, axis=0)).to(self.device)
        self.offsets = torch.from_numpy(self.host_offsets).to(self.device)
        self.scene_of_block = scene_of_block
        self.index = torch.from_numpy(host_index).to(self.device) if host_index is not None else None

    @classmethod
    def from_blocks(cls, blocks, device=None):
        return cls(blocks, device)

    @classmethod
    def from_records(cls, paths, device=None, verify=True, with_index=False):
        """with_index: also keep the records' index_label, and number the scenes by file — one record file is one scene, in
        path order (the records' own scene_idx is not consulted)"""
        from . import blockio
        if not with_index:
            return cls([blockio.parse_block(r) for p in paths for r in blockio.read_records(p, verify=verify)], device)
        blocks, index, scene = [], [], []
        for s, p in enumerate(paths):
            for r in blockio.read_records(p, verify=verify):
                blocks.append(blockio.parse_block(r))
                index.append(blockio.parse_block_index(r)[0])
                scene.append(s)
        return cls(blocks, device, index, scene)

    @classmethod
    def from_device(cls, rows, offsets, sizes, index, scene_of_block):
        """a pool whose tensors are on the device already (harness/sceneprep.py: sph3d_prep_block_fill wrote them): rows [T, 8]
        fp32, offsets [P+1] int64 and index [T] int32 device tensors, taken as they are — no host copy of the rows; sizes [P]
        and scene_of_block [P] on the host.  check_scene_index is NOT run: what it checks holds by construction for the
        block fill — a block's index values are the voxel rows inside a rectangle in ascending order, hence distinct and
        non-negative — and the caller numbers the scenes consecutively; only the shapes and the scene order are checked here"""
        import torch
        sizes = np.ascontiguousarray(np.asarray(sizes).reshape(-1), dtype=np.int64)
        scene_of_block = np.ascontiguousarray(np.asarray(scene_of_block).reshape(-1), dtype=np.int64)
        for t in (rows, offsets, index):
            if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.device == rows.device):
                raise ValueError("from_device: rows, offsets and index are contiguous tensors on one device")
        P, T = int(sizes.shape[0]), int(sizes.sum())
        if P == 0 or (sizes <= 0).any():
            raise ValueError("empty pool or empty block")
        if rows.dtype != torch.float32 or tuple(rows.shape) != (T, 8) or index.dtype != torch.int32 or tuple(index.shape) != (T,):
            raise ValueError("from_device: rows [T, 8] fp32 and index [T] int32 with T = sum of sizes expected")
        if offsets.dtype != torch.int64 or tuple(offsets.shape) != (P + 1,):
            raise ValueError("from_device: offsets [P+1] int64 expected")
        if scene_of_block.shape[0] != P or scene_of_block.min() < 0 or (np.diff(scene_of_block) < 0).any():
            raise ValueError("from_device: scene_of_block has one non-negative entry per block, ascending")
        self = cls.__new__(cls)
        self.sizes = sizes
        self.host_offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        self.device = rows.device
        self.rows, self.offsets, self.index, self.scene_of_block = rows, offsets, index, scene_of_block
        return self

    def __len__(self):
        return int(self.sizes.shape[0])


class TwoSetFeed:
    """The protocol DeviceFeed and harness/objfeed.py's ObjectFeed share: one epoch of batches per iteration, assembled on the
    feed's own stream into two alternating output sets.  A subclass says how a set is allocated (`_new_set`), what is launched
    for one batch (`_launch`) and, if anything, what an epoch uploads besides its table (`_begin_epoch`); one whose epoch is not
    one visit per block says how many ids an epoch permutes (`_epoch_ids`) and how they become pool ids (`_map_ids`).

    The epoch's order is one host permutation from (seed, epoch), identical on every rank; rank r takes batches r, r + world,
    ...; the last batch may be smaller.  The kernel runs on the feed's own stream (`stream`, else one the feed creates);
    `ready`, the last element of an item, is recorded behind it: hand it to the model as `points_ready`, or `wait_event` it on
    the consuming stream (the labels are consumed by the loss on the main stream: it must wait too — the model's plan does
    that for the streams it uses when it gets `points_ready`, see s3dis_net.GraphPlan).

    OWNERSHIP.  The tensors of an item are views of one of TWO preallocated output sets used alternately (no per-step
    allocation crosses streams), so item i is overwritten by item i+2: the consumer must have ISSUED all its work on item i
    before it asks for item i+2, and must not keep the tensors (clone what has to outlive the next step).  Before the feed
    overwrites a set it waits, on its stream, for the event handed back with `done(ready[, event])` for that set — or, when
    none was handed back, for everything issued so far on the stream that is current when the next item is asked for.  The
    second form is safe and slow: item i+2 is then assembled behind ALL of step i+1, so the plan of step i+2 no longer overlaps
    the step before it (+20 % per step); hand the event back, as early as the last reader of the batch.

    POST.  `post`, if given, is called as post(seed, step, out) behind every batch's launch, with the feed's stream current and
    before `ready` is recorded: a second stage that works in place on the assembled set (harness/augment.py: Stage).  Without
    it a feed launches exactly what its `_launch` launches."""

    def __init__(self, pool, batch_size, num_point, seed, rank=0, world=1, stream=None, post=None):
        import torch
        if batch_size <= 0 or num_point <= 0:
            raise ValueError("%s: batch_size>0 and num_point>0 required" % type(self).__name__)
        if world <= 0 or not 0 <= rank < world:
            raise ValueError("%s: bad rank / world" % type(self).__name__)
        self.pool, self.batch_size, self.num_point, self.seed = pool, int(batch_size), int(num_point), int(seed)
        self.rank, self.world, self.epoch = int(rank), int(world), 0
        self.stream = stream if stream is not None else torch.cuda.Stream(device=pool.device)
        self.post = post
        self._sets = [{"out": self._new_set(pool.device), "ready": torch.cuda.Event(), "released": None, "used": False}
                      for _ in range(2)]
        self._turn = 0

    def _new_set(self, dev):
        """-> the tensors of one output set, each with batch_size leading rows"""
        raise NotImplementedError

    def _launch(self, step, ids_dev, out):
        """fill `out` (a set cut to the batch's size) with the batch of ids_dev; torch's current stream is the feed's"""
        raise NotImplementedError

    def _begin_epoch(self, plan):
        """what an epoch uploads besides its table; torch's current stream is the feed's"""

    def _epoch_ids(self):
        """how many ids an epoch permutes (default: one per block of the pool)"""
        return len(self.pool)

    def _map_ids(self, table):
        """the epoch's id table [batches, batch_size] int32 -> the pool ids that go up (default: the ids themselves)"""
        return table

    def __len__(self):
        """batches of this rank per epoch"""
        return len(range(self.rank, batches_per_epoch(self._epoch_ids(), self.batch_size), self.world))

    def done(self, ready, event=None):
        """the consumer is finished with the item whose event is `ready`: after `event` (default: one recorded now on the current
        stream) its set may be overwritten"""
        import torch
        for s in self._sets:
            if s["ready"] is ready:
                if event is None:
                    event = torch.cuda.Event()
                    event.record()
                s["released"] = event
                return
        raise ValueError("done(): not the ready event of a live item")

    def _assemble(self, step, ids_dev, b):
        import torch
        s = self._sets[self._turn]
        self._turn ^= 1
        if s["used"]:
            if s["released"] is not None:
                self.stream.wait_event(s["released"])
            else:
                self.stream.wait_stream(torch.cuda.current_stream(self.pool.device))
        s["released"], s["used"] = None, True
        out = tuple(t[:b] for t in s["out"])
        with torch.cuda.stream(self.stream):
            self._launch(step, ids_dev, out)
            if self.post is not None:
                self.post(self.seed, step, out)
            s["ready"].record(self.stream)
        return out + (s["ready"],)

    def __iter__(self):
        import torch
        plan = epoch_plan(self._epoch_ids(), self.batch_size, self.seed, self.epoch, self.rank, self.world)
        self.epoch += 1
        if not plan:
            return
        # the ids of the whole epoch go up in one copy (a row per batch, the last one padded): no host copy per step
        table = np.zeros((len(plan), self.batch_size), dtype=np.int32)
        for i, (_step, ids) in enumerate(plan):
            table[i, :len(ids)] = ids
        self.stream.wait_stream(torch.cuda.current_stream(self.pool.device))      # (the pool's upload, a previous epoch's table)
        with torch.cuda.stream(self.stream):
            table_dev = torch.from_numpy(self._map_ids(table)).to(self.pool.device)
            self._begin_epoch(plan)
        for i, (step, ids) in enumerate(plan):
            yield self._assemble(step, table_dev[i, :len(ids)], len(ids))


class DeviceFeed(TwoSetFeed):
    """One epoch of S3DIS training batches per iteration, assembled on the device (TwoSetFeed states the protocol and who owns
    an item's tensors).

        feed = DeviceFeed(pool, 16, 8192, seed=1)
        for points, label, inner, ready in feed:                 # epoch 0; the next `for` is epoch 1
            pred, _ = model(points, is_training=True, points_ready=ready)
            loss = model.loss(pred, label, inner)
            feed.done(ready)                                     # the batch's last reader is issued
            ...                                                  # backward, optimiser
    """

    def __init__(self, pool, batch_size, num_point, seed, augment=True, rank=0, world=1, stream=None, post=None):
        self.augment = bool(augment)
        super().__init__(pool, batch_size, num_point, seed, rank, world, stream, post)

    def _new_set(self, dev):
        import torch
        return (torch.empty((self.batch_size, self.num_point, 6), dtype=torch.float32, device=dev),
                torch.empty((self.batch_size, self.num_point), dtype=torch.int32, device=dev),
                torch.empty((self.batch_size, self.num_point), dtype=torch.int32, device=dev))

    def _launch(self, step, ids_dev, out):
        assemble(self.pool.rows, self.pool.offsets, ids_dev, self.num_point, self.seed, step, self.augment, out=out)
