"""The augmentation stage: a second step behind the feeds, in place on an assembled batch (csrc/augment.hip, include/sph3d.h:
sph3d_augment_apply).  The feeds keep the reference's 2019 recipe; this adds what the indoor-segmentation recipes published since
use: Mix3D scene mixing, flips, anisotropic scaling, elastic distortion, and chromatic auto-contrast, translation, jitter and drop.

  * ``apply_reference``: the SPECIFICATION, in numpy, float64, no GPU — a pure function of its arguments, so an augmented batch is
    still reproduced from (seed, step) on any rank.  The kernels' integer outputs (label, inner, the gate masks, which slot came
    from which cloud, the counters) equal it bit for bit; their fp32 results are held to the per-element bound of
    tests/_augment_ref.py;
  * ``apply``: the C entry on torch's current stream;  ``Stage``: a callable that owns its workspace and counters and is handed to
    a feed as ``post``, so the stage runs on the feed's stream before the item's ``ready`` event.

Keys and draws are harness/feed.py's: the cloud key is feed.cloud_key(seed, step, b), a draw is feed.draw(ck, purpose, counter), with
the purposes below (32..38; 1-7 are the feeds', 8-15 the inverse-density sampler's, 16-31 dropout's).

GATES.  ``opts.enable`` is a bit mask, ``opts.prob[k]`` the probability of bit k, turned into a threshold in [0, 2^32]: bit k of
cloud b is on iff it is enabled and hi32(draw(ck, GATE, k)) < threshold[k] — integers, so the masks are exact.  MIX is gated once
per pair (2i, 2i+1) from the even cloud's key.  A cloud with every gate off is copied bit for bit.

ORDER on the destination cloud: MIX, FLIPX, FLIPY, ASCALE, ELASTIC (two passes), then AUTOCONTRAST, CTRANSLATE, CJITTER, CDROP.

  MIX           h = N // 2.  Both clouds of a mixed pair are shifted by minus their own centre ((min + max) / 2 in x and y, min z,
                over the whole cloud before the exchange), then exchange slots [h, N) with all channels, label and inner (the
                feeds' samples are in exchangeable order, so a half is a uniform subsample).  The last cloud of an odd batch has
                no partner.  Everything after MIX uses the destination cloud's key, slot, gates and statistics.
  FLIPX, FLIPY  negate the coordinate (and that component of the normal) exactly.
  ASCALE        s_a = 0.9 + 0.2 u_a per axis; a normal becomes normalize(n / s) (a zero normal stays zero).
  ELASTIC       passes (g, mag) of ``opts.elastic``.  The noise lives on the ABSOLUTE lattice with nodes at g (i, j, k): the raw
                noise of a node is one 21-bit field per component of ONE 64-bit draw whose counter packs the three node indices,
                each biased by 512 into 10 bits — a function of the key and the node, never of the cloud's bounding box.  As an
                integer, v - 2^20 in [-2^20, 2^20); blurred by the separable 5-tap kernel [1, 2, 3, 2, 1] (two box blurs of width 3)
                on each axis it stays an exact integer below 729 * 2^20 = FIELD_UNIT in magnitude, and the displacement is
                mag / FIELD_UNIT times its trilinear interpolation at x / g.  Pass two reads the coordinates pass one wrote.
                NORMALS ARE LEFT AS THEY ARE under this transform.  A pass is SKIPPED for a cloud, and counted, when a raw node
                index it needs (cells - 2 .. cells + 3) leaves [-500, 500] or the raw node box holds more than ``opts.max_nodes``.
  AUTOCONTRAST  c' = lo + (c - min_c) (hi - lo) / (max_c - min_c), min / max per channel over the destination cloud after MIX,
                blended (1 - a) c + a c' with one uniform a per cloud; nothing on a channel with max == min.
  CTRANSLATE    + (u - 0.5) 2 * 0.05 (hi - lo) per cloud and channel, clipped to [lo, hi].
  CJITTER       + 0.01 (hi - lo) times feed.normal_pair noise per point and channel (counters 2 slot, 2 slot + 1), clipped.
  CDROP         the whole cloud's colour becomes (lo + hi) / 2.

Coordinates and colours must be finite.
"""
import collections

import numpy as np

from . import feed

MIX, FLIPX, FLIPY, ASCALE, ELASTIC, AUTOCONTRAST, CTRANSLATE, CJITTER, CDROP = (1 << _k for _k in range(9))    # the gates' bits
NUM_GATES = 9
GEOMETRIC = MIX | FLIPX | FLIPY | ASCALE | ELASTIC
COLOUR = AUTOCONTRAST | CTRANSLATE | CJITTER | CDROP
GATE, SCALE, FIELD, CONTRAST, CTRANS, CNOISE = 32, 33, 34, 36, 37, 38       # the `purpose` of a draw (FIELD + pass: 34, 35)
NODE_LIMIT = 500
FIELD_UNIT = 729 * 2 ** 20
MAX_NODES = 32768
_U64 = np.uint64

Options = collections.namedtuple("Options", "enable prob rgb_offset normal_offset rgb_range elastic max_nodes")
Report = collections.namedtuple("Report", "gates elastic_skipped mixed_pairs boxes")

#        MIX  FLIPX FLIPY ASCALE ELASTIC AUTOCONTRAST CTRANSLATE CJITTER CDROP
_PROB = (0.5, 0.5, 0.5, 0.95, 0.95, 0.2, 0.95, 0.95, 0.2)
_LAYOUT = {"s3dis": (3, None), "scannet": (3, None), "ruemonge2014": (6, 3), "facade": (6, 3),
           "shapenet": (None, None), "modelnet40": (None, None), "object": (None, None)}


def default_options(dataset="s3dis", enable=None, max_nodes=MAX_NODES):
    """the usual recipe for a dataset's channel layout: flips 0.5 per axis, scaling / elastic / colour translation / jitter 0.95,
    auto-contrast and colour drop 0.2, mixing 0.5; the xyz-only datasets get the geometric bits"""
    if dataset not in _LAYOUT:
        raise ValueError("default_options: dataset is one of %s" % ", ".join(sorted(_LAYOUT)))
    rgb, normal = _LAYOUT[dataset]
    if enable is None:
        enable = GEOMETRIC | (COLOUR if rgb is not None else 0)
    return Options(int(enable), _PROB, rgb, normal, (-1.0, 1.0), ((0.2, 0.7), (0.8, 2.8)), int(max_nodes))


def check_options(opts, channels):
    C = int(channels)
    if C not in (3, 6, 9):
        raise ValueError("augment: 3, 6 or 9 channels, got %d" % C)
    if not 0 <= opts.enable < 1 << NUM_GATES or len(opts.prob) != NUM_GATES:
        raise ValueError("augment: enable is a mask of %d bits with one probability each" % NUM_GATES)
    if any(not 0.0 <= p <= 1.0 for p in opts.prob):
        raise ValueError("augment: a probability outside [0, 1]")
    if opts.rgb_offset is None and opts.enable & COLOUR:
        raise ValueError("augment: a colour transform is enabled but the layout has no colour (rgb_offset is None)")
    if opts.rgb_offset is not None and (opts.rgb_offset not in (3, 6) or opts.rgb_offset + 3 > C):
        raise ValueError("augment: rgb_offset is 3 or 6, inside the %d channels" % C)
    if opts.normal_offset is not None and (opts.normal_offset != 3 or C < 6 or opts.rgb_offset == 3):
        raise ValueError("augment: normal_offset is 3, beside the colour")
    if not opts.rgb_range[1] > opts.rgb_range[0]:
        raise ValueError("augment: empty rgb_range")
    if len(opts.elastic) != 2 or any(not (g > 0 and mag >= 0) for g, mag in opts.elastic):
        raise ValueError("augment: elastic is two passes (g > 0, mag >= 0)")
    if not 216 <= opts.max_nodes <= 1 << 24:
        raise ValueError("augment: 216 <= max_nodes <= 2^24")


def thresholds(opts):
    """prob -> the integers the gate draws are compared with, in [0, 2^32]"""
    return [min(1 << 32, max(0, int(round(float(p) * 4294967296.0)))) for p in opts.prob]


def gate_masks(seed, step, B, opts):
    """-> int32 [B]: the transforms of every cloud, a pure function of (seed, step, b) and the options"""
    thr = thresholds(opts)
    out = np.zeros((B,), dtype=np.int32)
    for b in range(B):
        ck = feed.cloud_key(seed, step, b)
        for k in range(1, NUM_GATES):
            if opts.enable >> k & 1 and int(feed._hi(feed.draw(ck, GATE, k))) < thr[k]:
                out[b] |= 1 << k
        even = b & ~1
        if opts.enable & MIX and even + 1 < B and int(feed._hi(feed.draw(feed.cloud_key(seed, step, even), GATE, 0))) < thr[0]:
            out[b] |= MIX
    return out


# ---------------------------------------------------------------------------------------------------------------
# the elastic field
# ---------------------------------------------------------------------------------------------------------------
def cell_index(x, g):
    """the lattice cell of a coordinate: floor(x / g), clamped so that any finite coordinate has one"""
    return np.floor(np.clip(np.asarray(x, dtype=np.float64) / g, -1000.0, 1000.0)).astype(np.int64)


def box_ok(cmin, cmax, max_nodes):
    """may a pass run on a cloud whose cells span [cmin, cmax] per axis: its raw nodes cmin - 2 .. cmax + 3 inside
    [-NODE_LIMIT, NODE_LIMIT] and at most max_nodes of them"""
    cmin, cmax = np.asarray(cmin, dtype=np.int64), np.asarray(cmax, dtype=np.int64)
    if (cmin - 2 < -NODE_LIMIT).any() or (cmax + 3 > NODE_LIMIT).any():
        return False
    return int(np.prod(cmax - cmin + 6)) <= int(max_nodes)


def raw_field(ck, which, lo, shape):
    """-> int64 [shape, 3]: the raw noise v - 2^20 of the nodes lo .. lo + shape - 1 of pass `which`"""
    ix, iy, iz = (np.arange(shape[a], dtype=np.int64) + int(lo[a]) + 512 for a in range(3))
    counter = (ix[:, None, None] << 20) | (iy[None, :, None] << 10) | iz[None, None, :]
    w = feed.draw(ck, FIELD + which, counter)
    return np.stack([((w >> _U64(21 * c)) & _U64(0x1fffff)).astype(np.int64) - (1 << 20) for c in range(3)], axis=-1)


BLUR = (1, 2, 3, 2, 1)          # over 9; weights sum to 1 per axis


def blur(a, axis):
    n = a.shape[axis] - 4
    return sum(t * np.take(a, np.arange(k, k + n), axis=axis) for k, t in enumerate(BLUR))


def lattice(ck, which, cmin, cmax):
    """-> int64 [nx + 1, ny + 1, nz + 1, 3]: the blurred field, in units of 1 / FIELD_UNIT, at the nodes cmin .. cmax + 1"""
    cmin, cmax = np.asarray(cmin, dtype=np.int64), np.asarray(cmax, dtype=np.int64)
    return blur(blur(blur(raw_field(ck, which, cmin - 2, cmax - cmin + 6), 0), 1), 2)


def displacement(xyz, ck, which, g, mag, max_nodes):
    """the displacement of pass `which` at xyz [n, 3] (float64) -> [n, 3], or None where the pass is skipped"""
    xyz = np.asarray(xyz, dtype=np.float64)
    cell = cell_index(xyz, g)
    cmin, cmax = cell.min(axis=0), cell.max(axis=0)
    if not box_ok(cmin, cmax, max_nodes):
        return None
    F = lattice(ck, which, cmin, cmax)
    f = xyz / g - cell
    l = cell - cmin
    out = np.zeros(xyz.shape, dtype=np.float64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                out += w[:, None] * F[l[:, 0] + dx, l[:, 1] + dy, l[:, 2] + dz]
    return out * (float(mag) / FIELD_UNIT)


# ---------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------
def centre(xyz):
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    return np.array([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, lo[2]])


def scale_factors(ck):
    return np.array([0.9 + 0.2 * float(feed.uniform(feed._hi(feed.draw(ck, SCALE, a)))) for a in range(3)])


def colour_noise(ck, num_point):
    """-> [N, 3] float64 N(0, 1): feed.normal_pair of the draws 2 slot and 2 slot + 1"""
    j = np.arange(num_point, dtype=np.int64)
    z0, z1 = feed.normal_pair(feed.draw(ck, CNOISE, 2 * j))
    z2, _ = feed.normal_pair(feed.draw(ck, CNOISE, 2 * j + 1))
    return np.stack([z0, z1, z2], axis=1)


def apply_reference(points, label, inner, seed, step, opts):
    """points [B, N, C] (xyz in 0:3), label [B, N], inner [B, N] or None -> points' (float64), label', inner' (new arrays; a
    cloud no transform touches holds the input's values exactly) and Report(gates int32 [B], elastic_skipped (pass 1, pass 2),
    mixed_pairs, boxes: (b, pass, cmin, cmax) — the cells of every elastic pass a cloud's gate asked for).  A pure function of
    its arguments.  Elastic distortion leaves normals as they are."""
    points = np.asarray(points)
    if points.ndim != 3:
        raise ValueError("augment: points is [B, N, C]")
    B, N, C = points.shape
    check_options(opts, C)
    out = points.astype(np.float64)
    lab = np.array(label, copy=True)
    inn = None if inner is None else np.array(inner, copy=True)
    if lab.shape != (B, N) or (inn is not None and inn.shape != (B, N)):
        raise ValueError("augment: label and inner are [B, N]")
    gates = gate_masks(seed, step, B, opts)
    lo, hi = float(opts.rgb_range[0]), float(opts.rgb_range[1])
    ro, no, h = opts.rgb_offset, opts.normal_offset, N // 2
    skipped, mixed, boxes = [0, 0], 0, []
    for b in range(0, B - 1, 2):
        if not gates[b] & MIX:
            continue
        mixed += 1
        for c in (b, b + 1):
            out[c, :, 0:3] -= centre(out[c, :, 0:3])
        for t in (out, lab) + (() if inn is None else (inn,)):
            t[b, h:], t[b + 1, h:] = t[b + 1, h:].copy(), t[b, h:].copy()
    for b in range(B):
        g, ck = int(gates[b]), feed.cloud_key(seed, step, b)
        xyz = out[b, :, 0:3]
        for bit, a in ((FLIPX, 0), (FLIPY, 1)):
            if g & bit:
                xyz[:, a] = np.negative(xyz[:, a])
                if no is not None:
                    out[b, :, no + a] = np.negative(out[b, :, no + a])
        if g & ASCALE:
            s = scale_factors(ck)
            xyz *= s
            if no is not None:
                n = out[b, :, no:no + 3] / s
                length = np.sqrt((n * n).sum(axis=1, keepdims=True))
                out[b, :, no:no + 3] = np.where(length > 0, n / np.where(length > 0, length, 1.0), n)
        if g & ELASTIC:
            for which, (gg, mag) in enumerate(opts.elastic):
                cell = cell_index(xyz, gg)
                boxes.append((b, which, cell.min(axis=0), cell.max(axis=0)))
                d = displacement(xyz, ck, which, gg, mag, opts.max_nodes)
                if d is None:
                    skipped[which] += 1
                else:
                    xyz += d
        if not g & COLOUR:
            continue
        rgb = out[b, :, ro:ro + 3]
        if g & AUTOCONTRAST:
            alpha = float(feed.uniform(feed._hi(feed.draw(ck, CONTRAST, 0))))
            mn, mx = rgb.min(axis=0), rgb.max(axis=0)
            for c in range(3):
                if mx[c] > mn[c]:
                    rgb[:, c] = (1 - alpha) * rgb[:, c] + alpha * (lo + (rgb[:, c] - mn[c]) * ((hi - lo) / (mx[c] - mn[c])))
        if g & CTRANSLATE:
            u = feed.uniform(feed._hi(feed.draw(ck, CTRANS, np.arange(3))))
            rgb[:] = np.clip(rgb + (u - 0.5) * (0.1 * (hi - lo)), lo, hi)
        if g & CJITTER:
            rgb[:] = np.clip(rgb + (0.01 * (hi - lo)) * colour_noise(ck, N), lo, hi)
        if g & CDROP:
            rgb[:] = (lo + hi) / 2
    return out, lab, inn, Report(gates, tuple(skipped), mixed, boxes)


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
def params(opts, channels):
    """-> the by-value argument of sph3d_augment_apply (_lib.AugmentParams)"""
    from .. import _lib
    check_options(opts, channels)
    p = _lib.AugmentParams()
    for k, t in enumerate(thresholds(opts)):
        p.threshold[k] = t
    p.enable = int(opts.enable)
    p.rgb_offset = -1 if opts.rgb_offset is None else int(opts.rgb_offset)
    p.normal_offset = -1 if opts.normal_offset is None else int(opts.normal_offset)
    p.max_nodes = int(opts.max_nodes)
    p.rgb_lo, p.rgb_hi = float(opts.rgb_range[0]), float(opts.rgb_range[1])
    for q, (g, mag) in enumerate(opts.elastic):
        p.inv_g[q] = float(np.float32(1.0 / g))
        p.scale[q] = float(np.float32(float(mag) / FIELD_UNIT))
    return p


def workspace_bytes(batch_size, num_point, max_nodes):
    from .. import _lib
    return int(_lib.lib().sph3d_augment_workspace(int(batch_size), int(num_point), int(max_nodes)))


def read_gates(workspace, B):
    """-> int32 [B] (host): the gate masks the last apply() on `workspace` left in it (a word per cloud in the workspace's head,
    csrc/augment.hip: kAugGateWord) — for tests and tools; a host read"""
    import torch
    return workspace[:B * 160].view(torch.int32).reshape(B, 40)[:, 36].cpu().numpy()


def apply(points, label, inner, seed, step, opts, workspace=None, status=None, _params=None):
    """sph3d_augment_apply on torch's current stream, IN PLACE.  points [B, N, C] fp32, label [B, N] int32, inner [B, N] int32 or
    None, contiguous, on the device.  workspace: a uint8 tensor of workspace_bytes(B, N, opts.max_nodes), else the stream's
    call-local scratch.  status: int64 [3] the counters are ADDED to (elastic passes skipped, pairs mixed), else none are kept.
    -> points, label, inner (the arguments)"""
    import torch
    from .. import _lib
    tensors = (points, label) + (() if inner is None else (inner,)) + tuple(t for t in (workspace, status) if t is not None)
    _lib.require_device(*tensors)
    if points.dtype != torch.float32 or points.dim() != 3 or not points.is_contiguous():
        raise ValueError("augment.apply: points is a contiguous fp32 [B, N, C]")
    B, N, C = (int(d) for d in points.shape)
    for t in (label,) + (() if inner is None else (inner,)):
        if t.dtype != torch.int32 or tuple(t.shape) != (B, N) or not t.is_contiguous():
            raise ValueError("augment.apply: label and inner are contiguous int32 [B, N]")
    if status is not None and (status.dtype != torch.int64 or status.numel() != 3 or not status.is_contiguous()):
        raise ValueError("augment.apply: status is int64 [3]")
    p = _params if _params is not None else params(opts, C)
    need = workspace_bytes(B, N, opts.max_nodes)
    if workspace is None:
        workspace = _lib.scratch(need, points.device)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("augment.apply: workspace is a contiguous uint8 tensor")
    _lib.check(_lib.lib().sph3d_augment_apply(B, N, C, _lib.ptr(points), _lib.ptr(label), _lib.ptr(inner), seed & 0xffffffffffffffff,
                                              step & 0xffffffffffffffff, p, _lib.ptr(workspace), int(workspace.numel()),
                                              _lib.ptr(status), _lib.stream_ptr()))
    return points, label, inner


class Stage:
    """The stage as a feed's ``post``: owns the workspace and the counters, and is called by feed.TwoSetFeed on the feed's stream
    after the batch is assembled and before its ``ready`` event.

        stage = augment.Stage(augment.default_options("s3dis"), 16, 8192, 6, pool.device)
        feed = DeviceFeed(pool, 16, 8192, seed=1, post=stage)
        ...                                                      # the Trainer and the loop are unchanged

    An item's first two tensors are points and label; a third of label's shape is inner (ObjectFeed's category is not)."""

    def __init__(self, opts, batch_size, num_point, channels, device):
        import torch
        self.opts, self.channels = opts, int(channels)
        self._params = params(opts, channels)
        self.workspace = torch.empty((workspace_bytes(batch_size, num_point, opts.max_nodes),), dtype=torch.uint8, device=device)
        self.status = torch.zeros((3,), dtype=torch.int64, device=device)

    def __call__(self, seed, step, out):
        points, label = out[0], out[1]
        inner = out[2] if len(out) > 2 and out[2].shape == label.shape else None
        if int(points.shape[2]) != self.channels:
            raise ValueError("augment.Stage: built for %d channels, the feed yields %d" % (self.channels, int(points.shape[2])))
        apply(points, label, inner, seed, step, self.opts, self.workspace, self.status, _params=self._params)

    def read(self):
        """-> Report(None, elastic_skipped, mixed_pairs, None) summed over every batch so far (a host read: it waits for the device)"""
        s = self.status.cpu().tolist()
        return Report(None, (int(s[0]), int(s[1])), int(s[2]), None)
