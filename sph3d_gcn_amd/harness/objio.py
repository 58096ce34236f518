"""The records of the object datasets without TensorFlow: ModelNet40 (io/make_tfrecord_modelnet.py:115-120, read by
modelnet40_cls/train_modelnet.py:118-129), ShapeNet per category (io/make_tfrecord_shapenet.py:111-115, read by
shapenet_seg/train_shapenet.py:155-167) and ShapeNet one-hot (io/make_tfrecord_shapenet_onehot.py:115-117, read by
train_shapenet_onehot.py:128-145).  Framing, CRC and the Example wire format are harness/blockio.py's.

  * ``encode_modelnet`` / ``parse_modelnet``: `xyz_raw`, `normal_raw` (fp32 bytes [n, 3]) and `label` (one int64);
  * ``encode_shapenet`` / ``parse_shapenet``: `xyz_raw` (fp32 bytes), `seg_label` and `part_label` (int32 bytes [n]; the one-hot
    writer's records have no `part_label`) and `cls_label` (one int64);
  * ``read_shapes``: the records of a list of files, parsed; a file that ends inside a record or fails a CRC is refused (IOError);
  * ``shape_pool_from_records``: an objfeed.ShapePool of them;
  * ``prepare_modelnet``: what the ModelNet writer does to a cloud before it stores it (make_tfrecord_modelnet.py:72-95):
    farthest-point sampling down to num_point on the device, then centre and scale in numpy.
"""
import struct

import numpy as np

from . import blockio, objfeed

DATASETS = ("modelnet", "shapenet", "shapenet_onehot")


def _xyz_bytes(a, what):
    a = np.ascontiguousarray(a, dtype="<f4")
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
        raise ValueError("%s [n, 3] with n > 0 expected" % what)
    return a


def _labels_bytes(a, n, what):
    a = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype="<i4")
    if a.shape[0] != n:
        raise ValueError("%s: one label per row expected" % what)
    return a


def _scalar(ex, name):
    v = ex.get(name)
    if not isinstance(v, np.ndarray) or v.dtype != np.int64 or v.shape != (1,):
        raise ValueError("record without a scalar int64 %s" % name)
    return int(v[0])


def _raw(ex, name, dtype, width):
    v = ex.get(name)
    if not isinstance(v, bytes) or len(v) % (4 * width):
        raise ValueError("record without a raw %s of whole rows" % name)
    return np.frombuffer(v, dtype=dtype).reshape((-1, width) if width > 1 else (-1,)).copy()


# ---------------------------------------------------------------------------------------------------------------
# ModelNet40
# ---------------------------------------------------------------------------------------------------------------
def encode_modelnet(xyz, normal, label):
    """one shape record with the feature names and raw layouts of io/make_tfrecord_modelnet.py:115-120"""
    xyz, normal = _xyz_bytes(xyz, "xyz"), _xyz_bytes(normal, "normal")
    if normal.shape != xyz.shape:
        raise ValueError("one normal per point expected")
    return blockio.encode_example({"xyz_raw": xyz.tobytes(), "normal_raw": normal.tobytes(),
                                   "label": np.array([int(label)], dtype=np.int64)})


def parse_modelnet(record):
    """-> (xyz [n, 3] fp32, normal [n, 3] fp32, label int): train_modelnet.py:118-129 reads xyz and label; the normals are in the
    record and are returned too"""
    ex = blockio.decode_example(record)
    xyz, normal = _raw(ex, "xyz_raw", "<f4", 3), _raw(ex, "normal_raw", "<f4", 3)
    if xyz.shape != normal.shape or xyz.shape[0] == 0:
        raise ValueError("shape record with inconsistent array lengths")
    return xyz, normal, _scalar(ex, "label")


# ---------------------------------------------------------------------------------------------------------------
# ShapeNet
# ---------------------------------------------------------------------------------------------------------------
def encode_shapenet(xyz, seg_label, part_label, cls_label):
    """one shape record of io/make_tfrecord_shapenet.py:111-115; part_label None: the one-hot writer's record
    (make_tfrecord_shapenet_onehot.py:115-117), which has none"""
    xyz = _xyz_bytes(xyz, "xyz")
    feats = {"xyz_raw": xyz.tobytes(), "seg_label": _labels_bytes(seg_label, xyz.shape[0], "seg_label").tobytes(),
             "cls_label": np.array([int(cls_label)], dtype=np.int64)}
    if part_label is not None:
        feats["part_label"] = _labels_bytes(part_label, xyz.shape[0], "part_label").tobytes()
    return blockio.encode_example(feats)


def parse_shapenet(record):
    """-> (xyz [n, 3] fp32, seg_label [n] int32, part_label [n] int32 or None, cls_label int)"""
    ex = blockio.decode_example(record)
    xyz, seg = _raw(ex, "xyz_raw", "<f4", 3), _raw(ex, "seg_label", "<i4", 1)
    part = _raw(ex, "part_label", "<i4", 1) if "part_label" in ex else None
    if xyz.shape[0] == 0 or seg.shape[0] != xyz.shape[0] or (part is not None and part.shape[0] != xyz.shape[0]):
        raise ValueError("shape record with inconsistent array lengths")
    return xyz, seg, part, _scalar(ex, "cls_label")


# ---------------------------------------------------------------------------------------------------------------
# files -> a pool
# ---------------------------------------------------------------------------------------------------------------
def read_shapes(paths, dataset, verify=True):
    """the parsed records of `paths`, in order: parse_modelnet's tuples for "modelnet", parse_shapenet's otherwise"""
    if dataset not in DATASETS:
        raise ValueError("dataset is one of %s" % (DATASETS,))
    parse = parse_modelnet if dataset == "modelnet" else parse_shapenet
    out = []
    for p in paths:
        try:
            out.extend(parse(r) for r in blockio.read_records(p, verify=verify))
        except struct.error:                       # (the file ends inside a record's length or CRC word)
            raise IOError("truncated record in %s" % p)
    return out


def shape_pool_from_records(paths, dataset, part_lo=None, part_n=None, device=None):
    """-> objfeed.ShapePool of the records.  "modelnet": the class on every row and as the category.  "shapenet": a per-category
    model's pool — the rows carry `part_label` (the part inside the category, what train_shapenet.py:160 reads), the category
    is `cls_label`.  "shapenet_onehot": the rows carry `seg_label` (the part among all categories' parts), the category is
    `cls_label`, and part_lo / part_n give the one-hot model's part table (objfeed.read_class_info)."""
    shapes = read_shapes(paths, dataset)
    if not shapes:
        raise ValueError("no records in %s" % (list(paths),))
    if dataset == "modelnet":
        xyz, label, category = [s[0] for s in shapes], [s[2] for s in shapes], [s[2] for s in shapes]
    elif dataset == "shapenet":
        if any(s[2] is None for s in shapes):
            raise ValueError("a per-category ShapeNet pool needs records with part_label")
        xyz, label, category = [s[0] for s in shapes], [s[2] for s in shapes], [s[3] for s in shapes]
    else:
        xyz, label, category = [s[0] for s in shapes], [s[1] for s in shapes], [s[3] for s in shapes]
    return objfeed.ShapePool.from_arrays(xyz, label, category, part_lo, part_n, device)


# ---------------------------------------------------------------------------------------------------------------
# the ModelNet writer's preparation
# ---------------------------------------------------------------------------------------------------------------
def prepare_modelnet(xyz, normal, num_point, device=None):
    """make_tfrecord_modelnet.py:72-95.  xyz, normal [n, 3] fp32 with n >= num_point (fewer is refused, as the writer exits).
    For n > num_point the rows tf_sample.farthest_point_sample picks (on the device, from row 0, in its order); then, in numpy as
    the writer does: xyz - np.mean(xyz, axis=0) in float32 and division by the largest norm, sqrt(amax(sum(square))).
    -> (xyz [num_point, 3] fp32, normal [num_point, 3] fp32, index int32 [num_point] or None when nothing was sampled)"""
    xyz, normal = np.array(xyz, dtype=np.float32), np.array(normal, dtype=np.float32)
    num_point = int(num_point)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or normal.shape != xyz.shape:
        raise ValueError("prepare_modelnet: xyz and normal [n, 3] expected")
    if num_point <= 0 or num_point > xyz.shape[0]:
        raise ValueError("prepare_modelnet: the cloud has %d points, fewer than the %d asked for" % (xyz.shape[0], num_point))
    index = None
    if num_point < xyz.shape[0]:
        import torch
        from .. import tf_sample
        dev = torch.device(device if device is not None else "cuda:0")
        index = tf_sample.farthest_point_sample(num_point, torch.from_numpy(xyz[None]).to(dev))[0].cpu().numpy()
        xyz, normal = xyz[index, :], normal[index, :]
    xyz = xyz - np.mean(xyz, axis=0)
    scale = np.sqrt(np.amax(np.sum(np.square(xyz), axis=1)))
    xyz /= scale
    return xyz, normal, index
