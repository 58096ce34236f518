"""Scene-level evaluation of the segmentation networks: the stage after the overlap-voting script, which the reference does in
MATLAB (post-merging/s3dis_merge.m:42-82, scannet_merge.m:28-55) and from which the paper's S3DIS and ScanNet figures come.

  1. every block's summed logits (evalvote's vote sums) are normalised per row: cut to a unit vector, then soft-max;
  2. the INNER rows' probabilities are added into a per-scene array through the record's `index_label`, the row's position in
     the scene's voxel cloud (blocks overlap: a scene point is inner in about four of them);
  3. the arg-max per scene point is the voxel-level prediction;
  4. every point of the full-resolution cloud takes the prediction of its nearest voxel point (MATLAB's knnsearch);
  5. the confusion matrix is counted on the full cloud (S3DIS); for ScanNet the predictions go through `labelid_set`.

  * ``normalise_reference`` / ``merge_reference`` / ``nearest_reference`` / ``lift_reference``: the SPECIFICATION in numpy, no
    GPU.  csrc/scene.hip (sph3d_scene_merge / _finalize / _lift, sph3d_nn1) equals it bit for bit, the fp32 probabilities
    included (tests/test_gpu_scenemerge.py) — which is why the normalisation is stated operation by operation, with the
    polynomial exp of include/sph3d_exp32.h instead of a library's;
  * ``evaluate_scenes_reference``: the loop below over those and evalvote.vote_reference;
  * ``evaluate_scenes``: the loop on the device -> ``SceneResult``.

What differs from the reference, on purpose.  A row whose sum of squares is 0 or not finite (all-zero sums, a non-finite sum,
an overflow) contributes nothing and is counted in `skipped_rows`, where the reference would spread NaN over the scene point.
An index outside the scene is counted in `out_of_scene` and ignored.  Duplicate inner indices within a block are refused when
the pool is built (feed.check_scene_index), where MATLAB's indexed `+` keeps the last one.  The nearest neighbour is the
minimum of the fp32 squared distance with ties to the lowest index (knnsearch works in double and leaves ties to its tree).
Work is shared between ranks by SCENE, and a scene's blocks are batched on their own, so a scene's result is a pure function of
(seed, scene) whatever the world size.
"""
import collections
import os
import re

import numpy as np

from . import evalvote

_F32 = np.float32
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include", "sph3d_exp32.h")
NN1_GRID, NN1_BRUTE = 0, 1          # include/sph3d.h: SPH3D_NN1_GRID, SPH3D_NN1_BRUTE
_coeffs = None


def exp32_coefficients():
    """c0 .. c10 as float32, read from include/sph3d_exp32.h (the list is written once, there)"""
    global _coeffs
    if _coeffs is None:
        text = open(_HEADER).read()
        body = re.search(r"#define\s+SPH3D_EXP32_COEFFS\s*\{([^}]*)\}", text).group(1)
        degree = int(re.search(r"#define\s+SPH3D_EXP32_DEGREE\s+(\d+)", text).group(1))
        vals = [_F32(t.strip().rstrip("f")) for t in body.split(",")]
        if len(vals) != degree + 1:
            raise ValueError("sph3d_exp32.h: %d coefficients for degree %d" % (len(vals), degree))
        _coeffs = np.array(vals, dtype=_F32)
    return _coeffs


def exp32(u):
    """sph3d_exp32 on a float32 array: Horner, one fp32 multiply and one fp32 add per coefficient"""
    u = np.asarray(u, dtype=_F32)
    c = exp32_coefficients()
    p = np.full(u.shape, c[-1], dtype=_F32)
    for k in range(len(c) - 2, -1, -1):
        p = p * u
        p = p + c[k]
    return p


# ---------------------------------------------------------------------------------------------------------------
# the statement (numpy, no device)
# ---------------------------------------------------------------------------------------------------------------
def normalise_reference(votes, return_skipped=False):
    """votes [n, C] fp32 -> probabilities [n, C] fp32, every operation a separately rounded fp32 one, in this order:
    s = ((v0*v0 + v1*v1) + v2*v2) + ...; r = sqrt(s); u_c = v_c / r; e_c = exp32(u_c); z = ((e0 + e1) + e2) + ...; p_c = e_c / z.
    A row with s == 0 or s not finite is SKIPPED: its probabilities are 0 here (return_skipped: also -> the mask [n])"""
    v = np.ascontiguousarray(votes, dtype=_F32)
    if v.ndim != 2:
        raise ValueError("normalise_reference: votes [n, C] expected")
    n, C = v.shape
    with np.errstate(all="ignore"):
        s = np.zeros((n,), dtype=_F32)
        for c in range(C):
            s = s + v[:, c] * v[:, c]
        skipped = ~((s > 0) & (s < np.inf))
        r = np.sqrt(np.where(skipped, _F32(1), s)).astype(_F32)
        e = exp32(np.where(skipped[:, None], _F32(0), v / r[:, None]))
        z = np.zeros((n,), dtype=_F32)
        for c in range(C):
            z = z + e[:, c]
        p = (e / z[:, None]).astype(_F32)
    p[skipped] = 0
    return (p, skipped) if return_skipped else p


def merge_update(merged, hits, votes, inner, index):
    """one block, in place: merged [V, C] fp32 and hits [V] int32 receive the block's inner rows; -> (skipped, out_of_scene)"""
    V = merged.shape[0]
    index = np.asarray(index).reshape(-1).astype(np.int64)
    inner = np.asarray(inner).reshape(-1) == 1
    p, bad = normalise_reference(votes, return_skipped=True)
    use = inner & ~bad
    inside = (index >= 0) & (index < V)
    at = index[use & inside]
    if np.unique(at).shape[0] != at.shape[0]:
        raise ValueError("merge: two inner rows of a block share an index value")
    merged[at] = merged[at] + p[use & inside]                      # one fp32 add per element
    hits[at] += 1
    return int((inner & bad).sum()), int((use & ~inside).sum())


def finalize_reference(merged, hits):
    """-> pred_voxel int32 [V] (first maximum; class 0 for a row without a hit), unseen_rows"""
    pred = np.argmax(merged, axis=1).astype(np.int32) if merged.shape[0] else np.zeros((0,), np.int32)
    unseen = np.asarray(hits) == 0
    pred[unseen] = 0
    return pred, int(unseen.sum())


Merged = collections.namedtuple("Merged", "merged hits pred_voxel skipped_rows out_of_scene unseen_rows")


def merge_reference(votes, inner, index, V, num_cls):
    """votes: per block [n_k, C] fp32 vote sums, inner / index: per block [n_k], blocks in ascending pool order -> Merged"""
    merged = np.zeros((int(V), int(num_cls)), dtype=_F32)
    hits = np.zeros((int(V),), dtype=np.int32)
    skipped = outside = 0
    for v, m, i in zip(votes, inner, index):
        a, b = merge_update(merged, hits, v, m, i)
        skipped, outside = skipped + a, outside + b
    pred, unseen = finalize_reference(merged, hits)
    return Merged(merged, hits, pred, skipped, outside, unseen)


def nearest_reference(ref_xyz, query_xyz, chunk_elements=1 << 20):
    """-> idx int32 [F]: for every query the reference point that minimises the fp32 d2 = (dx*dx + dy*dy) + dz*dz with
    dx = q.x - r.x; ties go to the lowest index; a d2 that is not finite never wins, so a reference point with a non-finite
    coordinate is never chosen; -1 for a query with a non-finite coordinate or without a candidate (an empty reference).
    Brute force over chunks of queries (chunk_elements distances at a time)."""
    ref = np.ascontiguousarray(ref_xyz, dtype=_F32).reshape(-1, 3)
    qry = np.ascontiguousarray(query_xyz, dtype=_F32).reshape(-1, 3)
    V, F = ref.shape[0], qry.shape[0]
    out = np.full((F,), -1, dtype=np.int32)
    if V == 0 or F == 0:
        return out
    rx, ry, rz = (np.ascontiguousarray(ref[:, a])[None, :] for a in range(3))
    step = max(1, int(chunk_elements) // V)
    with np.errstate(all="ignore"):
        for lo in range(0, F, step):
            q = qry[lo:lo + step]
            d = q[:, 0:1] - rx
            d2 = d * d
            d = q[:, 1:2] - ry
            d2 = d2 + d * d
            d = q[:, 2:3] - rz
            d2 = d2 + d * d
            d2[~np.isfinite(d2)] = np.inf
            j = np.argmin(d2, axis=1)
            found = d2[np.arange(q.shape[0]), j] < np.inf
            out[lo:lo + step] = np.where(found, j, -1)
    return out


def lift_reference(pred_voxel, idx, label_full=None, label_map=None, num_cls=13):
    """-> pred_full int32 [F]: pred_voxel[idx], -1 where idx is -1, mapped through label_map [C] when given; with label_full also
    -> confusion [C, C] int64 (label, UNMAPPED prediction) over the full points with a label in [0, C) and idx >= 0"""
    pred_voxel = np.asarray(pred_voxel, dtype=np.int32)
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < pred_voxel.shape[0])
    raw = np.full(idx.shape, -1, dtype=np.int32)
    raw[ok] = pred_voxel[idx[ok]]
    ok &= (raw >= 0) & (raw < num_cls)
    full = np.full(idx.shape, -1, dtype=np.int32)
    full[ok] = raw[ok] if label_map is None else np.asarray(label_map, dtype=np.int32)[raw[ok]]
    if label_full is None:
        return full
    label = np.asarray(label_full).reshape(-1).astype(np.int64)
    use = ok & (label >= 0) & (label < num_cls)
    confusion = np.zeros((num_cls, num_cls), dtype=np.int64)
    np.add.at(confusion, (label[use], raw[use].astype(np.int64)), 1)
    return full, confusion


def voxel_confusion(pred_voxel, voxel_label, num_cls):
    label = np.asarray(voxel_label).reshape(-1).astype(np.int64)
    use = (label >= 0) & (label < num_cls)
    confusion = np.zeros((num_cls, num_cls), dtype=np.int64)
    np.add.at(confusion, (label[use], np.asarray(pred_voxel)[use].astype(np.int64)), 1)
    return confusion


# ---------------------------------------------------------------------------------------------------------------
# scenes, the plan, the result
# ---------------------------------------------------------------------------------------------------------------
class Scene:
    """voxel_xyz [V, 3]: the cloud the blocks were cut from (what index_label points into); voxel_label [V] (optional);
    full_xyz [F, 3] / full_label [F] (optional): the full-resolution cloud the predictions are lifted to"""

    def __init__(self, voxel_xyz, voxel_label=None, full_xyz=None, full_label=None):
        self.voxel_xyz = np.ascontiguousarray(voxel_xyz, dtype=_F32).reshape(-1, 3)
        self.voxel_label = None if voxel_label is None else np.ascontiguousarray(voxel_label, dtype=np.int32).reshape(-1)
        self.full_xyz = None if full_xyz is None else np.ascontiguousarray(full_xyz, dtype=_F32).reshape(-1, 3)
        self.full_label = None if full_label is None else np.ascontiguousarray(full_label, dtype=np.int32).reshape(-1)
        if self.voxel_xyz.shape[0] == 0:
            raise ValueError("Scene: empty voxel cloud")
        if self.voxel_label is not None and self.voxel_label.shape[0] != self.voxel_xyz.shape[0]:
            raise ValueError("Scene: voxel_label and voxel_xyz differ in length")
        if self.full_label is not None and (self.full_xyz is None or self.full_label.shape[0] != self.full_xyz.shape[0]):
            raise ValueError("Scene: full_label needs a full_xyz of the same length")
        if self.full_xyz is not None and self.full_xyz.shape[0] == 0:
            raise ValueError("Scene: empty full cloud")


def scene_plan(scene_of_block, num_scenes, batch_size):
    """-> (first_block [S+1], first_batch [S+1]): scene s owns blocks [first_block[s], first_block[s+1]) of the pool (scene
    numbers ascend with the pool order) and batches first_batch[s] .. first_batch[s+1] - 1 of the evaluation"""
    sob = np.asarray(scene_of_block, dtype=np.int64).reshape(-1)
    if batch_size <= 0:
        raise ValueError("batch_size>0 required")
    if sob.size and (np.diff(sob) < 0).any():
        raise ValueError("scene numbers must ascend with the pool order")
    if sob.size and (sob.min() < 0 or sob.max() >= num_scenes):
        raise ValueError("a block names a scene outside the %d given" % num_scenes)
    first_block = np.searchsorted(sob, np.arange(num_scenes + 1)).astype(np.int64)
    batches = (np.diff(first_block) + batch_size - 1) // batch_size
    return first_block, np.concatenate(([0], np.cumsum(batches))).astype(np.int64)


def scene_batches(first_block, s, batch_size):
    """the block ids of scene s's batches, ascending; the last batch may be smaller"""
    lo, hi = int(first_block[s]), int(first_block[s + 1])
    return [np.arange(a, min(hi, a + batch_size), dtype=np.int32) for a in range(lo, hi, batch_size)]


class SceneResult:
    """confusion_full / confusion_voxel [C, C] int64 (label, prediction) on the full-resolution and on the voxel clouds, their
    metrics (`full`, `voxel`: evalvote.Metrics), the block-level `block` (evalvote.EvalResult, as evalvote.evaluate gives);
    per evaluated scene (`scenes`: their numbers): unseen_rows, skipped_rows, out_of_scene, complete; `pred`: with keep_pred
    {scene: dict(merged, hits, pred_voxel, pred_full, idx)} of host arrays (pred_full / idx None without a full cloud)"""

    def __init__(self, confusion_full, confusion_voxel, block, scenes, unseen_rows, skipped_rows, out_of_scene, complete, pred=None):
        self.confusion_full = np.asarray(confusion_full, dtype=np.int64)
        self.confusion_voxel = np.asarray(confusion_voxel, dtype=np.int64)
        self.block, self.scenes = block, list(scenes)
        self.unseen_rows, self.skipped_rows = list(unseen_rows), list(skipped_rows)
        self.out_of_scene, self.complete = list(out_of_scene), list(complete)
        self.pred = pred
        self.full, self.voxel = evalvote.metrics(self.confusion_full), evalvote.metrics(self.confusion_voxel)

    @classmethod
    def merge(cls, results):
        """the result of the ranks' shares together: equal to the world = 1 result"""
        results, pick, pred = evalvote.merge_order(results, "scenes", "scene", "pred")
        return cls(sum(res.confusion_full for res in results), sum(res.confusion_voxel for res in results),
                   evalvote.EvalResult.merge([res.block for res in results]), pick("scenes"), pick("unseen_rows"),
                   pick("skipped_rows"), pick("out_of_scene"), pick("complete"), pred)


def _check_scene_args(scenes, batch_size, rank, world):
    evalvote.check_share(batch_size, rank, world, "evaluate_scenes")
    if not scenes:
        raise ValueError("evaluate_scenes: no scenes")


def evaluate_scenes_reference(logits_fn, sizes, rows_label, rows_inner, index, scene_of_block, scenes, batch_size, num_point, seed,
                              num_cls=13, min_votes=1, max_passes=evalvote.MAX_PASSES, rank=0, world=1, label_map=None,
                              keep_pred=False, vote_fn=None):
    """`evaluate_scenes` stated in numpy.  sizes [P], rows_label / rows_inner / index [T]: the pool on the host;
    logits_fn(batch_index, pass, index [b, N]) -> [b, N, C] float32.  vote_fn: the pass loop of one batch, called with
    evalvote.vote_reference's positional arguments (the default) — the statement's side of `voter_factory`"""
    _check_scene_args(scenes, batch_size, rank, world)
    vote_fn = evalvote.vote_reference if vote_fn is None else vote_fn
    C = int(num_cls)
    first_block, first_batch = scene_plan(scene_of_block, len(scenes), batch_size)
    offsets = np.concatenate(([0], np.cumsum(np.asarray(sizes, dtype=np.int64))))
    index = np.asarray(index)
    mine = list(range(rank, len(scenes), world))
    cf, cv = np.zeros((C, C), np.int64), np.zeros((C, C), np.int64)
    done, numbers, unseen_all, skipped_all, outside_all, complete, pred = [], [], [], [], [], [], {}
    for s in mine:
        sc = scenes[s]
        V = sc.voxel_xyz.shape[0]
        merged, hits = np.zeros((V, C), _F32), np.zeros((V,), np.int32)
        skipped = outside = 0
        ok = True
        for j, ids in enumerate(scene_batches(first_block, s, batch_size)):
            i = int(first_batch[s]) + j
            d = vote_fn(sizes, rows_label, rows_inner, ids, num_point, seed, i, lambda p, idx, _i=i: logits_fn(_i, p, idx), C,
                        min_votes, max_passes)
            done.append(d)
            numbers.append(i)
            ok = ok and d.complete
            for k, b in enumerate(ids):
                lo, hi = int(offsets[b]), int(offsets[b + 1])
                a, o = merge_update(merged, hits, d.votes[k], rows_inner[lo:hi], index[lo:hi])
                skipped, outside = skipped + a, outside + o
        pv, unseen = finalize_reference(merged, hits)
        if sc.voxel_label is not None:
            cv += voxel_confusion(pv, sc.voxel_label, C)
        idx = pf = None
        if sc.full_xyz is not None:
            idx = nearest_reference(sc.voxel_xyz, sc.full_xyz)
            if sc.full_label is not None:
                pf, c = lift_reference(pv, idx, sc.full_label, label_map, C)
                cf += c
            else:
                pf = lift_reference(pv, idx, None, label_map, C)
        unseen_all.append(unseen); skipped_all.append(skipped); outside_all.append(outside); complete.append(ok)
        if keep_pred:
            pred[s] = dict(merged=merged, hits=hits, pred_voxel=pv, pred_full=pf, idx=idx)
    block = evalvote.EvalResult(sum((d.confusion for d in done), np.zeros((C, C), np.int64)), numbers, [d.passes for d in done],
                                [d.covered for d in done], [d.inner_size for d in done], sum(d.nonfinite_rows for d in done))
    return SceneResult(cf, cv, block, mine, unseen_all, skipped_all, outside_all, complete, pred if keep_pred else None)


# ---------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------
def nearest(ref_xyz, query_xyz, mode=NN1_GRID):
    """sph3d_nn1 on torch's current stream: ref_xyz [V, 3], query_xyz [F, 3] fp32 on the device -> idx [F] int32"""
    import torch
    from .. import _lib
    _lib.require_device(ref_xyz, query_xyz)
    ref, qry = _lib.f32(ref_xyz), _lib.f32(query_xyz)
    if ref.dim() != 2 or ref.shape[1] != 3 or qry.dim() != 2 or qry.shape[1] != 3:
        raise ValueError("nearest: [V, 3] and [F, 3] expected")
    V, F = int(ref.shape[0]), int(qry.shape[0])
    idx = torch.empty((F,), dtype=torch.int32, device=ref.device)
    need = int(_lib.lib().sph3d_nn1_workspace(V, F))
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=ref.device)
    _lib.check(_lib.lib().sph3d_nn1(V, F, _lib.ptr(ref), _lib.ptr(qry), int(mode), _lib.ptr(idx), _lib.ptr(ws), need,
                                    _lib.stream_ptr()))
    return idx


def evaluate_scenes(model_fn, pool, scenes, batch_size, num_point, seed, num_cls=13, min_votes=1, max_passes=evalvote.MAX_PASSES,
                    rank=0, world=1, label_map=None, keep_pred=False, on_pass=None, voter_factory=None):
    """Evaluate a network scene by scene -> SceneResult.

        pool = feed.BlockPool.from_records(scene_files, with_index=True)         # one record file per scene
        scenes = [scenemerge.Scene(voxel_xyz, voxel_label, full_xyz, full_label) for ... in scene_files]
        res = scenemerge.evaluate_scenes(lambda p, l, i: model(p, is_training=False)[0], pool, scenes, 16, 8192, seed=0)
        print(res.full.miou, res.full.overall_acc, res.voxel.miou, res.block.miou)

    `pool` carries `index` and `scene_of_block` (scene numbers 0 .. len(scenes) - 1, ascending).  Rank r of `world` takes
    scenes r, r + world, ...; a scene's blocks are batched on their own (the last batch may be smaller) and batch j of scene s
    runs evalvote.Voter.run_batch with batch_index = first_batch[s] + j, first_batch the prefix sum of the scenes' batch
    counts: a scene's result does not depend on `world`, and SceneResult.merge of the ranks equals the one-rank result.
    After every batch sph3d_scene_merge reads the vote sums while they are in the voter's buffer; after a scene's last batch
    come sph3d_scene_finalize, sph3d_nn1 (skipped without a full cloud) and sph3d_scene_lift.  A scene's clouds are uploaded
    for the scene and released after it.  label_map [C]: ScanNet's labelid_set, applied to pred_full only.
    model_fn, min_votes, max_passes, on_pass: as evalvote.evaluate.
    voter_factory(pool, batch_size, num_point, num_cls, capacity_rows, min_votes) -> the evalvote.Voter whose run_batch votes the
    batches (default: evalvote.Voter itself; harness/scannet.py hands in its three-view voter)."""
    import torch
    from .. import _lib
    _check_scene_args(scenes, batch_size, rank, world)
    if pool.index is None or pool.scene_of_block is None:
        raise ValueError("evaluate_scenes: the pool has no scene index (BlockPool(..., index=, scene_of_block=))")
    C = int(num_cls)
    evalvote._check_loop_args(num_point, C, min_votes, max_passes)
    first_block, first_batch = scene_plan(pool.scene_of_block, len(scenes), batch_size)
    mine = list(range(rank, len(scenes), world))
    plans = {s: scene_batches(first_block, s, batch_size) for s in mine}
    spans = [ids for s in mine for ids in plans[s]]
    dev, l = pool.device, _lib.lib()
    cap = max([int(pool.host_offsets[ids[-1] + 1] - pool.host_offsets[ids[0]]) for ids in spans] or [1])
    voter = (evalvote.Voter if voter_factory is None else voter_factory)(pool, batch_size, num_point, C, cap, min_votes)
    P, T = len(pool), int(pool.rows.shape[0])
    conf = torch.zeros((2, C * C), dtype=torch.int64, device=dev)          # full | voxel
    map_dev = None
    if label_map is not None:
        label_map = np.ascontiguousarray(label_map, dtype=np.int32).reshape(-1)
        if label_map.shape[0] != C:
            raise ValueError("label_map has one entry per class")
        map_dev = torch.from_numpy(label_map).to(dev)
    done, numbers, unseen_all, skipped_all, outside_all, complete, pred = [], [], [], [], [], [], {}
    for s in mine:
        sc = scenes[s]
        V = int(sc.voxel_xyz.shape[0])
        merged = torch.zeros((V, C), dtype=torch.float32, device=dev)
        hits = torch.zeros((V,), dtype=torch.int32, device=dev)
        counters = torch.zeros((3,), dtype=torch.int64, device=dev)        # skipped_rows, out_of_scene | unseen_rows
        ok = True
        for j, ids in enumerate(plans[s]):
            i = int(first_batch[s]) + j
            d = voter.run_batch(model_fn, ids, seed, i, max_passes, False, on_pass)
            done.append(d)
            numbers.append(i)
            ok = ok and d.complete
            base, nrows = voter.row_range(ids)
            ids_dev = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
            _lib.check(l.sph3d_scene_merge(len(ids), C, P, T, _lib.ptr(pool.rows), _lib.ptr(pool.offsets), _lib.ptr(pool.index),
                                           _lib.ptr(ids_dev), base, nrows, _lib.ptr(voter.votes), V, _lib.ptr(merged), _lib.ptr(hits),
                                           _lib.ptr(counters), _lib.stream_ptr()))
        pv = torch.empty((V,), dtype=torch.int32, device=dev)
        vlabel = torch.from_numpy(sc.voxel_label).to(dev) if sc.voxel_label is not None else None
        _lib.check(l.sph3d_scene_finalize(C, V, _lib.ptr(merged), _lib.ptr(hits), _lib.ptr(vlabel), _lib.ptr(pv),
                                          _lib.ptr(counters[2:]), _lib.ptr(conf[1]) if vlabel is not None else None,
                                          _lib.stream_ptr()))
        idx = pf = None
        if sc.full_xyz is not None:
            F = int(sc.full_xyz.shape[0])
            idx = nearest(torch.from_numpy(sc.voxel_xyz).to(dev), torch.from_numpy(sc.full_xyz).to(dev))
            pf = torch.empty((F,), dtype=torch.int32, device=dev)
            flabel = torch.from_numpy(sc.full_label).to(dev) if sc.full_label is not None else None
            _lib.check(l.sph3d_scene_lift(C, V, F, _lib.ptr(pv), _lib.ptr(idx), _lib.ptr(map_dev), _lib.ptr(flabel), _lib.ptr(pf),
                                          _lib.ptr(conf[0]) if flabel is not None else None, _lib.stream_ptr()))
        host = counters.cpu().numpy()                                      # (a synchronisation per scene)
        skipped_all.append(int(host[0])); outside_all.append(int(host[1])); unseen_all.append(int(host[2])); complete.append(ok)
        if keep_pred:
            pred[s] = dict(merged=merged.cpu().numpy(), hits=hits.cpu().numpy(), pred_voxel=pv.cpu().numpy(),
                           pred_full=None if pf is None else pf.cpu().numpy(), idx=None if idx is None else idx.cpu().numpy())
    confusion, nonfinite = voter.totals()
    block = evalvote.EvalResult(confusion, numbers, [d.passes for d in done], [d.covered for d in done],
                                [d.inner_size for d in done], nonfinite)
    host = conf.cpu().numpy().reshape(2, C, C)
    return SceneResult(host[0].copy(), host[1].copy(), block, mine, unseen_all, skipped_all, outside_all, complete,
                       pred if keep_pred else None)
