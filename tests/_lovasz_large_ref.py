"""The Lovasz-softmax loss with the sort in global memory (csrc/lovasz.hip: sph3d_lovasz_softmax_large) restated for its tests:
tests/_lovasz_ref.py's inputs and bounds, with the one thing that differs, the summation tree of class_loss.  numpy only.

Why every other bound carries over: the per-element operations are the same.  lovasz_probs_kernel is the same kernel; a key is the
same (bits(e), ~n, fg), so the order is exact by the same argument (valid keys are distinct: a merge of sorted runs of distinct
keys is THE sorted sequence); lovasz_finish_kernel forms g from the same integers G, F, U with the same product, division and
scaling by 1 / P_b (K_COEF), and N <= 2^20 keeps U < 2^21, so U, U - 1 and G - F still convert exactly and only the product
U (U - 1) rounds, as it already may above 2^12 rows; lovasz_large_grad_kernel runs lovasz_grad_kernel's row (C + 7) and its sum
over the classes and division (C - 1, 1).

The tree of class_loss (include/sph3d.h): a thread holds ONE term e g (no addition); the 64 lanes of a wave add by a 6-step
butterfly (6); the 16 waves of a tile are added in order onto 0.f (15; 0 + x is exact); lane l of one wave adds the tiles l,
l + 64, ... in order onto 0.f (ceil(tiles / 64) - 1); the 64 lanes by a 6-step butterfly (6).  tiles = ceil(N / tile) tile / 1024:
the segment is padded to whole runs and cut into tiles of 1024 sorted positions.  All terms are >= 0, so a path of d additions
adds d u times the sum, as in tests/_lovasz_ref.py.  No constant here is measured.
"""
import numpy as np

import _lovasz_ref as R

DEFAULT_TILE = 4096
MERGE_TILE = 1024


def tiles_of(N, tile=DEFAULT_TILE):
    return -(-N // tile) * tile // MERGE_TILE


def sum_depth_large(N, tile=DEFAULT_TILE):
    """lovasz_finish_kernel + lovasz_class_kernel: the additions on the longest path of the class sum"""
    return 6 + 15 + (-(-tiles_of(N, tile) // 64) - 1) + 6


def end_to_end_bound_large(logits, label, inner, pure_loss, tile=DEFAULT_TILE):
    """[B]: R.end_to_end_bound with the large entry's depth"""
    N, C = logits.shape[1:]
    valid = R.valid_rows(label, inner)
    worst_p = np.where(valid[..., None] & np.ones(logits.shape, bool), R.probs_bound(logits)[1], 0.0).max((1, 2))
    return worst_p + (4 + sum_depth_large(N, tile) + C - 1) * R.U * pure_loss


def check_stages_large(got, logits, label, inner, staged, pure, tile=DEFAULT_TILE, skip_blocks=()):
    """R.check_stages with sum_depth_large(N, tile) in the class_loss, loss and end-to-end bounds; everything else is its text"""
    B, N, C = logits.shape
    keep = np.array([b not in skip_blocks for b in range(B)])
    valid = R.valid_rows(label, inner)
    depth = sum_depth_large(N, tile)
    p64, pb = R.probs_bound(logits)
    out = {}
    out["probs"] = R._frac(np.abs(got["probs"].astype(np.float64) - p64)[keep], pb[keep])
    out["order_equal"] = bool(np.array_equal(got["order"][keep], staged["order"][keep]))
    out["coef"] = R._frac(np.abs(got["coef"] - staged["coef"])[keep], (R.K_COEF * R.U * np.abs(staged["coef"]))[keep])
    out["class_loss"] = R._frac(np.abs(got["class_loss"] - staged["class_loss"])[keep], ((4 + depth) * R.U * staged["class_loss"])[keep])
    loss_bound = (4 + depth + C - 1) * R.U * staged["loss"]
    out["loss"] = R._frac(np.abs(got["loss"] - staged["loss"])[keep], loss_bound[keep])
    if got.get("dlogits") is not None:
        p, cf = staged["probs"], np.abs(staged["coef"])
        mag = p * (cf + (cf * p).sum(-1, keepdims=True))
        bound = np.where(valid[..., None], (C + 7) * R.U * mag + R.F32_FLOOR, 0.0)
        out["dlogits"] = R._frac(np.abs(got["dlogits"] - staged["dlogits"])[keep], bound[keep])
    e2e = end_to_end_bound_large(logits, label, inner, pure["loss"], tile)
    out["end_to_end"] = R._frac(np.abs(got["loss"] - pure["loss"])[keep], e2e[keep])
    out["end_to_end_bound"] = e2e
    return out
