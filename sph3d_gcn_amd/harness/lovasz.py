"""The Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018), per block: the numpy STATEMENT of csrc/lovasz.hip
(include/sph3d.h: sph3d_lovasz_softmax), the same statement in torch ops, and the loss functions a Trainer takes.

The statement is per block (the paper's per_image=True), as the project's losses are: the batch loss is the sum of the blocks'.
scope="batch" is the same statement on the call reshaped to ONE block of B * N rows (the paper's per_image=False, its default): row
index n is then the flat index.  Blocks of more than MAX_N rows, which the batch scope usually is, run on the device through
sph3d_lovasz_softmax_large (the sort in global memory, up to MAX_N_LARGE rows) when loss() is called with large=True.

  valid     row n of block b is valid iff (inner is None or inner[b,n] > 0; NaN > 0 is false) and label[b,n] != ignore
  p         softmax(logits[b,n,:])
  class c   with G = #{valid n: label = c} > 0 (a "present" class): e_n = 1 - p[n,c] on the valid rows labelled c (foreground),
            p[n,c] on the other valid rows; the valid rows in the order of DESCENDING e, ties by ASCENDING n; F_j the foreground
            rows among the sorted positions 0..j, U_j = G + (j + 1) - F_j, and the Lovasz gradient of the Jaccard loss
                g_j = 1 / U_j  on a foreground position,    (G - F_j) / (U_j (U_j - 1))  on a background position
            L[b,c] = sum_j e_(j) g_j
  loss[b]   (1 / P_b) sum over the P_b present classes, ascending, of L[b,c]; 0 if P_b = 0
  coef      d loss[b] / d p[n,c] = s g_rank(n) / P_b, s = -1 on foreground, +1 on background; 0 on rows that are not valid and for
            classes that are not present
  dlogits   p_k (coef_k - sum_c coef_c p_c); zeros on rows that are not valid

The closed form of g is the paper's jaccard_j - jaccard_{j-1} with jaccard_j = 1 - (G - F_j) / U_j = (j + 1) / U_j, written without
the cancellation: in float32 (integers to float, one product, one correctly rounded division) it is accurate to two units of
relative error, where the difference of two numbers near 1 is accurate to 2^-24 ABSOLUTE, a thousandth of a typical g at 16 384 rows.
g >= 0 and sum_j g_j = 1, so L is a weighted mean of the errors; for one-hot predictions it is 1 - IoU_c.

A valid row whose label lies outside [0, C), or whose probabilities are not finite, makes loss[b] and every dlogits row of block
b NaN: nothing is clamped.

The order is where float32 and float64 part: given float32 probabilities e is ONE float32 operation, and the order is then an integer
function of them, but float32 and float64 probabilities rank a few rows in a thousand differently.  ``lovasz_reference(...,
probs=p32)`` therefore takes the probabilities as given, in float32, forms e in float32, sorts on (bits(e) descending, n ascending)
and does everything after that in float64: the kernels' `order` equals it exactly and their sums are held to it.
"""
import numpy as np
import torch

MAX_N = 16384                      # csrc/lovasz.hip: kLovMaxN (sph3d_lovasz_softmax_supported)
MAX_N_LARGE = 1 << 20              # csrc/lovasz_plan.hpp: kLovLargeMaxN (sph3d_lovasz_softmax_large_supported)
_SCOPES = ("block", "batch")


def _check_scope(scope):
    if scope not in _SCOPES:
        raise ValueError("lovasz: scope should be 'block' or 'batch', got %r" % (scope,))


def jaccard_gradient(fg_sorted):
    """fg_sorted [n] bool, the foreground flags in sorted order (G = their number > 0) -> g [n] float64, the closed form above"""
    fg = np.asarray(fg_sorted, bool)
    G = int(fg.sum())
    F = np.cumsum(fg).astype(np.int64)
    U = G + np.arange(1, len(fg) + 1, dtype=np.int64) - F
    den = np.where(fg, 1, U * (U - 1))                      # (a background position has U >= G + 1 >= 2)
    return np.where(fg, 1.0 / U, (G - F) / den.astype(np.float64))


def lovasz_reference(logits, label, inner=None, ignore=-1, probs=None, scope="block"):
    """logits [B,N,C], label [B,N] integer, inner [B,N] or None -> dict of float64 arrays: loss [B], class_loss [B,C] (L; 0 for a
    class that is not present), probs [B,N,C], coef [B,N,C], dlogits [B,N,C], and order [B,C,N] int32 (the row at every sorted
    position of every class, present or not; -1 past n_b), present [B,C] bool, n_valid [B].
    probs: probabilities to take as given, in float32 (see the module's text: the order is that of the bits of the float32 e), or in
    float64 (the statement as a function of p: the order is that of the float64 e); None: the float64 softmax of logits.
    scope="batch": the statement on the call reshaped to ONE block of B * N rows (the paper's per_image=False): row index n is the
    flat index, ties break by ascending flat index, and every array of the result has a leading 1."""
    _check_scope(scope)
    x = np.asarray(logits, np.float64)
    if scope == "batch":
        x = x.reshape(1, -1, x.shape[-1])
    B, N, C = x.shape
    label = np.asarray(label).reshape(B, N).astype(np.int64)
    valid = label != ignore
    if inner is not None:
        with np.errstate(invalid="ignore"):
            valid &= np.asarray(inner).reshape(B, N) > 0
    if probs is None:
        with np.errstate(all="ignore"):
            ex = np.exp(x - x.max(-1, keepdims=True))
            p_sort = ex / ex.sum(-1, keepdims=True)
    else:
        p_sort = np.ascontiguousarray(probs).reshape(B, N, C)
        if p_sort.dtype != np.float64:
            p_sort = p_sort.astype(np.float32)
    bits = p_sort.dtype == np.float32
    p = p_sort.astype(np.float64)
    one = p_sort.dtype.type(1)
    out = dict(loss=np.zeros(B), class_loss=np.zeros((B, C)), probs=p, coef=np.zeros((B, N, C)), dlogits=np.zeros((B, N, C)),
               order=np.full((B, C, N), -1, np.int32), present=np.zeros((B, C), bool), n_valid=valid.sum(1))
    for b in range(B):
        rows = np.flatnonzero(valid[b])
        lab = label[b, rows]
        inside = (lab >= 0) & (lab < C)
        pv = p_sort[b, rows]
        bad = bool((~inside).any()) or not bool(np.isfinite(pv).all())
        out["present"][b, np.unique(lab[inside])] = True
        P = int(out["present"][b].sum())
        for c in range(C):
            fg = lab == c
            with np.errstate(invalid="ignore"):
                e = np.where(fg, one - pv[:, c], pv[:, c])
            if not bits:
                perm = np.argsort(-e, kind="stable")
            else:
                perm = np.argsort(-e.view(np.uint32).astype(np.int64), kind="stable")
            out["order"][b, c, :len(rows)] = rows[perm]
            if bad or not fg.any():
                continue
            g = jaccard_gradient(fg[perm])
            out["class_loss"][b, c] = float((e[perm].astype(np.float64) * g).sum())
            out["coef"][b, rows[perm], c] = np.where(fg[perm], -g, g) / P
        if bad:
            for k in ("class_loss", "coef", "dlogits", "loss"):
                out[k][b] = np.nan
            continue
        s = 0.0
        for c in np.flatnonzero(out["present"][b]):
            s += out["class_loss"][b, c]
        out["loss"][b] = s / P if P else 0.0
        cf, pb = out["coef"][b, rows], p[b, rows]
        out["dlogits"][b, rows] = pb * (cf - (cf * pb).sum(-1, keepdims=True))
    return out


def lovasz_torch(pred, label, inner_label=None, ignore=-1, scope="block"):
    """the statement in torch ops, on any device and in pred's dtype, differentiable in pred: -> loss [B] ([1] for scope="batch":
    the call reshaped to one block of B * N rows).  The fallback for CPU tensors and for blocks the kernels do not cover, and the
    baseline the kernels are measured against."""
    _check_scope(scope)
    if scope == "batch":
        pred = pred.reshape(1, -1, pred.shape[-1])
    B, N, C = pred.shape
    label = label.reshape(B, N).long()
    valid = label != ignore
    if inner_label is not None:
        valid = valid & (inner_label.reshape(B, N) > 0)
    p = torch.softmax(pred, dim=-1)
    classes = torch.arange(C, device=pred.device)
    fg = (label[..., None] == classes) & valid[..., None]                                   # [B, N, C]
    bad = (valid & ((label < 0) | (label >= C) | ~torch.isfinite(p).all(-1))).any(1)         # [B]
    e = torch.where(fg, 1.0 - p, p)
    key = torch.where(valid[..., None], e, torch.full_like(e, -1.0)).transpose(1, 2)        # [B, C, N]; rows that are not valid: last
    es, idx = torch.sort(key, dim=-1, descending=True, stable=True)
    fgs = torch.gather(fg.transpose(1, 2), 2, idx)
    vs = torch.gather(valid[:, None, :].expand(B, C, N), 2, idx)
    F = torch.cumsum(fgs.long(), dim=-1)
    G = F[..., -1:]
    U = G + torch.arange(1, N + 1, device=pred.device) - F
    den = torch.where(fgs, U, U * (U - 1)).clamp(min=1)
    num = torch.where(fgs, torch.ones_like(U), G - F)
    g = num.to(pred.dtype) / den.to(pred.dtype)
    present = G[..., 0] > 0                                                                  # [B, C]
    g = torch.where(vs & present[..., None], g, torch.zeros_like(g))
    L = (es * g).sum(-1)                                                                     # [B, C]
    P = present.sum(-1)
    loss = L.sum(-1) / P.clamp(min=1).to(pred.dtype)
    # a bad block: NaN, and NaN through every probability of the block
    nan = torch.where(bad, torch.full_like(loss, float("nan")), torch.zeros_like(loss))
    return loss + nan * p.sum((1, 2))


def loss(pred, label, inner_label=None, ignore=-1, scope="block", large=False):
    """the batch loss: the sum of the blocks' losses (scope="block"), or the loss of the call as one block of B * N rows
    (scope="batch", the paper's per_image=False).  Device tensors go to the kernels where tf_loss.supported says so (N <= MAX_N rows
    per block); with large=True also to the global-memory sort where tf_loss.supported_large says so (N <= MAX_N_LARGE);
    lovasz_torch otherwise.  large is an opt-in: without it the dispatch, and the bits, are what they were before it existed."""
    _check_scope(scope)
    B, N, C = pred.shape
    if scope == "batch":
        pred = pred.reshape(1, B * N, C)
        B, N = 1, B * N
        label = label.reshape(B, N)
        inner_label = inner_label.reshape(B, N) if inner_label is not None else None
    if pred.is_cuda:
        from .. import tf_loss
        if tf_loss.supported(N, C):
            return tf_loss.lovasz_softmax(pred, label, inner_label, ignore).sum()
        if large and tf_loss.supported_large(N, C):
            return tf_loss.lovasz_softmax_large(pred, label, inner_label, ignore).sum()
    return lovasz_torch(pred, label, inner_label, ignore).sum()


def with_xent(xent_fn, weight=1.0, scope="block", large=False):
    """-> loss_fn(pred, label, *rest) = xent_fn(pred, label, *rest) + weight * loss(pred, label, *rest[:1], scope=scope, large=large):
    a Trainer's loss_fn for the segmentation lines (S3DIS / ScanNet hand it (pred, label, inner_label); ShapeNet and RueMonge
    (pred, label))"""
    _check_scope(scope)

    def loss_fn(pred, label, *rest):
        return xent_fn(pred, label, *rest) + weight * loss(pred, label, *rest[:1], scope=scope, large=large)
    return loss_fn
