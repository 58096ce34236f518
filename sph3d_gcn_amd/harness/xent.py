"""Softmax cross-entropy with class weights, label smoothing and an ignore label, per block: the numpy STATEMENT of csrc/xent.hip
(include/sph3d.h: sph3d_softmax_xent), the same statement in torch ops, class weights from label counts, and the loss functions a
Trainer takes.

For block b with logits x [N, C], labels y [N] and weights w [C] (fp32, finite, >= 0; absent: all 1), p = softmax(x), lse = log sum exp x:

  counted   R_b = {n: (inner is None or inner[b,n] > 0; NaN > 0 is false) and y_n != ignore}; ignore=None: no label is ignored
  targets   t[n,c] = (1 - eps) w_y [c == y_n] + (eps / C) w_c,   A_n = sum_c t[n,c]
  row       l_n = sum_c t[n,c] (lse_n - x[n,c])       (torch's cross_entropy with weight and label_smoothing)
  hist      h[b,c] = #{n in R_b: y_n = c}, exact integers
  D_b       "count": fp32(sum_c h[b,c]);  "weight": fp32(sum_c float64(h[b,c]) float64(w_c)), summed in ascending c (torch's
            reduction='mean').  A function of the integer histogram, so independent of the order in which rows are visited.
  loss_b    sum_{n in R_b} l_n / D_b;  dlogits[b,n,:] = (A_n p[n,:] - t[n,:]) / D_b on counted rows, exact zeros elsewhere;
            D_b = 0 (no counted row, or only zero-weight classes): loss 0 and a zero gradient

A counted row whose label lies outside [0, C) is in no class of the histogram; it makes its block's loss (its part of it) and its own
gradient row NaN.  scope="batch" treats the call as ONE block of B * N rows: the ShapeNet, RueMonge and ModelNet reductions.
"""
import numpy as np
import torch

from .. import tf_loss

MAX_PARTS = 256                    # csrc/xent.hip: kXentMaxParts


def xent_form(N):
    """sph3d_softmax_xent_parts and the slice a workgroup handles (csrc/xent.hip): S = ceil(N / 1024), at most 256 — for
    N <= 16384 sph3d_masked_softmax_xent_parts(N)"""
    S = min(MAX_PARTS, max(1, (N + 1023) // 1024))
    chunk = (N + S - 1) // S
    return dict(S=S, chunk=chunk, trips=(chunk + 1023) // 1024)


def _parts(v, S, chunk):
    """[B, N] -> [B, S, chunk], rows past N as zeros"""
    B, N = v.shape
    out = np.zeros((B, S * chunk), v.dtype)
    out[:, :N] = v
    return out.reshape(B, S, chunk)


def denominators(hist, class_weight=None, normalize="count"):
    """hist [B, C] integers -> D [B] float32, exactly as stated: one rounding of an integer sum, or of a float64 sum in ascending c"""
    hist = np.asarray(hist).astype(np.int64)
    if normalize == "count" or class_weight is None:
        return hist.sum(1).astype(np.float32)
    w = np.asarray(class_weight, np.float32).astype(np.float64)
    D = np.zeros(hist.shape[0], np.float32)
    for b in range(hist.shape[0]):
        d = 0.0
        for c in range(hist.shape[1]):
            d += float(hist[b, c]) * float(w[c])
        D[b] = np.float32(d)
    return D


def xent_reference(logits, label, inner=None, class_weight=None, label_smoothing=0.0, ignore=None, normalize="count", scope="block"):
    """logits [B,N,C] (or [B,C]: N = 1), label [B,N] integer, inner [B,N] or None, class_weight [C] or None -> dict of float64 arrays
    unless said otherwise: loss [B], loss_part [B,S] (the shares of the S slices of xent_form(N)), dlogits [B,N,C], hist [B,C] int32,
    D [B] float32 (bitwise the kernel's), counted and bad [B,N] bool, and the term magnitudes the bounds are written in: row_mag
    [B,N] = A (|m| + |log se| + 1) + sum_c t_c |x_c| on counted rows, part_mag [B,S] = the sum of a slice's row_mag / D, grad_mag
    [B,N,C] = (A p (1 + |x| + |m|) + t) / D.  Batch scope: B = 1 and N = B * N throughout."""
    tf_loss.check_xent_options(np.shape(logits)[-1], class_weight, label_smoothing, ignore, normalize, scope)
    x = np.asarray(logits, np.float64)
    if x.ndim == 2:
        x = x[:, None, :]
    B, N, C = x.shape
    if scope == "batch":
        x = x.reshape(1, B * N, C)
        B, N = 1, B * N
    label = np.asarray(label).reshape(B, N).astype(np.int64)
    counted = np.ones((B, N), bool) if ignore is None else label != ignore
    if inner is not None:
        with np.errstate(invalid="ignore"):
            counted &= np.asarray(inner).reshape(B, N) > 0
    eps = float(label_smoothing)
    w = np.ones(C) if class_weight is None else np.asarray(class_weight, np.float32).astype(np.float64)
    f = xent_form(N)
    oob = (label < 0) | (label >= C)
    bad = counted & oob
    y = np.where(oob, 0, label)
    hist = np.zeros((B, C), np.int64)
    for b in range(B):
        hist[b] = np.bincount(label[b][counted[b] & ~oob[b]], minlength=C)
    D = denominators(hist, class_weight, normalize)
    D64 = D.astype(np.float64)
    inv = np.where(D64 > 0, 1.0 / np.where(D64 > 0, D64, 1.0), 0.0)
    m = x.max(-1)
    e = np.exp(x - m[..., None])
    se = e.sum(-1)
    lse = m + np.log(se)
    xy = np.take_along_axis(x, y[..., None], -1)[..., 0]
    wy = w[y]
    row = wy * (lse - xy)
    if eps != 0.0:
        row = (1.0 - eps) * row + (eps / C) * ((lse[..., None] - x) * w).sum(-1)
    row = np.where(counted, row, 0.0)
    onehot = (np.arange(C) == y[..., None]).astype(np.float64)
    t = ((1.0 - eps) * wy)[..., None] * onehot
    if eps != 0.0:
        t = t + (eps / C) * w
    A = t.sum(-1) if eps != 0.0 else (1.0 - eps) * wy
    p = e / se[..., None]
    scale = (counted * inv[:, None])[..., None]
    d = scale * (A[..., None] * p - t)
    d[bad] = np.nan
    loss_part = _parts(row, f["S"], f["chunk"]).sum(-1) * inv[:, None]
    loss_part[_parts(bad, f["S"], f["chunk"]).any(-1)] = np.nan
    loss = np.where(D64 > 0, row.sum(-1) * inv, 0.0)
    loss[bad.any(-1)] = np.nan
    row_mag = np.where(counted, A * (np.abs(m) + np.abs(np.log(se)) + 1.0) + (t * np.abs(x)).sum(-1), 0.0)
    return dict(loss=loss, loss_part=loss_part, dlogits=d, hist=hist.astype(np.int32), D=D, counted=counted, bad=bad, row_mag=row_mag,
                part_mag=_parts(row_mag, f["S"], f["chunk"]).sum(-1) * inv[:, None],
                grad_mag=scale * (A[..., None] * p * (1.0 + np.abs(x) + np.abs(m)[..., None]) + t), form=f)


def xent_torch(pred, label, inner_label=None, class_weight=None, label_smoothing=0.0, ignore=None, normalize="count", scope="block",
               return_counts=False):
    """the statement in torch ops, on any device and in pred's dtype, differentiable in pred: -> loss [B] ([1] for batch scope), with
    return_counts also the int32 histogram.  The fallback for CPU tensors and for more than 4096 classes, and the baseline the
    kernels are measured against.  (D's float64 sum is torch's, not in ascending c: it is the numpy statement that is bitwise.)"""
    if pred.dim() == 2:
        pred = pred.unsqueeze(1)
    B, N, C = pred.shape
    eps, ignore = tf_loss.check_xent_options(C, class_weight, label_smoothing, ignore, normalize, scope)
    if scope == "batch":
        pred = pred.reshape(1, B * N, C)
        B, N = 1, B * N
    label = label.reshape(B, N).long()
    counted = torch.ones_like(label, dtype=torch.bool) if ignore is None else label != ignore
    if inner_label is not None:
        counted = counted & (inner_label.reshape(B, N) > 0)
    oob = (label < 0) | (label >= C)
    y = torch.where(oob, torch.zeros_like(label), label)
    w = torch.ones(C, dtype=pred.dtype, device=pred.device) if class_weight is None else \
        torch.as_tensor(class_weight, device=pred.device).to(pred.dtype)
    hist = torch.zeros((B, C), dtype=torch.int64, device=pred.device).scatter_add_(1, y, (counted & ~oob).long())
    if normalize == "count" or class_weight is None:
        D = hist.sum(1).float()
    else:
        D = (hist.double() * torch.as_tensor(class_weight, device=pred.device).float().double()).sum(1).float()
    D = D.to(pred.dtype)
    inv = torch.where(D > 0, 1.0 / torch.where(D > 0, D, torch.ones_like(D)), torch.zeros_like(D))
    lse = torch.logsumexp(pred, dim=-1)
    wy = w[y]
    row = wy * (lse - torch.gather(pred, 2, y[..., None])[..., 0])
    if eps != 0.0:
        row = (1.0 - eps) * row + (eps / C) * ((lse[..., None] - pred) * w).sum(-1)
    row = torch.where(counted, row, torch.zeros_like(row))
    # a counted label outside the classes: NaN, and NaN through the row's logits
    nan = torch.where(counted & oob, torch.full_like(row, float("nan")), torch.zeros_like(row))
    loss = ((row + nan * lse) * inv[:, None]).sum(-1)
    return (loss, hist.int()) if return_counts else loss


def loss(pred, label, inner_label=None, class_weight=None, label_smoothing=0.0, ignore=None, normalize="count", scope="block"):
    """the blocks' losses [B] ([1] for batch scope): the kernels for device tensors with C <= 4096, xent_torch otherwise"""
    if pred.is_cuda and tf_loss.xent_supported(1 if pred.dim() == 2 else pred.shape[1], pred.shape[-1]):
        if class_weight is not None and not (torch.is_tensor(class_weight) and class_weight.device == pred.device):
            class_weight = torch.as_tensor(class_weight, dtype=torch.float32).to(pred.device)
        return tf_loss.softmax_xent(pred, label, inner_label, class_weight, label_smoothing, ignore, normalize, scope)
    return xent_torch(pred, label, inner_label, class_weight, label_smoothing, ignore, normalize, scope)


# ---- class weights --------------------------------------------------------------------------------------------------------------------
def class_counts(pool_or_labels, C, inner_only=True):
    """a feed.BlockPool (rows [T, 8]: label in column 6, inner in column 7) or a tensor / array of labels -> counts [C] int64 numpy:
    torch.bincount of the labels inside [0, C); inner_only: of a pool's inner rows only.  It runs once, on whatever device the
    labels are."""
    rows = getattr(pool_or_labels, "rows", None)
    if rows is not None:
        label = rows[:, 6].long()
        if inner_only:
            label = label[rows[:, 7] > 0]
    else:
        label = torch.as_tensor(pool_or_labels).reshape(-1).long()
    label = label[(label >= 0) & (label < C)]
    return torch.bincount(label, minlength=C).cpu().numpy().astype(np.int64)


SCHEMES = ("inverse", "inverse_sqrt", "median", "log")


def class_weights(counts, scheme="inverse"):
    """counts [C] -> weights [C] float32, computed in float64; a class without a sample gets weight 0.  With f_c = n_c / sum n and P
    the number of classes present:
      "inverse"        1 / (P f_c)                 (the weighted class counts sum to the row count)
      "inverse_sqrt"   1 / sqrt(P f_c)
      "median"         median over the present classes of f / f_c       (median-frequency balancing, Eigen and Fergus 2015)
      "log"            1 / ln(1.02 + f_c)          (ENet, Paszke et al. 2016)"""
    n = np.asarray(counts, np.float64).reshape(-1)
    if scheme not in SCHEMES:
        raise ValueError("class_weights: scheme should be one of %s, got %r" % (", ".join(SCHEMES), scheme))
    if not (np.isfinite(n).all() and (n >= 0).all()):
        raise ValueError("class_weights: counts should be finite and >= 0")
    present = n > 0
    w = np.zeros_like(n)
    if present.any():
        f = n[present] / n.sum()
        P = float(present.sum())
        if scheme == "inverse":
            w[present] = 1.0 / (P * f)
        elif scheme == "inverse_sqrt":
            w[present] = 1.0 / np.sqrt(P * f)
        elif scheme == "median":
            w[present] = np.median(f) / f
        else:
            w[present] = 1.0 / np.log(1.02 + f)
    return w.astype(np.float32)


# ---- a Trainer's loss_fn ----------------------------------------------------------------------------------------------------------------
BLOCK_LINES = ("s3dis", "scannet")                                    # the sum of the blocks' losses (inner mask)
BATCH_LINES = ("shapenet", "shapenet_onehot", "ruemonge", "modelnet")  # one mean over every row of the batch


def make_loss(line, class_weight=None, label_smoothing=0.0, ignore=None, normalize=None):
    """-> loss_fn(pred, *loss_args) for a Trainer of the dataset line `line` (a key of train.LINES), with the line's own reduction:
    S3DIS / ScanNet (pred, label, inner_label): the sum of the blocks' losses; ShapeNet, one-hot, RueMonge (pred, label) and
    ModelNet (pred [B, C], label [B]): batch scope.  normalize=None is "count".  With every option absent the value is the line's
    model.loss (without the ModelNet net's regularisers, which the Trainer adds).  It composes: lovasz.with_xent(make_loss(...), w)."""
    if line not in BLOCK_LINES + BATCH_LINES:
        raise ValueError("make_loss: line should be one of %s, got %r" % (", ".join(BLOCK_LINES + BATCH_LINES), line))
    normalize = "count" if normalize is None else normalize
    scope = "block" if line in BLOCK_LINES else "batch"
    if class_weight is not None and not torch.is_tensor(class_weight):
        class_weight = torch.as_tensor(np.asarray(class_weight, np.float32))
    tf_loss.check_xent_options(len(class_weight) if class_weight is not None else 1, class_weight, label_smoothing, ignore, normalize,
                               scope)
    on_device = {}

    def weight_on(device):
        if class_weight is None:
            return None
        if device not in on_device:
            on_device[device] = class_weight.to(device=device, dtype=torch.float32)
        return on_device[device]

    def loss_fn(pred, label, *rest):
        inner = rest[0] if (scope == "block" and rest) else None
        return loss(pred, label, inner, weight_on(pred.device), label_smoothing, ignore, normalize, scope).sum()
    return loss_fn
