"""Training losses beyond the reference's op list, on the HIP device only.

``lovasz_softmax(pred, label, inner_label=None, ignore=-1) -> [B]``: the Lovasz-softmax loss of every block (include/sph3d.h:
sph3d_lovasz_softmax; csrc/lovasz.hip; the float64 statement is harness/lovasz.py: lovasz_reference), averaged over the classes
present in the block.  One call computes the losses AND the gradient with respect to the logits, so the backward pass is one
scaling by the upstream gradient.  N <= 16384 points per block (``supported(N, C)``); harness/lovasz.py: loss() falls back to the
torch statement above that.

``lovasz_softmax_large(pred, label, inner_label=None, ignore=-1, scope="block") -> [B]`` ([1] for scope="batch"): the same loss with
the sort in global memory (include/sph3d.h: sph3d_lovasz_softmax_large), for blocks of up to 2^20 rows and for the batch
reduction (``supported_large(N, C)``).  An opt-in: harness/lovasz.py: loss(..., large=True) dispatches to it.

``softmax_xent(pred, label, inner_label=None, class_weight=None, label_smoothing=0.0, ignore=None, normalize="count",
scope="block", return_counts=False) -> [B]`` ([1] for scope="batch"): the softmax cross-entropy with class weights, label smoothing
and an ignore label (include/sph3d.h: sph3d_softmax_xent; csrc/xent.hip; the float64 statement is harness/xent.py: xent_reference).
C <= 4096 (``xent_supported(N, C)``); harness/xent.py: loss() falls back to the torch statement beyond that.

``masked_softmax_xent(pred, label, inner_label) -> [B, S]``: the reference models' own training loss (include/sph3d.h:
sph3d_masked_softmax_xent), what harness/s3dis_net.py and harness/ruemonge_net.py: get_loss call.
"""
import weakref

import numpy as np
import torch

from . import _lib


def supported(N, C):
    return bool(_lib.lib().sph3d_lovasz_softmax_supported(int(N), int(C)))


class _LovaszSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label, inner_label, ignore, want_grad):
        B, N, C = pred.shape
        pred = _lib.f32(pred)
        label = label.reshape(B, N).long().contiguous()
        inner = inner_label.reshape(B, N).float().contiguous() if inner_label is not None else None
        loss = torch.empty((B,), dtype=torch.float32, device=pred.device)
        # probs, coef and class_loss are dead when the call's last kernel has run
        words = B * N * C
        ws = _lib.scratch(4 * (2 * words + B * C), pred.device)
        base = ws.data_ptr() if ws is not None else 0
        # (evaluation / no_grad: the losses only, no [B, N, C] gradient)
        dlogits = torch.empty_like(pred) if want_grad else None
        _lib.check(_lib.lib().sph3d_lovasz_softmax(B, N, C, _lib.ptr(pred), _lib.ptr(label), _lib.ptr(inner), int(ignore), base,
                                                   base + 4 * words, base + 8 * words, _lib.ptr(loss), _lib.ptr(dlogits), None,
                                                   _lib.stream_ptr()))
        if dlogits is not None:
            ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g[:, None, None], None, None, None, None


def lovasz_softmax(pred, label, inner_label=None, ignore=-1):
    """pred [B, N, C] logits, label [B, N] integer, inner_label [B, N] or None (rows with inner_label > 0 count; None: all rows);
    rows whose label equals `ignore` never count.  -> loss [B] float32"""
    tensors = (pred, label) if inner_label is None else (pred, label, inner_label)
    _lib.require_device(*tensors)
    # (grad mode is off inside forward(), and needs_input_grad ignores no_grad: the question is asked here)
    want_grad = torch.is_grad_enabled() and pred.requires_grad
    return _LovaszSoftmaxFn.apply(pred, label, inner_label, ignore, want_grad)


def supported_large(N, C):
    return bool(_lib.lib().sph3d_lovasz_softmax_large_supported(int(N), int(C)))


class _LovaszSoftmaxLargeFn(torch.autograd.Function):
    """_LovaszSoftmaxFn through sph3d_lovasz_softmax_large: the sort's workspace follows probs, coef and class_loss in the scratch"""

    @staticmethod
    def forward(ctx, pred, label, inner, ignore, want_grad):
        B, N, C = pred.shape
        l = _lib.lib()
        loss = torch.empty((B,), dtype=torch.float32, device=pred.device)
        words = B * N * C
        head = (4 * (2 * words + B * C) + 255) & ~255
        nbytes = l.sph3d_lovasz_softmax_large_workspace(B, N, C)
        ws = _lib.scratch(head + nbytes, pred.device)
        base = ws.data_ptr() if ws is not None else 0
        # (evaluation / no_grad: the losses only, no [B, N, C] gradient)
        dlogits = torch.empty_like(pred) if want_grad else None
        _lib.check(l.sph3d_lovasz_softmax_large(B, N, C, _lib.ptr(pred), _lib.ptr(label), _lib.ptr(inner), int(ignore), base,
                                                base + 4 * words, base + 8 * words, _lib.ptr(loss), _lib.ptr(dlogits), None,
                                                base + head, nbytes, 0, 0, _lib.stream_ptr()))
        if dlogits is not None:
            ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g[:, None, None], None, None, None, None


def lovasz_softmax_large(pred, label, inner_label=None, ignore=-1, scope="block"):
    """lovasz_softmax for blocks of up to 2^20 rows (``supported_large(N, C)``; include/sph3d.h: sph3d_lovasz_softmax_large): the
    sort runs in global memory.  scope="batch": the call is one block of B * N rows (the paper's per_image=False).
    -> loss [B] float32 ([1] for batch scope)"""
    tensors = (pred, label) if inner_label is None else (pred, label, inner_label)
    _lib.require_device(*tensors)
    if scope not in ("block", "batch"):
        raise ValueError("lovasz_softmax_large: scope should be 'block' or 'batch', got %r" % (scope,))
    B, N, C = pred.shape
    if scope == "batch":
        pred = pred.reshape(1, B * N, C)
        B, N = 1, B * N
    pred = _lib.f32(pred)
    label = label.reshape(B, N).long().contiguous()
    inner = inner_label.reshape(B, N).float().contiguous() if inner_label is not None else None
    # (grad mode is off inside forward(), and needs_input_grad ignores no_grad: the question is asked here)
    want_grad = torch.is_grad_enabled() and pred.requires_grad
    return _LovaszSoftmaxLargeFn.apply(pred, label, inner, ignore, want_grad)


# ---- the S3DIS / ScanNet / RueMonge training loss: mean cross-entropy over a block's inner points -------------------------------
class _MaskedXentFn(torch.autograd.Function):
    """one kernel that also produces the gradient with respect to the logits (include/sph3d.h: sph3d_masked_softmax_xent)"""

    @staticmethod
    def forward(ctx, pred, label, inner_label):
        B, N, C = pred.shape
        pred = _lib.f32(pred)
        label = label.reshape(B, N).long().contiguous()
        inner = inner_label.reshape(B, N).float().contiguous()
        S = _lib.lib().sph3d_masked_softmax_xent_parts(N)
        loss_part = torch.empty((B, S), dtype=torch.float32, device=pred.device)       # a block's loss in S slices of its points
        # (evaluation / no_grad: the losses only — no gradient pass, no [B, N, C] store)
        dlogits = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        _lib.check(_lib.lib().sph3d_masked_softmax_xent(B, N, C, _lib.ptr(pred), _lib.ptr(label), _lib.ptr(inner),
                                                        _lib.ptr(loss_part), _lib.ptr(dlogits), _lib.stream_ptr()))
        if dlogits is not None:
            ctx.save_for_backward(dlogits)
        return loss_part

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g[:, 0].reshape(-1, 1, 1), None, None       # (the slices of a block share its upstream gradient)


def masked_softmax_xent(pred, label, inner_label):
    """pred [B, N, C] logits, label [B, N], inner_label [B, N] (rows with inner_label > 0 count) -> [B, S] float32: a block's mean
    cross-entropy over its inner points in S shares (sum(1) is the block's loss; models/SPH3D_s3dis.py:116-133)"""
    return _MaskedXentFn.apply(pred, label, inner_label)


# ---- softmax cross-entropy with class weights, label smoothing and an ignore label ------------------------------------------------
XENT_MAX_C = 4096                  # csrc/xent.hip: kXentMaxC (sph3d_softmax_xent_supported)
_NORMALIZE = {"count": 0, "weight": 1}
_weights_seen = {}                 # id(tensor) -> (weak reference, version): class-weight tensors whose VALUES were found good


def xent_supported(N, C):
    return bool(_lib.lib().sph3d_softmax_xent_supported(int(N), int(C)))


def check_xent_options(C, class_weight=None, label_smoothing=0.0, ignore=None, normalize="count", scope="block"):
    """the options of softmax_xent, validated on the host (ValueError): class_weight [C] (its shape on every call), finite and >= 0
    (a tensor's values are read back once per tensor object and version); 0 <= label_smoothing < 1; ignore an integer or None; normalize "count" | "weight"; scope "block" |
    "batch".  -> (label_smoothing as float, ignore as int or None)"""
    if normalize not in _NORMALIZE:
        raise ValueError("softmax_xent: normalize should be 'count' or 'weight', got %r" % (normalize,))
    if scope not in ("block", "batch"):
        raise ValueError("softmax_xent: scope should be 'block' or 'batch', got %r" % (scope,))
    eps = float(label_smoothing)
    if not (0.0 <= eps < 1.0):
        raise ValueError("softmax_xent: label_smoothing should lie in [0, 1), got %r" % (label_smoothing,))
    if ignore is not None and (isinstance(ignore, bool) or int(ignore) != ignore):
        raise ValueError("softmax_xent: ignore should be an integer or None, got %r" % (ignore,))
    if class_weight is not None:
        if tuple(np.shape(class_weight)) != (C,):
            raise ValueError("softmax_xent: class_weight should be [%d], got %s" % (C, list(np.shape(class_weight))))
        # what is remembered is that THIS tensor object at THIS version holds good values: the entry dies with the tensor, so
        # another tensor at a recycled address or a recycled id is read back like any new one
        key = id(class_weight) if torch.is_tensor(class_weight) else None
        seen = _weights_seen.get(key)
        if seen is None or seen[0]() is not class_weight or seen[1] != class_weight._version:
            w = class_weight.detach().cpu().numpy() if key is not None else np.asarray(class_weight)
            if not (np.isfinite(w).all() and (w >= 0).all()):
                raise ValueError("softmax_xent: class_weight should be finite and >= 0")
            if key is not None:
                _weights_seen[key] = (weakref.ref(class_weight, lambda _r, _k=key: _weights_seen.pop(_k, None)), class_weight._version)
    return eps, (None if ignore is None else int(ignore))


class _SoftmaxXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label, inner, weight, eps, ignore, normalize, want_grad):
        B, N, C = pred.shape
        l = _lib.lib()
        S = l.sph3d_softmax_xent_parts(N)
        loss_part = torch.empty((B, S), dtype=torch.float32, device=pred.device)
        hist = torch.empty((B, C), dtype=torch.int32, device=pred.device)
        # the slices' histograms are dead when the call's second kernel has run
        nbytes = l.sph3d_softmax_xent_workspace(B, N, C)
        ws = _lib.scratch(nbytes, pred.device)
        # (evaluation / no_grad: the losses only, no [B, N, C] gradient)
        dlogits = torch.empty_like(pred) if want_grad else None
        _lib.check(l.sph3d_softmax_xent(B, N, C, _lib.ptr(pred), _lib.ptr(label), 64 if label.dtype == torch.int64 else 32,
                                        _lib.ptr(inner), _lib.ptr(weight), eps, ignore is not None, ignore if ignore is not None else 0,
                                        _NORMALIZE[normalize], _lib.ptr(loss_part), _lib.ptr(hist), _lib.ptr(dlogits), _lib.ptr(ws),
                                        nbytes, _lib.stream_ptr()))
        if dlogits is not None:
            ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(hist)
        return loss_part, hist

    @staticmethod
    def backward(ctx, g, _ghist):
        (dlogits,) = ctx.saved_tensors
        # (the slices of a block share its upstream gradient)
        return (dlogits * g[:, 0].reshape(-1, 1, 1),) + (None,) * 7


def softmax_xent(pred, label, inner_label=None, class_weight=None, label_smoothing=0.0, ignore=None, normalize="count",
                 scope="block", return_counts=False):
    """pred [B, N, C] logits (or [B, C]: N = 1), label [B, N] int32 or int64 (anything else is converted), inner_label [B, N] or None
    (rows with inner_label > 0 count; None: all rows), class_weight [C] fp32 or None; rows whose label equals `ignore` never count.
    scope="batch": the call is one block of B * N rows.  -> loss [B] float32 ([1] for batch scope); with return_counts also the
    int32 histogram [B, C] ([1, C]) of the counted rows' labels"""
    tensors = [pred, label] + [t for t in (inner_label, class_weight) if t is not None]
    if not all(torch.is_tensor(t) for t in tensors):
        raise _lib.Sph3dError("softmax_xent: pred, label, inner_label and class_weight are device tensors")
    _lib.require_device(*tensors)
    if pred.dim() == 2:
        pred = pred.unsqueeze(1)
    if pred.dim() != 3:
        raise ValueError("softmax_xent: pred should be [B, N, C] or [B, C], got %s" % (list(pred.shape),))
    B, N, C = pred.shape
    if label.numel() != B * N or (inner_label is not None and inner_label.numel() != B * N):
        raise ValueError("softmax_xent: label and inner_label should hold B * N = %d values" % (B * N))
    eps, ignore = check_xent_options(C, class_weight, label_smoothing, ignore, normalize, scope)
    if scope == "batch":
        pred = pred.reshape(1, B * N, C)
        B, N = 1, B * N
    pred = _lib.f32(pred)
    label = label.reshape(B, N)
    label = label.contiguous() if label.dtype in (torch.int32, torch.int64) else label.long().contiguous()
    inner = _lib.f32(inner_label.reshape(B, N)) if inner_label is not None else None
    weight = _lib.f32(class_weight) if class_weight is not None else None
    # (grad mode is off inside forward(), and needs_input_grad ignores no_grad: the question is asked here)
    want_grad = torch.is_grad_enabled() and pred.requires_grad
    loss_part, hist = _SoftmaxXentFn.apply(pred, label, inner, weight, eps, ignore, normalize, want_grad)
    loss = loss_part.sum(1) if loss_part.shape[1] > 1 else loss_part[:, 0]
    return (loss, hist) if return_counts else loss
