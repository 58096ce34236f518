"""Training losses beyond the reference's op list, on the HIP device only.

``lovasz_softmax(pred, label, inner_label=None, ignore=-1) -> [B]``: the Lovasz-softmax loss of every block (include/sph3d.h:
sph3d_lovasz_softmax; csrc/lovasz.hip; the float64 statement is harness/lovasz.py: lovasz_reference), averaged over the classes
present in the block.  One call computes the losses AND the gradient with respect to the logits, so the backward pass is one
scaling by the upstream gradient.  N <= 16384 points per block (``supported(N, C)``); harness/lovasz.py: loss() falls back to the
torch statement above that.
"""
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
