"""Fused ELU + batch normalisation — the tail of separable_conv3d / pointwise_conv3d
(utils/sph3gcn_util.py:152-161: activation_fn=tf.nn.elu then tf.layers.batch_normalization(momentum=0.99,
epsilon=1e-3); stock TF ops in the reference, SURVEY §8f item 3 here).

``elu_batch_norm(y, gamma, beta, moving_mean, moving_var, training)`` == batch_norm(elu(y)) over all but the last axis,
as ONE custom op (``sph3d::elu_bn``) whose backward needs only y.

``set_sync(reducer)`` / ``with sync(reducer):`` switch every training-mode batch norm of the layer functions to statistics over
all ranks' rows: the ops are cut at the statistics, and ``reducer`` sums the cut's float64 buffer over the ranks.
``tail_forward`` / ``tail_backward`` are the tail of every layer function, and the one place that chooses between the two.
"""
import contextlib
from typing import Optional, Tuple

import torch

from . import _lib

MOMENTUM = 0.99       # tf.layers.batch_normalization(momentum=0.99): weight of the OLD moving statistics
EPSILON = 1e-3        # TF default epsilon
MAX_ROWS = 2 ** 31 - 1024      # csrc/norm.hip: kNormMaxRows, the most rows the statistics pass indexes in int


def supported(C):
    return C % 4 == 0 and C <= 1024


# ---- batch statistics over all ranks' rows -----------------------------------------------------------------------------------
# A reducer is a callable reducer(buf): it replaces the 1-D float64 tensor `buf` IN PLACE by its sum over the ranks, orders the
# CURRENT stream after the result and does not block the host (harness/dist.py: stat_all_reduce).  While one is set, every
# training-mode batch norm calls it exactly once per forward pass, with [sum x, sum x^2, rows] = [2C + 1] values, and once per
# backward pass, with [sum dout, sum dout * xhat] = [2C]; the backward pass uses the reducer that was set in its forward pass.
# Inference mode never calls it.  Every rank must run the same sequence of layers, each with at least one row; the ranks' row
# counts may differ (the count travels in the buffer).
_sync = None


def set_sync(reducer):
    """reducer: a callable as described above, or None (each rank's own rows: the default) -> the previous value"""
    global _sync
    prev, _sync = _sync, reducer
    return prev


def sync_reducer():
    return _sync


@contextlib.contextmanager
def sync(reducer):
    prev = set_sync(reducer)
    try:
        yield reducer
    finally:
        set_sync(prev)


# ---- what every wrapper below does before its launch -------------------------------------------------------------------------------
def _rows(op, y):
    """y [..., C] -> y as contiguous float32 on the device, R, C.  More rows than the kernels index are a ValueError here: ctypes
    would wrap R into the C ABI's int without a word."""
    if not y.is_cuda:
        _lib.require_device(y)
    C = y.shape[-1]
    R = y.numel() // C
    if R > MAX_ROWS:
        raise ValueError("%s: %d rows, at most %d" % (op, R, MAX_ROWS))
    return _lib.f32(y), R, C


def _on_device(t):
    """another operand of y's kind (dout, partial) -> contiguous float32 on the device"""
    if not t.is_cuda:
        _lib.require_device(t)
    return _lib.f32(t)


def _workspace(R, C, device):
    """-> the address and size of the call-local workspace of one C-ABI call"""
    wsb = _lib.lib().sph3d_elu_bn_workspace(R, C)
    return _lib.ptr(_lib.scratch(wsb, device)), wsb


def _per_channel(op, C, names, *operands):
    """every per-channel operand of a launch: on the device, float32, contiguous, exactly [C].  The kernels take them as bare
    addresses and read C floats (write C floats into the moving statistics, which can therefore not be converted into a copy):
    anything else is a ValueError BEFORE the launch, so nothing is read out of bounds or as another type on the device."""
    for t in operands:
        # (a 1-D tensor of C > 1 elements is contiguous exactly when its stride is 1; the cheapest form: 34 launches a step come here)
        if t.stride() != _UNIT or t.numel() != C or t.dtype != _F32 or not t.is_cuda:
            _lib.require_device(*operands)
            for name, t in zip(names, operands):
                if t.dtype != _F32 or t.dim() != 1 or t.numel() != C or not t.is_contiguous():
                    raise ValueError("%s: %s should be a contiguous float32 [%d] (got %s %s, strides %s)"
                                     % (op, name, C, str(t.dtype).replace("torch.", ""), list(t.shape), list(t.stride())))


def _summed(op, name, t, n):
    """a float64 buffer of the cut: on the device, contiguous, exactly [n]"""
    _lib.require_device(t)
    if t.dtype != torch.float64 or t.numel() != n or not t.is_contiguous():
        raise ValueError("%s: %s should be a contiguous float64 [%d]" % (op, name, n))


_F32, _UNIT = torch.float32, (1,)
_FWD_NAMES = ("gamma", "beta", "moving_mean", "moving_var")
_BWD_NAMES = ("gamma", "save_mean", "save_rstd")


def _fwd_impl(y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, moving_mean: torch.Tensor,
              moving_var: torch.Tensor, training: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    y, R, C = _rows("elu_bn", y)
    _per_channel("elu_bn", C, _FWD_NAMES, gamma, beta, moving_mean, moving_var)
    out = torch.empty_like(y)
    save_mean, save_rstd = torch.empty_like(gamma), torch.empty_like(gamma)      # (gamma was just checked: float32 [C] on the device)
    ws, wsb = _workspace(R, C, y.device)
    _lib.check(_lib.lib().sph3d_elu_bn_forward(R, C, y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), moving_mean.data_ptr(),
                                                moving_var.data_ptr(), 1.0 - MOMENTUM, EPSILON, 1 if training else 0, out.data_ptr(),
                                                save_mean.data_ptr(), save_rstd.data_ptr(), ws, wsb, _lib.stream_ptr()))
    return out, save_mean, save_rstd


def _bwd_impl(y: torch.Tensor, dout: torch.Tensor, gamma: torch.Tensor, save_mean: torch.Tensor,
              save_rstd: torch.Tensor, training: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    y, R, C = _rows("elu_bn_grad", y)
    dout = _on_device(dout)
    _per_channel("elu_bn_grad", C, _BWD_NAMES, gamma, save_mean, save_rstd)
    dy = torch.empty_like(y)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    ws, wsb = _workspace(R, C, y.device)
    _lib.check(_lib.lib().sph3d_elu_bn_backward(R, C, y.data_ptr(), dout.data_ptr(), gamma.data_ptr(), save_mean.data_ptr(),
                                                 save_rstd.data_ptr(), 1 if training else 0, dy.data_ptr(), dgamma.data_ptr(),
                                                 dbeta.data_ptr(), ws, wsb, _lib.stream_ptr()))
    return dy, dgamma, dbeta


_elu_bn = torch.library.custom_op("sph3d::elu_bn", mutates_args=("moving_mean", "moving_var"))(_fwd_impl)
_elu_bn_grad = torch.library.custom_op("sph3d::elu_bn_grad", mutates_args=())(_bwd_impl)


@_elu_bn.register_fake
def _(y, gamma, beta, moving_mean, moving_var, training):
    return torch.empty_like(y), torch.empty_like(gamma), torch.empty_like(gamma)


@_elu_bn_grad.register_fake
def _(y, dout, gamma, save_mean, save_rstd, training):
    return torch.empty_like(y), torch.empty_like(gamma), torch.empty_like(gamma)


# ---- the two ops cut at the statistics (csrc/norm.hip: sph3d_elu_bn_{forward,backward}_{sums,apply}) ------------------------------
def elu_bn_forward_sums(y: torch.Tensor, partial: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> float64 [2C + 1]: per-channel sum elu(y), sum elu(y)^2 over this rank's rows, then the row count.  partial [nblk, 2, C]:
    the statistics' partial sums where a producer of y already wrote them (the GEMM's epilogue, the one-kernel separable layer)"""
    y, R, C = _rows("elu_bn_forward_sums", y)
    sums = torch.empty((2 * C + 1,), dtype=torch.float64, device=y.device)
    if partial is None:
        nblk, ws, wsb = 0, *_workspace(R, C, y.device)
    else:
        partial = _on_device(partial)
        if partial.dim() != 3 or partial.shape[1] != 2 or partial.shape[2] != C or partial.shape[0] < 1:
            raise ValueError("elu_bn_forward_sums: partial should be [nblk >= 1, 2, %d]" % C)
        nblk, ws, wsb = partial.shape[0], None, 0
    _lib.check(_lib.lib().sph3d_elu_bn_forward_sums(R, C, nblk, _lib.ptr(partial), _lib.ptr(y), _lib.ptr(sums), ws, wsb,
                                                     _lib.stream_ptr()))
    return sums


def elu_bn_forward_apply(y: torch.Tensor, sums: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, moving_mean: torch.Tensor,
                         moving_var: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """sums: the [2C + 1] buffer summed over the ranks -> out, save_mean, save_rstd, count (float64 [1]: the global row count,
    kept on the device for elu_bn_backward_apply); updates the moving statistics"""
    y, R, C = _rows("elu_bn_forward_apply", y)
    _summed("elu_bn_forward_apply", "sums", sums, 2 * C + 1)
    _per_channel("elu_bn_forward_apply", C, _FWD_NAMES, gamma, beta, moving_mean, moving_var)
    out = torch.empty_like(y)
    save_mean, save_rstd = torch.empty_like(gamma), torch.empty_like(gamma)
    count = torch.empty((1,), dtype=torch.float64, device=y.device)
    _lib.check(_lib.lib().sph3d_elu_bn_forward_apply(R, C, _lib.ptr(sums), _lib.ptr(y), _lib.ptr(gamma), _lib.ptr(beta),
                                                      _lib.ptr(moving_mean), _lib.ptr(moving_var), 1.0 - MOMENTUM, EPSILON,
                                                      _lib.ptr(out), _lib.ptr(save_mean), _lib.ptr(save_rstd), _lib.ptr(count),
                                                      _lib.stream_ptr()))
    return out, save_mean, save_rstd, count


def elu_bn_backward_sums(y: torch.Tensor, dout: torch.Tensor, save_mean: torch.Tensor,
                         save_rstd: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> dgamma, dbeta (this rank's sums, fp32: the gradient all-reduce adds the ranks') and float64 [2C]: per-channel
    sum dout, sum dout * zhat over this rank's rows"""
    y, R, C = _rows("elu_bn_backward_sums", y)
    dout = _on_device(dout)
    _per_channel("elu_bn_backward_sums", C, _BWD_NAMES[1:], save_mean, save_rstd)
    dgamma, dbeta = torch.empty_like(save_mean), torch.empty_like(save_mean)
    sums = torch.empty((2 * C,), dtype=torch.float64, device=y.device)
    ws, wsb = _workspace(R, C, y.device)
    _lib.check(_lib.lib().sph3d_elu_bn_backward_sums(R, C, _lib.ptr(y), _lib.ptr(dout), _lib.ptr(save_mean), _lib.ptr(save_rstd),
                                                      _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(sums), ws, wsb, _lib.stream_ptr()))
    return dgamma, dbeta, sums


def elu_bn_backward_apply(y: torch.Tensor, dout: torch.Tensor, gamma: torch.Tensor, save_mean: torch.Tensor,
                          save_rstd: torch.Tensor, sums: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """sums: the [2C] buffer summed over the ranks; count: elu_bn_forward_apply's -> dy over this rank's rows"""
    y, R, C = _rows("elu_bn_backward_apply", y)
    dout = _on_device(dout)
    _summed("elu_bn_backward_apply", "sums", sums, 2 * C)
    _summed("elu_bn_backward_apply", "count", count, 1)
    _per_channel("elu_bn_backward_apply", C, _BWD_NAMES, gamma, save_mean, save_rstd)
    dy = torch.empty_like(y)
    ws, wsb = _workspace(R, C, y.device)
    _lib.check(_lib.lib().sph3d_elu_bn_backward_apply(R, C, _lib.ptr(sums), _lib.ptr(count), _lib.ptr(y), _lib.ptr(dout),
                                                       _lib.ptr(gamma), _lib.ptr(save_mean), _lib.ptr(save_rstd), _lib.ptr(dy), ws, wsb,
                                                       _lib.stream_ptr()))
    return dy


_fwd_sums_op = torch.library.custom_op("sph3d::elu_bn_forward_sums", mutates_args=())(elu_bn_forward_sums)
_fwd_apply_op = torch.library.custom_op("sph3d::elu_bn_forward_apply", mutates_args=("moving_mean", "moving_var"))(elu_bn_forward_apply)
_bwd_sums_op = torch.library.custom_op("sph3d::elu_bn_backward_sums", mutates_args=())(elu_bn_backward_sums)
_bwd_apply_op = torch.library.custom_op("sph3d::elu_bn_backward_apply", mutates_args=())(elu_bn_backward_apply)


@_fwd_sums_op.register_fake
def _(y, partial=None):
    return y.new_empty((2 * y.shape[-1] + 1,), dtype=torch.float64)


@_fwd_apply_op.register_fake
def _(y, sums, gamma, beta, moving_mean, moving_var):
    return torch.empty_like(y), torch.empty_like(gamma), torch.empty_like(gamma), sums.new_empty((1,))


@_bwd_sums_op.register_fake
def _(y, dout, save_mean, save_rstd):
    return torch.empty_like(save_mean), torch.empty_like(save_mean), y.new_empty((2 * y.shape[-1],), dtype=torch.float64)


@_bwd_apply_op.register_fake
def _(y, dout, gamma, save_mean, save_rstd, sums, count):
    return torch.empty_like(y)


# ---- the tail of every layer function: the one place that asks whether a reducer is set ------------------------------------------
def tail_forward(y, partial, gamma, beta, moving_mean, moving_var, training):
    """out = batch_norm(elu(y)).  partial: the statistics' partial sums [nblk, 2, C] where the producer of y wrote them (training
    mode only), else None: the statistics pass over y runs.  -> out, saved = (save_mean, save_rstd, count, reducer), what
    tail_backward needs: count (float64 [1], the global row count) and reducer are None unless a reducer was in force."""
    reducer = _sync if training else None
    count = None
    if reducer is not None:
        sums = elu_bn_forward_sums(y, partial)
        reducer(sums)
        out, save_mean, save_rstd, count = elu_bn_forward_apply(y, sums, gamma, beta, moving_mean, moving_var)
    elif partial is not None:
        out, save_mean, save_rstd = _elu_bn_partials_impl(y, partial, gamma, beta, moving_mean, moving_var)
    else:
        out, save_mean, save_rstd = _fwd_impl(y, gamma, beta, moving_mean, moving_var, training)
    return out, (save_mean, save_rstd, count, reducer)


def tail_backward(saved, y, dout, gamma, training):
    """saved: tail_forward's -> dy, dgamma, dbeta"""
    save_mean, save_rstd, count, reducer = saved
    if reducer is None:
        return _bwd_impl(y, dout, gamma, save_mean, save_rstd, training)
    dgamma, dbeta, sums = elu_bn_backward_sums(y, dout, save_mean, save_rstd)
    reducer(sums)
    return elu_bn_backward_apply(y, dout, gamma, save_mean, save_rstd, sums, count), dgamma, dbeta


# (sph3d::elu_bn updates the moving statistics in place, so the dispatcher accepts no autograd formula for it: the
# gradient wiring of the fused tail is _EluBnFn below, over the functional sph3d::elu_bn_grad.)


class _EluBnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, gamma, beta, moving_mean, moving_var, training):
        out, (save_mean, save_rstd, count, ctx.reducer) = tail_forward(y, None, gamma, beta, moving_mean, moving_var, training)
        ctx.save_for_backward(y, gamma, save_mean, save_rstd, count)
        ctx.training = training
        return out

    @staticmethod
    def backward(ctx, dout):
        y, gamma, save_mean, save_rstd, count = ctx.saved_tensors
        dy, dgamma, dbeta = tail_backward((save_mean, save_rstd, count, ctx.reducer), y, dout, gamma, ctx.training)
        return dy, dgamma, dbeta, None, None, None


def elu_batch_norm(y, gamma, beta, moving_mean, moving_var, training=True):
    return _EluBnFn.apply(y, gamma, beta, moving_mean, moving_var, bool(training))


# ---- layer tail with the statistics in the GEMM's epilogue (first half) ---------------------------------
def gemm_bn_blocks(R, Cin, Cout):
    """row blocks of partial statistics sph3d_pointwise_gemm_bnstats writes for this shape; 0 = shape not covered"""
    return int(_lib.lib().sph3d_pointwise_gemm_bnstats_blocks(int(R), int(Cin), int(Cout)))


def _gemm_bnstats_impl(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """y[R,Cout] = x @ w (+ bias) and partial[nblk, 2, Cout] = per row block (sum elu(y), sum elu(y)^2)"""
    _lib.require_device(x, w)
    x, w = _lib.f32(x), _lib.f32(w)
    if bias is not None:
        bias = _lib.f32(bias)
    R, Cin = x.shape
    Cout = w.shape[1]
    nblk = gemm_bn_blocks(R, Cin, Cout)
    if nblk == 0:
        raise ValueError("pointwise_gemm_bnstats: shape (%d, %d -> %d) is not covered (whole tiles needed)" % (R, Cin, Cout))
    y = torch.empty((R, Cout), dtype=torch.float32, device=x.device)
    partial = torch.empty((nblk, 2, Cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().sph3d_pointwise_gemm_bnstats(R, Cin, Cout, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y),
                                                        _lib.ptr(partial), _lib.stream_ptr()))
    return y, partial


def _elu_bn_partials_impl(y: torch.Tensor, partial: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                          moving_mean: torch.Tensor, moving_var: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """training-mode elu_bn whose statistics come from `partial` instead of a pass over y"""
    y, R, C = _rows("elu_bn_partials", y)
    partial = _on_device(partial)
    _per_channel("elu_bn_partials", C, _FWD_NAMES, gamma, beta, moving_mean, moving_var)
    out = torch.empty_like(y)
    save_mean, save_rstd = torch.empty_like(gamma), torch.empty_like(gamma)
    _lib.check(_lib.lib().sph3d_elu_bn_forward_partials(R, C, partial.shape[0], partial.data_ptr(), y.data_ptr(), gamma.data_ptr(),
                                                         beta.data_ptr(), moving_mean.data_ptr(), moving_var.data_ptr(),
                                                         1.0 - MOMENTUM, EPSILON, out.data_ptr(), save_mean.data_ptr(),
                                                         save_rstd.data_ptr(), _lib.stream_ptr()))
    return out, save_mean, save_rstd


_gemm_bnstats = torch.library.custom_op("sph3d::pointwise_gemm_bnstats", mutates_args=())(_gemm_bnstats_impl)
_elu_bn_partials = torch.library.custom_op("sph3d::elu_bn_partials", mutates_args=("moving_mean", "moving_var"))(_elu_bn_partials_impl)


@_gemm_bnstats.register_fake
def _(x, w, bias=None):
    nblk = gemm_bn_blocks(x.shape[0], x.shape[1], w.shape[1])
    return x.new_empty((x.shape[0], w.shape[1])), x.new_empty((nblk, 2, w.shape[1]))


@_elu_bn_partials.register_fake
def _(y, partial, gamma, beta, moving_mean, moving_var):
    return torch.empty_like(y), torch.empty_like(gamma), torch.empty_like(gamma)


class _GemmEluBnFn(torch.autograd.Function):
    """out = batch_norm(elu(x @ w)) in training mode: GEMM (statistics in its epilogue) -> finalize -> apply.  Saves the raw
    product y; the backward is elu_bn's followed by the GEMM's two gradient products."""

    @staticmethod
    def forward(ctx, x, w, bias, gamma, beta, moving_mean, moving_var):
        y, partial = _gemm_bnstats_impl(x, w, bias)
        out, (save_mean, save_rstd, count, ctx.reducer) = tail_forward(y, partial, gamma, beta, moving_mean, moving_var, True)
        ctx.save_for_backward(x, w, y, gamma, save_mean, save_rstd, count)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import tf_gemm
        x, w, y, gamma, save_mean, save_rstd, count = ctx.saved_tensors
        dy, dgamma, dbeta = tail_backward((save_mean, save_rstd, count, ctx.reducer), y, dout, gamma, True)
        dx = tf_gemm._pointwise_gemm_impl(dy, w, True) if ctx.needs_input_grad[0] else None
        dw = tf_gemm._pointwise_gemm_tn_impl(x, dy) if ctx.needs_input_grad[1] else None
        db = dy.sum(0) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db, dgamma, dbeta, None, None


def gemm_elu_batch_norm(x, w, gamma, beta, moving_mean, moving_var, bias=None):
    """x[R,Cin] @ w[Cin,Cout] (+ bias) -> ELU -> batch norm (training statistics), one fused tail"""
    return _GemmEluBnFn.apply(x, w, bias, gamma, beta, moving_mean, moving_var)
