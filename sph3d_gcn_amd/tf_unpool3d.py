"""Graph un-pooling (feature interpolation) — mirrors tf_ops/unpooling/tf_unpool3d.py:9-28.

Custom ops ``sph3d::mean_interpolate`` / ``sph3d::weighted_interpolate`` (+ ``_grad``).
As in the reference (:21-28) ``weight`` receives no gradient.  The wiring is stated once for the dispatcher and the eager path
(_op.differentiable).
"""
import torch

from . import _lib, _op, _tgraph


def _mean_interpolate_impl(input: torch.Tensor, nn_index: torch.Tensor, nn_count: torch.Tensor) -> torch.Tensor:
    _lib.require_device(input, nn_index, nn_count)
    _op.check_graph_ranks(input, nn_index, nn_count)
    input, nn_index, nn_count = _lib.f32(input), _lib.i32(nn_index), _lib.i32(nn_count)
    B, M, C = input.shape
    N, K = nn_index.shape[1], nn_index.shape[2]
    output = torch.empty((B, N, C), dtype=torch.float32, device=input.device)
    _lib.check(_lib.lib().sph3d_mean_interpolate(B, N, M, C, K, _lib.ptr(nn_index), _lib.ptr(nn_count),
                                                 _lib.ptr(input), _lib.ptr(output), _lib.stream_ptr()))
    return output


_mean_interpolate = torch.library.custom_op("sph3d::mean_interpolate", mutates_args=())(_mean_interpolate_impl)


@_mean_interpolate.register_fake
def _(input, nn_index, nn_count):
    return input.new_empty((input.shape[0], nn_index.shape[1], input.shape[2]))


def _mean_interpolate_grad_impl(input: torch.Tensor, grad_output: torch.Tensor, nn_index: torch.Tensor,
                           nn_count: torch.Tensor) -> torch.Tensor:
    _lib.require_device(input, grad_output, nn_index, nn_count)
    grad_output, nn_index, nn_count = _lib.f32(grad_output), _lib.i32(nn_index), _lib.i32(nn_count)
    B, M, C = input.shape
    N, K = nn_index.shape[1], nn_index.shape[2]
    grad_input = torch.empty((B, M, C), dtype=torch.float32, device=input.device)
    offsets, ent_key, ent_scale, _ = _tgraph.transpose(nn_index, nn_count, M)   # source points = the M coarse points
    _lib.check(_lib.lib().sph3d_scatter_grad_t(B, M, N, C, _lib.ptr(offsets), _lib.ptr(ent_key), _lib.ptr(ent_scale),
                                               _lib.ptr(grad_output), _lib.ptr(grad_input), _lib.stream_ptr()))
    return grad_input


_mean_interpolate_grad = torch.library.custom_op("sph3d::mean_interpolate_grad", mutates_args=())(_mean_interpolate_grad_impl)


@_mean_interpolate_grad.register_fake
def _(input, grad_output, nn_index, nn_count):
    return torch.empty_like(input)


def _mean_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _mean_vjp(grad, ctx, grad_output):
    input, nn_index, nn_count = ctx.saved_tensors
    return grad(input, grad_output, nn_index, nn_count), None, None


_mean_interpolate_apply = _op.differentiable(_mean_interpolate, _mean_interpolate_impl, _mean_setup, _mean_vjp,
                                             _mean_interpolate_grad, _mean_interpolate_grad_impl)


def _weighted_interpolate_impl(input: torch.Tensor, weight: torch.Tensor, nn_index: torch.Tensor,
                          nn_count: torch.Tensor) -> torch.Tensor:
    _lib.require_device(input, weight, nn_index, nn_count)
    _op.check_graph_ranks(input, nn_index, nn_count)
    input, weight = _lib.f32(input), _lib.f32(weight)
    nn_index, nn_count = _lib.i32(nn_index), _lib.i32(nn_count)
    B, M, C = input.shape
    N, K = nn_index.shape[1], nn_index.shape[2]
    output = torch.empty((B, N, C), dtype=torch.float32, device=input.device)
    _lib.check(_lib.lib().sph3d_weighted_interpolate(B, N, M, C, K, _lib.ptr(nn_index), _lib.ptr(nn_count),
                                                     _lib.ptr(input), _lib.ptr(weight), _lib.ptr(output),
                                                     _lib.stream_ptr()))
    return output


_weighted_interpolate = torch.library.custom_op("sph3d::weighted_interpolate", mutates_args=())(_weighted_interpolate_impl)


@_weighted_interpolate.register_fake
def _(input, weight, nn_index, nn_count):
    return input.new_empty((input.shape[0], nn_index.shape[1], input.shape[2]))


def _weighted_interpolate_grad_impl(input: torch.Tensor, grad_output: torch.Tensor, weight: torch.Tensor,
                               nn_index: torch.Tensor, nn_count: torch.Tensor) -> torch.Tensor:
    _lib.require_device(input, grad_output, weight, nn_index, nn_count)
    grad_output, weight = _lib.f32(grad_output), _lib.f32(weight)
    nn_index, nn_count = _lib.i32(nn_index), _lib.i32(nn_count)
    B, M, C = input.shape
    N, K = nn_index.shape[1], nn_index.shape[2]
    grad_input = torch.empty((B, M, C), dtype=torch.float32, device=input.device)
    offsets, ent_key, ent_scale, _ = _tgraph.transpose(nn_index, nn_count, M, weight=weight)
    _lib.check(_lib.lib().sph3d_scatter_grad_t(B, M, N, C, _lib.ptr(offsets), _lib.ptr(ent_key), _lib.ptr(ent_scale),
                                               _lib.ptr(grad_output), _lib.ptr(grad_input), _lib.stream_ptr()))
    return grad_input


_weighted_interpolate_grad = torch.library.custom_op("sph3d::weighted_interpolate_grad", mutates_args=())(_weighted_interpolate_grad_impl)


@_weighted_interpolate_grad.register_fake
def _(input, grad_output, weight, nn_index, nn_count):
    return torch.empty_like(input)


def _w_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _w_vjp(grad, ctx, grad_output):
    input, weight, nn_index, nn_count = ctx.saved_tensors
    return grad(input, grad_output, weight, nn_index, nn_count), None, None, None


_weighted_interpolate_apply = _op.differentiable(_weighted_interpolate, _weighted_interpolate_impl, _w_setup, _w_vjp,
                                                 _weighted_interpolate_grad, _weighted_interpolate_grad_impl)


def mean_interpolate(input, nn_index, nn_count):
    return _mean_interpolate_apply(input, nn_index, nn_count)


def mean_interpolate_grad(input, grad_output, nn_index, nn_count):
    return _mean_interpolate_grad_impl(input, grad_output, nn_index, nn_count)


def weighted_interpolate(input, weight, nn_index, nn_count):
    return _weighted_interpolate_apply(input, weight, nn_index, nn_count)


def weighted_interpolate_grad(input, grad_output, weight, nn_index, nn_count):
    return _weighted_interpolate_grad_impl(input, grad_output, weight, nn_index, nn_count)


# ---- un-pooling followed by a plain product with few outputs (the logits layer behind the last un-pooling) -------------------
# Interpolation is linear over rows and the product linear over channels: interp(x) @ W = interp(x @ W).  The product runs on the
# COARSE points and the interpolation moves rows of num_cls floats (include/sph3d.h: sph3d_interpolate_narrow); the interpolated
# [B, N, C] tensor is neither written nor read, forward or backward.
def linear_supported(num_out_channels):
    return bool(_lib.lib().sph3d_interpolate_narrow_supported(int(num_out_channels)))


def _narrow_impl(z, weight, base, nn_index, nn_count):
    """base + interp(z): z [B, M, C <= 16], base [B, N, C] | None, weight [B, N, K] | None (mean) -> [B, N, C]"""
    B, M, C = z.shape
    N, K = nn_index.shape[1], nn_index.shape[2]
    out = torch.empty((B, N, C), dtype=torch.float32, device=z.device)
    _lib.check(_lib.lib().sph3d_interpolate_narrow(B, N, M, C, K, _lib.ptr(nn_index), _lib.ptr(nn_count), _lib.ptr(z),
                                                   _lib.ptr(weight), _lib.ptr(base), _lib.ptr(out), _lib.stream_ptr()))
    return out


def _narrow_grad_impl(grad_output, weight, nn_index, nn_count, M):
    """gradient of _narrow_impl with respect to z: a gather over the transposed graph -> [B, M, C]"""
    B, N, C = grad_output.shape
    grad_z = torch.empty((B, M, C), dtype=torch.float32, device=grad_output.device)
    offsets, ent_key, ent_scale, _ = _tgraph.transpose(nn_index, nn_count, M, weight=weight)
    _lib.check(_lib.lib().sph3d_interpolate_narrow_grad_t(B, M, N, C, _lib.ptr(offsets), _lib.ptr(ent_key), _lib.ptr(ent_scale),
                                                          _lib.ptr(grad_output), _lib.ptr(grad_z), _lib.stream_ptr()))
    return grad_z


def _product(a, w, bias):
    """a[R, K] @ w[K, N] (+ bias): the streaming few-output kernel where it covers the shape, else the general product"""
    from . import tf_gemm
    if tf_gemm.skinny_supported(a.shape[0], a.shape[1], 0, w.shape[1]):
        return tf_gemm._skinny_impl(a, None, w, bias)
    if bias is not None:
        return tf_gemm._gemm_bias_act_impl(a, w, bias, 0)
    return tf_gemm._pointwise_gemm_impl(a, w, False)


def _product_tn_into(a, dy, dw):
    """dw[K, N] (rows of a larger contiguous gradient) = a[R, K]^T @ dy[R, N]"""
    from . import tf_gemm
    R, K = a.shape
    N = dy.shape[1]
    l = _lib.lib()
    if tf_gemm.skinny_supported(R, K, 0, N):
        wsb = l.sph3d_pointwise_gemm_skinny_tn_workspace(R, K, 0, N)
        ws = _lib.scratch(wsb, a.device)
        _lib.check(l.sph3d_pointwise_gemm_skinny_tn(R, K, 0, N, _lib.ptr(a), None, _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(ws), wsb,
                                                    _lib.stream_ptr()))
        return
    wsb = l.sph3d_pointwise_gemm_tn_workspace(R, K, N)
    ws = _lib.scratch(wsb, a.device)
    _lib.check(l.sph3d_pointwise_gemm_tn(R, K, N, _lib.ptr(a), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(ws), wsb, _lib.stream_ptr()))


class _InterpolateLinearFn(torch.autograd.Function):
    """[interp(input) | skip] @ w + bias  as  (skip @ w[C:] + bias) + interp(input @ w[:C])"""

    @staticmethod
    def forward(ctx, input, skip, w, bias, weight, nn_index, nn_count):
        from . import tf_gemm                      # noqa: F401  (the products below)
        _lib.require_device(input, w, nn_index, nn_count)
        _op.check_graph_ranks(input, nn_index, nn_count)
        input, w = _lib.f32(input), _lib.f32(w)
        nn_index, nn_count = _lib.i32(nn_index), _lib.i32(nn_count)
        skip = None if skip is None or skip.shape[-1] == 0 else _lib.f32(skip)
        weight = None if weight is None else _lib.f32(weight)
        bias = None if bias is None else _lib.f32(bias)
        B, M, C = input.shape
        N = nn_index.shape[1]
        Cs = 0 if skip is None else skip.shape[-1]
        O = w.shape[1]
        if w.shape[0] != C + Cs:
            raise ValueError("weights should be [C + C_skip, num_out]")
        z = _product(input.reshape(B * M, C), w[:C], None).reshape(B, M, O)
        if skip is not None:
            base = _product(skip.reshape(B * N, Cs), w[C:], bias)
        else:
            base = None if bias is None else bias.expand(B * N, O).contiguous()
        ctx.save_for_backward(input, skip, w, weight, nn_index, nn_count)
        ctx.has_bias = bias is not None
        return _narrow_impl(z, weight, base, nn_index, nn_count)

    @staticmethod
    def backward(ctx, dy):
        from . import tf_gemm
        input, skip, w, weight, nn_index, nn_count = ctx.saved_tensors
        dy = _lib.f32(dy)
        B, M, C = input.shape
        N, O = dy.shape[1], dy.shape[2]
        Cs = 0 if skip is None else skip.shape[-1]
        dy2 = dy.reshape(B * N, O)
        need_in, need_skip, need_w, need_b = (ctx.needs_input_grad[i] for i in range(4))
        dz2 = _narrow_grad_impl(dy, weight, nn_index, nn_count, M).reshape(B * M, O) if (need_in or need_w) else None
        d_in = tf_gemm._pointwise_gemm_impl(dz2, w[:C], True).reshape(B, M, C) if need_in else None
        d_skip = tf_gemm._pointwise_gemm_impl(dy2, w[C:], True).reshape(B, N, Cs) if (skip is not None and need_skip) else None
        dw = None
        if need_w:
            # the coarse half's weight gradient runs over the M coarse rows: the N interpolated rows carry the same information
            dw = torch.empty_like(w)
            _product_tn_into(input.reshape(B * M, C), dz2, dw[:C])
            if skip is not None:
                _product_tn_into(skip.reshape(B * N, Cs), dy2, dw[C:])
        db = dy2.sum(0) if (ctx.has_bias and need_b) else None
        return d_in, d_skip, dw, db, None, None, None


def interpolate_linear(input, skip, w, bias, nn_index, nn_count, weight=None):
    """cat(interpolate(input), skip) @ w + bias for few output columns (w.shape[1] <= 16); weight None: mean interpolation;
    skip / bias may be None.  As in the reference, `weight` receives no gradient."""
    return _InterpolateLinearFn.apply(input, skip, w, bias, weight, nn_index, nn_count)
