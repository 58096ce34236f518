"""Pointwise 1x1 feature GEMM — the ``tf.matmul`` inside separable_conv3d / pointwise_conv3d /
fully_connected (utils/sph3gcn_util.py:146-150, 204-206, 260; cuBLAS SGEMM in the reference).

``matmul(x, w)`` computes x[R,Cin] @ w[Cin,Cout] in exact fp32 with libsph3d's hand-written fp32-MFMA kernels
(sph3d_pointwise_gemm*): custom op ``sph3d::pointwise_gemm`` with its two backward products, wired once for the dispatcher and
the eager path (_op.differentiable).  (The library yardstick,
torch.matmul on rocBLAS / hipBLASLt, lives in tools/exp_gemm.py, not here.)
"""
import contextlib

import torch

from . import _lib, _op

# ---- float32 matmul precision of the products on the bf16 matrix pipe (include/sph3d.h: sph3d_pointwise_gemm_pieces) ----
# The names and meanings of torch.set_float32_matmul_precision; torch's own global is NOT read: the default path cannot change
# behind a user who set torch's flag for other reasons.
_PIECES = {"highest": 3, "high": 2, "medium": 1}
_LEVELS = {v: k for k, v in _PIECES.items()}


def get_float32_matmul_precision():
    return _LEVELS[_lib.lib().sph3d_pointwise_gemm_pieces(0)]


def set_float32_matmul_precision(level):
    """process-wide (not to be flipped while another thread issues products): "highest" — every fp32 operand as three bf16 pieces,
    fp32-sized error, the default; "high" — two round-to-nearest pieces, error <= 3 * 2^-16 * (1 + 2^-7) of an element's summed term
    magnitudes; "medium" — one, error <= 2^-7 + 2^-16 of them.  A permission: products that run on the fp32 pipe stay there, and
    the products inside the one-kernel separable layers, the few-output logits layers and their gradients keep "highest".
    -> the previous level"""
    if level not in _PIECES:
        raise ValueError("float32 matmul precision should be 'highest', 'high' or 'medium', got %r" % (level,))
    return _LEVELS[_lib.lib().sph3d_pointwise_gemm_pieces(_PIECES[level])]


@contextlib.contextmanager
def float32_matmul_precision(level):
    prev = set_float32_matmul_precision(level)
    try:
        yield
    finally:
        set_float32_matmul_precision(prev)


def _pointwise_gemm_impl(x: torch.Tensor, w: torch.Tensor, trans_w: bool) -> torch.Tensor:
    """y[R,Cout] = x[R,Cin] @ w[Cin,Cout]   (trans_w: w is stored [Cout,Cin])"""
    _lib.require_device(x, w)
    x, w = _lib.f32(x), _lib.f32(w)
    R, Cin = x.shape
    Cout = w.shape[0] if trans_w else w.shape[1]
    y = torch.empty((R, Cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().sph3d_pointwise_gemm(R, Cin, Cout, _lib.ptr(x), _lib.ptr(w), None, 0, int(trans_w),
                                               _lib.ptr(y), _lib.stream_ptr()))
    return y


_pointwise_gemm = torch.library.custom_op("sph3d::pointwise_gemm", mutates_args=())(_pointwise_gemm_impl)


@_pointwise_gemm.register_fake
def _(x, w, trans_w):
    return x.new_empty((x.shape[0], w.shape[0] if trans_w else w.shape[1]))


def _pointwise_gemm_tn_impl(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dw[Cin,Cout] = x[R,Cin]^T @ dy[R,Cout]"""
    _lib.require_device(x, dy)
    x, dy = _lib.f32(x), _lib.f32(dy)
    dw = torch.empty((x.shape[1], dy.shape[1]), dtype=torch.float32, device=x.device)
    _pointwise_gemm_tn_into(x, dy, dw)
    return dw


_pointwise_gemm_tn = torch.library.custom_op("sph3d::pointwise_gemm_tn", mutates_args=())(_pointwise_gemm_tn_impl)


@_pointwise_gemm_tn.register_fake
def _(x, dy):
    return x.new_empty((x.shape[1], dy.shape[1]))


def _gemm_setup(ctx, inputs, output):
    x, w, trans_w = inputs
    ctx.save_for_backward(x, w)
    ctx.trans_w = trans_w


def _gemm_vjp(grad, ctx, dy):
    gemm, gemm_tn = grad
    x, w = ctx.saved_tensors
    if ctx.trans_w:
        raise RuntimeError("gradient of the transposed-weight form is not needed by the path")
    dx = gemm(dy, w, True) if ctx.needs_input_grad[0] else None
    dw = gemm_tn(x, dy) if ctx.needs_input_grad[1] else None
    return dx, dw, None


_pointwise_gemm_apply = _op.differentiable(_pointwise_gemm, _pointwise_gemm_impl, _gemm_setup, _gemm_vjp,
                                           (_pointwise_gemm, _pointwise_gemm_tn), (_pointwise_gemm_impl, _pointwise_gemm_tn_impl))


def matmul(x, w):
    return _pointwise_gemm_apply(x, w, False)


# ---- GEMM with the bias / ELU epilogue of the library (layers with biases and no batch norm) --------------------------
def _gemm_bias_act_impl(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, act: int) -> torch.Tensor:
    """elu?(x[R,Cin] @ w[Cin,Cout] + bias[Cout]); act = 0 (none) | 1 (ELU): bias and activation run in the GEMM's epilogue"""
    _lib.require_device(x, w, bias)
    x, w, bias = _lib.f32(x), _lib.f32(w), _lib.f32(bias)
    R, Cin = x.shape
    Cout = w.shape[1]
    y = torch.empty((R, Cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().sph3d_pointwise_gemm(R, Cin, Cout, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), int(act), 0,
                                               _lib.ptr(y), _lib.stream_ptr()))
    return y


_gemm_bias_act = torch.library.custom_op("sph3d::pointwise_gemm_bias_act", mutates_args=())(_gemm_bias_act_impl)


@_gemm_bias_act.register_fake
def _(x, w, bias, act):
    return x.new_empty((x.shape[0], w.shape[1]))


class _GemmBiasActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, act):
        out = _gemm_bias_act_impl(x, w, bias, act)
        ctx.save_for_backward(x, w, out)
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, out = ctx.saved_tensors
        # ELU'(z) from the output: 1 for z > 0, elu(z) + 1 = exp(z) otherwise
        g = dout * torch.where(out > 0, torch.ones_like(out), out + 1.0) if ctx.act == 1 else dout
        g = g.contiguous()
        dx = _pointwise_gemm_impl(g, w, True) if ctx.needs_input_grad[0] else None
        dw = _pointwise_gemm_tn_impl(x, g) if ctx.needs_input_grad[1] else None
        db = g.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None


def matmul_bias_act(x, w, bias, elu=False):
    """elu?(x @ w + bias) with the bias and the activation in the GEMM's epilogue"""
    return _GemmBiasActFn.apply(x, w, bias, 1 if elu else 0)


# ---- the 1x1 layer with few outputs over two operand halves: the logits layer without its concatenation (csrc/skinny.hip) ----
def skinny_supported(R, K1, K2, N):
    return bool(_lib.lib().sph3d_pointwise_gemm_skinny_supported(int(R), int(K1), int(K2), int(N)))


def _skinny_impl(a1: torch.Tensor, a2: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """a1[R,K1] @ w[:K1] + a2[R,K2] @ w[K1:] + bias -> [R,N]   (a2 / bias with zero elements: absent)"""
    _lib.require_device(a1, w)
    a1, w = _lib.f32(a1), _lib.f32(w)
    a2 = None if a2 is None or a2.numel() == 0 else _lib.f32(a2)
    bias = None if bias is None or bias.numel() == 0 else _lib.f32(bias)
    R, K1 = a1.shape
    K2 = 0 if a2 is None else a2.shape[1]
    N = w.shape[1]
    if w.shape[0] != K1 + K2:
        raise ValueError("weights should be [K1 + K2, N]")
    y = torch.empty((R, N), dtype=torch.float32, device=a1.device)
    _lib.check(_lib.lib().sph3d_pointwise_gemm_skinny(R, K1, K2, N, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(w), _lib.ptr(bias),
                                                      _lib.ptr(y), _lib.stream_ptr()))
    return y


def _skinny_tn_impl(a1: torch.Tensor, a2: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """[a1 | a2]^T @ dy -> [K1 + K2, N]"""
    _lib.require_device(a1, dy)
    a1, dy = _lib.f32(a1), _lib.f32(dy)
    a2 = None if a2 is None or a2.numel() == 0 else _lib.f32(a2)
    R, K1 = a1.shape
    K2 = 0 if a2 is None else a2.shape[1]
    N = dy.shape[1]
    l = _lib.lib()
    wsb = l.sph3d_pointwise_gemm_skinny_tn_workspace(R, K1, K2, N)
    ws = _lib.scratch(wsb, a1.device)
    dw = torch.empty((K1 + K2, N), dtype=torch.float32, device=a1.device)
    _lib.check(l.sph3d_pointwise_gemm_skinny_tn(R, K1, K2, N, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(ws), wsb,
                                                _lib.stream_ptr()))
    return dw


_skinny = torch.library.custom_op("sph3d::pointwise_gemm_skinny", mutates_args=())(_skinny_impl)


@_skinny.register_fake
def _(a1, a2, w, bias):
    return a1.new_empty((a1.shape[0], w.shape[1]))


_skinny_tn = torch.library.custom_op("sph3d::pointwise_gemm_skinny_tn", mutates_args=())(_skinny_tn_impl)


@_skinny_tn.register_fake
def _(a1, a2, dy):
    return a1.new_empty((a1.shape[1] + a2.shape[1], dy.shape[1]))


class _SkinnyLinear2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a1, a2, w, bias):
        ctx.save_for_backward(a1, a2, w)
        ctx.has_bias = bias is not None
        return _skinny_impl(a1, a2, w, bias)

    @staticmethod
    def backward(ctx, dy):
        a1, a2, w = ctx.saved_tensors
        dy = dy.contiguous()
        K1 = a1.shape[1]
        # the input gradients: the general product with the matching rows of w, one call per half (they are written where autograd
        # wants them: no slices of a concatenated gradient to copy)
        da1 = _pointwise_gemm_impl(dy, w[:K1], True) if ctx.needs_input_grad[0] else None
        da2 = _pointwise_gemm_impl(dy, w[K1:], True) if (a2 is not None and ctx.needs_input_grad[1]) else None
        dw = _skinny_tn_impl(a1, a2, dy) if ctx.needs_input_grad[2] else None
        db = dy.sum(0) if (ctx.has_bias and ctx.needs_input_grad[3]) else None
        return da1, da2, dw, db


def linear_concat2(a1, a2, w, bias=None):
    """[a1 | a2] @ w + bias for few output columns (N <= 16), the concatenation never materialised; a2 may be None"""
    return _SkinnyLinear2Fn.apply(a1, a2, w, bias)


# ---- the category-conditioned logits layer: two operand halves and one row of w per cloud (csrc/condlogits.hip) ----------------
def cond_supported(B, P, K1, K2, N, T):
    return bool(_lib.lib().sph3d_pointwise_gemm_cond_supported(int(B), int(P), int(K1), int(K2), int(N), int(T)))


def _cond_dims(a1, a2, w, rows_per_cloud):
    R, K1 = a1.shape
    K2 = 0 if a2 is None else a2.shape[1]
    P = int(rows_per_cloud)
    if P <= 0 or R % P != 0 or R == 0:
        raise ValueError("rows_per_cloud should divide the %d rows" % R)
    T = w.shape[0] - K1 - K2
    if T < 1:
        raise ValueError("weights should be [K1 + K2 + T, N] with T >= 1 category rows")
    return R // P, P, K1, K2, w.shape[1], T


def _cond_impl(a1: torch.Tensor, a2: torch.Tensor, cat: torch.Tensor, w: torch.Tensor, bias: torch.Tensor,
               rows_per_cloud: int) -> torch.Tensor:
    """a1[R,K1] @ w[:K1] + a2[R,K2] @ w[K1:K1+K2] + w[K1+K2+cat[row // rows_per_cloud]] + bias -> [R,N]
    (a2 / bias with zero elements: absent; a category outside the T rows adds nothing)"""
    _lib.require_device(a1, w, cat)
    a1, w, cat = _lib.f32(a1), _lib.f32(w), _lib.i32(cat)
    a2 = None if a2 is None or a2.numel() == 0 else _lib.f32(a2)
    bias = None if bias is None or bias.numel() == 0 else _lib.f32(bias)
    B, P, K1, K2, N, T = _cond_dims(a1, a2, w, rows_per_cloud)
    if cat.numel() != B:
        raise ValueError("one category per cloud expected (%d clouds, %d categories)" % (B, cat.numel()))
    y = torch.empty((B * P, N), dtype=torch.float32, device=a1.device)
    _lib.check(_lib.lib().sph3d_pointwise_gemm_cond(B, P, K1, K2, N, T, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(w), _lib.ptr(bias),
                                                    _lib.ptr(cat), _lib.ptr(y), _lib.stream_ptr()))
    return y


def _cond_grad_into(dy, cat, rows_per_cloud, dt, dbias):
    """dt[T,N] (a contiguous row range of the weight gradient) = per-category column sums of dy; dbias[N] (or None) = all rows"""
    B, (T, N) = cat.numel(), dt.shape
    l = _lib.lib()
    wsb = l.sph3d_pointwise_gemm_cond_grad_workspace(B, int(rows_per_cloud), N, T)
    ws = _lib.scratch(wsb, dy.device)
    _lib.check(l.sph3d_pointwise_gemm_cond_grad(B, int(rows_per_cloud), N, T, _lib.ptr(dy), _lib.ptr(cat), _lib.ptr(dt),
                                                _lib.ptr(dbias), _lib.ptr(ws), wsb, _lib.stream_ptr()))


def _cond_grad_impl(dy: torch.Tensor, cat: torch.Tensor, num_categories: int, rows_per_cloud: int, with_bias: bool) -> torch.Tensor:
    """-> [T + 1, N]: rows 0..T-1 the gradient of the category rows, row T the bias gradient (zeros without with_bias)"""
    _lib.require_device(dy, cat)
    dy, cat = _lib.f32(dy), _lib.i32(cat)
    if dy.shape[0] != cat.numel() * int(rows_per_cloud):
        raise ValueError("dy should have rows_per_cloud rows per category entry")
    out = torch.empty((num_categories + 1, dy.shape[1]), dtype=torch.float32, device=dy.device)
    if not with_bias:
        out[num_categories].zero_()
    _cond_grad_into(dy, cat, rows_per_cloud, out[:num_categories], out[num_categories] if with_bias else None)
    return out


def _pointwise_gemm_tn_into(x, dy, dw):
    """dw (a contiguous [Cin, Cout] row range) = x[R,Cin]^T @ dy[R,Cout]"""
    R, Cin = x.shape
    Cout = dy.shape[1]
    l = _lib.lib()
    wsb = l.sph3d_pointwise_gemm_tn_workspace(R, Cin, Cout)
    ws = _lib.scratch(wsb, x.device)
    _lib.check(l.sph3d_pointwise_gemm_tn(R, Cin, Cout, _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(ws), wsb,
                                         _lib.stream_ptr()))


_cond = torch.library.custom_op("sph3d::pointwise_gemm_cond", mutates_args=())(_cond_impl)


@_cond.register_fake
def _(a1, a2, cat, w, bias, rows_per_cloud):
    return a1.new_empty((a1.shape[0], w.shape[1]))


_cond_grad = torch.library.custom_op("sph3d::pointwise_gemm_cond_grad", mutates_args=())(_cond_grad_impl)


@_cond_grad.register_fake
def _(dy, cat, num_categories, rows_per_cloud, with_bias):
    return dy.new_empty((num_categories + 1, dy.shape[1]))


class _CondLinear2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a1, a2, cat, w, bias, rows_per_cloud):
        cat = _lib.i32(cat)
        ctx.save_for_backward(a1, a2, cat, w)
        ctx.has_bias = bias is not None
        ctx.rows_per_cloud = int(rows_per_cloud)
        return _cond_impl(a1, a2, cat, w, bias, rows_per_cloud)

    @staticmethod
    def backward(ctx, dy):
        a1, a2, cat, w = ctx.saved_tensors
        dy = _lib.f32(dy)
        K1 = a1.shape[1]
        K2 = 0 if a2 is None else a2.shape[1]
        # the input gradients: the general product with the matching rows of w, one call per half (_SkinnyLinear2Fn)
        da1 = _pointwise_gemm_impl(dy, w[:K1], True) if ctx.needs_input_grad[0] else None
        da2 = _pointwise_gemm_impl(dy, w[K1:K1 + K2], True) if (a2 is not None and ctx.needs_input_grad[1]) else None
        want_b = ctx.has_bias and ctx.needs_input_grad[4]
        dw = None
        db = torch.empty((w.shape[1],), dtype=torch.float32, device=dy.device) if want_b else None
        if ctx.needs_input_grad[3]:
            # ONE weight gradient, written in three contiguous row ranges: the two operand halves' products and the
            # per-category column sums of dy (which also give the bias gradient)
            dw = torch.empty_like(w, dtype=torch.float32, memory_format=torch.contiguous_format)
            _pointwise_gemm_tn_into(_lib.f32(a1), dy, dw[:K1])
            if a2 is not None:
                _pointwise_gemm_tn_into(_lib.f32(a2), dy, dw[K1:K1 + K2])
            _cond_grad_into(dy, cat, ctx.rows_per_cloud, dw[K1 + K2:], db)
        elif want_b:
            db = dy.sum(0)
        return da1, da2, None, dw, db, None


def linear_concat2_onehot(a1, a2, cat, w, bias, rows_per_cloud):
    """[a1 | a2 | onehot(cat[row // rows_per_cloud])] @ w + bias with neither concatenation nor the one-hot tile materialised;
    w is [K1 + K2 + T, N]; a2 (or a zero-width a2) and bias may be None.  Shapes: cond_supported(B, rows_per_cloud, K1, K2, N, T)"""
    if a2 is not None and a2.shape[-1] == 0:
        a2 = None
    return _CondLinear2Fn.apply(a1, a2, cat, w, bias, rows_per_cloud)
