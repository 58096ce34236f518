"""The three float32 matmul precision levels of the pointwise products (csrc/gemm.hip: gemm_split_mfma<NP>, include/sph3d.h:
sph3d_pointwise_gemm_pieces), restated: how an fp32 operand is cut into bf16 pieces, which piece products are kept, and the
per-element error bounds that follow.  torch on whatever device the operands live on (numpy arrays are taken and returned as
such); tests/test_gemm_precision.py holds this file to hand-computed patterns, tests/test_gpu_gemm_precision.py the kernels to it.

rn(x): fp32 -> bf16 by round-to-nearest-even, widened back to fp32; on the bit pattern u of a finite x,
    ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16.
tr(x): the top 16 bits of x (truncation).

  highest (3 pieces): h = tr(x), m = tr(x - h), l = x - h - m: x = h + m + l exactly; kept products
                      h h' + (h m' + m h') + (m m' + h l' + l h').
  high    (2 pieces): h = rn(x), m = rn(x - h) (the subtraction is exact in fp32); kept  h h' + h m' + m h'.
  medium  (1 piece) : h = rn(x); kept  h h'.

Bounds, per output element, with mag = sum_k |x_k| |w_k| (piece products are exact in the fp32 accumulator: 8 x 8 significant bits;
the accumulation itself is allowed for separately by the tests):

  high.   bf16 has 8 significant bits, so |x - h| <= 2^-8 |x|; m = rn(x - h) gives |m| <= (1 + 2^-8) 2^-8 |x| and, with
          x = h + m + e, |e| <= 2^-8 |x - h| <= 2^-16 |x|.  Then  x y = (h + m)(h' + m') + e y + (x - e) e'  and the kept terms are
          (h + m)(h' + m') - m m', so what is dropped is  m m' + e y + (x - e) e':
              |dropped| <= 2^-16 |x y| ((1 + 2^-8)^2 + 1 + (1 + 2^-16)) = 2^-16 |x y| (3 + 2^-7 + 2^-15)  <=  3 2^-16 (1 + 2^-7) |x y|.
          C_HIGH = 3 * 2^-16 * (1 + 2^-7).
  medium. h = x (1 + d), |d| <= 2^-8:  h h' = x y (1 + d)(1 + d'),  |error| <= (2^-7 + 2^-16) |x y|.
          C_MEDIUM = 2^-7 + 2^-16.

Both hold away from overflow (rn rounds the largest finite fp32 values to infinity) and underflow."""
import numpy as np
import torch

LEVELS = ("highest", "high", "medium")
PIECES = {"highest": 3, "high": 2, "medium": 1}
C_HIGH = 3.0 * 2.0 ** -16 * (1.0 + 2.0 ** -7)
C_MEDIUM = 2.0 ** -7 + 2.0 ** -16
C_LEVEL = {"high": C_HIGH, "medium": C_MEDIUM}


def _bits(x):
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff


def _from_bits(u):
    u = u & 0xffffffff
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


def rn(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, by the integer formula; finite x"""
    u = _bits(x)
    return _from_bits(((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16)


def tr(x):
    """the top 16 bits of x"""
    return _from_bits(_bits(x) & 0xffff0000)


def pieces(x, level):
    """-> the tuple of fp32 arrays (each exactly a bf16 number) that `level` cuts x into, leading piece first"""
    if isinstance(x, np.ndarray):
        return tuple(p.numpy() for p in pieces(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), level))
    if level not in PIECES:
        raise ValueError("unknown level %r" % (level,))
    x = x.float()
    if level == "highest":
        h = tr(x)
        r = x - h
        m = tr(r)
        return h, m, r - m
    h = rn(x)
    if level == "medium":
        return (h,)
    return h, rn(x - h)


# (A piece, B piece) of the kept products, in the kernel's order: small terms first
KEPT = {"highest": ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)), "high": ((1, 0), (0, 1), (0, 0)), "medium": ((0, 0),)}


def statement(pa, pb, level, product=lambda a, b: a @ b):
    """the float64 value of the kept products of the piece tuples pa (of A[M,K]) and pb (of B[K,N])"""
    da, db = [p.double() for p in pa], [p.double() for p in pb]
    out = None
    for i, j in KEPT[level]:
        t = product(da[i], db[j])
        out = t if out is None else out + t
    return out
