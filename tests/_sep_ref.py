"""The one-kernel separable layer (csrc/sepring.hip, csrc/sepconv.hip) stated in float64 (plain numpy: no torch, no oracle), and
the per-element bounds its three kernels are held to.

With d, magd = tests/_conv_ref.conv_ref(x, w_dw, idx, cnt, bins) — the depthwise convolution [B, M, C r] and the same sum over
absolute values — pointwise weights W [C r, Cout] and an optional bias:
  y   = d @ W + bias                      MAG = magd @ |W| + |bias|
  inference tail:   out = elu?(y) scale + shift         (each of ELU, scale, shift optional)
  training outputs: d, y, and per column  sum_rows elu(y), sum_rows elu(y)^2   (the kernel writes partial rows; the host adds them
                    in float64)

The bounds are derived, not measured, with one exception (E, below): u = 2^-24, every fp32 rounding is at most u times a partial
sum, every partial sum at most the magnitude sum.  Second-order terms are left to the slack, as in tests/_conv_ref.py.

depthwise tensor (training)   (cnt + 4) u magd        the gather is dwconv_fwd_multi's: tests/_conv_ref.py, "forward"
pre-activation y              (cnt + C r + 7) u MAG
  cnt + 4   the depthwise tensor's own error, carried through |W|
  C r       the product's accumulation chain.  This rests on the project's statement that the matrix cores do fp32 arithmetic here:
            "fp32 MFMA is exact fp32 FMA arithmetic; results differ from the separate kernels by summation order only"
            (sepconv.hip, header) and README, sph3d_pointwise_gemm_mode(0): "v_mfma_f32_16x16x4_f32 (exact fp32 FMA arithmetic)".
            Padded k columns add exact zeros.  The general kernel's one chain over all slices and the four chains of KT steps of
            the ring and the small kernel are both at most C r roundings per output.
  2         `(d0 + d1) + (d2 + d3)`;  1: `d[r4] + bv`
after ELU                     the bound on y (ELU is 1-Lipschitz) + E u
  E is MEASURED: tools/micro/elu_err.hip evaluates `y > 0.f ? y : __expf(y) - 1.f` for every fp32 y in [-104, 0] against float64
  expm1 (below -104 the expression is exactly -1).  See E_ELU.
after fmaf(z, scale, shift)   |scale| err_z + u (|scale z| + |shift|)
statistics partials, added over the partial rows in float64 on the host
  sum z     sum_rows err_z + n u sum |z|               n = 4 ceil(nrb_max / G) + 2: the longest chain of one lane (`sz += z`, four
  sum z^2   sum_rows 2 |z| err_z + (n + 1) u sum z^2   rows of every row block of its wave group) and the two `__shfl_xor` adds;
                                                       + 1: the rounding of fmaf(z, z, sq)'s own product is inside its one rounding,
                                                       the + 1 pays for z^2 of a z that is itself off (second order) with room
tests/_errors.assert_per_element at its defaults (1e-5 of the magnitude sum, 256 ULP where |ref| >= mag / 4, exact zeros where
nothing contributes) is applied to the depthwise tensor and to pre-activation outputs (training y, tails `none` and `bias`)."""
import numpy as np

from _conv_ref import U, assert_conv, conv_ref, make_bins, make_graph, make_values
from _errors import assert_per_element

# tools/micro/elu_err.hip on an MI355X (gfx950, ROCm 7.2.0, -O3 -ffp-contract=off), all 1 120 927 746 values of y in [-104, 0]:
#   max |elu_fp32(y) - expm1(y)| / 2^-24 = ELU_MEASURED at y = ELU_MEASURED_AT
# E = that maximum rounded up to an integer, + 1 for the expression being compiled inside a larger kernel.
ELU_MEASURED, ELU_MEASURED_AT = 1.232679, -0.779894412          # bits 0xbf47a729; no result NaN or outside [-1, 0]
E_ELU = 3                                                        # ceil(1.232679) + 1


def make_inputs(B, N, M, F, C, r, K, Cout):
    """graph (make_graph: rows of count 0, 1, 2, K - 1 and K in every cloud), synthetic bin ids, values that differ per cloud, and the
    statement "ref" of them; seeded by the shape"""
    rng = np.random.RandomState(B + 3 * M + 5 * F + 7 * C + 11 * r + 13 * K + 17 * Cout)
    idx, cnt = make_graph(rng, B, N, M, K)
    d = dict(idx=idx, cnt=cnt, bins=make_bins(rng, idx, cnt, F), x=make_values(rng, (B, N, C)), w_dw=make_values(rng, (F, C, r)),
             W=(make_values(rng, (C * r, Cout)) / np.float32(np.sqrt(C * r))).astype(np.float32),
             bias=rng.randn(Cout).astype(np.float32), scale=(rng.randn(Cout) * 1.5).astype(np.float32),
             shift=rng.randn(Cout).astype(np.float32))
    d["ref"] = SepRef(d["x"], d["w_dw"], d["W"], idx, cnt, d["bins"])
    return d


def elu64(y):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(y > 0, y, np.expm1(np.minimum(y, 0)))


class SepRef:
    """d, magd [B, M, C r]; y0 = d @ W, MAG0 = magd @ |W| [B, M, Cout] (the bias is added per tail: one reference, shared)"""

    def __init__(self, x, w_dw, W, idx, cnt, bins):
        self.d, self.magd, _ = conv_ref(x, w_dw, idx, cnt, bins)
        self.cnt = np.asarray(cnt, np.int64)
        self.B, self.M, self.CR = self.d.shape
        W64 = np.asarray(W).astype(np.float64)
        self.Cout = W64.shape[1]
        with np.errstate(invalid="ignore", over="ignore"):
            self.y0 = (self.d.reshape(-1, self.CR) @ W64).reshape(self.B, self.M, self.Cout)
            self.MAG0 = (self.magd.reshape(-1, self.CR) @ np.abs(W64)).reshape(self.B, self.M, self.Cout)
        self.y_terms = self.cnt[:, :, None] + self.CR + 7

    def pre(self, bias=None):
        """-> (y, MAG, err_y)"""
        if bias is None:
            y, MAG = self.y0, self.MAG0
        else:
            b64 = np.asarray(bias).astype(np.float64)
            y, MAG = self.y0 + b64, self.MAG0 + np.abs(b64)
        return y, MAG, self.y_terms * U * MAG

    def tail(self, bias=None, act=False, scale=None, shift=None):
        """the inference output -> (ref, bound)"""
        y, _, err = self.pre(bias)
        z = y
        if act:
            z, err = elu64(y), err + E_ELU * U
        if scale is None and shift is None:
            return z, err
        sc = 1.0 if scale is None else np.asarray(scale).astype(np.float64)
        sh = 0.0 if shift is None else np.asarray(shift).astype(np.float64)
        return z * sc + sh, np.abs(sc) * err + U * (np.abs(sc * z) + np.abs(sh))

    def stats(self, bias, nrb_max, G, rows=None):
        """-> (sums [2, Cout], bounds [2, Cout])"""
        y, _, err = self.pre(bias)
        z, err = elu64(y), err + E_ELU * U
        if rows is not None:
            z, err = z[rows], err[rows]
        z, err = z.reshape(-1, self.Cout), err.reshape(-1, self.Cout)
        n = 4 * ((nrb_max + G - 1) // G) + 2
        s = np.stack([z.sum(0), (z * z).sum(0)])
        b = np.stack([err.sum(0) + n * U * np.abs(z).sum(0), (2 * np.abs(z) * err).sum(0) + (n + 1) * U * (z * z).sum(0)])
        return s, b


def assert_bound(got, ref, bound, what):
    """|got - ref| <= bound per element, no NaN left (an unwritten element of a NaN-filled output, or a non-finite product).
    Prints and returns the largest used fraction of the bound."""
    got = np.asarray(got)
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, got.shape, ref.shape)
    nans = int(np.isnan(got).sum())
    assert nans == 0, "%s: %d elements are NaN (unwritten, a stale ring row, or a non-finite product)" % (what, nans)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    live = bound > 0
    frac = np.where(live, err / np.where(live, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    used = float(frac.max()) if frac.size else 0.0
    print("%s: max |err| / bound = %.3f" % (what, used))
    if used > 1.0:
        worst = np.unravel_index(int(np.argmax(frac)), err.shape)
        raise AssertionError("%s: element %s is off by %.3e, %.2f of its derived bound %.3e (reference %.6e)"
                             % (what, worst, err[worst], used, bound[worst], ref[worst]))
    return used


TAILS = {"none": (False, False, False), "bias": (True, False, False), "bias+elu+bn": (True, True, True)}     # bias, ELU, affine


def check_infer(got, ref, tail, bias, scale, shift, what, rows=None):
    """one inference output [B, M, Cout] against the statement; rows: bool [B, M], the rows that are compared (default: all)"""
    with_bias, act, bn = TAILS[tail]
    want, bound = ref.tail(bias if with_bias else None, act, scale if bn else None, shift if bn else None)
    got = np.asarray(got)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    sel = slice(None) if rows is None else rows
    if not act and not bn:
        y, MAG, _ = ref.pre(bias if with_bias else None)
        assert int(np.isnan(got[sel]).sum()) == 0, "%s: NaN left in the output" % what
        assert_per_element(got[sel], y[sel], MAG[sel], what)
    return assert_bound(got[sel], want[sel], bound[sel], what + " tail " + tail)


def check_train(dw, y, partial, ref, bias, form, what, rows=None):
    """the training kernel's three outputs: depthwise tensor [B, M, C r], y [B, M, Cout], partial [nblk, 2, Cout]"""
    dw, y, partial = np.asarray(dw), np.asarray(y), np.asarray(partial)
    sel = slice(None) if rows is None else rows
    want, MAG, err = ref.pre(bias)
    assert dw.shape == ref.d.shape and y.shape == want.shape, "%s: shapes %s %s" % (what, dw.shape, y.shape)
    used = [assert_conv(dw[sel], ref.d[sel], ref.magd[sel], (ref.cnt[:, :, None] + 4)[sel], what + " depthwise")]
    assert int(np.isnan(y[sel]).sum()) == 0, "%s: NaN left in y" % what
    assert_per_element(y[sel], want[sel], MAG[sel], what + " y")
    used.append(assert_bound(y[sel], want[sel], err[sel], what + " y"))
    if rows is None:
        assert partial.shape[1:] == (2, ref.Cout), "%s: partial %s" % (what, partial.shape)
        nans = int(np.isnan(partial).sum())
        assert nans == 0, "%s: %d partial statistics are NaN (a partial row that no workgroup wrote)" % (what, nans)
        s, b = ref.stats(bias, form["nrb_max"], form["G"])
        used.append(assert_bound(partial.astype(np.float64).sum(0), s, b, what + " statistics"))
    return max(used)
