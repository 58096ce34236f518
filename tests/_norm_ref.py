"""The ELU + batch-norm tail (csrc/norm.hip), restated:
  * the launch arithmetic of norm.hip in plain Python, each line with the function and the variable it restates;
  * FORM_CASES / FORMS: the smallest shape that reaches each distinct launch form, with the predicate that names the form;
  * float64 numpy statements of every quantity the seven entry points leave behind;
  * a float32 numpy restatement of each kernel in the kernel's own operation order, which entitles the bounds to be used on the
    kernels (tests/test_norm_ref.py holds it to them on the CPU), and beside it the MUTATIONS every bound must catch;
  * the bounds, and the operands of the GPU test (tests/test_gpu_norm_forms.py).
numpy only: no torch, no library.

Bounds, u = 2^-24, derived from the expressions and never fitted to a kernel.

E, the absolute error of `__expf(y) - 1.f` for y <= 0 (0 for y > 0, where ELU is the identity):
    __expf(y) is v_exp_f32 of fl(y * fl(log2 e)).  The argument carries two roundings, so it is y log2(e) (1 + d), |d| <= 2u + u^2,
    and 2^argument = e^y e^(y d): an absolute error of at most e^y |y| (2u + u^2) <= (2 / e) u = 0.74 u.  v_exp_f32 is accurate to
    1 ulp of a result in (0, 1]: at most 2u (the ulp of 1.0; u below 1.0).  The subtraction is exact for e^y >= 1/2 (Sterbenz) and
    rounds a result in (-1, -1/2] otherwise: u/2.  Sum 3.24 u, taken as E = 4u.  Cross-check: tools/micro/elu_err.hip measured
    1.232679 u over every fp32 y in [-104, 0] (ELU_MEASURED, the record of tests/_sep_ref.py and DESIGN.md section 2).
    A subnormal y or e^y may be flushed to zero: FLOOR = 2^-126 is added to E for every element.
forward sums of one channel (n = chain + fold: the additions of the longest per-thread chain and of the fold that follows it;
the float64 accumulation of the nblk float32 partials adds nblk 2^-53 of the same magnitudes):
    |S1_k - S1| <= n u (sum|z| + sum E) + sum E
    |S2_k - S2| <= n u (sum z^2 + Q) + Q,   Q = sum (2|z| E + E^2)            (the squares enter by ONE rounding each: fmaf)
backward sums, at the float32 mean / rstd the kernel was given, zhat = (z - mean) rstd:
    the kernel's zhat is fl(fl(z_k - mean) rstd): |zhat_k - zhat| <= Z = E rstd (1 + 2u) + 2u |zhat|   (2u: (1 + u)^2 - 1)
    |Sd_k - Sd|   <= n u sum|dout|
    |Sdz_k - Sdz| <= n u (sum|dout zhat| + W) + W,   W = sum |dout| Z
    dgamma / dbeta are one float32 rounding of the float64 sums: + u |value|.
statistics from sums: the float64 expressions of norm_fwd_stats evaluated here, one float32 rounding: u |value| (+ 2^-149).
apply, forward, per element, against the float64 formula AT THE KERNEL'S OWN float32 mean and rstd:
    o = fma(fl(fl(z_k - mean) rstd), gamma, beta):   (E + 3u |z - mean|) rstd |gamma| + u |out|
apply, backward, per element, at the kernel's float32 statistics and float32 coef (SPH3D_BN_BWD), T = |dout| + |c0| + |zhat c1|:
    inner = fl(fl(dout - c0) - fl(zhat_k c1)): Z |c1| + 3u T;   dz = fl(fl(gamma rstd) inner): |gamma| rstd (Z |c1| + 5u T)
    y <= 0: elu' = fl(z_k + 1) is off by E + u/2, and the product rounds once more:
    |dy_k - dy| <= |gamma| rstd ((Z |c1| + 5u T) + [y <= 0] T (E + u/2)) + u |dy|
    (every bound above is multiplied by 1 + 8u for the second-order terms)
    For y below log(2^-25) = -17.33 the kernel's e^y is below u/2, fl(e^y - 1) is -1 and fl(-1 + 1) is 0: the code GUARANTEES
    dy == 0 there (the statement's dy is not 0 but below T |gamma| rstd 2^-25, inside the bound).
end to end, against the statistics of the float64 statement (the one-pass bound):
    dmean = dS1 / R + u |m|;   dvar = dS2 / R + 2|m| dS1 / R + (dS1 / R)^2;
    drstd = 0.5 (var + eps - dvar)^-1.5 dvar + u rstd      (first order 0.5 rstd^3 dvar; grows with kappa = (m^2 + var) / (var + eps))
    out: the apply bound + |gamma| (|z - m| drstd + (rstd + drstd) dmean)."""
import numpy as np

U = 2.0 ** -24                       # float32 unit roundoff
E_UNITS = 4                          # E = 4u (derivation above)
E_ELU = E_UNITS * U
ELU_MEASURED = 1.232679              # tools/micro/elu_err.hip on an MI355X, in u (tests/_sep_ref.py: ELU_MEASURED)
FLOOR = 2.0 ** -126                  # smallest normal float32: a subnormal operand or result may be flushed
TINY = 2.0 ** -149
SECOND = 1.0 + 8 * U                 # second-order terms of every bound
EPS = np.float32(1e-3)               # tf_norm.EPSILON as the C ABI receives it (a float argument)
MOM = np.float32(0.01)               # 1 - tf_norm.MOMENTUM as the C ABI receives it


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- csrc/norm.hip: launch arithmetic --------------------------------------------------------------------------------------------
K_NORM_MAX_BLOCKS = 1024             # kNormMaxBlocks
K_FIN_LANES = 32                     # kFinLanes
K_FIN_UN = 8                         # UN of sum_partials_32x8
K_REDUCE_UN = 4                      # UN of norm_reduce_kernel
K_APPLY_MAX_BLOCKS = 4096            # launch_apply: the cap of the grid
MAX_ROWS = 2 ** 31 - 1024            # kNormMaxRows: R + 1023 is the largest int norm_reduce_kernel forms


def supported(R, C):
    """norm_enter: the dimension check of every entry point"""
    return 0 < R <= MAX_ROWS and C > 0 and C % 4 == 0 and C <= 1024


def norm_blocks(R):
    """norm_blocks"""
    return max(1, min(K_NORM_MAX_BLOCKS, _cdiv(R, 32)))


def workspace_bytes(R, C):
    """sph3d_elu_bn_workspace (NormWorkspace): the partials [nblk][2][C] and coef [2][C]"""
    return 4 * (norm_blocks(R) * 2 * C + 2 * C)


def finalize_form(nblk, C):
    """sum_partials_32x8: the loop over k0, and the finalize grids (launch_stats)"""
    return dict(fin_trips=_cdiv(nblk, K_FIN_LANES * K_FIN_UN),                  # k0 = py; k0 < nblk; k0 += 256 (py = 0)
                fin_idle_py=max(0, K_FIN_LANES - nblk),                         # lanes with py >= nblk never enter
                fin_ragged=nblk % (K_FIN_LANES * K_FIN_UN) != 0,                # kc: some k >= nblk in the last trip: clamped
                fin_idle_lanes=_cdiv(C, 32) * 32 - C)                           # c >= C in the last workgroup of a finalize kernel


def reduce_form(R, C):
    """norm_reduce_kernel: its row ranges, its row loop and its fold"""
    nblk = norm_blocks(R)                                                       # norm_enter: ws->nblk
    cg = C >> 2                                                                 # cg
    rpi = max(1, 256 // cg)                                                     # rows_per_iter
    rpb = _cdiv(R, nblk)                                                        # rows_per_block
    used = _cdiv(R, rpb)                                                        # r0: blocks with r0 < R
    f = dict(nblk=nblk, cg=cg, rows_per_iter=rpi, idle_threads=256 - cg * rpi,  # act: ty >= rows_per_iter
             rows_per_block=rpb, used=used, empty=nblk - used,
             last_rows=R - (used - 1) * rpb,                                    # r1 = min(r0 + rows_per_block, R)
             chain=_cdiv(rpb, rpi),                                             # rb = r0 + ty; rb < r1; rows_per_iter apart
             fold=min(rpi, rpb))                                                # the fold: the ty that hold a row
    f.update(finalize_form(nblk, C))
    return f


def apply_form(R, C):
    """the apply launches (launch_apply) and norm_apply_kernel's loop"""
    total4 = R * C // 4                                                         # launch_apply: total4
    blocks = min(K_APPLY_MAX_BLOCKS, _cdiv(total4, 256))                        # launch_apply: blocks
    stride = blocks * 256                                                       # stride
    return dict(total4=total4, blocks=blocks, stride=stride, trips=_cdiv(total4, stride),          # i < total4
                cstep=stride % (C >> 2),                                        # cstep
                last_trip=total4 - (_cdiv(total4, stride) - 1) * stride,        # float4 of the last trip
                tail=total4 % 256)                                              # threads of the last workgroup with work


def case_form(R, C):
    f = reduce_form(R, C)
    f.update(apply_form(R, C))
    f.update(R=R, C=C, workspace=workspace_bytes(R, C))
    return f


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# (form, R, C).  FORMS names each form by a predicate on the form dict; tests/test_norm_ref.py asserts that every predicate holds
# for the case that claims it and for no other.  The largest new case holds 8.4 M floats.
FORM_CASES = [
    ("one float4, one block, R = 1", 1, 4),
    ("cg = 256, chain 2", 2, 1024),
    ("rows_per_iter 85, one idle thread, single block", 31, 12),
    ("two blocks of 17 and 16 rows", 33, 12),
    ("32 of 256 ty active", 64, 4),
    ("56 idle threads, cstep 24, one trip", 777, 400),
    ("127 idle threads, ragged last block", 4100, 516),
    ("cg = 255", 1000, 1020),
    ("block cap, 31 empty blocks, C = 4", 32769, 4),
    ("block cap, 31 empty blocks, C = 12", 32769, 12),
    ("apply: 2 trips, cstep 16, no tail", 22000, 192),
    ("apply: 2 trips, cstep 76, tail 144", 10500, 400),
    ("apply: 3 trips, cstep 1, chain 9, finalize 4 trips", 700000, 12),
    ("apply: second trip of 5 float4, one empty block", 349527, 12),
    ("apply: multi-trip with cstep 0", 20000, 512),
]
FORMS = {
    "one float4, one block, R = 1": lambda f: f["R"] == 1 and f["total4"] == 1 and f["nblk"] == 1,
    "cg = 256, chain 2": lambda f: f["cg"] == 256 and f["rows_per_iter"] == 1 and f["chain"] == 2,
    "rows_per_iter 85, one idle thread, single block": lambda f: (f["rows_per_iter"], f["idle_threads"], f["nblk"]) == (85, 1, 1),
    "two blocks of 17 and 16 rows": lambda f: (f["nblk"], f["rows_per_block"], f["last_rows"]) == (2, 17, 16),
    "32 of 256 ty active": lambda f: (f["cg"], f["rows_per_iter"], f["fold"], f["nblk"]) == (1, 256, 32, 2),
    "56 idle threads, cstep 24, one trip": lambda f: (f["idle_threads"], f["cstep"], f["trips"]) == (56, 24, 1),
    "127 idle threads, ragged last block": lambda f: f["idle_threads"] == 127 and f["last_rows"] < f["rows_per_block"],
    "cg = 255": lambda f: f["cg"] == 255 and f["idle_threads"] == 1,
    "block cap, 31 empty blocks, C = 4": lambda f: (f["nblk"], f["rows_per_block"], f["empty"], f["cg"]) == (1024, 33, 31, 1),
    "block cap, 31 empty blocks, C = 12": lambda f: (f["nblk"], f["rows_per_block"], f["empty"], f["cg"]) == (1024, 33, 31, 3),
    "apply: 2 trips, cstep 16, no tail": lambda f: (f["trips"], f["cstep"], f["tail"]) == (2, 16, 0),
    "apply: 2 trips, cstep 76, tail 144": lambda f: (f["trips"], f["cstep"], f["tail"]) == (2, 76, 144),
    "apply: 3 trips, cstep 1, chain 9, finalize 4 trips": lambda f: (f["trips"], f["cstep"], f["chain"], f["fin_trips"]) == (3, 1, 9, 4),
    "apply: second trip of 5 float4, one empty block": lambda f: (f["trips"], f["last_trip"], f["empty"]) == (2, 5, 1),
    "apply: multi-trip with cstep 0": lambda f: f["trips"] >= 2 and f["cstep"] == 0,
}
APPLY_CASES = [c for c in FORM_CASES if c[0].startswith("apply:")]       # the five multi-trip and tail cases of the apply grid
SMALL_CASES = [c for c in FORM_CASES if c[1] * c[2] <= 1100000]


def case_id(c):
    return "R%d-C%d" % (c[1], c[2])


# ---- operands ------------------------------------------------------------------------------------------------------------------------
FAMILIES = [(0.0, 1.0), (-0.3, 2.0), (3.0, 1.0), (30.0, 1.0), (3.0, 0.01), (0.1, 0.0)]      # (mean, std) of y, by channel % 6
EDGE = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, -1e-4, -20.0, -87.5, -104.0], np.float32)
GAMMAS = np.array([1.5, -1.0, 0.0, 0.75, 1.25], np.float32)                                  # by channel % 5
BIG = 1e4                            # +-BIG join y for the apply stages


def inputs(R, C, big=False):
    """-> dict y [R,C], dout [R,C], gamma, beta [C] float32, fam [C].  y: FAMILIES by channel, EDGE in the first rows of channel
    0 (as many as R holds); big: +-1e4 in the first two rows of channel 1.  dout: scale 1, channel 2 all zero, channel 3 of
    constant sign."""
    rng = np.random.RandomState(1031 * R + C)
    fam = np.arange(C) % len(FAMILIES)
    m = np.array([a for a, _ in FAMILIES])[fam]
    s = np.array([b for _, b in FAMILIES])[fam]
    y = (m + s * rng.standard_normal((R, C))).astype(np.float32)
    k = min(R, len(EDGE))
    y[:k, 0] = EDGE[:k]
    if big:
        y[R - 1, 1] = -BIG
        y[0, 1] = BIG
    dout = rng.standard_normal((R, C)).astype(np.float32)
    dout[:, 2] = 0.0
    dout[:, 3] = np.abs(dout[:, 3])
    gamma = GAMMAS[np.arange(C) % len(GAMMAS)].copy()
    beta = rng.standard_normal(C).astype(np.float32)
    return dict(y=y, dout=dout, gamma=gamma, beta=beta, fam=fam)


def synthetic_stats(R, C, count=None):
    """float64 sums [2C + 1] whose statistics are ANYTHING: rstd from 0.03 (var 1111) to 31.6 (var 0), means of both signs"""
    count = float(R if count is None else count)
    var = np.array([0.0, 0.01, 1.0, 100.0, 1111.0])[np.arange(C) % 5]
    mean = np.array([0.0, -0.7, 3.0, 30.0, -3.0, 0.1, 0.5])[np.arange(C) % 7]
    return np.concatenate([mean * count, (var + mean * mean) * count, [count]])


def synthetic_partials(nblk, C):
    """float32 [nblk, 2, C] with magnitudes mixed WITHIN a channel (1e8 next to 1e-8 and ones of both signs): a float32
    accumulation of these visibly loses"""
    rng = np.random.RandomState(7 * nblk + C)
    p = rng.standard_normal((nblk, 2, C))
    scale = np.array([1e8, 1e-8, 1.0, 1e4])[rng.randint(0, 4, (nblk, 2, C))]
    return (p * scale).astype(np.float32)


# ---- float64 statements ------------------------------------------------------------------------------------------------------------
def f64(a):
    return np.asarray(a, np.float64)


_last_z = [None, None]             # elu64 of the array it was last asked for: a case's statements all start from the same y


def elu64(y):
    """z = elu(y) through expm1 (read-only: the result is shared)"""
    if _last_z[0] is not y:
        x = f64(y)
        z = np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
        z.setflags(write=False)
        _last_z[:] = [y, z]
    return _last_z[1]


def elu_grad64(y):
    y = f64(y)
    return np.where(y > 0, 1.0, np.exp(np.minimum(y, 0.0)))


def _eabs(y):
    """E per element: E for y <= 0, 0 for y > 0, + FLOOR"""
    return np.where(np.asarray(y) > 0, 0.0, E_ELU) + FLOOR


def fwd_sums_ref(y):
    """the four sums' statement and the magnitudes their bounds are written in, per channel"""
    z = elu64(y)
    e = _eabs(y)
    return dict(S1=z.sum(0), S2=(z * z).sum(0), A1=np.abs(z).sum(0), sE=e.sum(0), Q=(2 * np.abs(z) * e + e * e).sum(0))


def fwd_sums_bound(ref, form):
    n = form["chain"] + form["fold"]
    nb = form["nblk"] * 2.0 ** -53
    b1 = ((n * U + nb) * (ref["A1"] + ref["sE"]) + ref["sE"]) * SECOND
    b2 = ((n * U + nb) * (ref["S2"] + ref["Q"]) + ref["Q"]) * SECOND
    return b1, b2


def stats_from_sums(sums, mm_old=None, mv_old=None):
    """norm_fwd_stats, as norm_fwd_stats_from_sums and norm_fwd_finalize call it, in float64: -> dict of float64 values BEFORE the
    float32 rounding (mean, var, rstd, moving_mean, moving_var, count)"""
    sums = f64(sums)
    C = (len(sums) - 1) // 2
    R = sums[2 * C]
    m = sums[:C] / R                                                            # m
    var = np.maximum(sums[C:2 * C] / R - m * m, 0.0)                            # var, clamped
    out = dict(mean=m, var=var, rstd=1.0 / np.sqrt(var + np.float64(EPS)), count=R)           # mean, rstd
    if mm_old is not None:
        mom = np.float64(MOM)
        out["moving_mean"] = (1.0 - mom) * f64(mm_old) + mom * m                # run_mean
        out["moving_var"] = (1.0 - mom) * f64(mv_old) + mom * var               # run_var
    return out


def eval_stats(mm, mv):
    """norm_eval_stats -> float32 save_mean (a copy), float64 rstd before its rounding"""
    return np.asarray(mm, np.float32).copy(), 1.0 / np.sqrt(f64(mv) + np.float64(EPS))


def out_ref(y, mean, rstd, gamma, beta):
    """out = (elu(y) - mean) rstd gamma + beta at the given statistics -> (out, bound per element)"""
    z = elu64(y)
    mean, rstd, gamma, beta = f64(mean), f64(rstd), f64(gamma), f64(beta)
    out = (z - mean) * rstd * gamma + beta
    bound = ((_eabs(y) + 3 * U * np.abs(z - mean)) * rstd * np.abs(gamma) + U * np.abs(out) + TINY) * SECOND
    return out, bound


def bwd_sums_ref(y, dout, mean, rstd):
    """sum dout, sum dout zhat at the given float32 statistics, and the magnitudes of their bounds, per channel"""
    z, g = elu64(y), f64(dout)
    mean, rstd = f64(mean), f64(rstd)
    zh = (z - mean) * rstd
    Z = _eabs(y) * rstd * (1 + 2 * U) + 2 * U * np.abs(zh)
    return dict(Sd=g.sum(0), Sdz=(g * zh).sum(0), Ad=np.abs(g).sum(0), Adz=np.abs(g * zh).sum(0), W=(np.abs(g) * Z).sum(0))


def bwd_sums_bound(ref, form):
    n = form["chain"] + form["fold"]
    nb = form["nblk"] * 2.0 ** -53
    return (n * U + nb) * ref["Ad"] * SECOND + TINY, ((n * U + nb) * (ref["Adz"] + ref["W"]) + ref["W"]) * SECOND + TINY


def dy_ref(y, dout, gamma, mean, rstd, c0, c1):
    """dy = gamma rstd (dout - c0 - zhat c1) elu'(y) at the given float32 statistics and coefficients (zeros in inference mode)
    -> (dy, bound per element)"""
    z, g = elu64(y), f64(dout)
    mean, rstd, gamma, c0, c1 = f64(mean), f64(rstd), f64(gamma), f64(c0), f64(c1)
    zh = (z - mean) * rstd
    dy = gamma * rstd * (g - c0 - zh * c1) * elu_grad64(y)
    e = _eabs(y)
    Z = e * rstd * (1 + 2 * U) + 2 * U * np.abs(zh)
    T = np.abs(g) + np.abs(c0) + np.abs(zh * c1)
    G = np.abs(gamma) * rstd
    neg = ~(np.asarray(y) > 0)
    bound = (G * ((Z * np.abs(c1) + 5 * U * T) + neg * T * (e + U / 2)) + U * np.abs(dy) + TINY) * SECOND
    return dy, bound


def statement(y, dout, gamma, beta, mm, mv, training=True):
    """the whole op in float64, its own statistics throughout -> dict (out, mean, var, rstd, moving_mean, moving_var, dgamma,
    dbeta, c0, c1, dy)"""
    R = y.shape[0]
    z, g = elu64(y), f64(dout)
    if training:
        # (two passes: in one pass even float64 loses kappa 2^-53 of the variance, 1e-11 at kappa 1e4, and this is the reference)
        mean = z.mean(0)
        var = np.maximum(((z - mean) ** 2).mean(0), 0.0)
        rstd = 1.0 / np.sqrt(var + np.float64(EPS))
        mom = np.float64(MOM)
        mm_new, mv_new = (1.0 - mom) * f64(mm) + mom * mean, (1.0 - mom) * f64(mv) + mom * var
    else:
        mean, var = f64(mm), f64(mv)
        rstd = 1.0 / np.sqrt(var + np.float64(EPS))
        mm_new, mv_new = f64(mm), f64(mv)
    zh = (z - mean) * rstd
    out = zh * f64(gamma) + f64(beta)
    dbeta, dgamma = g.sum(0), (g * zh).sum(0)
    c0, c1 = (dbeta / R, dgamma / R) if training else (np.zeros_like(dbeta), np.zeros_like(dbeta))
    dy = f64(gamma) * rstd * (g - c0 - zh * c1) * elu_grad64(y)
    return dict(out=out, mean=mean, var=var, rstd=rstd, moving_mean=mm_new, moving_var=mv_new, dgamma=dgamma, dbeta=dbeta,
                c0=c0, c1=c1, dy=dy)


def e2e_bounds(y, gamma, form, st):
    """the one-pass bound against the float64 statement's own statistics `st` (statement()) -> dict dmean, drstd (per channel),
    kappa, and out_extra(mean_k, rstd_k): what the statistics' error adds to an element's apply bound"""
    R = y.shape[0]
    ref = fwd_sums_ref(y)
    d1, d2 = fwd_sums_bound(ref, form)
    m, var = st["mean"], st["var"]
    dm = d1 / R
    dvar = d2 / R + 2 * np.abs(m) * dm + dm * dm
    room = var + np.float64(EPS) - dvar
    with np.errstate(divide="ignore", invalid="ignore"):
        drstd = np.where(room > 0, 0.5 * np.maximum(room, TINY) ** -1.5 * dvar, np.inf) + U * st["rstd"]
    dmean = dm + U * np.abs(m) + TINY
    z = elu64(y)
    extra = np.abs(f64(gamma)) * (np.abs(z - m) * drstd + (st["rstd"] + drstd) * dmean)
    return dict(dmean=dmean, drstd=drstd, dvar=dvar, kappa=(m * m + var) / (var + np.float64(EPS)), out_extra=extra)


# ---- measuring ---------------------------------------------------------------------------------------------------------------------
def worst(got, want, bound):
    """max |got - want| / bound; inf where got is not finite, or off where the bound is 0"""
    got, want, bound = np.broadcast_arrays(f64(got), f64(want), f64(bound))
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nan_to_num(r, nan=np.inf).max())


def first_bad(got, want, bound, C):
    """-> None, or (i, message): the flat index of the first element outside its bound and its row, channel, channel group and
    float4: a slip of norm_apply_kernel's carried channel group is named by where it begins"""
    got, want = f64(got).ravel(), f64(want).ravel()
    bad = ~(np.abs(got - want) <= np.broadcast_to(bound, (got.size // C, C)).ravel())
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    return i, ("%d of %d elements outside the bound, first at flat index %d (row %d, channel %d, channel group %d, float4 %d): got %r, "
            "want %r, bound %.3g" % (int(bad.sum()), got.size, i, i // C, i % C, (i % C) // 4, i // 4, got[i], want[i],
                                     float(np.broadcast_to(bound, (got.size // C, C)).ravel()[i])))


def rounding(want):
    """one float32 rounding of a float64 value"""
    return U * np.abs(want) + TINY


# ---- float32 restatement of the kernels, and the mutations the bounds must catch -----------------------------------------------
REDUCE_MUTATIONS = ("last row of a block dropped", "trip's first row counted again", "empty block's partial left stale")
APPLY_MUTATIONS = ("cq not wrapped", "cq wrapped one trip late")
F32 = np.float32


def elu32(y):
    """elu1 (common.hpp), with numpy's float32 exp standing in for __expf"""
    y = np.asarray(y, F32)
    return np.where(y > 0, y, np.exp(np.minimum(y, F32(0))) - F32(1)).astype(F32)


def fma32(a, b, c):
    """fmaf: the product is exact in float64"""
    return (f64(a) * f64(b) + f64(c)).astype(F32)


def reduce_f32(form, y, dout=None, mean=None, rstd=None, mutate=None):
    """norm_reduce_kernel<BWD = dout is not None> -> partial [nblk, 2, C] float32.  Per ty a chain over the rows
    r0 + ty + k rows_per_iter, four per trip (the loop over rb), the squares by fmaf; then the fold of the ty in order."""
    R, C = y.shape
    nblk, rpb, rpi = form["nblk"], form["rows_per_block"], form["rows_per_iter"]
    K = K_REDUCE_UN * _cdiv(form["chain"], K_REDUCE_UN)
    nrows = np.clip(R - np.arange(nblk) * rpb, 0, rpb)                       # r0, r1
    if mutate == REDUCE_MUTATIONS[0]:
        nrows = np.maximum(nrows - 1, 0)
    local = np.arange(K * rpi).reshape(K, rpi)                                # row k rows_per_iter + ty of the block
    valid = local[None] < nrows[:, None, None]                                # rb + u * rows_per_iter < r1   [nblk, K, rpi]
    idx = np.minimum(np.arange(nblk)[:, None, None] * rpb + local[None], R - 1)
    bwd = dout is not None
    a = np.zeros((nblk, rpi, C), F32)
    b = np.zeros((nblk, rpi, C), F32)
    for k in range(K):
        k0 = k - k % K_REDUCE_UN
        m, rows = valid[:, k], idx[:, k]
        if mutate == REDUCE_MUTATIONS[1]:                                     # the clamp rc without the mask
            rows = np.where(m, rows, idx[:, k0])
            m = valid[:, k0]
        if not m.any():
            continue
        z = elu32(y[rows])
        m = m[..., None]
        if not bwd:
            a = np.where(m, a + z, a)
            b = np.where(m, fma32(z, z, b), b)
        else:
            g = dout[rows]
            a = np.where(m, a + g, a)
            b = np.where(m, fma32(g, (z - mean.astype(F32)) * rstd.astype(F32), b), b)
    sa, sb = a[:, 0].copy(), b[:, 0].copy()
    for j in range(1, rpi):
        sa = sa + a[:, j]
        sb = sb + b[:, j]
    part = np.stack([sa, sb], 1)
    assert part.dtype == F32 and part.shape == (nblk, 2, C)
    if mutate == REDUCE_MUTATIONS[2]:                                         # no store for r0 >= R: what the last call left there
        part[form["used"]:] = part[0]
    return part


def sum_partials(partial):
    """sum_partials_32x8: per lane py the partials py, py + 32, ... in order, then the 32 lanes in order, all in
    double -> float64 [2, C].  (numpy's float64 additions are the device's: this is the kernel's result bit for bit.)"""
    nblk = partial.shape[0]
    T = _cdiv(nblk, K_FIN_LANES)
    p = np.zeros((T * K_FIN_LANES,) + partial.shape[1:], np.float64)
    p[:nblk] = partial
    p = p.reshape((T, K_FIN_LANES) + partial.shape[1:])
    lanes = np.zeros(p.shape[1:], np.float64)
    for t in range(T):
        lanes = lanes + p[t]
    s = lanes[0].copy()
    for j in range(1, K_FIN_LANES):
        s = s + lanes[j]
    return s


def fwd_sums_f32(form, y, mutate=None):
    """sph3d_elu_bn_forward_sums -> float64 [2C + 1]"""
    s = sum_partials(reduce_f32(form, y, mutate=mutate))
    return np.concatenate([s[0], s[1], [float(y.shape[0])]])


def stats_f32(sums, mm, mv):
    """the float32 values norm_fwd_stats_from_sums stores"""
    st = stats_from_sums(sums, mm, mv)
    return dict(mean=st["mean"].astype(F32), rstd=st["rstd"].astype(F32), moving_mean=st["moving_mean"].astype(F32),
                moving_var=st["moving_var"].astype(F32), count=st["count"])


def channel_of(form, C, mutate=None):
    """the channel group norm_apply_kernel carries (cq) for every float4 -> int [total4]; cg and beyond: out of range"""
    total4, stride, cg, cstep = form["total4"], form["stride"], C >> 2, form["cstep"]
    cq = np.arange(min(stride, total4)) % cg                                  # cq = i0 % cg
    out = np.empty(total4, np.int64)
    for t in range(form["trips"]):
        n = min(stride, total4 - t * stride)
        out[t * stride:t * stride + n] = cq[:n]                               # c = cq * 4
        cq = cq + cstep                                                       # cq += cstep
        if mutate == APPLY_MUTATIONS[0]:
            pass
        elif mutate == APPLY_MUTATIONS[1]:
            cq = np.where(cq > cg, cq - cg, cq)
        else:
            cq = np.where(cq >= cg, cq - cg, cq)                              # the wrap
    return out


def _per_element(form, C, v, mutate):
    """a per-channel float32 vector as every element of [R, C] reads it; NaN where the channel group is out of range"""
    cq = channel_of(form, C, mutate)
    pad = np.concatenate([np.asarray(v, F32), np.full(max(0, 4 * (int(cq.max()) + 1) - C), np.nan, F32)])
    c = (cq[:, None] * 4 + np.arange(4)[None]).reshape(-1, C)
    return pad[c]


def apply_fwd_f32(form, y, mean, rstd, gamma, beta, mutate=None):
    """norm_apply_kernel<false>"""
    C = y.shape[1]
    mu, rs, ga, be = (_per_element(form, C, v, mutate) for v in (mean, rstd, gamma, beta))
    return fma32((elu32(y) - mu) * rs, ga, be)


def apply_bwd_f32(form, y, dout, gamma, mean, rstd, c0, c1, mutate=None):
    """norm_apply_kernel<true>: SPH3D_BN_BWD"""
    C = y.shape[1]
    mu, rs, ga, k0, k1 = (_per_element(form, C, v, mutate) for v in (mean, rstd, gamma, c0, c1))
    z = elu32(y)
    zh = (z - mu) * rs
    dz = (ga * rs) * ((dout - k0) - zh * k1)
    out = np.where(y > 0, dz, dz * (z + F32(1)))
    assert out.dtype == F32
    return out


# ---- the checks both test files apply: each returns the worst |error| / bound (allowed: 1) -----------------------------------------
def check_fwd_sums(sums, y, form):
    """sums: float64 [2C + 1] -> (worst S1, worst S2); the row count must be exact"""
    C = y.shape[1]
    ref = fwd_sums_ref(y)
    b1, b2 = fwd_sums_bound(ref, form)
    assert sums.shape == (2 * C + 1,) and sums[2 * C] == y.shape[0], (sums.shape, sums[2 * C])
    return worst(sums[:C], ref["S1"], b1), worst(sums[C:2 * C], ref["S2"], b2)


def check_stats(got, sums, mm_old, mv_old):
    """got: dict mean, rstd, moving_mean, moving_var (float32 [C]), count -> worst over the five, each held to one float32
    rounding of the float64 expression on `sums`"""
    st = stats_from_sums(sums, mm_old, mv_old)
    assert float(got["count"]) == st["count"]
    return max(worst(got[k], st[k], rounding(st[k])) for k in ("mean", "rstd", "moving_mean", "moving_var"))


def check_bwd_sums(dgamma, dbeta, sums, y, dout, mean, rstd, form):
    """-> (worst sum dout, worst sum dout zhat) over the float64 [2C] and the float32 dbeta / dgamma, which must be the float32
    roundings of the float64 sums"""
    C = y.shape[1]
    ref = bwd_sums_ref(y, dout, mean, rstd)
    bd, bdz = bwd_sums_bound(ref, form)
    assert np.array_equal(np.asarray(dbeta, F32), sums[:C].astype(F32)) and np.array_equal(np.asarray(dgamma, F32), sums[C:].astype(F32))
    return (max(worst(sums[:C], ref["Sd"], bd), worst(dbeta, ref["Sd"], bd + rounding(ref["Sd"]) + U * bd)),
            max(worst(sums[C:], ref["Sdz"], bdz), worst(dgamma, ref["Sdz"], bdz + rounding(ref["Sdz"]) + U * bdz)))


def coef32(sums, count):
    """norm_bwd_coef, as norm_bwd_coef_from_sums calls it -> float32 c0, c1"""
    C = len(sums) // 2
    c = (f64(sums) / float(count)).astype(F32)
    return c[:C], c[C:]
