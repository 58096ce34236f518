"""The last stretch of a segmentation step, restated: the logits layer (csrc/skinny.hip) and the training loss (csrc/loss.hip).
  * the launch arithmetic of both files in plain Python, with the source lines it is copied from;
  * FORM_CASES: for each kernel the smallest shape that reaches each distinct launch form, with the predicate that names the form;
  * float64 numpy statements of the three operations, with the term magnitudes the bounds are written in;
  * a float32 numpy restatement of the loss in the kernel's operation order, which entitles the loss bounds to be used on the kernel
    (tests/test_head_ref.py holds it to them on the CPU);
  * the operands of the GPU tests (tests/test_gpu_skinny_forms.py, tests/test_gpu_xent_forms.py).
numpy only: no torch, no library."""
import numpy as np

U = 2.0 ** -24                       # float32 unit roundoff


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- csrc/skinny.hip: launch arithmetic ------------------------------------------------------------------------------------------
K_SK_MAX_K = 256                     # skinny.hip:24   kSkMaxK
K_SK_NN_MAX_WGS = 2048               # skinny.hip:217  if (wgs > 2048) wgs = 2048
K_SK_ROWS_PER_TRIP = 8               # skinny.hip:82   kSkRowsPerTrip
K_SK_TN_WGS = 512                    # skinny.hip:198  kSkTnWGs


def skinny_supported(R, K1, K2, N):
    """sk_ok, skinny.hip:191-196"""
    return (R > 0 and 1 <= N <= 16 and K1 >= 16 and K1 % 16 == 0 and K2 >= 0 and K2 % 16 == 0 and K1 + K2 <= K_SK_MAX_K
            and _cdiv(K1, 64) + _cdiv(K2, 64) <= 4)


def skinny_nn_form(R, K1, K2, N):
    """sph3d_pointwise_gemm_skinny, skinny.hip:215-219 (the grid) and skinny_nn_kernel, skinny.hip:36, 44-46 (a wave's tiles)"""
    tiles = _cdiv(R, 16)                                        # :215
    wgs = max(1, min(K_SK_NN_MAX_WGS, _cdiv(tiles, 8)))         # :216-218, two tiles per wave
    waves = 4 * wgs                                             # :45   nw = gridDim.x * 4
    return dict(tiles=tiles, wgs=wgs, trips=_cdiv(tiles, waves),                   # :46   the busiest wave (wid = 0)
                min_trips=tiles // waves, idle_waves=max(0, waves - tiles),
                ragged=R % 16,                                                     # :48   rows of the last tile, 0 = whole
                kt1=K1 // 16, kt=(K1 + K2) // 16, N=N)                             # :36   k-groups of the first half, of both


def skinny_tn_form(R, K1, K2):
    """sph3d_pointwise_gemm_skinny_tn, skinny.hip:245-251, skinny_tn_kernel :92, :98-101 and skinny_tn_reduce :165-180"""
    unit = 4 * K_SK_ROWS_PER_TRIP                                                  # :245
    rows_per_wg = _cdiv(_cdiv(R, K_SK_TN_WGS), unit) * unit                        # :246
    wgs = _cdiv(R, rows_per_wg)                                                    # :247  = nslabs of the reduce
    return dict(rows_per_wg=rows_per_wg, wgs=wgs, last_rows=R - (wgs - 1) * rows_per_wg,
                reduce_trips=_cdiv(wgs, 64),                                       # :170  p0 = py, py + 64, ... (py = 0)
                reduce_ragged=wgs % 64 != 0,                                       # :175  some p0 + 8u >= nslabs in the last trip
                reduce_idle=max(0, 8 - wgs),                                       # :170  lanes with py >= nslabs never enter
                ns1=_cdiv(K1, 64), ns2=_cdiv(K2, 64),                              # :92
                partial1=K1 % 64 != 0, partial2=K2 % 64 != 0,                      # :117, :143  ch < Kh cuts the last group
                slabs_bytes=4 * K_SK_TN_WGS * (K1 + K2) * 16)                      # :226


# ---- csrc/loss.hip: launch arithmetic --------------------------------------------------------------------------------------------
def xent_form(N):
    """sph3d_masked_softmax_xent_parts, loss.hip:77-78; sph3d_masked_softmax_xent, loss.hip:86-88; masked_xent_kernel :38, :41, :44"""
    S = min(16, max(1, _cdiv(N, 1024)))                                            # :77-78
    chunk = _cdiv(N, S)                                                            # :87
    return dict(S=S, chunk=chunk, trips=_cdiv(chunk, 1024),                        # :44   n = n0 + tid; n < n1; n += 1024
                count_trips=_cdiv(N, 1024),                                        # :38
                last_rows=N - (S - 1) * chunk)                                     # :41


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# kernel -> [(form, shape...)]: nn (R, K1, K2, N, bias), tn (R, K1, K2, N), xent (B, N, C).  FORMS names each form by a predicate on
# (the form dict, the shape); tests/test_head_ref.py asserts that every predicate holds for the case that claims it and for no other.
# A split between the halves next to the first and the last k-group: 16 + 240 and 240 + 16 start five groups of 64 channels, which
# both entry points refuse (include/sph3d.h, sk_ok); 16 + 192 and 192 + 16 are the widest splits of that kind the layer accepts, and
# the two refused shapes are held as refusals (REFUSED_GROUPS).
REFUSED_GROUPS = [(200, 16, 240, 13), (200, 240, 16, 13), (200, 112, 144, 13)]
FORM_CASES = {
    "nn": [
        ("one row", 1, 16, 0, 1, 1),
        ("one tile, R < 16", 15, 16, 0, 1, 1),
        ("one whole tile, three idle waves", 16, 16, 0, 1, 1),
        ("two tiles, the second of one row", 17, 16, 0, 1, 1),
        ("halves 128 + 64, N = 5", 77, 128, 64, 5, 1),
        ("split after the first k-group", 200, 16, 192, 13, 1),
        ("split before the last k-group", 200, 192, 16, 13, 1),
        ("one operand of 256, N = 16", 130, 256, 0, 16, 1),
        ("halves 128 + 128, N = 15", 130, 128, 128, 15, 1),
        ("halves 112 + 128", 130, 112, 128, 13, 1),
        ("no bias", 130, 128, 128, 13, 0),
        ("two trips in eight workgroups", 1000, 64, 0, 16, 1),
        ("capped grid, third trip, ragged end", 262144 + 16 * 5 + 7, 16, 0, 1, 1),
    ],
    "tn": [
        ("one workgroup of one row", 1, 16, 16, 13),
        ("one workgroup, a ragged 4-row group", 5, 16, 16, 13),
        ("one workgroup, one row short", 31, 16, 16, 13),
        ("one whole workgroup", 32, 16, 16, 13),
        ("two workgroups, the last of one row", 33, 16, 16, 13),
        ("7 slabs, one idle reduce lane", 7 * 32, 16, 16, 13),
        ("8 slabs", 8 * 32, 16, 16, 13),
        ("65 slabs, ragged second reduce trip", 64 * 32 + 1, 16, 16, 13),
        ("512 slabs of 32 rows", 16384, 16, 16, 13),
        ("rows_per_wg 64", 16385, 16, 16, 13),
        ("rows_per_wg 96", 512 * 64 + 1, 16, 16, 13),
        ("channels 16 + 0", 1000, 16, 0, 1),
        ("channels 256 + 0", 1000, 256, 0, 16),
        ("channels 128 + 128", 1000, 128, 128, 13),
        ("channels 112 + 128", 1000, 112, 128, 16),
        ("channels 64 + 192", 1000, 64, 192, 1),
        ("channels 48 + 80", 1000, 48, 80, 13),
    ],
    "xent": [
        ("one point", 4, 1, 13),
        ("less than a wave", 4, 63, 13),
        ("one part, ragged", 4, 1000, 13),
        ("one part of 1024", 4, 1024, 13),
        ("two parts", 4, 1025, 13),
        ("16 parts of 1024", 4, 16384, 13),
        ("chunk 1025, second trip of one thread", 4, 16385, 13),
        ("chunk 2500, three trips", 4, 40000, 13),
        ("one class", 4, 1025, 1),
        ("two classes", 4, 1025, 2),
        ("21 classes", 4, 1025, 21),
        ("64 classes", 4, 1025, 64),
    ],
}

_RK16 = lambda s: s[1] == 16 and s[2] == 16                    # noqa: E731  (the row-count cases of the weight gradient)
FORMS = {
    "nn": {
        "one row": lambda f, s: s[0] == 1,
        "one tile, R < 16": lambda f, s: f["tiles"] == 1 and 1 < s[0] < 16,
        "one whole tile, three idle waves": lambda f, s: f["tiles"] == 1 and f["ragged"] == 0 and f["idle_waves"] == 3,
        "two tiles, the second of one row": lambda f, s: f["tiles"] == 2 and f["ragged"] == 1,
        "halves 128 + 64, N = 5": lambda f, s: (f["kt1"], f["kt"], f["N"]) == (8, 12, 5),
        "split after the first k-group": lambda f, s: (f["kt1"], f["kt"]) == (1, 13),
        "split before the last k-group": lambda f, s: (f["kt1"], f["kt"]) == (12, 13),
        "one operand of 256, N = 16": lambda f, s: (f["kt1"], f["kt"], f["N"]) == (16, 16, 16) and s[2] == 0,
        "halves 128 + 128, N = 15": lambda f, s: (f["kt1"], f["kt"], f["N"]) == (8, 16, 15) and s[4] == 1,
        "halves 112 + 128": lambda f, s: (f["kt1"], f["kt"]) == (7, 15),
        "no bias": lambda f, s: s[4] == 0,
        "two trips in eight workgroups": lambda f, s: f["trips"] == 2 and f["wgs"] == 8,
        "capped grid, third trip, ragged end": lambda f, s: (f["wgs"] == K_SK_NN_MAX_WGS and f["trips"] == 3 and f["min_trips"] == 2
                                                             and f["ragged"] != 0),
    },
    "tn": {
        "one workgroup of one row": lambda f, s: _RK16(s) and f["wgs"] == 1 and f["last_rows"] == 1,
        "one workgroup, a ragged 4-row group": lambda f, s: _RK16(s) and f["wgs"] == 1 and 4 < f["last_rows"] < 8,
        "one workgroup, one row short": lambda f, s: _RK16(s) and f["wgs"] == 1 and f["last_rows"] == f["rows_per_wg"] - 1,
        "one whole workgroup": lambda f, s: _RK16(s) and f["wgs"] == 1 and f["last_rows"] == f["rows_per_wg"],
        "two workgroups, the last of one row": lambda f, s: _RK16(s) and f["wgs"] == 2 and f["last_rows"] == 1,
        "7 slabs, one idle reduce lane": lambda f, s: _RK16(s) and f["wgs"] == 7 and f["reduce_idle"] == 1,
        "8 slabs": lambda f, s: _RK16(s) and f["wgs"] == 8 and f["reduce_idle"] == 0,
        "65 slabs, ragged second reduce trip": lambda f, s: _RK16(s) and f["wgs"] == 65 and f["reduce_trips"] == 2 and f["reduce_ragged"],
        "512 slabs of 32 rows": lambda f, s: _RK16(s) and f["wgs"] == 512 and f["rows_per_wg"] == 32 and not f["reduce_ragged"],
        "rows_per_wg 64": lambda f, s: _RK16(s) and f["rows_per_wg"] == 64,
        "rows_per_wg 96": lambda f, s: _RK16(s) and f["rows_per_wg"] == 96,
        "channels 16 + 0": lambda f, s: (f["ns1"], f["ns2"], f["partial1"]) == (1, 0, True) and s[3] == 1,
        "channels 256 + 0": lambda f, s: (f["ns1"], f["ns2"], f["partial1"]) == (4, 0, False) and s[3] == 16,
        "channels 128 + 128": lambda f, s: (f["ns1"], f["ns2"], f["partial1"], f["partial2"]) == (2, 2, False, False) and s[3] == 13,
        "channels 112 + 128": lambda f, s: (f["ns1"], f["ns2"], f["partial1"], f["partial2"]) == (2, 2, True, False) and s[3] == 16,
        "channels 64 + 192": lambda f, s: (f["ns1"], f["ns2"], f["partial1"], f["partial2"]) == (1, 3, False, False) and s[3] == 1,
        "channels 48 + 80": lambda f, s: (f["ns1"], f["ns2"], f["partial1"], f["partial2"]) == (1, 2, True, True) and s[3] == 13,
    },
    "xent": {
        "one point": lambda f, s: s[1] == 1,
        "less than a wave": lambda f, s: 1 < s[1] < 64,
        "one part, ragged": lambda f, s: f["S"] == 1 and 64 <= s[1] < 1024,
        "one part of 1024": lambda f, s: f["S"] == 1 and f["chunk"] == 1024,
        "two parts": lambda f, s: f["S"] == 2 and s[2] == 13,
        "16 parts of 1024": lambda f, s: f["S"] == 16 and f["chunk"] == 1024 and f["trips"] == 1,
        "chunk 1025, second trip of one thread": lambda f, s: f["S"] == 16 and f["chunk"] == 1025 and f["trips"] == 2,
        "chunk 2500, three trips": lambda f, s: f["S"] == 16 and f["chunk"] == 2500 and f["trips"] == 3,
        "one class": lambda f, s: s[2] == 1,
        "two classes": lambda f, s: s[2] == 2,
        "21 classes": lambda f, s: s[2] == 21,
        "64 classes": lambda f, s: s[2] == 64,
    },
}


def case_form(kernel, shape):
    if kernel == "nn":
        return skinny_nn_form(*shape[:4])
    if kernel == "tn":
        return skinny_tn_form(*shape[:3])
    return xent_form(shape[1])


# ---- the products: float64 statements and the exact operands ---------------------------------------------------------------------
def _cat(a1, a2):
    return a1 if a2 is None else np.concatenate([a1, a2], axis=1)


def skinny_ref(a1, a2, w, bias):
    """Y = A1 W[:K1] + A2 W[K1:] + bias -> (Y, the summed magnitudes of every element's terms), float64"""
    a, w = _cat(a1, a2).astype(np.float64), w.astype(np.float64)
    y, mag = a @ w, np.abs(a) @ np.abs(w)
    if bias is not None:
        y, mag = y + bias.astype(np.float64), mag + np.abs(bias.astype(np.float64))
    return y, mag


def skinny_tn_ref(a1, a2, dy):
    """dW = [A1 | A2]^T dY -> (dW, term magnitudes), float64"""
    a, dy = _cat(a1, a2).astype(np.float64), dy.astype(np.float64)
    return a.T @ dy, np.abs(a).T @ np.abs(dy)


def int_operand(rows, cols, salt, lim=4):
    """integers in [-lim, lim] as float32, hashed from (row, column, salt): every row and every column differs from its neighbours,
    so a dropped, doubled or misplaced one changes the product"""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(cols, dtype=np.uint64)[None, :]
    h = (r * np.uint64(0x9E3779B1) + c * np.uint64(0x85EBCA6B) + np.uint64(salt) * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    return ((h % np.uint64(2 * lim + 1)).astype(np.int64) - lim).astype(np.float32)


def int_product(a1, a2, b, bias=None, transpose=False):
    """the int64 product cast to float32: [A1|A2] B (+ bias), or [A1|A2]^T B.  Every partial sum of these operands is an integer
    below 2^24 (rows x 16 < 2^24 up to a million rows), so a float32 kernel computes exactly this in whatever order it sums."""
    a = _cat(a1, a2).astype(np.int64)
    out = (a.T if transpose else a) @ b.astype(np.int64)
    if bias is not None:
        out = out + bias.astype(np.int64)
    assert np.abs(out).max() < 2 ** 24 and a.shape[0 if transpose else 1] * 16 < 2 ** 24
    return out.astype(np.float32)


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
K_XENT_TREE = 26                     # a loss part's bound: the 1024-thread tree of block_sum_1024 (loss.hip:13-23) ...
K_XENT_UNITS = 8                     # ... and the bounds' factor for the row arithmetic
# The gradient bound is relative to p, and float32 cannot hold every p / cnt to a relative error: with one dominant class (+80) in
# a block of 40 000 inner points, e^-84 / 40000 = 8e-42 is a subnormal, and on this alone the float32 restatement below reaches 110
# units.  A gradient element is therefore allowed the format's floor on top of its bound: the smallest normal float32, whether a
# result below it is rounded to a subnormal or flushed to zero.
F32_FLOOR = 2.0 ** -126
BAD_LABELS = (2 ** 32 + 3, -2 ** 40)
MASK_VALUES = np.array([0.0, 1.0, 2.5, -1.0, np.nan], np.float32)


def xent_inputs(B, N, C):
    """-> logits [B,N,C] float32, label [B,N] int64, inner [B,N] float32: B = 4 blocks — no inner point; all inner; exactly three
    inner points at rows 0, min(1023, N-1), N-1; a mask drawn from 0, 1, 2.5, -1, NaN (only values > 0 count).  Six kinds of rows:
    scale 1; scale 30; all classes equal; one dominant class (+80); shifted by +1000; shifted by -1000."""
    assert B == 4
    rng = np.random.RandomState(1000 * C + N % 1000 + N // 1000)
    x = rng.randn(B, N, C).astype(np.float32)
    kind = rng.randint(0, 6, (B, N))
    k = min(N, 6)
    kind[:, :k] = np.arange(k)
    kind[:, N - 1] = (np.arange(B) + 1) % 6 if N > 6 else kind[:, N - 1]
    x = np.where((kind == 1)[..., None], 30.0 * x, x)
    x = np.where((kind == 2)[..., None], 3.0 * x[..., :1], x)
    dom = rng.randint(0, C, (B, N))
    x = np.where((kind == 3)[..., None] & (np.arange(C) == dom[..., None]), x + 80.0, x)
    x = np.where((kind == 4)[..., None], x + 1000.0, x)
    x = np.where((kind == 5)[..., None], x - 1000.0, x)
    label = rng.randint(0, C, (B, N)).astype(np.int64)
    label = np.where((kind == 3) & (rng.rand(B, N) < 0.5), dom, label)        # half of the dominant rows are labelled with that class
    inner = np.zeros((B, N), np.float32)
    inner[1] = 1.0
    inner[2, [0, min(1023, N - 1), N - 1]] = 1.0
    inner[3] = MASK_VALUES[rng.randint(0, len(MASK_VALUES), N)]
    return x.astype(np.float32), label, inner


def _parts(v, S, chunk):
    """[B, N] -> [B, S, chunk], rows past N as zeros"""
    B, N = v.shape
    out = np.zeros((B, S * chunk), v.dtype)
    out[:, :N] = v
    return out.reshape(B, S, chunk)


def xent_ref(logits, label, inner):
    """float64 statement of sph3d_masked_softmax_xent (models/SPH3D_s3dis.py:116-133 and the gradient of the batch sum):
         cnt_b = #{n: inner[b,n] > 0},  loss_part[b,s] = sum over the inner rows n of part s of (lse - x_y) / cnt_b,
         dlogits[b,n,:] = inner_n / cnt_b (softmax(x) - onehot(y));  a block without inner points: zeros;
         an inner row with a label outside [0, C): its part and its gradient row are NaN.
    -> dict: loss_part, dlogits, part_mag (sum of (|m| + |lse - m| + |x_y| + 1) / cnt_b over the part's inner rows), grad_mag
       (inv_b (p (1 + |x| + |m|) + onehot) on inner rows), cnt, form"""
    B, N, C = logits.shape
    f = xent_form(N)
    x = logits.astype(np.float64)
    act = inner > 0                                                   # (NaN > 0 is false)
    cnt = act.sum(1)
    inv = np.where(cnt > 0, 1.0 / np.maximum(cnt, 1), 0.0)
    bad = act & ((label < 0) | (label >= C))
    y = np.where((label < 0) | (label >= C), 0, label)
    m = x.max(-1)
    e = np.exp(x - m[..., None])
    se = e.sum(-1)
    xy = np.take_along_axis(x, y[..., None], -1)[..., 0]
    row = np.where(act, (m + np.log(se)) - xy, 0.0)
    rmag = np.where(act, np.abs(m) + np.abs(np.log(se)) + np.abs(xy) + 1.0, 0.0)
    p = e / se[..., None]
    onehot = (np.arange(C) == y[..., None]).astype(np.float64)
    w = (act * inv[:, None])[..., None]
    d = w * (p - onehot)
    d[bad] = np.nan
    loss_part = _parts(row, f["S"], f["chunk"]).sum(-1) * inv[:, None]
    loss_part[_parts(bad, f["S"], f["chunk"]).any(-1)] = np.nan
    return dict(loss_part=loss_part, dlogits=d, part_mag=_parts(rmag, f["S"], f["chunk"]).sum(-1) * inv[:, None],
                grad_mag=w * (p * (1.0 + np.abs(x) + np.abs(m)[..., None]) + onehot), cnt=cnt, bad=bad, form=f)


def xent_units(got, want, mag, floor=0.0):
    """the worst |got - want| over the elements, in units of u x the element's magnitude, after `floor` has been taken off the
    error.  inf if an element whose magnitude is 0 is not exactly 0, or if got has a NaN where want has none or the reverse."""
    got = np.asarray(got, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    ok = ~np.isnan(want)
    err, mag = np.abs(got - want)[ok], mag[ok]
    if (err[mag == 0] != 0).any():
        return float("inf")
    live = mag > 0
    return float((np.maximum(err[live] - floor, 0.0) / (U * mag[live])).max()) if live.any() else 0.0


def xent_check(loss_part, dlogits, ref):
    """-> (worst loss part, worst gradient element) in units of u x magnitude; the bounds allow 8 + trips + 26 and 8"""
    return (xent_units(loss_part, ref["loss_part"], ref["part_mag"]),
            xent_units(dlogits, ref["dlogits"], ref["grad_mag"], F32_FLOOR))


def xent_allowed(ref):
    return K_XENT_UNITS + ref["form"]["trips"] + K_XENT_TREE, K_XENT_UNITS


def _block_sum_1024_f32(v):
    """block_sum_1024, loss.hip:13-23, on float32 [..., 1024]: the butterfly of each 64-lane wave, then the 16 waves in order"""
    v = v.reshape(v.shape[:-1] + (16, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    s = np.zeros(v.shape[:-2], np.float32)
    for k in range(16):
        s = s + v[..., k, 0]
    return s


def xent_f32(logits, label, inner):
    """masked_xent_kernel (loss.hip:28-69) in float32 numpy, in its operation order: the maximum, a sequential sum of exp(x - m),
    (m + log se) - x_y; per thread a sequential sum over its trips, then the workgroup's tree; the gradient
    exp(x - m) * (inv / se) - onehot * inv.  numpy's exp and log stand in for the device's.  -> (loss_part, dlogits)"""
    B, N, C = logits.shape
    f = xent_form(N)
    S, chunk, trips = f["S"], f["chunk"], f["trips"]
    x = logits.astype(np.float32)
    act = inner > 0
    cnt = act.sum(1).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(cnt > 0, np.float32(1.0) / cnt, np.float32(0.0)).astype(np.float32)
    oob = (label < 0) | (label >= C)
    y = np.where(oob, 0, label)
    m = x.max(-1)
    e = np.exp(x - m[..., None])
    se = np.zeros_like(m)
    for c in range(C):
        se = se + e[..., c]
    xy = np.take_along_axis(x, y[..., None], -1)[..., 0]
    row = (m + np.log(se)) - xy
    row = np.where(act, np.where(oob, np.float32(np.nan), row), np.float32(0.0)).astype(np.float32)
    per = np.zeros((B, S, trips * 1024), np.float32)
    per[:, :, :chunk] = _parts(row, S, chunk)
    per = per.reshape(B, S, trips, 1024)
    t = np.zeros((B, S, 1024), np.float32)
    for j in range(trips):
        t = t + per[:, :, j]
    loss_part = _block_sum_1024_f32(t) * inv[:, None]
    r = inv[:, None] / se
    onehot = np.arange(C) == y[..., None]
    d = e * r[..., None] - np.where(onehot, inv[:, None, None], np.float32(0.0))
    d = np.where(act[..., None], np.where(oob[..., None], np.float32(np.nan), d), np.float32(0.0)).astype(np.float32)
    assert loss_part.dtype == np.float32 and e.dtype == np.float32 and r.dtype == np.float32
    return loss_part, d
