"""Every launch form of the ELU + batch-norm tail (csrc/norm.hip; tests/_norm_ref.py: FORM_CASES) through the C ABI against the
float64 statement, entry point by entry point and element by element.  Every call writes into outputs that start as NaN, uses a
workspace the test owns, of exactly sph3d_elu_bn_workspace(R, C) bytes and filled with NaN, and every buffer it may write ends in
a sentinel band that must come back untouched.  Operands: six (mean, std) families of y by channel, the edge values 0, -0, +-1e-30,
+-1e-40, -1e-4, -20, -87.5, -104 in channel 0 (+-1e4 at the apply stages), dout with an all-zero channel and one of constant sign,
gamma of 0, -1, 1.5.  The bounds are derived in tests/_norm_ref.py (u = 2^-24, E = 4u for `__expf(y) - 1`); the allowed value is 1
unit of each.  For y <= -88 (indeed below -17.33) the code guarantees dy == 0 exactly: asserted as such.

Worst |error| / bound over the cases, the float32 restatement on the CPU (tests/test_norm_ref.py, numpy's exp) | measured on an MI355X:
    A  forward sums          sum z 0.34, sum z^2 0.42           | 0.33, 0.42
    B  supplied partials     0.09 of nblk 2^-53 sum|p|          | 0.09: the same bits as the kernel's order on the host
    C  statistics from sums  0.99                               | 0.99
    D  apply forward         0.99                               | 0.99
    E  backward sums         sum dout 0.33, sum dout zhat 0.39  | 0.33, 0.39
    F  apply backward        0.60                               | 0.60
    G  inference             rstd 0.97, out 0.95, dy 0.33       | 0.97, 0.95, 0.33; training: bit for bit at every case
    H  end to end            mean 0.34, rstd 0.33, out 0.29     | 0.25, 0.31, 0.29
  rstd against the float64 statement at R = 700000, relative: 3e-8 at y ~ (0, 1), 1.2e-5 at (30, 1), 1.1e-5 at (3, 0.01); bounds
  4e-6, 8e-3, 9e-2 (kappa 1, 900, 8200).
(C and D reach 1 by construction: where the other terms vanish, the bound is the final float32 rounding itself.)"""
import numpy as np
import pytest
import torch

import _norm_ref as N
from sph3d_gcn_amd import _lib, tf_norm

pytestmark = pytest.mark.gpu

BAND = 64                            # sentinel elements after every buffer a call may write
SENT = 12345.0
NAN = float("nan")


class Buf:
    """n elements (NaN, or `init`) followed by the sentinel band, on the device"""

    def __init__(self, dev, n, dtype=torch.float32, init=None):
        self.n = n
        self.t = torch.full((n + BAND,), NAN, dtype=dtype, device=dev)
        self.t[n:] = SENT
        if init is not None:
            self.t[:n] = torch.from_numpy(np.ascontiguousarray(init)).to(dev).reshape(-1)

    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        return self.t[:self.n].cpu().numpy()

    def intact(self):
        return bool((self.t[self.n:] == SENT).all())


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ws(dev, R, C):
    nbytes = _lib.lib().sph3d_elu_bn_workspace(R, C)
    assert nbytes == N.workspace_bytes(R, C)
    return Buf(dev, nbytes // 4), nbytes


MOMENTUM_ARG, EPS_ARG = 1.0 - tf_norm.MOMENTUM, tf_norm.EPSILON


# ---- the seven entry points, each on NaN-filled outputs and a private workspace -----------------------------------------------
def fwd_sums(dev, R, C, y=None, partial=None):
    """-> (sums float64 [2C + 1], the workspace's floats or None)"""
    l = _lib.lib()
    sums = Buf(dev, 2 * C + 1, torch.float64)
    if partial is None:
        ws, nbytes = _ws(dev, R, C)
        _lib.check(l.sph3d_elu_bn_forward_sums(R, C, 0, None, y.data_ptr(), sums.ptr(), ws.ptr(), nbytes, _lib.stream_ptr()))
        assert ws.intact()
    else:
        ws = None
        _lib.check(l.sph3d_elu_bn_forward_sums(R, C, partial.shape[0], partial.data_ptr(), None, sums.ptr(), None, 0, _lib.stream_ptr()))
    assert sums.intact()
    return sums.np(), (ws.np() if ws is not None else None)


def fwd_apply(dev, R, C, sums, y, gamma, beta, mm, mv):
    """-> dict out [R, C], mean, rstd, moving_mean, moving_var [C], count"""
    b = dict(out=Buf(dev, R * C), mean=Buf(dev, C), rstd=Buf(dev, C), moving_mean=Buf(dev, C, init=mm), moving_var=Buf(dev, C, init=mv),
             count=Buf(dev, 1, torch.float64))
    s = _dev(sums, dev)                                                       # (held until the results are back)
    _lib.check(_lib.lib().sph3d_elu_bn_forward_apply(R, C, s.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                      b["moving_mean"].ptr(), b["moving_var"].ptr(), MOMENTUM_ARG, EPS_ARG, b["out"].ptr(),
                                                      b["mean"].ptr(), b["rstd"].ptr(), b["count"].ptr(), _lib.stream_ptr()))
    assert all(v.intact() for v in b.values())
    r = {k: v.np() for k, v in b.items()}
    r["out"], r["count"] = r["out"].reshape(R, C), r["count"][0]
    return r


def bwd_sums(dev, R, C, y, dout, mean, rstd):
    """-> (dgamma, dbeta, sums float64 [2C])"""
    dg, db, sums = Buf(dev, C), Buf(dev, C), Buf(dev, 2 * C, torch.float64)
    ws, nbytes = _ws(dev, R, C)
    m, r = _dev(mean, dev), _dev(rstd, dev)
    _lib.check(_lib.lib().sph3d_elu_bn_backward_sums(R, C, y.data_ptr(), dout.data_ptr(), m.data_ptr(), r.data_ptr(),
                                                      dg.ptr(), db.ptr(), sums.ptr(), ws.ptr(), nbytes, _lib.stream_ptr()))
    assert dg.intact() and db.intact() and sums.intact() and ws.intact()
    part = ws.np()[:N.norm_blocks(R) * 2 * C].reshape(-1, 2, C)
    assert not _bits(part[N.reduce_form(R, C)["used"]:]).any(), "an empty block's partial is not +0.0"
    return dg.np(), db.np(), sums.np()


def bwd_apply(dev, R, C, sums, count, y, dout, gamma, mean, rstd):
    """-> dy [R, C]"""
    dy = Buf(dev, R * C)
    ws, nbytes = _ws(dev, R, C)
    cnt = torch.tensor([count], dtype=torch.float64, device=dev)
    s, m, r = _dev(sums, dev), _dev(mean, dev), _dev(rstd, dev)
    _lib.check(_lib.lib().sph3d_elu_bn_backward_apply(R, C, s.data_ptr(), cnt.data_ptr(), y.data_ptr(), dout.data_ptr(),
                                                       gamma.data_ptr(), m.data_ptr(), r.data_ptr(), dy.ptr(),
                                                       ws.ptr(), nbytes, _lib.stream_ptr()))
    assert dy.intact() and ws.intact()
    w = ws.np()
    assert np.isnan(w[:N.norm_blocks(R) * 2 * C]).all()                       # only coef [2][C] is written
    c0, c1 = N.coef32(sums, count)
    assert _same(w[-2 * C:-C], c0) and _same(w[-C:], c1)                      # coef = (float)(sums / count)
    return dy.np().reshape(R, C)


def uncut_forward(dev, R, C, y, gamma, beta, mm, mv, training):
    b = dict(out=Buf(dev, R * C), mean=Buf(dev, C), rstd=Buf(dev, C), moving_mean=Buf(dev, C, init=mm), moving_var=Buf(dev, C, init=mv))
    ws, nbytes = _ws(dev, R, C)
    _lib.check(_lib.lib().sph3d_elu_bn_forward(R, C, y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), b["moving_mean"].ptr(), b["moving_var"].ptr(),
                                                MOMENTUM_ARG, EPS_ARG, int(training), b["out"].ptr(), b["mean"].ptr(), b["rstd"].ptr(), ws.ptr(),
                                                nbytes, _lib.stream_ptr()))
    assert all(v.intact() for v in b.values()) and ws.intact()
    r = {k: v.np() for k, v in b.items()}
    r["out"] = r["out"].reshape(R, C)
    return r


def uncut_backward(dev, R, C, y, dout, gamma, mean, rstd, training):
    """-> (dy, dgamma, dbeta, coef [2C] as the workspace holds it)"""
    dy, dg, db = Buf(dev, R * C), Buf(dev, C), Buf(dev, C)
    ws, nbytes = _ws(dev, R, C)
    m, r = _dev(mean, dev), _dev(rstd, dev)
    _lib.check(_lib.lib().sph3d_elu_bn_backward(R, C, y.data_ptr(), dout.data_ptr(), gamma.data_ptr(), m.data_ptr(),
                                                 r.data_ptr(), int(training), dy.ptr(), dg.ptr(), db.ptr(), ws.ptr(), nbytes,
                                                 _lib.stream_ptr()))
    assert dy.intact() and dg.intact() and db.intact() and ws.intact()
    return dy.np().reshape(R, C), dg.np(), db.np(), ws.np()[-2 * C:]


# ---- per case -------------------------------------------------------------------------------------------------------------------------
_host = {}


def _case(dev, R, C, big=False):
    """operands on the host and on the device, once per shape (one shape at a time)"""
    key = (R, C, big)
    if key not in _host:
        _host.clear()
        d = N.inputs(R, C, big=big)
        d["form"] = N.case_form(R, C)
        d["mm"], d["mv"] = np.linspace(-0.5, 3.0, C).astype(np.float32), np.linspace(0.0, 2.0, C).astype(np.float32)
        d["dev"] = {k: _dev(d[k], dev) for k in ("y", "dout", "gamma", "beta")}
        _host[key] = d
    return _host[key]


def _within(what, got, want, bound, C):
    """-> worst ratio; fails with the first element outside its bound named by flat index, row, channel and channel group"""
    r = N.worst(got, want, bound)
    assert r <= 1, "%s: %s" % (what, N.first_bad(got, want, bound, C)[1])
    return r


@pytest.mark.parametrize("case", N.FORM_CASES, ids=N.case_id)
def test_form_vs_float64(dev, case):
    """stages A, C, D, E, F on the case's own statistics, G (training) and H"""
    name, R, C = case
    d = _case(dev, R, C)
    f, y, dout, gamma, beta = d["form"], d["y"], d["dout"], d["gamma"], d["beta"]
    t = d["dev"]
    assert N.FORMS[name](f)
    r = {}
    # A: forward sums; the empty blocks' partials are +0.0; a second call gives the same bits
    sums, ws = fwd_sums(dev, R, C, t["y"])
    part = ws[:f["nblk"] * 2 * C].reshape(f["nblk"], 2, C)
    assert np.isfinite(part[:f["used"]]).all() and not _bits(part[f["used"]:]).any(), "an empty block's partial is not +0.0"
    assert np.isnan(ws[f["nblk"] * 2 * C:]).all()                              # coef is not this call's
    r["A sum z"], r["A sum z^2"] = N.check_fwd_sums(sums, y, f)
    again, ws2 = fwd_sums(dev, R, C, t["y"])
    assert _same(again, sums) and _same(ws2[:part.size], part.reshape(-1))
    assert r["A sum z"] <= 1 and r["A sum z^2"] <= 1, r
    # C, D: statistics from these sums, and out at the kernel's own float32 statistics
    fw = fwd_apply(dev, R, C, sums, t["y"], t["gamma"], t["beta"], d["mm"], d["mv"])
    r["C statistics"] = N.check_stats(fw, sums, d["mm"], d["mv"])
    assert r["C statistics"] <= 1, r
    want, bound = N.out_ref(y, fw["mean"], fw["rstd"], gamma, beta)
    r["D out"] = _within("apply forward", fw["out"], want, bound, C)
    # E: backward sums at those statistics
    dg, db, s2 = bwd_sums(dev, R, C, t["y"], t["dout"], fw["mean"], fw["rstd"])
    r["E sum dout"], r["E sum dout zhat"] = N.check_bwd_sums(dg, db, s2, y, dout, fw["mean"], fw["rstd"], f)
    assert r["E sum dout"] <= 1 and r["E sum dout zhat"] <= 1, r
    assert not _bits(s2[2:3]).any() and not _bits(db[2:3]).any()               # the all-zero channel of dout: exactly zero
    # F: dy at the kernel's statistics and coef = (float)(sums / count)
    dy = bwd_apply(dev, R, C, s2, fw["count"], t["y"], t["dout"], t["gamma"], fw["mean"], fw["rstd"])
    c0, c1 = N.coef32(s2, fw["count"])
    want, bound = N.dy_ref(y, dout, gamma, fw["mean"], fw["rstd"], c0, c1)
    r["F dy"] = _within("apply backward", dy, want, bound, C)
    assert not dy[y <= -88].any() and not dy[:, gamma == 0].any()              # exactly zero, as the code guarantees
    # G: the uncut entries in training mode are the cut composition bit for bit
    un = uncut_forward(dev, R, C, t["y"], t["gamma"], t["beta"], d["mm"], d["mv"], True)
    for k in ("out", "mean", "rstd", "moving_mean", "moving_var"):
        assert _same(un[k], fw[k]), "sph3d_elu_bn_forward differs from sums + apply in %s" % k
    udy, udg, udb, ucoef = uncut_backward(dev, R, C, t["y"], t["dout"], t["gamma"], fw["mean"], fw["rstd"], True)
    assert _same(udy, dy) and _same(udg, dg) and _same(udb, db) and _same(ucoef, np.concatenate([c0, c1]))
    # H: against the float64 statement's own statistics, under the one-pass bound
    ref = N.statement(y, dout, gamma, beta, d["mm"], d["mv"])
    e = N.e2e_bounds(y, gamma, f, ref)
    r["H mean"] = N.worst(fw["mean"], ref["mean"], e["dmean"])
    r["H rstd"] = N.worst(fw["rstd"], ref["rstd"], e["drstd"])
    r["H out"] = _within("end to end", fw["out"], ref["out"], N.out_ref(y, fw["mean"], fw["rstd"], gamma, beta)[1] + e["out_extra"], C)
    mom = float(N.MOM)
    r["H moving"] = max(N.worst(fw["moving_mean"], ref["moving_mean"], mom * e["dmean"] + N.rounding(ref["moving_mean"])),
                        N.worst(fw["moving_var"], ref["moving_var"], mom * e["dvar"] + N.rounding(ref["moving_var"])))
    for k, (m, s) in enumerate(N.FAMILIES[:min(C, 6)]):
        ch = np.arange(C) % len(N.FAMILIES) == k
        rel = np.abs(fw["rstd"][ch] - ref["rstd"][ch]) / ref["rstd"][ch]
        print("    y ~ (%g, %g): kappa %.3g, rstd off by %.3g relative, bound %.3g" % (m, s, e["kappa"][ch].max(), rel.max(),
                                                                                     (e["drstd"][ch] / ref["rstd"][ch]).max()))
    print("R=%d C=%d (%s): %s" % (R, C, name, ", ".join("%s %.3f" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("case", N.FORM_CASES, ids=N.case_id)
def test_apply_at_any_statistics(dev, case):
    """stages D and F with statistics that have nothing to do with y (rstd 0.03 ... 31.6, means of both signs, a count that is not
    R) and y holding +-1e4: every element against the float64 formula at the kernel's float32 statistics"""
    name, R, C = case
    d = _case(dev, R, C, big=True)
    y, dout, gamma, beta, t = d["y"], d["dout"], d["gamma"], d["beta"], d["dev"]
    sums = N.synthetic_stats(R, C, count=3 * R + 5)
    fw = fwd_apply(dev, R, C, sums, t["y"], t["gamma"], t["beta"], d["mm"], d["mv"])
    r = {"C statistics": N.check_stats(fw, sums, d["mm"], d["mv"])}
    assert (C < 5 or fw["rstd"].min() < 0.031) and fw["rstd"].max() > 31.6 and r["C statistics"] <= 1
    want, bound = N.out_ref(y, fw["mean"], fw["rstd"], gamma, beta)
    r["D out"] = _within("apply forward", fw["out"], want, bound, C)
    assert _same(fw["out"][:, gamma == 0], np.broadcast_to(beta[gamma == 0], (R, int((gamma == 0).sum()))))      # gamma 0: beta itself
    dg, db, s2 = bwd_sums(dev, R, C, t["y"], t["dout"], fw["mean"], fw["rstd"])
    r["E sum dout"], r["E sum dout zhat"] = N.check_bwd_sums(dg, db, s2, y, dout, fw["mean"], fw["rstd"], d["form"])
    dy = bwd_apply(dev, R, C, s2, fw["count"], t["y"], t["dout"], t["gamma"], fw["mean"], fw["rstd"])
    c0, c1 = N.coef32(s2, fw["count"])
    want, bound = N.dy_ref(y, dout, gamma, fw["mean"], fw["rstd"], c0, c1)
    r["F dy"] = _within("apply backward", dy, want, bound, C)
    assert not dy[y <= -88].any()
    print("R=%d C=%d (%s), synthetic statistics: %s" % (R, C, name, ", ".join("%s %.3f" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("case", N.SMALL_CASES, ids=N.case_id)
def test_uncut_entries_in_inference_mode(dev, case):
    """stage G, training = 0: save_mean is a copy of running_mean, rstd comes from running_var (0 included), the coefficient terms
    are absent and the moving statistics are unchanged bit for bit"""
    name, R, C = case
    d = _case(dev, R, C)
    y, dout, gamma, beta, t = d["y"], d["dout"], d["gamma"], d["beta"], d["dev"]
    assert d["mv"][0] == 0
    un = uncut_forward(dev, R, C, t["y"], t["gamma"], t["beta"], d["mm"], d["mv"], False)
    mean, rstd = N.eval_stats(d["mm"], d["mv"])
    assert _same(un["mean"], mean) and _same(un["moving_mean"], d["mm"]) and _same(un["moving_var"], d["mv"])
    r = {"rstd": N.worst(un["rstd"], rstd, N.rounding(rstd))}
    assert un["rstd"][0] == np.float32(1.0 / np.sqrt(np.float64(N.EPS)))
    want, bound = N.out_ref(y, un["mean"], un["rstd"], gamma, beta)
    r["out"] = _within("inference forward", un["out"], want, bound, C)
    dy, dg, db, coef = uncut_backward(dev, R, C, t["y"], t["dout"], t["gamma"], un["mean"], un["rstd"], False)
    assert not _bits(coef).any()                                               # coef is +0.0: the two mean terms are absent
    zero = np.zeros(C, np.float32)
    want, bound = N.dy_ref(y, dout, gamma, un["mean"], un["rstd"], zero, zero)
    r["dy"] = _within("inference backward", dy, want, bound, C)
    ref = N.bwd_sums_ref(y, dout, un["mean"], un["rstd"])
    bd, bdz = N.bwd_sums_bound(ref, d["form"])
    r["dbeta"] = N.worst(db, ref["Sd"], bd * (1 + N.U) + N.rounding(ref["Sd"]))
    r["dgamma"] = N.worst(dg, ref["Sdz"], bdz * (1 + N.U) + N.rounding(ref["Sdz"]))
    st = N.statement(y, dout, gamma, beta, d["mm"], d["mv"], training=False)
    r["statement dy"] = N.worst(dy, st["dy"], bound + np.abs(st["dy"]) * 2 * N.U)          # (+ the rounding of rstd, which enters dy once)
    print("R=%d C=%d (%s), inference: %s" % (R, C, name, ", ".join("%s %.3f" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, r


# ---- B: caller-supplied partials ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 36, 1024])
@pytest.mark.parametrize("nblk", [1, 31, 32, 33, 256, 257, 1500])
def test_supplied_partials_are_summed_in_float64(dev, nblk, C):
    R = 64
    p = N.synthetic_partials(nblk, C)
    p64 = p.astype(np.float64)
    assert (np.abs(p64).max(0) / np.abs(p64).min(0)).max() > 1e12 or nblk == 1        # float32 accumulation would visibly lose
    pt = _dev(p, dev)
    sums, _ = fwd_sums(dev, R, C, partial=pt)
    want = p.astype(np.longdouble).sum(0).reshape(-1)                         # (64 bits of mantissa: exact beside 2^-53)
    bound = nblk * 2.0 ** -53 * np.abs(p64).sum(0).reshape(-1)

    def off(v):
        return float((np.abs(v.astype(np.longdouble) - want).astype(np.float64) / bound).max())

    r = off(sums[:2 * C])
    print("nblk=%d C=%d: sums %.3f of nblk 2^-53 sum|p| (a float32 accumulation: %.3g); the kernel's own order on the host: %s"
          % (nblk, C, r, off(p.sum(0, dtype=np.float32).reshape(-1)),
             "the same bits" if _same(sums[:2 * C], N.sum_partials(p).reshape(-1)) else "other bits"))
    assert np.isfinite(sums).all() and sums[2 * C] == R and (r <= 1 if nblk > 1 else _same(sums[:2 * C], p64.reshape(-1)))
    # sph3d_elu_bn_forward_partials: the statistics of these sums, and out at them
    d = N.inputs(R, C)
    mm, mv = np.linspace(-0.5, 3.0, C).astype(np.float32), np.linspace(0.0, 2.0, C).astype(np.float32)
    b = dict(out=Buf(dev, R * C), mean=Buf(dev, C), rstd=Buf(dev, C), moving_mean=Buf(dev, C, init=mm), moving_var=Buf(dev, C, init=mv))
    y, gamma, beta = (_dev(d[k], dev) for k in ("y", "gamma", "beta"))
    _lib.check(_lib.lib().sph3d_elu_bn_forward_partials(R, C, nblk, pt.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                         b["moving_mean"].ptr(), b["moving_var"].ptr(), MOMENTUM_ARG, EPS_ARG, b["out"].ptr(),
                                                         b["mean"].ptr(), b["rstd"].ptr(), _lib.stream_ptr()))
    assert all(v.intact() for v in b.values())
    got = {k: v.np() for k, v in b.items()}
    got["count"] = float(R)
    assert N.check_stats(got, sums, mm, mv) <= 1                               # (the same sums: both run sum_partials_32x8)
    want, bound = N.out_ref(d["y"], got["mean"], got["rstd"], d["gamma"], d["beta"])
    _within("forward_partials", got["out"].reshape(R, C), want, bound, C)


# ---- C: statistics from synthetic sums -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("R,count", [(1, 1), (8, 8), (8, 1000), (33, 2 ** 40)], ids=lambda v: str(v))
def test_statistics_from_sums(dev, R, count, C):
    """S2 / R < (S1 / R)^2 (the clamp: rstd == (float)(1 / sqrt((double)eps)) exactly), R = 1, a count beyond the local rows, a
    negative mean, moving statistics that start anywhere; C floats per output and not one more"""
    sums = N.synthetic_stats(R, C, count)
    mean = sums[:C] / count
    sums[C + 1] = (mean[1] ** 2 - 0.5) * count                                # channel 1 (mean -0.7): below the square of the mean
    sums[C + 2] = mean[2] ** 2 * count * (1 - 2.0 ** -40)                     # channel 2 (mean 3): below it by rounding noise
    mm = np.linspace(-2.0, 5.0, C).astype(np.float32)
    mv = np.linspace(0.3, 9.0, C).astype(np.float32)
    d = N.inputs(R, C)
    y, gamma, beta = (_dev(d[k], dev) for k in ("y", "gamma", "beta"))
    fw = fwd_apply(dev, R, C, sums, y, gamma, beta, mm, mv)
    r = N.check_stats(fw, sums, mm, mv)
    clamp = np.float32(1.0 / np.sqrt(np.float64(N.EPS)))
    assert fw["rstd"][1] == clamp and fw["rstd"][2] == clamp and fw["rstd"][0] == clamp and fw["count"] == count and fw["mean"][1] < 0
    assert _same(fw["moving_var"][1:3], ((1.0 - np.float64(N.MOM)) * mv[1:3].astype(np.float64)).astype(np.float32))
    want, bound = N.out_ref(d["y"], fw["mean"], fw["rstd"], d["gamma"], d["beta"])
    _within("apply forward", fw["out"], want, bound, C)
    print("R=%d count=%d C=%d: statistics %.3f of one float32 rounding" % (R, count, C, r))
    assert r <= 1


# ---- the Python wrappers refuse a per-channel operand they cannot pass on as it is ----------------------------------------------
def test_wrappers_refuse_bad_per_channel_operands_before_any_launch(dev):
    R, C = 33, 12
    d = N.inputs(R, C)
    y, dout, gamma, beta = (_dev(d[k], dev) for k in ("y", "dout", "gamma", "beta"))
    mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    sums = tf_norm.elu_bn_forward_sums(y)
    _out, mean, rstd, count = tf_norm.elu_bn_forward_apply(y, sums, gamma, beta, mm.clone(), mv.clone())
    _dg, _db, s2 = tf_norm.elu_bn_backward_sums(y, dout, mean, rstd)
    partial = torch.zeros(2, 2, C, device=dev)
    short, wide = gamma[:C - 4].clone(), beta.double()
    strided = torch.ones(2 * C, device=dev)[::2]
    column = rstd.reshape(C, 1)
    assert short.shape == (C - 4,) and wide.dtype == torch.float64 and not strided.is_contiguous() and column.shape == (C, 1)
    bad = [
        ("a [C-4] gamma", lambda: tf_norm.elu_batch_norm(y, short, beta, mm, mv, True)),
        ("a [C-4] gamma, inference", lambda: tf_norm.elu_batch_norm(y, short, beta, mm, mv, False)),
        ("a float64 beta", lambda: tf_norm.elu_batch_norm(y, gamma, wide, mm, mv, True)),
        ("a strided moving_var", lambda: tf_norm.elu_batch_norm(y, gamma, beta, mm, strided, True)),
        ("a float64 moving_mean", lambda: tf_norm.elu_batch_norm(y, gamma, beta, mm.double(), mv, True)),
        ("a [C,1] save_rstd", lambda: tf_norm._bwd_impl(y, dout, gamma, mean, column, True)),
        ("a [C-4] gamma in the gradient", lambda: tf_norm._bwd_impl(y, dout, short, mean, rstd, True)),
        ("forward_apply: a float64 beta", lambda: tf_norm.elu_bn_forward_apply(y, sums, gamma, wide, mm, mv)),
        ("forward_apply: a strided moving_var", lambda: tf_norm.elu_bn_forward_apply(y, sums, gamma, beta, mm, strided)),
        ("backward_sums: a [C,1] save_rstd", lambda: tf_norm.elu_bn_backward_sums(y, dout, mean, column)),
        ("backward_sums: a [C-4] save_mean", lambda: tf_norm.elu_bn_backward_sums(y, dout, mean[:C - 4].clone(), rstd)),
        ("backward_apply: a [C,1] save_rstd", lambda: tf_norm.elu_bn_backward_apply(y, dout, gamma, mean, column, s2, count)),
        ("backward_apply: a [C-4] gamma", lambda: tf_norm.elu_bn_backward_apply(y, dout, short, mean, rstd, s2, count)),
        ("partials: a [C-4] gamma", lambda: tf_norm._elu_bn_partials_impl(y, partial, short, beta, mm, mv)),
        ("partials: a strided moving_var", lambda: tf_norm._elu_bn_partials_impl(y, partial, gamma, beta, mm, strided)),
    ]
    before = (mm.clone(), mv.clone())
    for what, call in bad:
        _lib.timing_start()
        try:
            with pytest.raises(ValueError, match="contiguous float32"):
                call()
        finally:
            names = [n for n, *_ in _lib.timing_stop()]
        assert names == [], "%s: launched %s" % (what, names)
    assert torch.equal(mm, before[0]) and torch.equal(mv, before[1])
    # and the operands as they should be still pass
    _lib.timing_start()
    tf_norm.elu_batch_norm(y, gamma, beta, mm, mv, True)
    assert [n for n, *_ in _lib.timing_stop()] == ["sph3d_elu_bn_forward"]
    _host.clear()
