"""tests/_sep_ref.py and tests/_sep_forms.py proved on the CPU: the case lists of tests/test_gpu_sep_forms.py name every reachable
launch form and every situation they are meant for (computed from the restated rules alone), the float64 statement of the
separable layer agrees with the fp32 C oracle followed by a float64 product, an fp32 numpy emulation of the kernels' order of
operations passes the derived bounds, and the same emulation with one defect each fails them."""
import numpy as np
import pytest

import oracle
from _errors import assert_per_element
from _sep_forms import (ALL_CASES, EDGE_CASES, GENERAL_INSTS, GENERAL_LDS_CASES, K130_CASES, PARTITION_CASES, RING_REUSE_CASES, TRIPLES,
                        UNREACHED_TRIPLES, Case, form_of, partition, reachable_triples, sr_ring_depth, sr_shape_ok, sc_shape_ok)
from _sep_ref import E_ELU, ELU_MEASURED, check_infer, check_train, make_inputs


# ---- the case lists name every form and every situation -------------------------------------------------------------------------------
def test_every_launch_form_has_a_gpu_case():
    assert reachable_triples() == TRIPLES
    assert sorted(list(TRIPLES) + UNREACHED_TRIPLES) == sorted((R, lpe, kt) for R in (1, 2) for lpe in (16, 32) for kt in (4, 8, 16))
    forms = [(c, form_of(c)) for c in ALL_CASES]
    assert all(f["tag"] == c.tag and f["kernel"] not in ("unsupported", "empty") for c, f in forms)

    def insts(kernel):
        return {f["inst"] for c, f in forms if f["kernel"] == kernel}
    assert insts("ring") == insts("train") == insts("small") == set(TRIPLES) and len(TRIPLES) == 5
    assert insts("general") == set(GENERAL_INSTS) and len(GENERAL_INSTS) == 12
    # the smallest and the largest C of every ring / small form, and the Cout the issue names
    for kernel, couts in (("ring", {16, 64, 256}), ("train", {16, 64, 256}), ("small", {48, 96, 112})):
        for t, (lo, hi, r) in TRIPLES.items():
            mine = [c for c, f in forms if f["kernel"] == kernel and f["inst"] == t]
            assert {lo, hi} <= {c.C for c in mine} and couts <= {c.Cout for c in mine}
    assert {144, 272, 512} <= {c.Cout for c, f in forms if f["kernel"] == "general"}
    assert any(f["kernel"] == "general" and c.C == 256 and c.Cout == 16 for c, f in forms)
    # the small kernel is reached only where the ring does not cover the shape
    assert all(not sr_shape_ok(c.N, c.F, c.C, c.r, c.K, c.Cout) for c, f in forms if f["kernel"] == "small")


def test_the_case_lists_hold_every_situation():
    forms = [(c, form_of(c)) for c in ALL_CASES]

    def some(pred):
        return any(pred(c, f) for c, f in forms)
    # ring slot reuse: three slots, seven row blocks, epochs 0..2; G = 16 > NB and G = 1; inference and training; affine or not
    for kind in ("ring", "train"):
        for G in (16, 1):
            for affine in (False, True):
                assert some(lambda c, f: f["kernel"] == kind and f["inst"] == (2, 32, 16) and f["NB"] == 3 and f["nrb_max"] == 7
                            and f["wrap"] == 2 and f["G"] == G and f["affine"] == affine and c.F == 100 and c.C == 68 and c.K == 8
                            and c.B * c.M == 28672)
        assert some(lambda c, f: f["kernel"] == kind and f["NB"] == 8 and f["wrap"] >= 1 and c.B * c.M >= 40960)
    assert all(form_of(c)["wrap"] >= 1 for c in RING_REUSE_CASES)
    # the general kernel: tile heights by point count for both LPE, lowered by LDS, slices, partial slices, 17 column blocks
    for lpe in (16, 32):
        for rbk in (1, 2, 4):
            assert some(lambda c, f: f["kernel"] == "general" and f["inst"][1:] == (lpe, rbk) and f["rbk_by_points"] == rbk)
    assert [(form_of(c)["rbk_by_points"], form_of(c)["rbk"]) for c in GENERAL_LDS_CASES] == [(4, 2), (4, 1)]
    assert all(sr_ring_depth(c.F, c.C, c.r) < 3 and not sc_shape_ok(c.N, c.F, c.C, c.r, c.K, c.Cout) and c.Cout in (16, 32, 64, 128, 256)
               and sr_shape_ok(c.N, 110, c.C, c.r, c.K, c.Cout) for c in GENERAL_LDS_CASES)          # the step from ring to general
    assert some(lambda c, f: f.get("nslices") == 2 and c.C == 256) and some(lambda c, f: f.get("nslices") == 3 and c.C == 384)
    assert some(lambda c, f: f.get("partial_slice") and (c.C, c.r, c.Cout) == (100, 1, 144))
    assert some(lambda c, f: f.get("partial_slice") and (c.C, c.r, c.Cout) == (36, 2, 144))
    assert some(lambda c, f: f.get("ncb") == 17)
    # the partition
    for kernel in ("ring", "train", "small", "general"):
        assert {1, 3, 8, 9, 16} <= {c.B for c, f in forms if f["kernel"] == kernel and c in PARTITION_CASES}
        assert some(lambda c, f: f["kernel"] == kernel and f["idle"] > 0) and some(lambda c, f: f["kernel"] == kernel and f["idle"] == 0)
    assert some(lambda c, f: f["kernel"] == "ring" and f["units"] == 3) and some(lambda c, f: f["kernel"] == "train" and f["units"] == 3)
    assert some(lambda c, f: f["kernel"] == "train" and f["idle"] == 253)                  # all-zero partial rows of idle workgroups
    # counts above 64, and one form per kernel for the bad bin ids and the non-finite input
    for cases in (K130_CASES, EDGE_CASES):
        assert {form_of(c)["kernel"] for c in cases} == {"ring", "train", "small", "general"}
    assert all(c.K == 130 for c in K130_CASES)
    # shapes: every case has M < N; the small-shape cases' M is no multiple of 16
    assert all(c.M < c.N for c in ALL_CASES)


def test_partition_covers_every_unit_once():
    for B, per_cloud in ((1, 3), (3, 7), (7, 256), (8, 5), (8, 224), (9, 17), (16, 38), (0, 5), (3, 0)):
        units = [u for wg in partition(B, per_cloud) for u in wg]
        assert sorted(units) == [(b, j) for b in range(B) for j in range(per_cloud)]
        if B % 8 == 0:                                                        # a workgroup of XCD x takes clouds b = x (mod 8) only
            assert all(b % 8 == blk % 8 for blk, wg in enumerate(partition(B, per_cloud)) for b, _ in wg)


def test_the_elu_constant_is_the_measured_one():
    assert E_ELU == int(np.ceil(ELU_MEASURED)) + 1 and E_ELU <= 4


# ---- the statement against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 96, 50, 17, 8, 2, 19, 32), (3, 60, 60, 33, 12, 1, 7, 48)], ids=["inter", "intra"])
def test_statement_equals_the_oracle_and_a_float64_product(shape):
    d = make_inputs(*shape)
    ref = d["ref"]
    d_o = oracle.depthwise_conv3d(d["x"], d["w_dw"], d["idx"], d["cnt"], d["bins"])
    assert_per_element(d_o, ref.d, ref.magd, "oracle depthwise")
    y_o = d_o.astype(np.float64).reshape(-1, ref.CR) @ d["W"].astype(np.float64) + d["bias"].astype(np.float64)
    y, MAG, _ = ref.pre(d["bias"])
    assert (np.abs(y_o.reshape(y.shape) - y) <= 1e-5 * MAG).all()
    z_o = np.where(y_o > 0, y_o, np.expm1(np.minimum(y_o, 0))) * d["scale"].astype(np.float64) + d["shift"].astype(np.float64)
    z, bound = ref.tail(d["bias"], True, d["scale"], d["shift"])
    assert (np.abs(z_o.reshape(z.shape) - z) <= 1e-5 * np.abs(d["scale"]) * MAG + 1e-12).all() and (bound > 0).all()


# ---- an fp32 emulation of the kernels' order of operations -----------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf: the product of two fp32 is exact in float64; one rounding to fp32 (the sum's own float64 rounding is 2^-29 of that)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _elu32(y):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(y > 0, y, np.exp(np.minimum(y, np.float32(0))).astype(np.float32) - np.float32(1)).astype(np.float32)


def gather32(d, lpe, max_edges=None):
    """the split gather chain: slot k of a 64-slot chunk belongs to lane group k mod EPL, each group one fmaf chain over its slots in
    order, the groups added by `acc += __shfl_xor(acc, o)`, o = LPE .. 32, then `* (1.0f / cnt)` -> A [B, M, C r]"""
    x, w, idx, cnt, bins = d["x"], d["w_dw"], d["idx"], d["cnt"], d["bins"]
    (B, M, K), (F, C, r), EPL = idx.shape, w.shape, 64 // lpe
    acc = np.zeros((EPL, B, M, C * r), np.float32)
    for b in range(B):
        top = int(cnt[b].max()) if M else 0
        for k in range(top if max_edges is None else min(top, max_edges)):
            sel = np.nonzero(cnt[b] > k)[0]
            g = (k % 64) % EPL
            f = np.clip(bins[b, sel, k], 0, F - 1)
            xs = np.repeat(x[b][idx[b, sel, k]], r, axis=1)
            acc[g, b, sel] = _fma(xs, w[f].reshape(sel.size, C * r), acc[g, b, sel])
    s = (acc[0] + acc[1]) + (acc[2] + acc[3]) if EPL == 4 else acc[0] + acc[1]
    inv = np.where(cnt > 0, np.float32(1) / np.maximum(cnt, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return (s * inv[:, :, None]).astype(np.float32)


def product32(A, W, bias, form, pad_term=False, no_bias_in_last_block=False):
    """ring and small kernel: four chains, chain u over k = 16 t + 4 kq + u in (t, kq) order, combined as (d0 + d1) + (d2 + d3);
    general kernel: one chain over the slices, inside a slice in (t, u, kq) order; then `+ bias`"""
    B, M, CR = A.shape
    Cout, A2 = W.shape[1], A.reshape(B * M, CR)
    R, lpe = form["inst"][0], form["inst"][1]
    if form["kernel"] == "general":
        y = np.zeros((B * M, Cout), np.float32)
        KP = 4 * lpe * R
        for s in range(form["nslices"]):
            for t in range(KP // 16):
                for u in range(4):
                    for kq in range(4):
                        k = s * KP + 16 * t + 4 * kq + u
                        if k < CR:
                            y = _fma(A2[:, k:k + 1], W[k:k + 1], y)
    else:
        ch = [np.zeros((B * M, Cout), np.float32) for _ in range(4)]
        for t in range(form["inst"][2]):
            for kq in range(4):
                for u in range(4):
                    k = 16 * t + 4 * kq + u
                    if k < CR:
                        ch[u] = _fma(A2[:, k:k + 1], W[k:k + 1], ch[u])
                    elif pad_term and k == CR:                 # DEFECT: the first padding column holds 1.0 and meets a W row
                        ch[u] = _fma(np.float32(1), W[CR - 1:CR], ch[u])
        y = (ch[0] + ch[1]) + (ch[2] + ch[3])
    if bias is not None:
        yb = (y + bias).astype(np.float32)
        if no_bias_in_last_block:                              # DEFECT
            yb[:, -16:] = y[:, -16:]
        y = yb
    return y.reshape(B, M, Cout)


def tail32(y, act, scale, shift):
    z = _elu32(y) if act else y
    if scale is None and shift is None:
        return z
    return _fma(z, np.float32(1) if scale is None else scale, np.float32(0) if shift is None else shift)


def partials32(y, form, idle_rows_written=True):
    """the training kernel's partial rows [256 G, 2, Cout]: lane (kq, column) of wave group grp adds rows 4 kq + r4 of the row blocks
    jl = grp (mod G) of its workgroup in turn (`sz += z; sq = fmaf(z, z, sq)`), the four kq are folded as (0 + 1) + (2 + 3)"""
    B, M, Cout = y.shape
    G = form["G"]
    out = np.full((256 * G, 2, Cout), np.nan, np.float32)               # as the caller's NaN fill leaves it
    z = _elu32(y)
    for blk, units in enumerate(partition(B, (M + 15) // 16)):
        if not units and not idle_rows_written:                         # DEFECT
            continue
        for grp in range(G):
            sz, sq = np.zeros((4, Cout), np.float32), np.zeros((4, Cout), np.float32)
            for b, rbi in units[grp::G]:
                for r4 in range(4):
                    for kq in range(4):
                        m = 16 * rbi + 4 * kq + r4
                        if m < M:
                            sz[kq] = sz[kq] + z[b, m]
                            sq[kq] = _fma(z[b, m], z[b, m], sq[kq])
            out[blk * G + grp, 0] = (sz[0] + sz[1]) + (sz[2] + sz[3])
            out[blk * G + grp, 1] = (sq[0] + sq[1]) + (sq[2] + sq[3])
    return out


def late_slot(A, form):
    """DEFECT: a ring slot read one epoch late — local row block jl >= NB of a workgroup is multiplied with the 16 rows block jl - NB
    left in the slot"""
    B, M, _ = A.shape
    out, hit = A.copy(), 0
    for units in partition(B, (M + 15) // 16):
        for jl in range(form["NB"], len(units)):
            (b, rbi), (b0, rbi0) = units[jl], units[jl - form["NB"]]
            n = min(16, M - 16 * rbi)
            rows = np.zeros((16, A.shape[2]), np.float32)
            rows[:min(16, M - 16 * rbi0)] = A[b0, 16 * rbi0:16 * rbi0 + 16]
            out[b, 16 * rbi:16 * rbi + n] = rows[:n]
            hit += 1
    return out, hit


EMU = {"ring": Case("infer", 3, 150, 107, 33, 36, 2, 12, 64, None), "train": Case("train", 3, 150, 107, 33, 36, 2, 12, 64, None),
       "small": Case("infer", 3, 150, 107, 33, 64, 1, 12, 80, None), "general": Case("infer", 3, 150, 107, 33, 100, 2, 12, 272, None),
       "slices": Case("infer", 2, 90, 37, 9, 256, 1, 6, 16, None), "K130": Case("infer", 2, 160, 43, 33, 32, 2, 130, 96, None),
       "affine": Case("train", 8, 99, 75, 33, 16, 2, 12, 32, None),
       "wrap": Case("infer", 8, 1664, 1600, 100, 68, 2, 8, 16, None), "wrap-train": Case("train", 8, 1664, 1600, 100, 68, 2, 8, 16, None)}
_cache = {}


def _emu(name):
    """-> (case, form, inputs, A): computed once per case, never changed"""
    if name not in _cache:
        c = EMU[name]
        d = _cache[c[1:9]][2] if c[1:9] in _cache else make_inputs(*c[1:9])
        form = form_of(c)
        _cache[name] = _cache[c[1:9]] = (c, form, d, gather32(d, form["inst"][1]))
    return _cache[name]


def _check(name, A=None, out_edit=None, **defect):
    c, form, d, A0 = _emu(name)
    A = A0 if A is None else A
    what = "emulated [%s] %s" % (form["tag"], name)
    prod = {k: v for k, v in defect.items() if k in ("pad_term", "no_bias_in_last_block")}
    if c.kind == "infer":
        used = []
        for tail, (with_bias, act, bn) in (("none", (0, 0, 0)), ("bias", (1, 0, 0)), ("bias+elu+bn", (1, 1, 1))):
            y = product32(A, d["W"], d["bias"] if with_bias else None, form, **prod)
            out = tail32(y, act, d["scale"] if bn else None, d["shift"] if bn else None)
            out = out if out_edit is None else out_edit(out)
            used.append(check_infer(out, d["ref"], tail, d["bias"], d["scale"], d["shift"], what))
        return max(used)
    y = product32(A, d["W"], d["bias"], form, **prod)
    y = y if out_edit is None else out_edit(y)
    partial = partials32(y, form, idle_rows_written=not defect.get("idle_rows_unwritten", False))
    return check_train(A if out_edit is None else out_edit(A), y, partial, d["ref"], d["bias"], form, what)


@pytest.mark.parametrize("name", list(EMU))
def test_the_emulations_pass_without_a_defect(name):
    c, form, d, A = _emu(name)
    assert form["kernel"] == {"slices": "general", "K130": "small", "affine": "train", "wrap": "ring", "wrap-train": "train"}.get(name, name)
    used = _check(name)
    print("%s: used %.3f of the derived bounds at most" % (name, used))
    assert used <= 1.0


def test_a_ring_slot_read_one_epoch_late_is_caught():
    for name in ("wrap", "wrap-train"):
        c, form, d, A = _emu(name)
        assert form["NB"] == 3 and form["nrb_max"] == 4 and form["wrap"] == 1
        bad, hit = late_slot(A, form)
        assert hit >= 1
        with pytest.raises(AssertionError, match="per-element error|derived bound|exactly 0"):
            _check(name, A=bad)


def test_a_non_zero_k_padding_column_is_caught():
    c, form, d, A = _emu("ring")
    assert c.C * c.r == 72 and form["inst"][2] * 16 == 128
    with pytest.raises(AssertionError):
        _check("ring", pad_term=True)


def test_a_bias_dropped_in_the_last_column_block_is_caught():
    for name in ("ring", "train", "small"):
        with pytest.raises(AssertionError):
            _check(name, no_bias_in_last_block=True)


def test_edges_after_the_64th_dropped_are_caught():
    c, form, d, A = _emu("K130")
    assert (d["cnt"] > 64).any()
    with pytest.raises(AssertionError):
        _check("K130", A=gather32(d, form["inst"][1], max_edges=64))


def test_unwritten_rows_of_the_ragged_row_block_are_caught():
    def ragged(out):
        out = out.copy()
        out[:, 16 * (out.shape[1] // 16):] = np.nan                      # what a skipped store leaves of the caller's NaN fill
        return out
    for name in ("ring", "train", "small", "general"):
        assert EMU[name].M % 16
        with pytest.raises(AssertionError, match="NaN"):
            _check(name, out_edit=ragged)


def test_a_cloud_taken_from_cl_instead_of_xcd_plus_8_cl_is_caught():
    c, form, d, A = _emu("affine")
    assert form["affine"] and c.B == 8

    def wrong_cloud(out):
        return out[np.arange(c.B) // 8]                                      # b = xcd + 8 cl -> cl
    with pytest.raises(AssertionError):
        _check("affine", out_edit=wrong_cloud)


def test_an_idle_workgroups_partial_row_left_as_it_was_is_caught():
    c, form, d, A = _emu("train")
    assert form["idle"] > 200
    with pytest.raises(AssertionError, match="partial statistics are NaN"):
        _check("train", idle_rows_unwritten=True)
