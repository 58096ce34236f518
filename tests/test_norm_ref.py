"""The ELU + batch-norm tail held on the host (tests/_norm_ref.py): the library's workspace query against the restated launch
arithmetic; every launch form of FORM_CASES reached by exactly the case that claims it; the float64 statement against autograd on
batch_norm(elu(y)) in float64, training and inference; the float32 restatement of every kernel inside the bounds that
tests/test_gpu_norm_forms.py applies to the kernels; and every mutation of the restatement (a dropped row, a clamped row counted
again, a stale partial of an empty block, a channel group that is not wrapped or wrapped a trip late) OUTSIDE at least one of
them, which is what keeps the bounds from being so loose that they would hide one.  No device is touched.

Measured here (numpy's float32 exp for __expf), worst over the cases, in units of the bound: forward sums 0.34 / 0.42, statistics
0.99, apply forward 0.99, backward sums 0.33 / 0.32, apply backward 0.60, end to end mean 0.34, rstd 0.33, out 0.29 (statistics and
apply reach 1 by construction: where the other terms vanish, the bound is the final float32 rounding itself).  The weakest break
of a mutation: 27 units (one stale partial of 1024 in the sum of dout zhat at (349527, 12)); a dropped row is 4000 units and more."""
import numpy as np
import pytest

import _norm_ref as N

_cache = {}


def _case(R, C):
    """operands, form and the float32 restatement's forward half, once per shape (read-only afterwards)"""
    if (R, C) not in _cache:
        _cache.clear()                                        # (one shape at a time: the largest holds 8.4 M elements)
        d = N.inputs(R, C)
        d["form"] = N.case_form(R, C)
        d["mm"], d["mv"] = np.full(C, 0.1, np.float32), np.full(C, 0.7, np.float32)
        _cache[(R, C)] = d
    return _cache[(R, C)]


def test_workspace_query_and_the_issues_figures():
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    for R in (1, 2, 31, 32, 33, 64, 1000, 4100, 32767, 32768, 32769, 349527, 700000, 2 ** 22):
        for C in (4, 12, 36, 192, 400, 516, 1020, 1024):
            assert l.sph3d_elu_bn_workspace(R, C) == N.workspace_bytes(R, C), (R, C)
            f = N.case_form(R, C)
            # the blocks cover the rows exactly; the threads of a workgroup cover a row's channel groups
            assert (f["used"] - 1) * f["rows_per_block"] < R <= f["used"] * f["rows_per_block"] and 1 <= f["last_rows"] <= f["rows_per_block"]
            assert f["cg"] * f["rows_per_iter"] + f["idle_threads"] == 256 and f["chain"] * f["rows_per_iter"] >= f["rows_per_block"]
            assert (f["trips"] - 1) * f["stride"] + f["last_trip"] == f["total4"] == R * C // 4
    tab = {4: (1, 256, 0), 12: (3, 85, 1), 400: (100, 2, 56), 516: (129, 1, 127), 1020: (255, 1, 1), 1024: (256, 1, 0)}
    for C, want in tab.items():
        f = N.reduce_form(1000, C)
        assert (f["cg"], f["rows_per_iter"], f["idle_threads"]) == want
    f = N.reduce_form(32769, 4)
    assert (f["nblk"], f["rows_per_block"], f["used"], f["empty"]) == (1024, 33, 993, 31)
    assert N.finalize_form(1500, 36) == dict(fin_trips=6, fin_idle_py=0, fin_ragged=True, fin_idle_lanes=28)
    assert N.finalize_form(1, 4)["fin_idle_py"] == 31 and not N.finalize_form(256, 1024)["fin_ragged"]


def test_every_form_is_reached_by_exactly_the_case_that_claims_it():
    assert [c[0] for c in N.FORM_CASES] == list(N.FORMS), "one case per form, in the forms' order"
    for name, pred in N.FORMS.items():
        hit = [c[0] for c in N.FORM_CASES if pred(N.case_form(c[1], c[2]))]
        assert hit == [name], (name, hit)
    assert all(N.supported(c[1], c[2]) for c in N.FORM_CASES)


def test_the_cases_are_those_of_the_issue():
    shapes = [c[1:] for c in N.FORM_CASES]
    assert shapes == [(1, 4), (2, 1024), (31, 12), (33, 12), (64, 4), (777, 400), (4100, 516), (1000, 1020), (32769, 4), (32769, 12),
                      (22000, 192), (10500, 400), (700000, 12), (349527, 12), (20000, 512)]
    # (the new shapes end at 8.4 M floats; (20000, 512), kept from tests/test_gpu_parity.py, holds 10.24 M)
    assert sorted(R * C for R, C in shapes)[-2:] == [8400000, 10240000] and [c[1:] for c in N.APPLY_CASES] == shapes[10:]
    f = N.case_form(700000, 12)
    assert (f["trips"], f["cstep"], f["chain"], f["fin_trips"]) == (3, 1, 9, 4)
    assert N.case_form(10500, 400)["cstep"] == 76 and N.case_form(22000, 192)["cstep"] == 16 and N.case_form(777, 400)["cstep"] == 24


def test_inputs_hold_what_the_cases_promise():
    import _sep_ref
    assert N.ELU_MEASURED == _sep_ref.ELU_MEASURED <= _sep_ref.E_ELU <= N.E_UNITS          # the record, under the derived E
    for _, R, C in N.SMALL_CASES:
        d = N.inputs(R, C, big=True)
        y, dout = d["y"], d["dout"]
        assert y.dtype == dout.dtype == d["gamma"].dtype == d["beta"].dtype == np.float32 and y.shape == dout.shape == (R, C)
        k = min(R, len(N.EDGE))
        assert np.array_equal(y[:k, 0].view(np.int32), N.EDGE[:k].view(np.int32))
        assert not dout[:, 2].any() and (dout[:, 3] >= 0).all() and y[0, 1] == N.BIG and (R == 1 or y[R - 1, 1] == -N.BIG)
        if R >= 31 and C >= 12:
            assert (y[:, 5] == np.float32(0.1)).all() and abs(y[:, 3].mean() - 30) < 1 and y[:, 4].std() < 0.02
            assert {0.0, -1.0, 1.5} <= set(d["gamma"].tolist())
    assert (N.EDGE[4:6] != 0).all() and (np.abs(N.EDGE[4:6]) < 2.0 ** -126).all()              # +-1e-40: float32 subnormals


@pytest.mark.parametrize("training", [True, False], ids=["training", "inference"])
def test_statement_equals_autograd_in_float64(training):
    import torch
    import torch.nn.functional as F
    for _, R, C in N.SMALL_CASES[1:8]:
        d = N.inputs(R, C)
        mm = np.linspace(-0.5, 3.0, C).astype(np.float32)
        mv = np.linspace(0.0, 2.0, C).astype(np.float32)
        st = N.statement(d["y"], d["dout"], d["gamma"], d["beta"], mm, mv, training)
        y = torch.from_numpy(d["y"]).double().requires_grad_(True)
        ga, be = (torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("gamma", "beta"))
        rm, rv = torch.from_numpy(mm).double(), torch.from_numpy(mv).double()
        z = F.elu(y)
        out = F.batch_norm(z, rm, rv, ga, be, training, 0.01, float(N.EPS))
        out.backward(torch.from_numpy(d["dout"]).double())
        for got, want in ((st["out"], out.detach()), (st["dy"], y.grad), (st["dgamma"], ga.grad), (st["dbeta"], be.grad)):
            want = want.numpy()
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(want).max())))
        if training:
            zd = z.detach()
            mom = float(N.MOM)
            np.testing.assert_allclose(st["moving_mean"], (1 - mom) * mm.astype(np.float64) + mom * zd.mean(0).numpy(), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(st["moving_var"], (1 - mom) * mv.astype(np.float64) + mom * zd.var(0, unbiased=False).numpy(),
                                       rtol=1e-12, atol=1e-15)
        else:
            assert np.array_equal(st["moving_mean"], mm) and np.array_equal(st["moving_var"], mv) and not st["c0"].any() and not st["c1"].any()


def _ratios(d, mutate=None):
    """the restatement's pipeline on one case -> {stage: worst |error| / bound}; a reduce mutation enters both reduce passes, an
    apply mutation both apply passes"""
    f, y, dout, gamma, beta = d["form"], d["y"], d["dout"], d["gamma"], d["beta"]
    rm = mutate if mutate in N.REDUCE_MUTATIONS else None
    am = mutate if mutate in N.APPLY_MUTATIONS else None
    r = {}
    sums = N.fwd_sums_f32(f, y, rm)
    r["forward sum z"], r["forward sum z^2"] = N.check_fwd_sums(sums, y, f)
    st = N.stats_f32(sums, d["mm"], d["mv"])
    r["statistics from sums"] = N.check_stats(st, sums, d["mm"], d["mv"])
    out = N.apply_fwd_f32(f, y, st["mean"], st["rstd"], gamma, beta, am)
    want, bound = N.out_ref(y, st["mean"], st["rstd"], gamma, beta)
    r["apply forward"] = N.worst(out, want, bound)
    part = N.reduce_f32(f, y, dout, st["mean"], st["rstd"], rm)
    s2 = N.sum_partials(part).reshape(-1)
    r["backward sum dout"], r["backward sum dout zhat"] = N.check_bwd_sums(s2[y.shape[1]:].astype(np.float32), s2[:y.shape[1]].astype(np.float32),
                                                                          s2, y, dout, st["mean"], st["rstd"], f)
    c0, c1 = N.coef32(s2, st["count"])
    dy = N.apply_bwd_f32(f, y, dout, gamma, st["mean"], st["rstd"], c0, c1, am)
    want, bound = N.dy_ref(y, dout, gamma, st["mean"], st["rstd"], c0, c1)
    r["apply backward"] = N.worst(dy, want, bound)
    assert not dy[y <= -88].any()                                             # exactly zero, as the code guarantees
    if mutate is None:
        ref = N.statement(y, dout, gamma, beta, d["mm"], d["mv"])
        e = N.e2e_bounds(y, gamma, f, ref)
        r["end to end mean"] = N.worst(st["mean"], ref["mean"], e["dmean"])
        r["end to end rstd"] = N.worst(st["rstd"], ref["rstd"], e["drstd"])
        r["end to end out"] = N.worst(out, ref["out"], bound_out(y, st, gamma, beta) + e["out_extra"])
    return r


def bound_out(y, st, gamma, beta):
    return N.out_ref(y, st["mean"], st["rstd"], gamma, beta)[1]


@pytest.mark.parametrize("case", N.FORM_CASES, ids=N.case_id)
def test_float32_restatement_stays_inside_every_bound(case):
    """the kernels' operation order in float32 numpy against the float64 statement under the very bounds of the GPU test: this
    entitles those bounds to be used on the kernels"""
    _, R, C = case
    r = _ratios(_case(R, C))
    print("R=%d C=%d: float32 restatement, worst ratio %.3f  (%s)" % (R, C, max(r.values()), ", ".join("%s %.3f" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, r


MUTATION_OWNERS = {
    N.REDUCE_MUTATIONS[0]: [(33, 12), (4100, 516), (64, 4)],
    N.REDUCE_MUTATIONS[1]: [(2, 1024), (31, 12), (33, 12), (777, 400)],
    N.REDUCE_MUTATIONS[2]: [(32769, 4), (32769, 12), (349527, 12)],
}
APPLY_OWNERS = [(22000, 192), (10500, 400), (700000, 12), (349527, 12)]          # every multi-trip case whose cstep is not 0


def _stats(d):
    """float32 statistics for the passes after the cut: the float64 sums' (the bounds there hold at any float32 statistics)"""
    ref = N.fwd_sums_ref(d["y"])
    return N.stats_f32(np.concatenate([ref["S1"], ref["S2"], [float(d["y"].shape[0])]]), d["mm"], d["mv"])


@pytest.mark.parametrize("mutation", list(MUTATION_OWNERS))
def test_every_reduce_mutation_breaks_a_bound(mutation):
    """on every case that owns the mutated form: a bound that let one of these through would be no check of the kernel"""
    for R, C in MUTATION_OWNERS[mutation]:
        d = _case(R, C)
        f, y = d["form"], d["y"]
        sums = N.fwd_sums_f32(f, y, mutation)
        r = dict(zip(("forward sum z", "forward sum z^2"), N.check_fwd_sums(sums, y, f)))
        clean = _stats(d)
        s2 = N.sum_partials(N.reduce_f32(f, y, d["dout"], clean["mean"], clean["rstd"], mutation)).reshape(-1)
        r["backward sum dout"], r["backward sum dout zhat"] = N.check_bwd_sums(s2[C:].astype(np.float32), s2[:C].astype(np.float32), s2, y,
                                                                              d["dout"], clean["mean"], clean["rstd"], f)
        print("R=%d C=%d, %s: breaks %s" % (R, C, mutation, ", ".join("%s (%.3g)" % kv for kv in r.items() if kv[1] > 1)))
        assert min(r.values()) > 1, (R, C, r)


@pytest.mark.parametrize("shape", APPLY_OWNERS, ids=lambda s: "R%d-C%d" % s)
def test_every_apply_mutation_breaks_a_bound(shape):
    R, C = shape
    d = _case(R, C)
    f, y = d["form"], d["y"]
    assert f["trips"] >= 2 and f["cstep"] != 0
    st = _stats(d)
    c0, c1 = np.full(C, 0.01, np.float32), np.full(C, -0.02, np.float32)
    want, bound = N.out_ref(y, st["mean"], st["rstd"], d["gamma"], d["beta"])
    wdy, bdy = N.dy_ref(y, d["dout"], d["gamma"], st["mean"], st["rstd"], c0, c1)
    for mutation in N.APPLY_MUTATIONS:
        out = N.apply_fwd_f32(f, y, st["mean"], st["rstd"], d["gamma"], d["beta"], mutation)
        dy = N.apply_bwd_f32(f, y, d["dout"], d["gamma"], st["mean"], st["rstd"], c0, c1, mutation)
        r = {"apply forward": N.worst(out, want, bound), "apply backward": N.worst(dy, wdy, bdy)}
        where = N.first_bad(out, want, bound, C)
        print("R=%d C=%d, %s: breaks %s" % (R, C, mutation, ", ".join("%s (%.3g)" % kv for kv in r.items() if kv[1] > 1)))
        assert min(r.values()) > 1 and where is not None, (R, C, mutation, r)
        # the slip is named where it begins: in the second trip, at or just after the first float4 whose channel group differs
        first4 = int(np.flatnonzero(N.channel_of(f, C, mutation) != N.channel_of(f, C))[0])
        assert f["stride"] <= first4 <= where[0] // 4 < first4 + C and "float4 %d)" % (where[0] // 4) in where[1], (first4, where)
    _cache.clear()
