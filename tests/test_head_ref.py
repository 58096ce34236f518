"""The logits layer and the training loss, held on the host: the library's host-only queries (sph3d_pointwise_gemm_skinny_supported,
sph3d_pointwise_gemm_skinny_tn_workspace, sph3d_masked_softmax_xent_parts) against tests/_head_ref.py over a sweep; the float64 loss
statement against the framework's cross-entropy combined as s3dis_net.get_loss combines it; every launch form of FORM_CASES reached
by exactly the case that claims it; and the float32 restatement of the loss kernel inside the bounds that
tests/test_gpu_xent_forms.py applies to the kernel.  No device is touched."""
import numpy as np
import pytest

import _head_ref as H


def test_host_queries_equal_the_statements():
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    n = 0
    for R in (-1, 0, 1, 15, 16, 1000, 131072, 262231):
        for K1 in (-16, 0, 8, 16, 24, 48, 64, 112, 128, 144, 192, 240, 256, 272):
            for K2 in (-16, 0, 8, 16, 24, 64, 80, 128, 144, 192, 240, 256):
                for N in (-1, 0, 1, 5, 13, 15, 16, 17, 64):
                    assert l.sph3d_pointwise_gemm_skinny_supported(R, K1, K2, N) == int(H.skinny_supported(R, K1, K2, N)), (R, K1, K2, N)
                    if H.skinny_supported(R, K1, K2, N):
                        n += 1
                        assert l.sph3d_pointwise_gemm_skinny_tn_workspace(R, K1, K2, N) == H.skinny_tn_form(R, K1, K2)["slabs_bytes"]
                        # the slabs the launch writes fit the workspace, and no workgroup starts past the last row
                        f = H.skinny_tn_form(R, K1, K2)
                        assert 1 <= f["wgs"] <= H.K_SK_TN_WGS and f["rows_per_wg"] % 32 == 0 and 1 <= f["last_rows"] <= f["rows_per_wg"]
                        assert 4 * f["wgs"] * (K1 + K2) * 16 <= f["slabs_bytes"]
    assert n > 1000
    for N in list(range(1, 70)) + [1000, 1023, 1024, 1025, 2048, 2049, 4097, 16383, 16384, 16385, 16400, 40000, 65536, 2 ** 20 + 1]:
        f = H.xent_form(N)
        assert l.sph3d_masked_softmax_xent_parts(N) == f["S"], N
        assert (f["S"] - 1) * f["chunk"] < N <= f["S"] * f["chunk"] and 1 <= f["last_rows"] <= f["chunk"], (N, f)
    assert H.xent_form(40000) == dict(S=16, chunk=2500, trips=3, count_trips=40, last_rows=2500)


@pytest.mark.parametrize("kernel", ["nn", "tn", "xent"])
def test_every_form_is_reached_by_exactly_the_case_that_claims_it(kernel):
    cases, forms = H.FORM_CASES[kernel], H.FORMS[kernel]
    assert [c[0] for c in cases] == list(forms), "one case per form, in the forms' order"
    for name, pred in forms.items():
        hit = [c[0] for c in cases if pred(H.case_form(kernel, c[1:]), c[1:])]
        assert hit == [name], (name, hit)
    if kernel != "xent":
        for c in cases:
            assert H.skinny_supported(*c[1:5]), c


def test_the_cases_are_those_of_the_issue():
    """the shapes, spelled out once more and independently of FORMS"""
    nn = {c[1:] for c in H.FORM_CASES["nn"]}
    assert {(R, 16, 0, 1, 1) for R in (1, 15, 16, 17, 262144 + 87)} <= nn
    assert {(77, 128, 64, 5, 1), (200, 16, 192, 13, 1), (200, 192, 16, 13, 1), (130, 256, 0, 16, 1), (130, 128, 128, 15, 1),
            (130, 112, 128, 13, 1), (1000, 64, 0, 16, 1)} <= nn and any(c[4] == 0 for c in nn)
    # 16 + 240 and 240 + 16 start five groups of 64 channels: the layer refuses them, the widest such splits it accepts stand in
    assert {(200, 16, 240, 13), (200, 240, 16, 13)} <= set(H.REFUSED_GROUPS) and not any(H.skinny_supported(*s) for s in H.REFUSED_GROUPS)
    assert not any(H.skinny_supported(200, 16, K2, 13) for K2 in (208, 224, 240)) and not H.skinny_supported(200, 208, 16, 13)
    f = H.skinny_nn_form(262144 + 87, 16, 0, 1)
    assert (f["tiles"], f["wgs"], f["trips"]) == (16384 + 6, 2048, 3)
    tn = {c[1:] for c in H.FORM_CASES["tn"]}
    assert {(R, 16, 16, 13) for R in (1, 5, 31, 32, 33, 224, 256, 2049, 16384, 16385)} <= tn
    assert {c[1:3] for c in tn} >= {(16, 0), (256, 0), (128, 128), (112, 128), (64, 192), (48, 80)} and {c[3] for c in tn} == {1, 13, 16}
    assert max(H.skinny_tn_form(*c[:3])["slabs_bytes"] for c in tn) == 8 << 20
    xe = {c[2:] for c in H.FORM_CASES["xent"]}
    assert {(N, 13) for N in (1, 63, 1000, 1024, 1025, 16384, 16385, 40000)} | {(1025, C) for C in (1, 2, 13, 21, 64)} == xe
    assert {H.xent_form(N)["S"] for N, _ in xe} == {1, 2, 16} and {1024, 1025, 2500} <= {H.xent_form(N)["chunk"] for N, _ in xe}


def test_product_statements_and_exact_operands():
    a1, a2, w = H.int_operand(77, 48, 1), H.int_operand(77, 80, 2), H.int_operand(128, 13, 3)
    bias, dy = H.int_operand(1, 13, 4)[0], H.int_operand(77, 13, 5)
    for t in (a1, a2, w, dy):
        assert t.dtype == np.float32 and np.abs(t).max() == 4 and len({r.tobytes() for r in t}) == len(t) and len({c.tobytes() for c in t.T}) == t.shape[1]
    y, mag = H.skinny_ref(a1, a2, w, bias)
    cat = np.concatenate([a1, a2], 1).astype(np.float64)
    assert np.array_equal(y, cat @ w + bias) and np.array_equal(y.astype(np.float32), H.int_product(a1, a2, w, bias))
    assert np.array_equal(mag, np.abs(cat) @ np.abs(w) + np.abs(bias))
    dw, dmag = H.skinny_tn_ref(a1, a2, dy)
    assert np.array_equal(dw, cat.T @ dy) and np.array_equal(dw.astype(np.float32), H.int_product(a1, a2, dy, transpose=True))
    assert np.array_equal(H.skinny_ref(a1, None, w[:48], None)[0], a1.astype(np.float64) @ w[:48]) and (dmag >= np.abs(dw)).all()


def test_loss_statement_equals_the_framework_formula():
    import torch
    import torch.nn.functional as F
    from sph3d_gcn_amd.harness import s3dis_net
    for _, B, N, C in H.FORM_CASES["xent"][:5] + H.FORM_CASES["xent"][8:]:
        x, label, inner = H.xent_inputs(B, N, C)
        ref = H.xent_ref(x, label, inner)
        pred = torch.from_numpy(x).double().requires_grad_(True)
        mask = torch.from_numpy(np.nan_to_num(inner, nan=0.0))                 # (get_loss counts inner_label > 0: NaN does not)
        loss = s3dis_net.get_loss(pred, torch.from_numpy(label), None, mask)
        (grad,) = torch.autograd.grad(loss, pred)
        # and the same written out here: F.cross_entropy per point, mean over the inner points, sum over the blocks
        ce = F.cross_entropy(pred.detach().reshape(-1, C), torch.from_numpy(label).reshape(-1), reduction="none").reshape(B, N)
        m = (mask > 0).double()
        per = torch.where(m.sum(1) > 0, (ce * m).sum(1) / m.sum(1).clamp(min=1.0), torch.zeros(B, dtype=torch.float64))
        np.testing.assert_allclose(ref["loss_part"].sum(1), per.numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(ref["loss_part"].sum(), float(loss.detach()), rtol=1e-13)
        np.testing.assert_allclose(ref["dlogits"], grad.numpy(), rtol=1e-11, atol=1e-17)
        assert ref["cnt"][0] == 0 and ref["cnt"][1] == N and ref["cnt"][2] == min(N, 3 if N > 1024 else 2)
        assert not ref["loss_part"][0].any() and not ref["dlogits"][0].any()


def test_loss_inputs_hold_what_the_cases_promise():
    for _, B, N, C in H.FORM_CASES["xent"]:
        x, label, inner = H.xent_inputs(B, N, C)
        assert x.dtype == np.float32 and label.dtype == np.int64 and inner.dtype == np.float32
        assert not (inner[0] > 0).any() and (inner[1] > 0).all()
        assert sorted(set(np.flatnonzero(inner[2] > 0))) == sorted({0, min(1023, N - 1), N - 1})
        if N >= 63:
            assert np.isnan(inner[3]).any() and {0.0, 1.0, 2.5, -1.0} <= set(inner[3][~np.isnan(inner[3])])
            if C > 1:
                spread = x.max(-1) - x.min(-1)
                assert (spread == 0).any() and (spread > 70).any() and (x.max(-1) > 990).any() and (x.max(-1) < -990).any()


@pytest.mark.parametrize("case", H.FORM_CASES["xent"], ids=lambda c: "N%d-C%d" % c[2:])
def test_float32_restatement_stays_inside_the_loss_bounds(case):
    """the kernel's operation order in float32 numpy against the float64 statement, under the very bounds of the GPU test: this is
    what entitles those bounds to be used on the kernel.  Measured here (numpy's exp and log): at most 1.5 units of u x magnitude
    for a loss part (allowed: 8 + trips + 26), 3.1 for a gradient element (allowed: 8, above float32's underflow floor)."""
    _, B, N, C = case
    x, label, inner = H.xent_inputs(B, N, C)
    ref = H.xent_ref(x, label, inner)
    loss_part, d = H.xent_f32(x, label, inner)
    r_loss, r_grad = H.xent_check(loss_part, d, ref)
    print("N=%d C=%d: float32 restatement, worst loss part %.2f u, worst gradient element %.2f u" % (N, C, r_loss, r_grad))
    a_loss, a_grad = H.xent_allowed(ref)
    assert r_loss <= a_loss and r_grad <= a_grad, (r_loss, a_loss, r_grad, a_grad)
    assert not loss_part[0].any() and not d[0].any()
    # the same labels outside [0, C) as the GPU test: NaN in the statement and in the restatement, in the same places
    if N >= 1025:
        bad = label.copy()
        rows = np.flatnonzero(inner[3] > 0)
        bad[3, rows[1]], bad[3, rows[-2]] = H.BAD_LABELS
        rb, (lb, db) = H.xent_ref(x, bad, inner), H.xent_f32(x, bad, inner)
        assert np.array_equal(np.isnan(lb), np.isnan(rb["loss_part"])) and np.array_equal(np.isnan(db), np.isnan(rb["dlogits"]))
        assert np.isnan(rb["loss_part"]).sum() in (1, 2) and np.isnan(rb["dlogits"]).sum() == 2 * C
