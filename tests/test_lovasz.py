"""The Lovasz-softmax statement (sph3d_gcn_amd/harness/lovasz.py) without a device: the closed form against the paper's difference
form, the properties of the Lovasz gradient, one-hot predictions against 1 - IoU, the tie rule, coef against a finite difference,
the torch statement against the numpy one, and the host-side answers of the two entry points (csrc/lovasz.hip)."""
import numpy as np
import pytest
import torch

import _lovasz_ref as R
from sph3d_gcn_amd.harness import lovasz


def _paper_gradient(fg_sorted):
    """Berman et al., Alg. 1 (lovasz_grad of the authors' code): jaccard = 1 - intersection / union over the sorted prefix, then
    its first difference"""
    gt = np.asarray(fg_sorted, np.float64)
    gts = gt.sum()
    intersection = gts - np.cumsum(gt)
    union = gts + np.cumsum(1.0 - gt)
    jaccard = 1.0 - intersection / union
    jaccard[1:] = jaccard[1:] - jaccard[:-1]
    return jaccard


def _flag_cases():
    rng = np.random.RandomState(5)
    cases = [np.array([True]), np.array([True, False]), np.array([False, True]), np.ones(7, bool)]
    for n in (2, 3, 17, 1000, 16384):
        for frac in (0.02, 0.5, 0.97):
            fg = rng.rand(n) < frac
            fg[rng.randint(n)] = True
            cases.append(fg)
    return cases


def test_closed_form_is_the_papers_difference_form():
    for fg in _flag_cases():
        g = lovasz.jaccard_gradient(fg)
        assert np.abs(g - _paper_gradient(fg)).max() <= 1e-12
        assert (g >= 0).all() and abs(g.sum() - 1.0) <= 1e-12


def _one_hot_logits(pred, C):
    return np.where(np.arange(C) == pred[..., None], 0.0, -np.inf)


def test_one_hot_predictions_give_one_minus_iou():
    rng = np.random.RandomState(11)
    B, N, C = 3, 200, 5
    label = rng.randint(0, C - 1, (B, N))                      # class C - 1 is never a label ...
    pred = rng.randint(0, C, (B, N))                           # ... but is predicted
    label[1, :9] = R.IGNORE
    inner = (rng.rand(B, N) < 0.7).astype(np.float32)
    pred[2] = label[2]                                         # a perfect block
    ref = lovasz.lovasz_reference(_one_hot_logits(pred, C), label, inner)
    valid = R.valid_rows(label, inner)
    for b in range(B):
        lab, pr = label[b, valid[b]], pred[b, valid[b]]
        ious = []
        for c in range(C):
            inter, union = ((lab == c) & (pr == c)).sum(), ((lab == c) | (pr == c)).sum()
            if (lab == c).any():
                assert ref["present"][b, c] and abs(ref["class_loss"][b, c] - (1.0 - inter / union)) <= 1e-12
                ious.append(inter / union)
            else:
                assert not ref["present"][b, c] and ref["class_loss"][b, c] == 0.0
        assert abs(ref["loss"][b] - (1.0 - np.mean(ious))) <= 1e-12
    assert ref["loss"][2] == 0.0 and not ref["present"][:, C - 1].any()


def test_tie_rule_on_duplicated_rows():
    """rows copied verbatim: among equal e the lower row comes first, in float64 and on float32 probabilities alike"""
    x, label, inner = R.lovasz_inputs(4, 64, 4)
    pure = lovasz.lovasz_reference(x, label, inner)
    p32 = R.softmax64(x)[0].astype(np.float32)
    staged = lovasz.lovasz_reference(x, label, inner, probs=p32)
    valid = R.valid_rows(label, inner)
    seen = 0
    for ref, p in ((pure, pure["probs"]), (staged, p32)):
        one = p.dtype.type(1)
        for b in range(4):
            nb = int(valid[b].sum())
            assert ref["n_valid"][b] == nb
            for c in range(4):
                order = ref["order"][b, c]
                assert (order[nb:] == -1).all() and sorted(order[:nb]) == list(np.flatnonzero(valid[b]))
                rows = order[:nb]
                e = np.where(label[b, rows] == c, one - p[b, rows, c], p[b, rows, c])
                assert (e[:-1] >= e[1:]).all()
                ties = e[:-1] == e[1:]
                assert (rows[:-1][ties] < rows[1:][ties]).all()
                # the planted pair (t, 32 + t) with one label: equal e in every class, so adjacent in that order when both count
                for t in (0, 2, 4, 6):
                    if valid[b, t] and valid[b, 32 + t] and label[b, t] == label[b, 32 + t]:
                        i, j = list(rows).index(t), list(rows).index(32 + t)
                        assert i < j and (e[i:j + 1] == e[i]).all()
                        seen += 1
    assert seen >= 8


def test_coef_is_the_derivative_in_p():
    """N = 40, C = 4, no ties: the statement is piecewise linear in p, so a step below half the smallest gap of e stays on one piece
    and the forward difference is the derivative up to rounding"""
    rng = np.random.RandomState(2)
    N, C = 40, 4
    p = rng.dirichlet(np.ones(C), (1, N))
    label = rng.randint(0, C, (1, N))
    label[0, 7] = -1
    inner = np.ones((1, N), np.float32)
    inner[0, 11] = 0.0
    ref = lovasz.lovasz_reference(np.zeros((1, N, C)), label, inner, probs=p)
    valid = R.valid_rows(label, inner)[0]
    gap = np.inf
    for c in range(C):
        e = np.where(label[0] == c, 1.0 - p[0, :, c], p[0, :, c])[valid]
        gap = min(gap, np.diff(np.sort(e)).min())
    assert gap > 1e-7
    h = gap / 4
    for n in range(N):
        for c in range(C):
            q = p.copy()
            q[0, n, c] += h
            d = (lovasz.lovasz_reference(np.zeros((1, N, C)), label, inner, probs=q)["loss"][0] - ref["loss"][0]) / h
            assert abs(d - ref["coef"][0, n, c]) <= 1e-9, (n, c, d, ref["coef"][0, n, c])
    assert not ref["coef"][0, 7].any() and not ref["coef"][0, 11].any() and ref["coef"][0, 0].any()


@pytest.mark.parametrize("shape", [(64, 4), (1025, 13), (5, 2), (1, 3)], ids=lambda s: "N%d-C%d" % s)
def test_torch_statement_equals_the_numpy_one(shape):
    """float64 on the CPU, loss and autograd gradient; the inputs hold the empty block, an absent class and ignored labels"""
    N, C = shape
    x, label, inner = R.lovasz_inputs(4, N, C)
    ref = lovasz.lovasz_reference(x, label, inner)
    assert ref["n_valid"][0] == 0 and ref["loss"][0] == 0.0
    if N >= 64:
        assert not ref["present"][1].all() and (label == R.IGNORE).any()
    pred = torch.from_numpy(x).double().requires_grad_(True)
    w = torch.tensor([1.0, -2.0, 0.5, 3.0], dtype=torch.float64)
    out = lovasz.lovasz_torch(pred, torch.from_numpy(label), torch.from_numpy(inner))
    (out * w).sum().backward()
    assert np.abs(out.detach().numpy() - ref["loss"]).max() <= 1e-12
    assert np.abs(pred.grad.numpy() - ref["dlogits"] * w.numpy()[:, None, None]).max() <= 1e-12
    # without a mask, and through loss(): the batch sum, on the CPU the torch statement
    ref2 = lovasz.lovasz_reference(x, label)
    got2 = lovasz.loss(torch.from_numpy(x).double(), torch.from_numpy(label))
    assert abs(float(got2) - ref2["loss"].sum()) <= 1e-12


def test_bad_labels_make_the_block_nan():
    x, label, inner = R.lovasz_inputs(4, 64, 4)
    label = label.copy()
    label[1, 5], label[0, 3] = R.BAD_LABELS                       # block 0 has no valid row: nothing changes there
    ref = lovasz.lovasz_reference(x, label, inner)
    assert np.isnan(ref["loss"][1]) and np.isnan(ref["dlogits"][1]).all() and np.isfinite(ref["loss"][[0, 2, 3]]).all()
    pred = torch.from_numpy(x).double().requires_grad_(True)
    out = lovasz.lovasz_torch(pred, torch.from_numpy(label), torch.from_numpy(inner))
    out.sum().backward()
    assert np.array_equal(np.isnan(out.detach().numpy()), np.isnan(ref["loss"]))
    assert np.isnan(pred.grad[1].numpy()).all() and np.isfinite(pred.grad[[0, 2, 3]].numpy()).all()


def test_with_xent_adds_the_weighted_loss():
    x, label, inner = R.lovasz_inputs(4, 64, 4)
    pred, lab, inn = torch.from_numpy(x).double(), torch.from_numpy(label), torch.from_numpy(inner)
    calls = []

    def xent(p, l, *rest):
        calls.append(len(rest))
        return p.sum() * 0.0 + 2.0
    want = lovasz.lovasz_reference(x, label, inner)["loss"].sum()
    assert abs(float(lovasz.with_xent(xent, 0.5)(pred, lab, inn)) - (2.0 + 0.5 * want)) <= 1e-12
    want2 = lovasz.lovasz_reference(x, label)["loss"].sum()
    assert abs(float(lovasz.with_xent(xent)(pred, lab)) - (2.0 + want2)) <= 1e-12
    assert calls == [1, 0]


def test_entry_points_answer_on_the_host():
    """shape predicate and argument checks, before any launch (null pointers throughout)"""
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    assert l.sph3d_lovasz_softmax_supported(16384, 13) == 1
    assert l.sph3d_lovasz_softmax_supported(16385, 13) == 0
    assert l.sph3d_lovasz_softmax_supported(1, 1) == 1
    assert l.sph3d_lovasz_softmax_supported(0, 13) == 0 and l.sph3d_lovasz_softmax_supported(8192, 0) == 0
    null = [None] * 3 + [-1] + [None] * 7
    for dims in ((-1, 8, 4), (1, 0, 4), (1, 8, 0), (1, -8, 4), (65535, 16384, 8192)):
        assert l.sph3d_lovasz_softmax(*dims, *null) == -1 and b"bad dims" in l.sph3d_last_error(), dims
    assert l.sph3d_lovasz_softmax(4, 16385, 13, *null) == -4 and b"not covered" in l.sph3d_last_error()
    assert l.sph3d_lovasz_softmax(0, 8, 4, *null) == 0                                # no block: nothing to do
    assert l.sph3d_lovasz_softmax(1, 8, 4, *null) == -1 and b"null" in l.sph3d_last_error()
    with pytest.raises(_lib.Sph3dError):
        from sph3d_gcn_amd import tf_loss
        tf_loss.lovasz_softmax(torch.zeros(1, 8, 4), torch.zeros(1, 8, dtype=torch.long))
    assert lovasz.MAX_N == 16384
