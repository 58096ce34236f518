"""The cross-entropy with class weights, label smoothing and an ignore label on the device (csrc/xent.hip) through the C ABI and
tf_loss.softmax_xent: with every option at its default the existing op's bits; with the options on, every loss part and gradient
element within the bounds tests/_xent_ref.py derives from the kernel's operation order, against the float64 statement
(harness/xent.py: xent_reference), the histogram bit for bit and D bit for bit where the gradient shows it exactly, exact zeros on rows that do not count, NaN exactly where the
statement has it.  Outputs start as NaN (the histogram as -7).
Measured on an MI355X, worst over the 30 shapes, as fractions of the bounds: loss part 0.035, gradient element 0.118 (DESIGN.md 2
and 4.32)."""
import itertools

import numpy as np
import pytest
import torch

import _head_ref as H
import _xent_ref as R
from sph3d_gcn_amd import _lib, tf_loss
from sph3d_gcn_amd.harness import lovasz, xent

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.view(np.int32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None


def _call(dev, x, label, inner, class_weight=None, label_smoothing=0.0, ignore=None, normalize="count", grad=True, wide=True):
    """one C-ABI call -> (loss_part [B, S], hist [B, C], dlogits or None) as numpy"""
    l = _lib.lib()
    B, N, C = x.shape
    S = l.sph3d_softmax_xent_parts(N)
    xs, ms, ws = _dev(x, dev), _dev(inner, dev), _dev(class_weight, dev)
    ls = _dev(label if wide else label.astype(np.int32), dev)
    loss_part = torch.full((B, S), float("nan"), device=dev)
    hist = torch.full((B, C), -7, dtype=torch.int32, device=dev)
    d = torch.full((B, N, C), float("nan"), device=dev) if grad else None
    nbytes = l.sph3d_softmax_xent_workspace(B, N, C)
    assert nbytes == 4 * B * S * C
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(l.sph3d_softmax_xent(B, N, C, _lib.ptr(xs), _lib.ptr(ls), 64 if wide else 32, _lib.ptr(ms), _lib.ptr(ws), label_smoothing,
                                    ignore is not None, ignore if ignore is not None else 0, {"count": 0, "weight": 1}[normalize],
                                    _lib.ptr(loss_part), _lib.ptr(hist), _lib.ptr(d), _lib.ptr(work), nbytes, _lib.stream_ptr()))
    return loss_part.cpu().numpy(), hist.cpu().numpy(), (d.cpu().numpy() if grad else None)


def _old(dev, x, label, inner):
    l = _lib.lib()
    B, N, C = x.shape
    xs, ls, ms = _dev(x, dev), _dev(label, dev), _dev(inner, dev)
    loss_part = torch.full((B, l.sph3d_masked_softmax_xent_parts(N)), float("nan"), device=dev)
    d = torch.full((B, N, C), float("nan"), device=dev)
    _lib.check(l.sph3d_masked_softmax_xent(B, N, C, _lib.ptr(xs), _lib.ptr(ls), _lib.ptr(ms), _lib.ptr(loss_part), _lib.ptr(d),
                                           _lib.stream_ptr()))
    return loss_part.cpu().numpy(), d.cpu().numpy()


@pytest.mark.parametrize("shape", list(itertools.product(R.EQUAL_N, R.EQUAL_C)), ids=lambda s: "N%d-C%d" % s)
def test_defaults_are_the_existing_ops_bits(dev, shape):
    """no weights, eps = 0, no ignore label, "count", block scope, a mask, int64 labels: sph3d_masked_softmax_xent's loss_part and
    dlogits bit for bit"""
    N, C = shape
    x, label, inner = H.xent_inputs(4, N, C)
    want_part, want_d = _old(dev, x, label, inner)
    part, hist, d = _call(dev, x, label, inner)
    assert part.shape == want_part.shape
    assert np.array_equal(_bits(part), _bits(want_part)) and np.array_equal(_bits(d), _bits(want_d))
    counted = inner > 0
    assert hist.tolist() == [np.bincount(label[b][counted[b]], minlength=C).tolist() for b in range(4)]
    only, hist2, none = _call(dev, x, label, inner, grad=False)
    assert none is None and np.array_equal(_bits(only), _bits(part)) and np.array_equal(hist2, hist)


def _held(dev, x, label, inner, opts, wide, worst):
    """one call against the statement -> the call's outputs; the fractions of the bounds are kept in `worst`"""
    C = x.shape[2]
    ref = xent.xent_reference(x, label, inner, **opts)
    part, hist, d = _call(dev, x, label, inner, wide=wide, **opts)
    assert hist.dtype == np.int32 and np.array_equal(hist, ref["hist"])
    # (D_b is no output: test_the_kernels_own_denominator reads it off the gradient where that can be done exactly)
    assert not d[~ref["counted"]].any() and not part[ref["D"] == 0].any() and not d[ref["D"] == 0].any()
    r_loss, r_grad = R.check(part, d, ref)
    a_loss, a_grad = R.allowed(ref, C)
    worst[0], worst[1] = max(worst[0], r_loss / a_loss), max(worst[1], r_grad / a_grad)
    assert r_loss <= a_loss and r_grad <= a_grad, (opts, r_loss, a_loss, r_grad, a_grad)
    return part, hist, d


@pytest.mark.parametrize("shape", list(itertools.product(R.BOUND_N, R.BOUND_C)) + list(R.EXTRA_SHAPES), ids=lambda s: "N%d-C%d" % s)
def test_options_vs_float64(dev, shape):
    """weights, eps = 0.1, an ignore label inside and outside the classes, both normalisations, int32 and int64 labels, with a mask and
    without: up to 1025 rows every option set of tests/_xent_ref.py: option_sets in all four forms; above, the two sets that hold
    every option, one with a mask and int32 labels, one without and with int64 labels.  Bounds, u = 2^-24 (derived in
    tests/_xent_ref.py): gradient element (C + 24) u (A p (1 + |x| + |m|) + t) / D + 2^-126; loss part (2 C + 16 + trips + 26) u x the
    slice's row magnitudes / D."""
    N, C = shape
    worst = [0.0, 0.0]
    sets = R.option_sets(C)
    assert xent.xent_form(N)["trips"] == (2 if N > 262144 else 1)
    if N <= 1025:
        runs = [(name, o, wide, mask) for name, o in sets for wide in (False, True) for mask in (False, True)]
    else:
        runs = [(sets[-2][0], sets[-2][1], False, True), (sets[-1][0], sets[-1][1], True, False)]
    for name, o, wide, mask in runs:
        x, label, inner = R.inputs(N, C, o.get("ignore"))
        assert R.check_condition(label, inner if mask else None, o.get("ignore"))
        out = _held(dev, x, label, inner if mask else None, o, wide, worst)
    # the last run again: the same bits; and its losses alone
    again = _call(dev, x, label, inner if mask else None, wide=wide, **o)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(out, again))
    only = _call(dev, x, label, inner if mask else None, wide=wide, grad=False, **o)
    assert only[2] is None and np.array_equal(_bits(only[0]), _bits(out[0])) and np.array_equal(only[1], out[1])
    print("N=%d C=%d: worst fractions of the bounds over %d runs: loss part %.4f  gradient element %.4f" % (N, C, len(runs), *worst))


@pytest.mark.parametrize("name", sorted(R.D_CASES))
def test_the_kernels_own_denominator(dev, name):
    """D_b itself, read off the gradient: on all-zero logits with eps = 0 every element is a chain of correctly rounded float32
    operations on 1 / D_b (tests/_xent_ref.py: d_exact_gradient), so the bits of dlogits are the bits that the float64 sum in
    ascending c, rounded once, gives — and not those of a descending or a float32 sum, which differ (tests/test_xent.py)"""
    x, label, w = R.d_case_inputs(name)
    ref = xent.xent_reference(x, label, None, class_weight=w, normalize="weight")
    for wide in (True, False):
        part, hist, d = _call(dev, x, label, None, class_weight=w, normalize="weight", wide=wide)
        assert np.array_equal(hist, ref["hist"])
        assert np.array_equal(_bits(d), _bits(R.d_exact_gradient(label, w, ref["D"][0])))
        other = R.d_alternatives(w, R.D_CASES[name][1])
        assert not any(np.array_equal(_bits(d), _bits(R.d_exact_gradient(label, w, D))) for D in other if D != ref["D"][0])
        # the part: sum of w_y logf(4) over the rows, times the same inv
        assert H.xent_units(part, ref["loss_part"], ref["part_mag"]) <= R.allowed(ref, 4)[0]


def test_labels_outside_the_classes(dev):
    """labels 2^32 + 3 and -2^40 on counted rows: NaN in the row's part and its gradient row and nowhere else, and in no class of the
    histogram; on rows that do not count (masked out, or ignored: the ignore label itself may lie outside) they change nothing"""
    N, C = 1025, 13
    o = dict(R.option_sets(C)[-1][1])                                          # every option, ignore = 255
    x, label, inner = R.inputs(N, C, o["ignore"])
    clean = _call(dev, x, label, inner, **o)
    off = label.copy()
    out = np.flatnonzero(~(inner[3] > 0))
    off[0, 0], off[3, out[0]], off[3, out[-1]] = H.BAD_LABELS[0], H.BAD_LABELS[1], H.BAD_LABELS[0]
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(clean, _call(dev, x, off, inner, **o)))
    bad = label.copy()
    rows = np.flatnonzero((inner[3] > 0) & (label[3] != o["ignore"]))
    where = [(1, 5), (1, N - 1), (3, rows[1]), (3, rows[-2])]
    for i, (b, n) in enumerate(where):
        bad[b, n] = H.BAD_LABELS[i % 2]
    worst = [0.0, 0.0]
    for wide in (True, False):                                                 # (as int32 the two labels are 3 and 0: nothing is outside)
        lab = bad if wide else np.where(np.isin(bad, H.BAD_LABELS), -5, bad)
        part, hist, d = _held(dev, x, lab, inner, o, wide, worst)
        for b, n in where:
            assert np.isnan(d[b, n]).all() and np.isnan(part[b, n // xent.xent_form(N)["chunk"]]) and np.isfinite(d[b, n - 1]).all()
        assert int(np.isnan(d).sum()) == len(where) * C and np.isfinite(part[[0, 2]]).all()
    # the ignore label itself outside the label width's classes, and negative
    neg = np.where(label == o["ignore"], -1, label)
    o["ignore"] = -1
    _held(dev, x, neg, inner, o, False, worst)


@pytest.mark.parametrize("shape", [(4, 2048, 50), (32, 40)], ids=lambda s: "x".join(map(str, s)))
def test_batch_scope(dev, shape):
    """scope="batch": one block of B * N rows ([32, 40]: the ModelNet form, N = 1) through tf_loss.softmax_xent.  The loss is the
    sum of S parts in torch: S u x the parts' magnitudes on top of the parts' bounds"""
    C = shape[-1]
    if len(shape) == 3:
        x, label, inner = R.inputs(shape[1], C, R.ignore_in(C))
    else:
        rng = np.random.RandomState(40)
        x, label, inner = rng.randn(*shape).astype(np.float32) * 4, rng.randint(0, C, shape[0]), None
    w = R.weights(C)
    for normalize in ("count", "weight"):
        o = dict(class_weight=w, label_smoothing=R.EPS, ignore=R.ignore_in(C), normalize=normalize)
        ref = xent.xent_reference(x, label, inner, scope="batch", **o)
        assert ref["loss"].shape == (1,) and ref["D"][0] > 0
        pred = _dev(x, dev).requires_grad_(True)
        loss, hist = tf_loss.softmax_xent(pred, _dev(label.astype(np.int32), dev), _dev(inner, dev), _dev(w, dev), scope="batch",
                                          return_counts=True, **{k: v for k, v in o.items() if k != "class_weight"})
        assert loss.shape == (1,) and hist.shape == (1, C) and np.array_equal(hist.cpu().numpy(), ref["hist"])
        a_loss, a_grad = R.allowed(ref, C)
        S = ref["form"]["S"]
        assert abs(float(loss.detach()) - ref["loss"][0]) <= (a_loss + S) * R.U * ref["part_mag"].sum()
        loss.sum().backward()
        grad = pred.grad.cpu().numpy().reshape(ref["dlogits"].shape)
        assert H.xent_units(grad, ref["dlogits"], ref["grad_mag"], H.F32_FLOOR) <= a_grad
        assert torch.equal(xent.loss(pred.detach(), _dev(label, dev), _dev(inner, dev), w, scope="batch",
                                     **{k: v for k, v in o.items() if k != "class_weight"}), loss.detach())


def test_autograd_and_no_grad(dev):
    N, C = 8192, 13
    o = dict(R.option_sets(C)[-2][1])
    x, label, inner = R.inputs(N, C, o["ignore"])
    part, hist, d = _call(dev, x, label, inner, **o)
    pred = _dev(x, dev).requires_grad_(True)
    lab, inn = _dev(label, dev), _dev(inner, dev)
    o["class_weight"] = _dev(o["class_weight"], dev)
    up = torch.tensor([1.0, -2.0, 0.5, 3.0], device=dev)
    out, counts = tf_loss.softmax_xent(pred, lab, inn, return_counts=True, **o)
    assert out.shape == (4,) and np.array_equal(counts.cpu().numpy(), hist) and not counts.requires_grad
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(_dev(part, dev).sum(1).cpu().numpy()))
    (out * up).sum().backward()
    assert np.array_equal(_bits(pred.grad.cpu().numpy()), _bits(d * up.cpu().numpy()[:, None, None]))
    # no_grad: no [B, N, C] gradient is allocated (the scratch is warm by now)
    nbytes = 4 * x.size
    for grad in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.enable_grad() if grad else torch.no_grad():
            res = tf_loss.softmax_xent(pred, lab, inn, **o)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert (peak >= nbytes) == grad, (grad, peak, nbytes)
        assert torch.equal(res.detach(), out.detach())
    with pytest.raises(_lib.Sph3dError):
        tf_loss.softmax_xent(pred.detach().cpu(), lab.cpu(), inn.cpu())
    with pytest.raises(ValueError):
        tf_loss.softmax_xent(pred, lab, inn, class_weight=-o["class_weight"])


def test_training_with_the_options_on(dev):
    """three deterministic Trainer steps on the small S3DIS plan of tests/test_gpu_lovasz.py with the weighted, smoothed cross-entropy
    (class 0 ignored) and the Lovasz loss added: finite, and the same bits twice"""
    from test_gpu_lovasz import _train
    w = xent.class_weights(np.arange(13) % 5, "median")

    def loss_of(model):
        return lovasz.with_xent(xent.make_loss("s3dis", class_weight=w, label_smoothing=0.1, ignore=0), 1.0)
    la, pa = _train(dev, loss_of)
    lb, pb = _train(dev, loss_of)
    assert np.isfinite(la) and la == lb and torch.isfinite(pa.view(torch.float32)).all() and torch.equal(pa, pb)
    _, plain = _train(dev, lambda m: lovasz.with_xent(m.loss, 1.0))
    assert not torch.equal(pa, plain), "the options change nothing"
