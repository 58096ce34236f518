"""The cross-entropy with class weights, label smoothing and an ignore label without a GPU: the float64 statement
(sph3d_gcn_amd/harness/xent.py: xent_reference) against torch's cross_entropy and against tests/_head_ref.py's statement of the
existing op, the torch statement against it, D and the histogram on hand-built cases, class_weights on hand numbers, make_loss
against every line's get_loss, the test inputs' condition, and the host-side validation of the C ABI and the wrappers."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _head_ref as H
import _xent_ref as R
from sph3d_gcn_amd import _lib, tf_loss
from sph3d_gcn_amd.harness import lovasz, xent

N, C = 257, 13
COMBOS = list(itertools.product((False, True), (0.0, 0.1), (None, "in", "out"), ("count", "weight")))


def _opts(with_w, eps, ign, normalize, C=C):
    ignore = {None: None, "in": R.ignore_in(C), "out": R.IGNORE_OUT}[ign]
    # weights in 64ths: every D of these shapes (< 2^10, a multiple of 2^-6) is exact in float32, so the statement's one float32
    # rounding of D is no rounding and torch's float64 denominator is the same number
    w = np.round(R.weights(C) * 64.0).astype(np.float32) / np.float32(64.0)
    return dict(class_weight=w if with_w else None, label_smoothing=eps, ignore=ignore, normalize=normalize)


def _torch_blocks(x, label, inner, o):
    """F.cross_entropy in float64 per block -> (loss [B] under o['normalize'], dlogits [B,N,C] of the sum of the blocks)"""
    B = x.shape[0]
    pred = torch.from_numpy(x).double().requires_grad_(True)
    w = torch.from_numpy(o["class_weight"]).double() if o["class_weight"] is not None else None
    sentinel = -100
    lab = torch.from_numpy(label).clone()
    if o["ignore"] is not None:
        lab[lab == o["ignore"]] = sentinel
    if inner is not None:
        lab[~torch.from_numpy(inner > 0)] = sentinel
    out = []
    for b in range(B):
        if o["normalize"] == "weight":
            out.append(F.cross_entropy(pred[b], lab[b], weight=w, ignore_index=sentinel, label_smoothing=o["label_smoothing"]))
        else:
            s = F.cross_entropy(pred[b], lab[b], weight=w, ignore_index=sentinel, label_smoothing=o["label_smoothing"], reduction="sum")
            out.append(s / (lab[b] != sentinel).sum())
    loss = torch.stack(out)
    loss.sum().backward()
    return loss.detach().numpy(), pred.grad.numpy()


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "w%d-eps%g-ign%s-%s" % c)
def test_reference_vs_torch_cross_entropy(combo):
    """relative 1e-12: float64 rounding over at most ~10^4 terms.  Blocks with D = 0 (0 / 0 in torch) are held to the statement's
    zeros instead"""
    o = _opts(*combo)
    x, label, inner = R.inputs(N, C, o["ignore"])
    for mask in (None, inner):
        ref = xent.xent_reference(x, label, mask, **o)
        loss, grad = _torch_blocks(x, label, mask, o)
        live = ref["D"] > 0
        assert live.any()
        if o["class_weight"] is not None and o["normalize"] == "weight":
            assert np.array_equal(ref["D"].astype(np.float64), ref["hist"].astype(np.float64) @ o["class_weight"].astype(np.float64))
        assert not ref["loss"][~live].any() and not ref["dlogits"][~live].any()
        assert np.allclose(ref["loss"][live], loss[live], rtol=1e-12, atol=0)
        scale = np.abs(grad[live]).max()
        assert np.abs(ref["dlogits"][live] - grad[live]).max() <= 1e-12 * scale
        assert np.allclose(ref["loss_part"].sum(1), ref["loss"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", [(1, 13), (1025, 13), (16384, 2), (4097, 21)], ids=lambda s: "N%d-C%d" % s)
def test_reference_defaults_are_the_existing_statement(shape):
    x, label, inner = H.xent_inputs(4, *shape)
    old, new = H.xent_ref(x, label, inner), xent.xent_reference(x, label, inner)
    assert new["form"]["S"] == old["form"]["S"] and new["form"]["chunk"] == old["form"]["chunk"]
    assert np.array_equal(new["loss_part"], old["loss_part"]) and np.array_equal(new["dlogits"], old["dlogits"])
    assert np.array_equal(new["D"], old["cnt"].astype(np.float32))
    assert np.allclose(new["part_mag"], old["part_mag"], rtol=1e-12) and np.allclose(new["grad_mag"], old["grad_mag"], rtol=1e-12)


def test_parts_keep_growing():
    l = _lib.lib()
    for n in (1, 1000, 1024, 1025, 16384):
        assert l.sph3d_softmax_xent_parts(n) == l.sph3d_masked_softmax_xent_parts(n) == xent.xent_form(n)["S"]
    for n, s in ((16385, 17), (40000, 40), (131072, 128), (262144, 256), (262145, 256), (2 ** 22, 256)):
        assert l.sph3d_softmax_xent_parts(n) == s == xent.xent_form(n)["S"]
    assert l.sph3d_softmax_xent_workspace(4, 40000, 13) == 4 * 40 * 13 * 4


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "w%d-eps%g-ign%s-%s" % c)
def test_torch_statement_vs_reference(combo):
    o = _opts(*combo)
    x, label, inner = R.inputs(N, C, o["ignore"])
    for scope in ("block", "batch"):
        ref = xent.xent_reference(x, label, inner, scope=scope, **o)
        pred = torch.from_numpy(x).double().requires_grad_(True)
        w = torch.from_numpy(o["class_weight"]) if o["class_weight"] is not None else None
        loss, hist = xent.xent_torch(pred, torch.from_numpy(label), torch.from_numpy(inner), w, o["label_smoothing"], o["ignore"],
                                     o["normalize"], scope, return_counts=True)
        assert hist.dtype == torch.int32 and np.array_equal(hist.numpy(), ref["hist"])
        assert np.allclose(loss.detach().numpy(), ref["loss"], rtol=1e-12, atol=1e-300)
        loss.sum().backward()
        got = pred.grad.numpy().reshape(ref["dlogits"].shape)
        assert np.abs(got - ref["dlogits"]).max() <= 1e-12 * np.abs(ref["dlogits"]).max()
        # the dispatcher takes CPU tensors to the torch statement
        assert torch.equal(xent.loss(pred.detach(), torch.from_numpy(label), torch.from_numpy(inner), w, o["label_smoothing"],
                                     o["ignore"], o["normalize"], scope), loss.detach())


def test_labels_outside_the_classes():
    """a counted label outside [0, C): NaN in its part, its block's loss and its gradient row, and in no class of the histogram; an
    uncounted one changes nothing"""
    x, label, inner = R.inputs(1025, 13)
    clean = xent.xent_reference(x, label, inner)
    label[0, 3], label[1, 5], label[1, 1024] = H.BAD_LABELS[0], H.BAD_LABELS[0], H.BAD_LABELS[1]
    ref = xent.xent_reference(x, label, inner)
    assert np.array_equal(ref["loss_part"][[0, 2, 3]], clean["loss_part"][[0, 2, 3]]) and np.isnan(ref["loss_part"][1]).all()
    assert np.isnan(ref["dlogits"][1, [5, 1024]]).all() and int(np.isnan(ref["dlogits"]).sum()) == 2 * 13
    assert ref["hist"][1].sum() == 1023 and ref["D"][1] == 1023 and np.isnan(ref["loss"][1])
    pred = torch.from_numpy(x).double().requires_grad_(True)
    loss = xent.xent_torch(pred, torch.from_numpy(label), torch.from_numpy(inner))
    loss.sum().backward()
    assert np.array_equal(np.isnan(loss.detach().numpy()), np.isnan(ref["loss"]))
    assert np.array_equal(np.isnan(pred.grad.numpy()), np.isnan(ref["dlogits"]))


def test_histogram_and_denominators_by_hand():
    x = np.zeros((2, 6, 3), np.float32)
    label = np.array([[0, 1, 1, 2, 2, 2], [2, 2, 7, 0, 1, 2]])
    inner = np.array([[1, 1, 0, 1, np.nan, 2.5], [1, 1, 1, -1, 1, 1]], np.float32)
    w = np.array([0.25, 3.5, 0.1], np.float32)
    ref = xent.xent_reference(x, label, inner, class_weight=w, normalize="weight")
    assert ref["hist"].tolist() == [[1, 1, 2], [0, 1, 3]] and ref["hist"].dtype == np.int32
    want = [np.float32(0.25 + 3.5 + 2 * float(np.float32(0.1))), np.float32(3.5 + 3 * float(np.float32(0.1)))]
    assert ref["D"].dtype == np.float32 and ref["D"].tolist() == want
    assert xent.xent_reference(x, label, inner, class_weight=w)["D"].tolist() == [4.0, 4.0]
    assert np.isnan(ref["loss"][1])                                            # (the counted 7)
    # ignoring class 2, inside the classes: block 1 keeps class 1 only; outside: nothing changes but the 7
    ref = xent.xent_reference(x, label, inner, class_weight=w, ignore=2, normalize="weight")
    assert ref["hist"].tolist() == [[1, 1, 0], [0, 1, 0]] and ref["D"].tolist() == [3.75, 3.5]
    ref = xent.xent_reference(x, label, inner, ignore=7)
    assert ref["hist"].tolist() == [[1, 1, 2], [0, 1, 3]] and ref["D"].tolist() == [4.0, 4.0] and np.isfinite(ref["loss"]).all()
    # all logits equal: every counted row's loss is A ln 3; eps = 0.5 with unit weights: A = 1
    ref = xent.xent_reference(x, label, inner, ignore=7, label_smoothing=0.5)
    assert np.allclose(ref["loss"], np.log(3.0), rtol=1e-15)
    # one term at a time in float64: a quarter of an ulp of 2^24 is lost twice
    assert xent.denominators(np.array([[1, 1, 1]]), np.array([2.0 ** 24, 2.0 ** -30, 2.0 ** -30], np.float32), "weight")[0] == 2.0 ** 24
    # only zero-weight classes: D = 0, loss and gradient zero, no NaN
    ref = xent.xent_reference(x[:1], np.zeros((1, 6), np.int64), None, class_weight=np.array([0, 1, 1], np.float32),
                              label_smoothing=0.1, normalize="weight")
    assert ref["D"][0] == 0 and ref["loss"][0] == 0 and not ref["dlogits"].any()


def test_class_weights_by_hand():
    counts = np.array([10, 30, 0, 60])
    f = np.array([0.1, 0.3, 0.6])
    for scheme, want in (("inverse", 1 / (3 * f)), ("inverse_sqrt", 1 / np.sqrt(3 * f)), ("median", 0.3 / f),
                         ("log", 1 / np.log(1.02 + f))):
        w = xent.class_weights(counts, scheme)
        assert w.dtype == np.float32 and w[2] == 0.0
        assert np.array_equal(w[[0, 1, 3]], want.astype(np.float32)), scheme
    assert np.allclose(xent.class_weights(counts, "inverse") @ counts, 100.0)
    assert not xent.class_weights(np.zeros(4)).any()
    with pytest.raises(ValueError):
        xent.class_weights(counts, "focal")
    labels = torch.tensor([[0, 1, 1, 3, 3, 3, -1, 9]])
    assert xent.class_counts(labels, 4).tolist() == [1, 2, 0, 3]

    class Pool:
        rows = torch.zeros(5, 8)
    Pool.rows[:, 6] = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0])
    Pool.rows[:, 7] = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0])
    assert xent.class_counts(Pool, 3).tolist() == [1, 1, 1] and xent.class_counts(Pool, 3, inner_only=False).tolist() == [1, 2, 2]


def test_make_loss_is_each_lines_loss():
    """with every option absent make_loss(line) is the line's get_loss on CPU tensors, in float64 to 1e-12"""
    from sph3d_gcn_amd.harness import modelnet_net, ruemonge_net, s3dis_net, shapenet_net, train
    g = torch.Generator().manual_seed(11)
    pred = torch.randn(3, 50, 7, generator=g, dtype=torch.float64)
    label = torch.randint(0, 7, (3, 50), generator=g, dtype=torch.int32)
    inner = (torch.rand(3, 50, generator=g) < 0.6).int()
    inner[2] = 0
    args = {"s3dis": (pred, label, inner), "scannet": (pred, label, inner), "shapenet": (pred, label), "shapenet_onehot": (pred, label),
            "ruemonge": (pred, label), "modelnet": (pred[:, 0], label[:, 0])}
    want = {"s3dis": s3dis_net.get_loss(pred, label.long(), None, inner), "shapenet": shapenet_net.get_loss(pred, label),
            "ruemonge": ruemonge_net.get_loss(pred, label), "modelnet": modelnet_net.get_loss(pred[:, 0], label[:, 0])}
    want["scannet"], want["shapenet_onehot"] = want["s3dis"], want["shapenet"]
    assert sorted(args) == sorted(train.LINES)
    for line in train.LINES:
        got = xent.make_loss(line)(*args[line])
        assert got.dim() == 0 and abs(float(got) - float(want[line])) <= 1e-12 * abs(float(want[line])), line
    # the options reach the statement, and the result composes with the Lovasz loss
    w = R.weights(7)
    fn = xent.make_loss("s3dis", class_weight=w, label_smoothing=0.1, ignore=0, normalize="weight")
    ref = xent.xent_reference(pred.numpy(), label.numpy(), inner.numpy(), w, 0.1, 0, "weight")
    assert abs(float(fn(pred, label, inner)) - ref["loss"].sum()) <= 1e-12 * ref["loss"].sum()
    both = lovasz.with_xent(fn, 0.5)(pred, label, inner)
    assert abs(float(both) - float(fn(pred, label, inner)) - 0.5 * float(lovasz.loss(pred, label, inner))) <= 1e-12
    with pytest.raises(ValueError):
        xent.make_loss("kitti")
    with pytest.raises(ValueError):
        xent.make_loss("s3dis", class_weight=[1.0, -1.0])


def test_inputs_keep_their_condition():
    shapes = sorted(set(itertools.product(R.EQUAL_N, R.EQUAL_C)) | set(itertools.product(R.BOUND_N, R.BOUND_C)) | set(R.EXTRA_SHAPES))
    for n, c in shapes:
        w = R.weights(c)
        assert w.dtype == np.float32 and w[R.ZERO_CLASS] == 0 and w[1 % c] > 0 and np.isfinite(w).all() and (w >= 0).all()
        assert 0 <= R.ignore_in(c) < c <= R.IGNORE_OUT and R.ignore_in(c) != R.ZERO_CLASS
        for ignore in (None, R.ignore_in(c), R.IGNORE_OUT):
            x, label, inner = R.inputs(n, c, ignore)
            assert R.check_condition(label, inner, ignore) and R.check_condition(label, None, ignore), (n, c, ignore)
            if ignore is not None and n >= 1000:
                assert 0.02 * n < (label[1] == ignore).sum() < (0.12 if ignore < c else 0.08) * n + n / c
    # block 2 has D = 0 under "weight" with and without the mask, and > 0 under "count"
    x, label, inner = R.inputs(1025, 13, R.IGNORE_OUT)
    for mask in (None, inner):
        assert xent.xent_reference(x, label, mask, R.weights(13), 0.1, R.IGNORE_OUT, "weight")["D"][2] == 0
        assert xent.xent_reference(x, label, mask, R.weights(13), 0.1, R.IGNORE_OUT, "count")["D"][2] > 0


def test_validation_on_the_host():
    l = _lib.lib()
    tail = (None, None, None, None, 0, None)

    def call(B, N, C, eps=0.0, bits=64, normalize=0):
        return l.sph3d_softmax_xent(B, N, C, None, None, bits, None, None, eps, 0, 0, normalize, *tail)
    for dims in ((-1, 8, 4), (1, 0, 4), (1, 8, 0), (1 << 16, 8, 4), (4, 1 << 29, 4), (1, (1 << 30) + 1, 4)):
        assert call(*dims) == -1 and b"bad dims" in l.sph3d_last_error(), dims
    assert l.sph3d_softmax_xent_supported(131072, 4096) == 1 and l.sph3d_softmax_xent_supported(8, 4097) == 0
    assert l.sph3d_softmax_xent_supported(0, 13) == 0 and l.sph3d_softmax_xent_supported(8, 0) == 0
    assert call(1, 8, 4097) == -4 and b"not covered" in l.sph3d_last_error()
    for eps in (-0.1, 1.0, float("nan"), float("inf")):
        assert call(1, 8, 4, eps=eps) == -1 and b"label_smoothing" in l.sph3d_last_error(), eps
    assert call(1, 8, 4, bits=16) == -1 and b"label_bits" in l.sph3d_last_error()
    assert call(1, 8, 4, normalize=2) == -1 and b"normalize" in l.sph3d_last_error()
    assert call(0, 8, 4) == 0                                                  # no block: nothing to do
    assert call(1, 8, 4) == -1 and b"null" in l.sph3d_last_error()
    # the wrappers: weights, smoothing, ignore, normalize, scope — and no CPU tensors
    for bad in (dict(class_weight=np.array([1.0, -0.5, 1, 1])), dict(class_weight=torch.tensor([1.0, float("nan"), 1, 1])),
                dict(class_weight=np.array([1.0, np.inf, 1, 1])), dict(class_weight=np.ones(3)), dict(label_smoothing=1.0),
                dict(label_smoothing=-0.01), dict(label_smoothing=float("nan")), dict(ignore=1.5), dict(normalize="mean"),
                dict(scope="all")):
        with pytest.raises(ValueError):
            tf_loss.check_xent_options(4, **bad)
        with pytest.raises(ValueError):
            xent.xent_torch(torch.zeros(1, 8, 4), torch.zeros(1, 8, dtype=torch.long), **bad)
    assert tf_loss.check_xent_options(4, np.array([0, 1, 2.5, 0]), 0.1, -1, "weight", "batch") == (0.1, -1)
    with pytest.raises(_lib.Sph3dError):
        tf_loss.softmax_xent(torch.zeros(1, 8, 4), torch.zeros(1, 8, dtype=torch.long))


def test_weight_shape_is_checked_on_every_call():
    """a weight tensor found good at one C is refused at another, and a tensor that takes a dead one's place is read like any new one"""
    w = torch.tensor([1.0, 0.5, 2.0, 0.0])
    assert tf_loss.check_xent_options(4, w) == (0.0, None)
    assert tf_loss.check_xent_options(4, w) == (0.0, None)                     # (answered from what is remembered)
    for C in (3, 5, 13):
        with pytest.raises(ValueError, match="class_weight should be"):
            tf_loss.check_xent_options(C, w)
        with pytest.raises(ValueError, match="class_weight should be"):
            xent.xent_torch(torch.zeros(1, 8, C), torch.zeros(1, 8, dtype=torch.long), class_weight=w)
    with pytest.raises(ValueError):
        tf_loss.check_xent_options(4, w.reshape(2, 2))
    # a change in place is a new version
    w[1] = -1.0
    with pytest.raises(ValueError, match="finite"):
        tf_loss.check_xent_options(4, w)
    # tensors created and dropped in turn share addresses and ids: each one is read
    for k in range(8):
        good = torch.tensor([1.0, 0.5, 2.0, float(k)])
        tf_loss.check_xent_options(4, good)
        del good
        bad = torch.tensor([1.0, float("nan"), 2.0, float(k)])
        with pytest.raises(ValueError, match="finite"):
            tf_loss.check_xent_options(4, bad)
        del bad
    assert len(tf_loss._weights_seen) <= 1                                     # (entries die with their tensors)


def test_d_cases_tell_the_orders_apart():
    """the cases the GPU test reads the kernel's D from: the stated D differs from the descending-c sum or from the float32 sum, and
    the gradient the kernel would produce from either differs from the stated one in its bits"""
    for name, which in (("order", 0), ("float32", 1)):
        x, label, w = R.d_case_inputs(name)
        ref = xent.xent_reference(x, label, None, class_weight=w, normalize="weight")
        assert ref["hist"][0].tolist() == list(R.D_CASES[name][1])
        other = R.d_alternatives(w, R.D_CASES[name][1])[which]
        assert other != ref["D"][0] and abs(float(other) - float(ref["D"][0])) <= 2.0 ** -22 * float(ref["D"][0])
        want, wrong = R.d_exact_gradient(label, w, ref["D"][0]), R.d_exact_gradient(label, w, other)
        assert want.dtype == np.float32 and not np.array_equal(want.view(np.int32), wrong.view(np.int32))
        assert np.abs(want - ref["dlogits"]).max() <= 8 * R.U * np.abs(ref["dlogits"]).max()
    assert R.D_CASES["order"][0][2] == 2.0 ** -55 and xent.xent_reference(*R.d_case_inputs("order")[:2], None, R.D_CASES["order"][0],
                                                                              normalize="weight")["D"][0] == 1.0
    # an empty batch goes through the dispatcher
    assert xent.loss(torch.zeros(0, 8, 4), torch.zeros(0, 8, dtype=torch.long)).shape == (0,)
