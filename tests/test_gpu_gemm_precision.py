"""The lower float32 matmul precision levels of the pointwise products on the device (csrc/gemm.hip: gemm_split_mfma<NP>, NP = 2 "high",
NP = 1 "medium"; the statement and its constants: tests/_gemm_precision_ref.py) at every launch form of the bf16 pipe
(tests/_gemm_forms.py: FORM_CASES, the smallest shape that reaches each form), called through the C ABI as tests/test_gpu_gemm_forms.py
does — outputs start as NaN, the workspace as 0xFF bytes:
  * against the exact float64 product: |error| <= (c_level + 1e-5) of an element's summed term magnitudes;
  * against the float64 evaluation of the STATEMENT on the same pieces: <= max(4 x the fp32 kernel's own error at the shape, 4e-7) of
    them — no piece and no piece product is lost or doubled;
  * the statistics forms' partial sums against float64 ELU statistics of the level's own Y; the exchange forms twice, bit for bit;
  * known answers, bit for bit: a one-hot operand makes every output ONE product, 1 * w, and the three levels return three different
    exact values — w, h' + m' and h' of the statement;
  * scaling by powers of two, the 1x1 layer with its two gradients, and the Trainer's option."""
import ctypes

import numpy as np
import pytest
import torch

import _gemm_forms as G
import _gemm_precision_ref as P
import sph3d_gcn_amd as pkg
from sph3d_gcn_amd import _lib, tf_gemm
from sph3d_gcn_amd import sph3gcn_util as s3g_util

pytestmark = pytest.mark.gpu

SPLIT_CASES = [c for c in G.FORM_CASES if "split" in c[0] and c[5] == 1]
LEVELS = ("high", "medium")
_runs = {}


@pytest.fixture
def levels():
    """the library with the product mode and the piece count restored afterwards"""
    l = _lib.lib()
    mode, pieces = l.sph3d_pointwise_gemm_mode(-1), l.sph3d_pointwise_gemm_pieces(0)
    yield l
    l.sph3d_pointwise_gemm_mode(mode)
    l.sph3d_pointwise_gemm_pieces(pieces)


def _operands(dev, product, R, Ci, Co):
    """tests/test_gpu_gemm_forms.py: _operands -> (a, b, bias, float64 product, summed term magnitudes), once per product and shape"""
    key = ("ops", product, R, Ci, Co)
    if key not in _runs:
        g = torch.Generator(device=dev).manual_seed(1000 * product + R + Ci + Co)
        if product == G.NNS:
            x, w = torch.randn(R, Ci, device=dev, generator=g), torch.randn(Ci, Co, device=dev, generator=g) / Ci ** 0.5
            bias = torch.randn(Co, device=dev, generator=g)
            _runs[key] = (x, w, bias, x.double() @ w.double() + bias.double(), x.double().abs() @ w.double().abs() + bias.double().abs())
            return _runs[key]
        a = torch.randn(R, Ci, device=dev, generator=g) * torch.exp2(torch.randint(-6, 6, (R, Ci), device=dev, generator=g).float())
        if product == G.TN:
            b = torch.randn(R, Co, device=dev, generator=g) * torch.exp2(torch.randint(-6, 6, (R, Co), device=dev, generator=g).float())
            want, mag = a.double().t() @ b.double(), a.double().abs().t() @ b.double().abs()
        elif product == G.NT:
            b = torch.randn(Co, Ci, device=dev, generator=g) / Ci ** 0.5                        # W stored [Cout][Cin]
            want, mag = a.double() @ b.double().t(), a.double().abs() @ b.double().abs().t()
        else:
            b = torch.randn(Ci, Co, device=dev, generator=g) / Ci ** 0.5
            want, mag = a.double() @ b.double(), a.double().abs() @ b.double().abs()
        _runs[key] = (a, b, None, want, mag)
    return _runs[key]


def _matmul(product):
    if product == G.TN:
        return lambda a, b: a.t() @ b
    if product == G.NT:
        return lambda a, b: a @ b.t()
    return lambda a, b: a @ b


def _call(l, dev, product, R, Ci, Co, a, b, bias=None):
    """one call through the C ABI on a NaN-filled output and a 0xFF-filled workspace -> (output, partial sums or None)"""
    st = _lib.stream_ptr()
    if product == G.TN:
        out = torch.full((Ci, Co), float("nan"), device=dev)
        nbytes = l.sph3d_pointwise_gemm_tn_workspace(R, Ci, Co)
        ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev) if nbytes else None
        _lib.check(l.sph3d_pointwise_gemm_tn(R, Ci, Co, _lib.ptr(a), _lib.ptr(b), _lib.ptr(out), _lib.ptr(ws), nbytes, st))
        return out, None
    out = torch.full((R, Co), float("nan"), device=dev)
    if product == G.NNS:
        partial = torch.full((l.sph3d_pointwise_gemm_bnstats_blocks(R, Ci, Co), 2, Co), float("nan"), device=dev)
        _lib.check(l.sph3d_pointwise_gemm_bnstats(R, Ci, Co, _lib.ptr(a), _lib.ptr(b), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(partial), st))
        return out, partial
    _lib.check(l.sph3d_pointwise_gemm(R, Ci, Co, _lib.ptr(a), _lib.ptr(b), None, 0, int(product == G.NT), _lib.ptr(out), st))
    return out, None


def _plan(l, product, R, Ci, Co, mode):
    out = (ctypes.c_int * len(G.FIELDS))()
    assert l.sph3d_pointwise_gemm_plan(product, R, Ci, Co, 1, mode, 1, ctypes.cast(out, ctypes.c_void_p)) == 0
    return dict(zip(G.FIELDS, out))


def _fp32_kernel_error(l, dev, product, R, Ci, Co):
    """the mode-0 kernels' max |error| / summed term magnitudes at the shape, once"""
    key = ("e32", product, R, Ci, Co)
    if key not in _runs:
        a, b, bias, want, mag = _operands(dev, product, R, Ci, Co)
        l.sph3d_pointwise_gemm_mode(0)
        out, _ = _call(l, dev, product, R, Ci, Co, a, b, bias)
        l.sph3d_pointwise_gemm_mode(1)
        _runs[key] = float(((out.double() - want).abs() / mag).max())
    return _runs[key]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: c[0].replace(" ", "-"))
def test_level_at_every_split_form(dev, levels, case, level):
    tag, product, R, Ci, Co, _, mode, _ = case
    l = levels
    l.sph3d_pointwise_gemm_mode(mode)
    l.sph3d_pointwise_gemm_pieces(P.PIECES[level])
    plan = _plan(l, product, R, Ci, Co, -1)
    assert G.tag(product, plan) == tag and plan["pipe"] == G.SPLIT             # the plan does not depend on the level
    a, b, bias, want, mag = _operands(dev, product, R, Ci, Co)
    assert all(t is None or t.data_ptr() % 16 == 0 for t in (a, b, bias))
    e_f32 = _fp32_kernel_error(l, dev, product, R, Ci, Co)
    out, partial = _call(l, dev, product, R, Ci, Co, a, b, bias)
    # 1. the exact product (NaN if an element was not written)
    err = float(((out.double() - want).abs() / mag).max())
    # 2. the statement on the same pieces
    stmt = P.statement(P.pieces(a, level), P.pieces(b, level), level, _matmul(product))
    if bias is not None:
        stmt = stmt + bias.double()
    dev_stmt = float(((out.double() - stmt).abs() / mag).max())
    print("%s %s: error / term magnitudes %.3g (bound %.3g); against the statement %.3g (fp32 kernels' error %.3g)"
          % (tag, level, err, P.C_LEVEL[level] + 1e-5, dev_stmt, e_f32))
    assert err <= P.C_LEVEL[level] + 1e-5, (tag, level, err)
    assert dev_stmt <= max(4 * e_f32, 4e-7), (tag, level, dev_stmt, e_f32)
    if product == G.NNS:
        # 3. the partial sums are those of the Y this level returned
        assert plan["stats_blocks"] == partial.shape[0] > 0
        y = out.double()
        z = torch.where(y > 0, y, torch.expm1(y))
        p = partial.double().sum(0)
        np.testing.assert_allclose((p[0] / R).cpu().numpy(), (z.sum(0) / R).cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose((p[1] / R).cpu().numpy(), ((z * z).sum(0) / R).cpu().numpy(), rtol=1e-5, atol=1e-6)
    if plan["xs"] > 1:
        # 4. fixed summation order, arrival counters back at zero: a second call is bit-equal
        out2, partial2 = _call(l, dev, product, R, Ci, Co, a, b, bias)
        assert torch.equal(out2, out) and (partial is None or torch.equal(partial2, partial))


def _full_mantissa(shape, dev, g):
    """finite values of ~1 that need all 24 significant bits (the last one is set)"""
    w = torch.randn(shape, device=dev, generator=g) + 3.0 * torch.sign(torch.randn(shape, device=dev, generator=g))
    return (w.view(torch.int32) | 1).view(torch.float32)


@pytest.mark.parametrize("case", [c for c in SPLIT_CASES if c[1] != G.NNS], ids=lambda c: c[0].replace(" ", "-"))
def test_known_answers_of_a_one_hot_operand(dev, levels, case):
    """every output is one product 1 * w: "highest" returns w, "high" h' + m', "medium" h' — exactly, at the place the permutation says"""
    tag, product, R, Ci, Co, _, mode, _ = case
    l = levels
    l.sph3d_pointwise_gemm_mode(mode)
    g = torch.Generator(device=dev).manual_seed(R + 7 * Ci + 13 * Co)
    rows = torch.arange(R, device=dev)
    if product == G.TN:
        # x [R, Cin]: min(R, Cin) of the rows one-hot with distinct columns, the others zero -> dW: rows of dy, zero rows elsewhere
        n = min(R, Ci)
        hot, cols = torch.randperm(R, device=dev, generator=g)[:n], torch.randperm(Ci, device=dev, generator=g)[:n]
        a = torch.zeros(R, Ci, device=dev)
        a[hot, cols] = 1.0
        b = _full_mantissa((R, Co), dev, g)

        def expect(v):
            return torch.zeros(Ci, Co, device=dev).index_copy_(0, cols, v[hot])
    else:
        perm = torch.randperm(Ci, device=dev, generator=g)
        a = torch.zeros(R, Ci, device=dev)
        a[rows, perm[rows % Ci]] = 1.0
        if product == G.NT:
            b = _full_mantissa((Co, Ci), dev, g)                                # stored [Cout][Cin]

            def expect(v):
                return v.t()[perm[rows % Ci]]
        else:
            b = _full_mantissa((Ci, Co), dev, g)

            def expect(v):
                return v[perm[rows % Ci]]
    answers = {}
    for level in P.LEVELS:
        l.sph3d_pointwise_gemm_pieces(P.PIECES[level])
        assert G.tag(product, _plan(l, product, R, Ci, Co, -1)) == tag
        out, _ = _call(l, dev, product, R, Ci, Co, a, b)
        ps = P.pieces(b, level)
        value = b if level == "highest" else (ps[0] + ps[1] if level == "high" else ps[0])      # (h' + m': 16 bits, exact in fp32)
        assert torch.equal(out, expect(value)), (tag, level)
        answers[level] = out
    assert not torch.equal(answers["highest"], answers["high"]) and not torch.equal(answers["high"], answers["medium"])


@pytest.mark.parametrize("level", LEVELS)
def test_products_scale_exactly_by_powers_of_two(dev, levels, level):
    """round-to-nearest-even commutes with exact scaling (away from overflow and underflow): the pieces of 2^k x are 2^k times the pieces
    of x, so every piece product and fp32 accumulation scales exactly — NN, NT and TN, bit for bit"""
    levels.sph3d_pointwise_gemm_mode(1)
    R, Ci, Co = 4096, 64, 128
    g = torch.Generator(device=dev).manual_seed(17)
    x = torch.randn(R, Ci, device=dev, generator=g)
    w = torch.randn(Ci, Co, device=dev, generator=g) / 8
    dy = torch.randn(R, Co, device=dev, generator=g)

    def products(x, w, dy):
        return (tf_gemm._pointwise_gemm_impl(x, w, False), tf_gemm._pointwise_gemm_impl(dy, w, True), tf_gemm._pointwise_gemm_tn_impl(x, dy))
    with pkg.float32_matmul_precision(level):
        y, dx, dw = products(x, w, dy)
        y2, dx2, dw2 = products(x * 8.0, w * 0.25, dy * 8.0)
    assert torch.equal(y2, y * 2.0)
    assert torch.equal(dx2, dx * 2.0)
    assert torch.equal(dw2, dw * 64.0)
    highest = products(x, w, dy)
    assert not torch.equal(highest[0], y) and not torch.equal(highest[1], dx) and not torch.equal(highest[2], dw)


def _layer(dev, x, dout, cout):
    store = s3g_util.VariableStore(device=dev, seed=5)
    xs = x.to(dev).requires_grad_(True)
    with s3g_util.variable_store(store):
        out = s3g_util.pointwise_conv3d(xs, cout, 'p1', with_bn=False, with_bias=False, activation_fn=None, is_training=True)
    out.backward(dout.to(dev))
    (_, w), = store.params.items()
    return out.detach(), xs.grad, w.grad, w.detach()


def test_pointwise_layer_and_its_gradients_under_high(dev, levels):
    """s3g_util.pointwise_conv3d on 2 x 512 x 64 -> 128, forward and backward, inside `with float32_matmul_precision("high")`: output,
    input gradient and weight gradient each within (c_high + 1e-5) of their summed term magnitudes of float64; after the block the same
    call is bit-equal to the call made before it"""
    levels.sph3d_pointwise_gemm_mode(1)
    cin, cout = 64, 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 512, cin, generator=g)
    dout = torch.randn(2, 512, cout, generator=g)
    before = _layer(dev, x, dout, cout)
    with pkg.float32_matmul_precision("high"):
        assert _lib.lib().sph3d_pointwise_gemm_pieces(0) == 2
        out, dx, dw, w = _layer(dev, x, dout, cout)
    assert pkg.get_float32_matmul_precision() == "highest"
    after = _layer(dev, x, dout, cout)
    assert all(torch.equal(p, q) for p, q in zip(before, after))
    assert not torch.equal(out, before[0]) and torch.equal(w, before[3])
    x64, w64, d64 = x.double().reshape(-1, cin), w.cpu().double(), dout.double().reshape(-1, cout)
    checks = (("out", out.cpu().reshape(-1, cout), x64 @ w64, x64.abs() @ w64.abs()),
              ("dx", dx.cpu().reshape(-1, cin), d64 @ w64.t(), d64.abs() @ w64.abs().t()),
              ("dw", dw.cpu(), x64.t() @ d64, x64.abs().t() @ d64.abs()))
    for name, got, want, mag in checks:
        assert got.shape == want.shape
        err = float(((got.double() - want).abs() / mag).max())
        print("pointwise layer under high, %s: error / term magnitudes %.3g (bound %.3g)" % (name, err, P.C_HIGH + 1e-5))
        assert err <= P.C_HIGH + 1e-5, (name, err)


def test_trainer_option_reaches_the_kernels_and_is_restored(dev, levels):
    from sph3d_gcn_amd.harness import optim, s3dis_net, synth, train
    n_pts, batch = 1024, 2
    items = []
    for step in range(3):
        xyz, label, inner = synth.s3dis_batch(10 + step * batch, batch, n_pts, extent=(1.0, 1.0, 1.5))
        items.append((torch.from_numpy(xyz).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev), None))

    def run(level):
        model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(n_pts), device=dev, seed=3)
        tr = train.Trainer(model, model.loss, lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4), train.Schedule(1e-3, batch), 13,
                           prime=items[0][:3], seed=5, log=lambda s: None, matmul_precision=level)
        kept, add = [], tr.metrics.add
        tr.metrics.add = lambda pred, label, inner, loss_part: (kept.append(pred.detach().clone()), add(pred, label, inner, loss_part))[1]
        seen = []
        for item in items:
            tr.train_step(item)
            seen.append(pkg.get_float32_matmul_precision())
        r = tr.metrics.read()
        return kept[0], r.mean_loss, seen

    first_medium, loss, seen = run("medium")
    assert np.isfinite(loss)
    assert seen == ["highest"] * 3 and _lib.lib().sph3d_pointwise_gemm_pieces(0) == 3       # restored after every step
    first_highest, loss_highest, _ = run(None)
    assert np.isfinite(loss_highest)
    assert torch.isfinite(first_medium).all() and not torch.equal(first_medium, first_highest)
    with pytest.raises(ValueError):
        train.Trainer(None, None, None, None, 13, prime=items[0][:3], matmul_precision="low")


def test_no_exchange_gave_up_waiting_and_references_are_released(dev):
    assert _lib.lib().sph3d_pointwise_gemm_exchange_failures() == 0
    assert _lib.lib().sph3d_pointwise_gemm_pieces(0) == 3
    _runs.clear()
