"""The guarded update without a GPU: harness/guard.py's statement (the fixed-order sum of squares against math.fsum under its
derived bound, the running powers against optim.tf_adam_lr_t, clipping, the skip, the EMA), the CPU-tensor branch of the
optimisers that calls it, state_dict round trips, the Trainer on the oracle-backed ops (a skipped step restores the moving
statistics, ema_weights(), skip_limit) and two gloo ranks that skip together."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _train_ref as R
from oracle import torch_ops
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import guard, optim, train
from test_train import HostFeed, _blocks, _same, _state, _trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, MOM, EPS = 1e-3, 0.9, 0.999, 0.9, 1e-4
U53 = 2.0 ** -53


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _wide(rng, n, lo=-20, hi=10):
    return (rng.randn(n) * 10.0 ** rng.uniform(lo, hi, n)).astype(np.float32)


# ---- the sum ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 2 ** 18 + 1, 2 ** 20 + 13])
def test_sumsq_holds_the_derived_bound_against_fsum(n):
    """all terms are >= 0: a lane adds ceil(n / LANES) terms, the tree has 18 levels, every addition rounds by 2^-53 relative"""
    rng = np.random.RandomState(n % 1000)
    for scale in (1.0, 0.125, R.f32(1.0 / 3.0)):
        g = _wide(rng, n)
        gg0 = guard.scaled(g, scale)
        assert gg0.dtype == np.float32 and np.array_equal(_bits(gg0), _bits(np.float32(scale) * g))
        S = guard.sumsq(gg0)
        exact = math.fsum((gg0.astype(np.float64) ** 2).tolist())
        bound = (-(-n // guard.LANES) + 18) * U53 * exact
        print("n=%d scale=%g: |S - fsum| = %.2f units of 2^-53" % (n, scale, abs(S - exact) / (U53 * exact)))
        assert abs(S - exact) <= bound
        # where an fp32 accumulation would have lost the small terms or overflowed
        assert np.isfinite(S) and S > 0
    assert guard.sumsq(np.zeros(7, np.float32)) == 0.0 and guard.sumsq(np.zeros(0, np.float32)) == 0.0
    # the order is the statement's: lanes first, then adjacent pairs
    if n == 5:
        x = np.array([1.0, 2.0 ** -30, 2.0 ** -30, 1.0, 3.0], np.float32).astype(np.float64) ** 2
        assert guard.sumsq(np.sqrt(x).astype(np.float32)) == ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + 0.0) + 0.0)


def _settings():
    """every (lr, betas) the reference's defaults reach in 4096 steps of any schedule stage, and those of the tests below"""
    out = set()
    for d in train.DEFAULTS.values():
        # DEFAULTS names no betas today (the scripts use tf.train.AdamOptimizer's 0.9, 0.999 = FlatTFAdam's); a line that
        # gets its own is checked with them
        b1, b2 = d.get("betas", (d.get("beta1", B1), d.get("beta2", B2)))
        for k in range(4):
            out.add((max(d["base"] * d["decay_rate"] ** k, 1e-6), b1, b2))
        out.add((1e-6, b1, b2))
    out.add((LR, B1, B2))
    return sorted(out)


def _assert_lr_t_precondition(lr, b1, b2, steps):
    p1 = p2 = 1.0
    for t in range(1, steps + 1):
        p1 *= guard.f32(b1)
        p2 *= guard.f32(b2)
        assert guard.lr_t_from_powers(lr, p1, p2) == optim.tf_adam_lr_t(lr, b1, b2, t) == R.lr_t(lr, b1, b2, t), (lr, b1, b2, t)
    assert (p1, p2) == guard.powers_after(b1, b2, steps)


def test_running_powers_give_the_unguarded_lr_t():
    """the precondition of every bit equality with the unguarded path: iterated float64 products round to the fp32 lr_t that
    pow() gives sph3d_train_update"""
    for lr, b1, b2 in _settings():
        _assert_lr_t_precondition(lr, b1, b2, 4096)


# ---- the optimisers' CPU branch ---------------------------------------------------------------------------------------------
def _param(p):
    return torch.nn.Parameter(torch.from_numpy(p.copy()))


def _make(rule, p, **guard_kw):
    fp = _param(p)
    opt = optim.FlatTFAdam(fp, lr=LR, betas=(B1, B2), eps=EPS) if rule == 0 else optim.FlatNesterov(fp, lr=LR, momentum=MOM)
    if guard_kw:
        opt.guard = optim.Guard(**guard_kw)
    return fp, opt


def _buffers(fp, opt):
    out = [fp.detach().numpy().copy()] + [opt.state[k].numpy().copy() for k in opt.slots]
    if opt.guard is not None and opt.guard.ema is not None:
        out.append(opt.guard.ema.numpy().copy())
    return out


def _equal_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("rule", [0, 1], ids=["tf-adam", "nesterov"])
def test_a_guard_that_never_triggers_gives_the_unguarded_bits(rule):
    _assert_lr_t_precondition(LR, B1, B2, 10)
    rng = np.random.RandomState(40 + rule)
    n = 5003
    p0, _ = R.why_inputs(rng, n)
    (fa, oa), (fb, ob) = _make(rule, p0), _make(rule, p0, clip_norm=1e30, skip_nonfinite=True)
    oa.grad_scale = ob.grad_scale = 0.125
    for step in range(10):
        g = (R.why_inputs if step % 2 else R.wide_inputs)(rng, n)[1]
        fa.grad, fb.grad = torch.from_numpy(g.copy()), torch.from_numpy(g.copy())
        oa.step()
        ob.step()
        assert _equal_bits(_buffers(fa, oa), _buffers(fb, ob)), step
    assert ob.guard.read()[:3] == (10, 0, 0) and int(ob.nonfinite) == 0
    assert ob.state_dict()["step"] == 10 == oa.state_dict()["step"]


def test_clipping_scales_by_the_statements_factor():
    rng = np.random.RandomState(7)
    n = 2 ** 18 + 77
    p0, _ = R.why_inputs(rng, n)
    g = (rng.randn(n) * 3.0).astype(np.float32)
    clip = 2.5
    fp, opt = _make(0, p0, clip_norm=clip)
    opt.grad_scale = 0.5
    fp.grad = torch.from_numpy(g.copy())
    opt.step()
    w = guard.fields(opt.guard.words())
    gg0 = np.float32(0.5) * g
    S = guard.sumsq(gg0)
    c = R.f32(clip) / (math.sqrt(S) + 1e-6)
    assert w["S"] == S and w["last_norm"] == math.sqrt(S) == w["max_norm_seen"] and c < 1
    assert w["c32"] == R.f32(c) and w["flag"] == 3 and w["clipped_steps"] == 1 and w["applied"] == 1
    gg = np.float32(w["c32"]) * gg0
    eff = math.sqrt(math.fsum((gg.astype(np.float64) ** 2).tolist()))
    # c32 <= c (1 + 2^-24), every product rounds by 2^-24 relative, norm / (norm + 1e-6) < 1
    print("effective norm / clip_norm - 1 = %.3g" % (eff / clip - 1))
    assert eff <= clip * (1 + 2.0 ** -22)
    assert eff >= clip * (1 - 2.0 ** -18)               # (and it IS scaled to the threshold, up to the 1e-6 of the denominator)
    want, bound = R.tf_adam_ref(p0, gg, np.zeros_like(p0), np.zeros_like(p0), LR, B1, B2, EPS, 1)
    for got, x, b in zip(_buffers(fp, opt), want, bound):
        assert R.worst(got, x, b)[1] == 0
    # below the threshold nothing is scaled: c32 is recorded, the flag says not clipped
    fp.grad = torch.from_numpy((g * np.float32(1e-3)).copy())
    opt.step()
    w = guard.fields(opt.guard.words())
    assert w["flag"] == 1 and w["c32"] > 1 and w["clipped_steps"] == 1 and w["applied"] == 2
    assert w["max_norm_seen"] == math.sqrt(S) and w["last_norm"] < 1e-2 * math.sqrt(S)


@pytest.mark.parametrize("rule", [0, 1], ids=["tf-adam", "nesterov"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_planted_nonfinite_element_changes_nothing(rule, value):
    rng = np.random.RandomState(3)
    n = 4099
    p0, g0 = R.why_inputs(rng, n)
    fp, opt = _make(rule, p0, clip_norm=1.0, skip_nonfinite=True, ema_decay=0.999)
    for _ in range(2):
        fp.grad = torch.from_numpy(R.why_inputs(rng, n)[1])
        opt.step()
    before, words = _buffers(fp, opt), opt.guard.words()
    bad = g0.copy()
    bad[[0, 1000, n - 1]] = value
    fp.grad = torch.from_numpy(bad)
    opt.step()
    after = guard.fields(opt.guard.words())
    assert _equal_bits(before, _buffers(fp, opt))
    was = guard.fields(words)
    for k in ("applied", "clipped_steps", "b1pow", "b2pow", "last_norm", "max_norm_seen", "lr_t", "c32", "om"):
        assert after[k] == was[k], k
    assert after["flag"] == 0 and after["skipped"] == 1 and after["bad"] == 3 and int(opt.nonfinite) == 3
    assert opt.guard.read()[:3] == (2, 1, was["clipped_steps"])
    # the next clean step is the one a run without the bad step takes
    fq, oq = _make(rule, before[0], clip_norm=1.0, skip_nonfinite=True, ema_decay=0.999)
    for k, a in zip(oq.slots, before[1:]):
        oq.state[k].copy_(torch.from_numpy(a))
    oq.guard.bind(fq)
    oq.guard.state.copy_(torch.from_numpy(words))
    oq.guard.ema.copy_(torch.from_numpy(before[-1]))
    fp.grad, fq.grad = torch.from_numpy(g0.copy()), torch.from_numpy(g0.copy())
    opt.step()
    oq.step()
    assert _equal_bits(_buffers(fp, opt), _buffers(fq, oq)) and not _equal_bits(before, _buffers(fp, opt))
    # without skip_nonfinite the NaN propagates and is counted, as in the unguarded update
    fr, orr = _make(rule, p0, clip_norm=1.0)
    fr.grad = torch.from_numpy(bad)
    orr.step()
    assert int(orr.nonfinite) == 3 and not np.isfinite(fr.detach().numpy()[[0, 1000, n - 1]]).any()
    assert orr.guard.read()[:3] == (1, 0, 0) and np.isfinite(np.delete(fr.detach().numpy(), [0, 1000, n - 1])).all()


def test_ema_recursion_and_warm_up():
    rng = np.random.RandomState(5)
    n, decay = 3001, 0.9
    p0, _ = R.why_inputs(rng, n)
    fp, opt = _make(0, p0, ema_decay=decay)
    opt.guard.bind(fp)
    assert np.array_equal(_bits(opt.guard.ema.numpy()), _bits(p0))          # the shadow starts at the parameters
    for a in range(100):
        fp.grad = torch.from_numpy(R.why_inputs(rng, n)[1])
        e = opt.guard.ema.numpy().astype(np.float64)
        opt.step()
        d_t = min(R.f32(decay), (1.0 + a) / (10.0 + a))
        om = guard.fields(opt.guard.words())["om"]
        assert om == R.f32(1.0 - d_t)
        assert (d_t < R.f32(decay)) == (a < 80)                            # (1 + a) / (10 + a) reaches 0.9 at a = 80
        p1 = fp.detach().numpy().astype(np.float64)
        want = e - (e - p1) * om
        bound = R.gamma(3) * (np.abs(e - p1) * om + np.abs(want))           # the difference, the product, the difference
        assert R.worst(opt.guard.ema.numpy(), want, bound)[1] == 0, a
    assert not np.array_equal(opt.guard.ema.numpy(), fp.detach().numpy())


def test_guard_refuses_bad_options_and_flat_adam():
    for kw in (dict(clip_norm=0.0), dict(clip_norm=-1.0), dict(ema_decay=0.0), dict(ema_decay=1.0), dict(clip_norm=float("nan"))):
        with pytest.raises(ValueError):
            optim.Guard(**kw)
    fp = _param(np.zeros(8, np.float32))
    with pytest.raises(ValueError):
        optim.FlatAdam(fp, guard=optim.Guard(clip_norm=1.0))
    plain = optim.FlatAdam(fp)
    assert plain.guard is None
    with pytest.raises(ValueError):
        plain.guard = optim.Guard(clip_norm=1.0)
    assert optim._FlatRule.guard is None and optim.FlatTFAdam(fp).guard is None


def test_state_dict_round_trip_and_a_parent_format_state():
    rng = np.random.RandomState(9)
    n = 1000
    p0, _ = R.why_inputs(rng, n)
    kw = dict(clip_norm=0.05, skip_nonfinite=True, ema_decay=0.99)
    fp, opt = _make(0, p0, **kw)
    grads = [R.why_inputs(rng, n)[1] for _ in range(6)]
    grads[1][5] = np.nan
    for g in grads[:4]:
        fp.grad = torch.from_numpy(g.copy())
        opt.step()
    sd = opt.state_dict()
    assert sd["step"] == 3 and opt.t == 4 and sd["guard"] == kw and sd["guard_state"].dtype == torch.int64
    fq, oq = _make(0, fp.detach().numpy(), **kw)
    oq.load_state_dict(sd)
    assert _equal_bits(_buffers(fp, opt), _buffers(fq, oq)) and np.array_equal(opt.guard.words(), oq.guard.words())
    for g in grads[4:]:
        fp.grad, fq.grad = torch.from_numpy(g.copy()), torch.from_numpy(g.copy())
        opt.step()
        oq.step()
    assert _equal_bits(_buffers(fp, opt), _buffers(fq, oq)) and np.array_equal(opt.guard.words(), oq.guard.words())
    assert oq.guard.read()[:2] == (5, 1)
    # a state written without a guard: the powers from its step by iterated products, the EMA from the parameters
    fu, ou = _make(0, p0)
    for g in grads[2:5]:
        fu.grad = torch.from_numpy(g.copy())
        ou.step()
    parent = ou.state_dict()
    assert "guard_state" not in parent and parent["step"] == 3
    fg, og = _make(0, fu.detach().numpy(), clip_norm=1e30, ema_decay=0.99)
    og.load_state_dict(parent)
    w = guard.fields(og.guard.words())
    assert (w["applied"], w["b1pow"], w["b2pow"]) == (3,) + guard.powers_after(B1, B2, 3) and w["flag"] == 1
    assert np.array_equal(_bits(og.guard.ema.numpy()), _bits(fu.detach().numpy()))
    fu.grad, fg.grad = torch.from_numpy(grads[5].copy()), torch.from_numpy(grads[5].copy())
    ou.step()
    og.step()
    assert _equal_bits(_buffers(fu, ou), _buffers(fg, og)[:3])            # the fourth update, bias-corrected as the fourth
    # and a guarded state loads into an optimiser without a guard: step is the applied count
    ou.load_state_dict(sd)
    assert ou.t == 3


# ---- the Trainer on the oracle ops --------------------------------------------------------------------------------------------
def _plant(tr, at_steps):
    backward = tr.flat.backward

    def planted(loss):
        out = backward(loss)
        if tr.global_step in at_steps:
            tr.flat.flat[3] = float("nan")
        return out
    tr.flat.backward = planted


def _moving(tr):
    return {k: v.detach().clone() for k, v in tr.model.state_dict().items() if "moving" in k}


def test_trainer_without_options_has_no_guard_and_flat_adam_is_refused():
    blocks = _blocks()
    with torch_ops.patched_util():
        tr = _trainer(blocks)
        assert tr.guard is None and tr.opt.guard is None and tr._buf_flat is None
        with pytest.raises(_lib.Sph3dError):
            with tr.ema_weights():
                pass
        from sph3d_gcn_amd.harness import s3dis_net
        model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(1024), device=None, seed=3)
        prime = HostFeed(blocks).batch(0, np.array([0, 1]))[:3]
        with pytest.raises(ValueError):
            train.Trainer(model, model.loss, lambda p: optim.FlatAdam(p), train.Schedule(1e-3, 2, decay_step=4), 13, prime=prime,
                          clip_norm=1.0, log=lambda s: None)


def test_trainer_skips_a_bad_step_and_restores_the_moving_statistics():
    blocks = _blocks()
    log = []
    with torch_ops.patched_util():
        tr = _trainer(blocks, log, log_every=2, skip_nonfinite=True, ema_decay=0.99, clip_norm=1e30)
        _plant(tr, {1})
        items = list(HostFeed(blocks))
        fresh = _moving(tr)
        tr.train_step(items[0])
        after_one = dict(model=_state(tr), m=tr.opt.m.clone(), v=tr.opt.v.clone(), ema=tr.guard.ema.clone())
        assert not _same(fresh, _moving(tr))                              # a step that is applied moves the statistics
        lo, hi = tr._buf_flat.data_ptr(), tr._buf_flat.data_ptr() + 4 * tr._buf_flat.numel()
        assert all(lo <= b.data_ptr() < hi and b.data_ptr() % 16 == 0 for _n, b in tr.model.named_buffers() if b.dtype == torch.float32)
        tr.train_step(items[1])                                           # the planted one
        assert tr.global_step == 2 and tr.guard.read()[:3] == (1, 1, 0)
        assert _same(_state(tr), after_one["model"]) and torch.equal(tr.opt.m, after_one["m"]) and torch.equal(tr.opt.v, after_one["v"])
        assert torch.equal(tr.guard.ema, after_one["ema"])
        r = tr.metrics.read()
        assert r.update_nonfinite == 1 and r.batches == 2
        # ema_weights(): the averaged weights inside, the live ones back with the same bits
        live, ema = tr.flat.flat_param.detach().clone(), tr.guard.ema.clone()
        assert not torch.equal(live, ema)
        with tr.ema_weights():
            assert torch.equal(tr.flat.flat_param.detach(), ema) and torch.equal(tr.guard.ema, live)
            assert all(p.data.untyped_storage().data_ptr() == tr.flat.flat_param.data.untyped_storage().data_ptr()
                       for p in tr.model.parameters())
        assert torch.equal(tr.flat.flat_param.detach().view(torch.int32), live.view(torch.int32))
        assert torch.equal(tr.guard.ema.view(torch.int32), ema.view(torch.int32))
        # an epoch with one skipped step does not stop the run, and its log interval names the guard's figures
        tr2 = _trainer(blocks, log, log_every=2, skip_nonfinite=True)
        _plant(tr2, {0})
        out = tr2.train_one_epoch(HostFeed(blocks))
        assert tr2.global_step == 2 and out[0].update_nonfinite == 1 and tr2.guard.read()[:2] == (1, 1)
        assert any(s.startswith("guard: applied 1 skipped 1 clipped 0") for s in log)
        r = tr2.eval_one_epoch(HostFeed(blocks, augment=False))           # (no EMA: the live weights)
        assert np.isfinite(r.mean_loss)


def test_trainer_raises_past_the_skip_limit_and_names_the_counts():
    blocks = _blocks()
    with torch_ops.patched_util():
        tr = _trainer(blocks, log_every=2, skip_nonfinite=True, skip_limit=1)
        _plant(tr, {0, 1})
        with pytest.raises(_lib.Sph3dError, match=r"skipped 2 of the steps 0\.\.1 \(skip_limit 1\)"):
            tr.train_one_epoch(HostFeed(blocks))
        assert tr.guard.read()[:2] == (0, 2)


def test_trainer_checkpoint_holds_both_copies_of_the_weights(tmp_path):
    blocks = _blocks()
    with torch_ops.patched_util():
        tr = _trainer(blocks, ema_decay=0.9, clip_norm=0.5)
        for item in HostFeed(blocks):
            tr.train_step(item)
        tr.epoch = 0
        path = tr.save(str(tmp_path))
        tr2 = _trainer(blocks, ema_decay=0.9, clip_norm=0.5)
        state = tr2.load(path)
        assert "ema" in state["optimizer"] and state["optimizer"]["step"] == 2
        assert _same(_state(tr), _state(tr2)) and torch.equal(tr.guard.ema, tr2.guard.ema)
        assert np.array_equal(tr.guard.words(), tr2.guard.words()) and tr2._guard_seen == tr.guard.read()
        r1 = tr.eval_one_epoch(HostFeed(blocks, augment=False))
        r2 = tr2.eval_one_epoch(HostFeed(blocks, augment=False), use_ema=True)
        r3 = tr2.eval_one_epoch(HostFeed(blocks, augment=False), use_ema=False)
        assert r1.loss_sum == r2.loss_sum and r3.loss_sum != r2.loss_sum


def test_gloo_world2_ranks_skip_together():
    """two gloo ranks: rank 1's LOCAL gradient holds a NaN at the second step; the guard runs on the summed gradient, so both skip
    with no collective of their own, and parameters and guard states stay equal (the worker checks)"""
    script = os.path.join(ROOT, "tests", "_guard_gloo_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", OMP_NUM_THREADS="2")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29547", script],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "GUARD_GLOO_OK" in p.stdout
