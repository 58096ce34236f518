"""csrc/train.hip on the device: sph3d_train_update against the float64 statement under the derived per-element bound
(tests/_train_ref.py) at every launch form, sph3d_train_metrics bit for bit against harness/train.py's numpy statement, and the
Trainer over a DeviceFeed: six steps, the metrics of the steps' own logits, bit-equal checkpoint state and the resumed run."""
import numpy as np
import pytest
import torch

import _train_ref as R
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import feed, optim, s3dis_net, train

pytestmark = pytest.mark.gpu

SIZES_N = [0, 1, 3, 4, 5, 255, 256, 257, 1025, 4099]
STEPS = [1, 2, 1000, 100000]
LR, B1, B2, MOM = 1e-3, 0.9, 0.999, 0.9


def _dev(a, dev, offset):
    """a device copy of `a` whose first element is 16-byte aligned (offset 0) or one element past such a boundary (offset 1)"""
    t = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
    assert t.data_ptr() % 16 == 0
    view = t[offset:offset + a.size]
    view.copy_(torch.from_numpy(a))
    assert (view.data_ptr() % 16 == 0) == (offset == 0) or a.size == 0
    return view


def _update(p, g, s0, s1, rule, step, scale, eps, counter=None):
    _lib.check(_lib.lib().sph3d_train_update(p.numel(), _lib.ptr(p), _lib.ptr(g), _lib.ptr(s0), _lib.ptr(s1), rule, LR,
                                             B1 if rule == 0 else MOM, B2, eps, step, scale, _lib.ptr(counter), _lib.stream_ptr()))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-by-one"])
@pytest.mark.parametrize("rule", [0, 1], ids=["tf-adam", "nesterov"])
def test_update_holds_the_float64_statement_at_every_launch_form(dev, rule, offset):
    """every n, step and grad_scale; each step from the kernel's own previous fp32 state; zero gradients on zero state leave p as it is"""
    rng = np.random.RandomState(17 + rule)
    worst = {}
    eps = 1e-4
    for n in SIZES_N:
        for scale in (1.0, 0.125):
            p0, _ = R.wide_inputs(rng, n)
            p = _dev(p0, dev, offset)
            s0 = _dev(np.zeros(n, np.float32), dev, offset)
            s1 = _dev(np.zeros(n, np.float32), dev, offset)
            for k, step in enumerate(STEPS):
                draw = R.wide_inputs if k % 2 == 0 else R.why_inputs
                g0 = draw(rng, n)[1]
                if n:
                    g0[0] = 0.0
                before = [p.cpu().numpy(), s0.cpu().numpy(), s1.cpu().numpy()]
                _update(p, _dev(g0, dev, offset), s0, s1, rule, step, scale, eps)
                got = [p.cpu().numpy(), s0.cpu().numpy(), s1.cpu().numpy()]
                if n == 0:
                    continue
                if rule == 0:
                    want, bound = R.tf_adam_ref(before[0], g0, before[1], before[2], LR, B1, B2, eps, step, scale)
                    names = "pmv"
                else:
                    (wp, wa), (bp, ba) = R.nesterov_ref(before[0], g0, before[1], LR, MOM, scale)
                    want, bound, names = (wp, wa), (bp, ba), "pa"
                    assert not got[2].any()                  # slot1 is not touched
                for name, x, w, b in zip(names, got, want, bound):
                    ratio, outside = R.worst(x, w, b)
                    worst[name] = max(worst.get(name, 0.0), ratio)
                    assert outside == 0, (n, scale, step, name, ratio)
                if k == 0:
                    zero = g0 == 0
                    assert zero[0] and np.array_equal(got[0][zero], before[0][zero])
    print("rule %d offset %d: worst error / bound %s" % (rule, offset, {k: round(v, 4) for k, v in worst.items()}))


def test_update_with_the_shapenet_epsilon(dev):
    """eps = 1e-8 (ShapeNet, ModelNet): the denominator is the root alone for all but the smallest gradients"""
    rng = np.random.RandomState(23)
    n = 4099
    p0, g0 = R.wide_inputs(rng, n)
    p, m, v = _dev(p0, dev, 0), _dev(np.zeros(n, np.float32), dev, 0), _dev(np.zeros(n, np.float32), dev, 0)
    for step in (1, 2, 3):
        g0 = R.wide_inputs(rng, n)[1]
        before = [p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()]
        _update(p, _dev(g0, dev, 0), m, v, 0, step, 1.0, 1e-8)
        want, bound = R.tf_adam_ref(before[0], g0, before[1], before[2], LR, B1, B2, 1e-8, step)
        for x, w, b in zip((p, m, v), want, bound):
            assert R.worst(x.cpu().numpy(), w, b)[1] == 0


@pytest.mark.parametrize("rule", [0, 1])
def test_update_counts_nonfinite_gradients_and_leaves_the_rest_alone(dev, rule):
    rng = np.random.RandomState(29)
    n = 4099
    p0, g0 = R.why_inputs(rng, n)
    bad = [5, 1000, 4098]                                   # lanes of waves 0 and 3 of the vector part, and the scalar tail
    g1 = g0.copy()
    g1[bad] = [np.nan, np.inf, -np.inf]
    out = []
    for g, counter in ((g0, None), (g1, torch.zeros(1, dtype=torch.int64, device=dev))):
        p, a, b = _dev(p0, dev, 0), _dev(np.zeros(n, np.float32), dev, 0), _dev(np.zeros(n, np.float32), dev, 0)
        _update(p, _dev(g, dev, 0), a, b, rule, 1, 1.0, 1e-4, counter)       # (a NULL counter is accepted)
        out.append((p.cpu().numpy(), a.cpu().numpy(), counter))
    assert int(out[1][2]) == 3
    ok = np.ones(n, bool)
    ok[bad] = False
    assert np.array_equal(out[0][0][ok].view(np.int32), out[1][0][ok].view(np.int32))
    assert np.array_equal(out[0][1][ok].view(np.int32), out[1][1][ok].view(np.int32))
    assert not np.isfinite(out[1][0][bad]).any()            # updated as written: the NaN propagates
    # a second launch adds to the counter
    p, a, b = _dev(p0, dev, 1), _dev(np.zeros(n, np.float32), dev, 1), _dev(np.zeros(n, np.float32), dev, 1)
    _update(p, _dev(g1, dev, 1), a, b, rule, 1, 1.0, 1e-4, out[1][2])
    assert int(out[1][2]) == 6


def test_update_refuses_bad_requests_on_the_host(dev):
    t = torch.zeros(8, dtype=torch.float32, device=dev)
    l = _lib.lib()
    args = lambda n, rule, step: (n, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), rule, LR, B1, B2, 1e-4, step, 1.0, None, None)
    assert l.sph3d_train_update(*args(8, 2, 1)) == -1 and l.sph3d_train_update(*args(8, -1, 1)) == -1
    assert l.sph3d_train_update(*args(8, 0, 0)) == -1 and l.sph3d_train_update(*args(-1, 0, 1)) == -1
    assert l.sph3d_train_update(*args(0, 0, 1)) == 0
    with pytest.raises(ValueError):
        _lib.check(l.sph3d_train_update(*args(8, 0, 0)))


def test_flat_optimisers_call_the_kernel_and_equal_their_cpu_branch_within_the_bound(dev):
    rng = np.random.RandomState(31)
    p0, g0 = R.why_inputs(rng, 1025)
    for make in (lambda p: optim.FlatTFAdam(p, lr=LR, eps=1e-4), lambda p: optim.FlatNesterov(p, lr=LR, momentum=MOM)):
        fp = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dev))
        fp.grad = torch.from_numpy(g0.copy()).to(dev)
        opt = make(fp)
        opt.grad_scale = 0.125
        opt.step()
        if isinstance(opt, optim.FlatTFAdam):
            want, bound = R.tf_adam_ref(p0, g0, np.zeros_like(p0), np.zeros_like(p0), LR, B1, B2, 1e-4, 1, 0.125)
        else:
            want, bound = R.nesterov_ref(p0, g0, np.zeros_like(p0), LR, MOM, 0.125)
        assert R.worst(fp.detach().cpu().numpy(), want[0], bound[0])[1] == 0
        assert opt.t == 1 and int(opt.nonfinite) == 0 and not torch.equal(fp.detach().cpu(), torch.from_numpy(p0))


# ---- sph3d_train_metrics -------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (32, 1), (3, 1000), (2, 8192)]


def _equal(r, state):
    assert np.array_equal(r.confusion, state[0])
    assert [r.seen, r.correct, r.bad_label, r.nonfinite, r.batches] == state[1].tolist()
    assert np.float64(r.loss_sum).view(np.int64) == state[2].view(np.int64)[0]


@pytest.mark.parametrize("C", [1, 2, 13, 21, 40, 50, 64])
def test_metrics_equal_the_numpy_statement_bit_for_bit(dev, C):
    rng = np.random.RandomState(100 + C)
    m = train.TrainMetrics(C, dev)
    for B, N in SHAPES:
        logits, label, inner = R.metric_case(rng, B, N, C)
        parts = (rng.rand(7) * 3).astype(np.float32)
        d = lambda a: torch.from_numpy(a).to(dev) if a is not None else None
        # with inner and the loss; two calls accumulate
        m.reset()
        m.add(d(logits), d(label), d(inner), d(parts))
        state = train.metrics_reference(logits, label, inner, parts)
        _equal(m.read(), state)
        logits2, label2, _ = R.metric_case(rng, B, N, C, with_inner=False)
        m.add(d(logits2), d(label2), None, None)                      # inner = NULL, loss_part = NULL
        train.metrics_reference(logits2, label2, None, None, state)
        r = m.read()
        _equal(r, state)
        assert r.batches == 2 and r.seen + r.bad_label >= B * N
        m.reset()
        r = m.read()
        assert r.batches == 0 and r.seen == 0 and r.loss_sum == 0.0 and not r.confusion.any()
    # [B, C] logits with [B] labels: the ModelNet line
    logits, label, _ = R.metric_case(rng, 32, 1, C, with_inner=False)
    m.add(torch.from_numpy(logits[:, 0]).to(dev), torch.from_numpy(label[:, 0]).to(dev))
    _equal(m.read(), train.metrics_reference(logits, label))


def test_metrics_refuse_more_than_64_classes(dev):
    with pytest.raises(_lib.Sph3dError):
        train.TrainMetrics(65, dev)
    t = torch.zeros(65 * 65 + 8, dtype=torch.int64, device=dev)
    x = torch.zeros(65, dtype=torch.float32, device=dev)
    i = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().sph3d_train_metrics(1, 1, 65, _lib.ptr(x), _lib.ptr(i), None, None, 0, _lib.ptr(t), _lib.ptr(t), None, None)
    assert rc == -4
    assert not t.any()


# ---- the Trainer over a DeviceFeed ---------------------------------------------------------------------------------------------
N_PTS, BATCH, SEED = 1024, 3, 21


def _pool(dev):
    rng = np.random.RandomState(3)
    blocks = []
    for n in (1500, 1024, 900, 2000, 3000, 1100, 1300, 700, 2500):
        b = np.empty((n, 8), np.float32)
        b[:, 0:3] = rng.rand(n, 3) * np.array([1.0, 1.0, 1.5])
        b[:, 3:6] = rng.rand(n, 3)
        b[:, 6] = rng.randint(0, 13, n)
        b[:, 7] = rng.randint(0, 2, n)
        blocks.append(b)
    return feed.BlockPool.from_blocks(blocks, dev)


def _batch(pool, dev, step, ids):
    return feed.assemble(pool.rows, pool.offsets, torch.from_numpy(np.asarray(ids, np.int32)).to(dev), N_PTS, SEED, step, True)


def _trainer(pool, dev, factory=None, sample=None, **kw):
    cfg = s3dis_net.small_config(N_PTS)
    if sample is not None:
        cfg.sample = sample
    model = s3dis_net.SPH3DS3DIS(cfg, device=dev, seed=3)
    factory = factory or (lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4))
    return train.Trainer(model, model.loss, factory, train.Schedule(1e-3, BATCH, decay_step=9, decay_rate=0.7), 13,
                         prime=_batch(pool, dev, 0, [0, 1, 2]), seed=SEED, log=lambda s: None, **kw)


def _state(tr):
    return {k: v.detach().clone() for k, v in tr.model.state_dict().items()}


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def _new_feed(pool):
    return feed.DeviceFeed(pool, BATCH, N_PTS, seed=SEED, augment=True)


def test_trainer_six_steps_metrics_checkpoint_and_resume(dev, tmp_path):
    """Measured on the MI355X: uninterrupted runs from one seed differ by 5.96e-8 or 1.19e-7 in the worst parameter (never 0: the
    gradient kernels use floating-point atomics), the resumed run differed from the first uninterrupted one by 1.19e-7, 1.19e-7 and 1.49e-8 in three runs of the test."""
    pool = _pool(dev)
    ckpt = str(tmp_path)
    # ---- the uninterrupted run: two epochs of three batches, a checkpoint after the first; the steps' logits kept on the side
    tr = _trainer(pool, dev, log_every=3)
    created = _state(tr)
    assert tr.global_step == 0 and all(not v.any() for k, v in created.items() if "moving_mean" in k)
    assert all(bool((v == 1).all()) for k, v in created.items() if "moving_variance" in k)
    fresh = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(N_PTS), device=dev, seed=3)
    fresh(_batch(pool, dev, 0, [0, 1, 2])[0], is_training=True)        # a fresh model's first forward, in training mode
    assert all(torch.equal(v, created[k]) for k, v in fresh.state_dict().items() if "moving" not in k)
    assert set(fresh.state_dict()) == set(created)
    kept, add = [], tr.metrics.add
    tr.metrics.add = lambda pred, label, inner, loss_part: (kept.append((pred.detach().clone(), loss_part.clone())),
                                                            add(pred, label, inner, loss_part))[1]
    reads = tr.train_one_epoch(_new_feed(pool))
    tr.epoch = 0
    tr.save(ckpt)
    saved = dict(model=_state(tr), m=tr.opt.m.clone(), v=tr.opt.v.clone(), t=tr.opt.t, lr=tr.opt.lr, step=tr.global_step)
    f = _new_feed(pool)
    f.epoch = 1
    reads += tr.train_one_epoch(f)
    torch.cuda.synchronize()
    assert tr.global_step == 6 and len(kept) == 6 and len(reads) == 2
    final = tr.flat.flat_param.detach().clone()
    assert not _same(created, saved["model"]) and torch.isfinite(final).all()
    # the loss is finite, and each read equals the statement on the logits of its three steps and the batches of the plan
    plan = feed.epoch_plan(len(pool), BATCH, SEED, 0) + feed.epoch_plan(len(pool), BATCH, SEED, 1)
    assert [s for s, _ in plan] == list(range(6))
    for e, r in enumerate(reads):
        state = None
        for k in range(3 * e, 3 * e + 3):
            _pts, label, inner = _batch(pool, dev, *plan[k])
            state = train.metrics_reference(kept[k][0].cpu().numpy(), label.cpu().numpy(), inner.cpu().numpy(),
                                            kept[k][1].cpu().numpy(), state)
        _equal(r, state)
        assert r.batches == 3 and np.isfinite(r.mean_loss) and r.nonfinite == 0 and r.update_nonfinite == 0 and r.seen > 0
    assert saved["lr"] == 1e-3 and tr.opt.lr == 1e-3 * 0.7          # steps 3.. have decayed: 9 samples = 3 steps of B = 3

    # ---- further uninterrupted runs from the same seed: the allowance of the resumed one is the largest difference between two
    # uninterrupted runs.  The gradient kernels add with floating-point atomics, so two runs differ in the last bit of a few
    # parameters; the largest of those differences is one ulp of the parameter it falls on — 2^-24 below 1.0, 2^-23 above, and
    # the batch-norm scales sit on both sides of 1.0 — so ONE pair returns either value at random.  Six runs give fifteen pairs.
    finals = [final]
    for _ in range(5):
        tr2 = _trainer(pool, dev, log_every=3)
        tr2.fit(lambda epoch: _new_feed(pool), 2)
        torch.cuda.synchronize()
        finals.append(tr2.flat.flat_param.detach().clone())
    allowance = max(float((a - b).abs().max()) for i, a in enumerate(finals) for b in finals[i + 1:])

    # ---- load into a fresh Trainer: bit-equal state, the next batch, the continued run
    tr3 = _trainer(pool, dev, log_every=3)
    assert train.latest_checkpoint(ckpt).endswith("model.ckpt-0.pt")
    tr3.load(train.latest_checkpoint(ckpt))
    assert _same(_state(tr3), saved["model"]) and torch.equal(tr3.opt.m, saved["m"]) and torch.equal(tr3.opt.v, saved["v"])
    assert (tr3.opt.t, tr3.opt.lr, tr3.global_step, tr3.epoch) == (saved["t"], saved["lr"], 3, 0)
    lo, hi = tr3.flat.flat_param.data_ptr(), tr3.flat.flat_param.data_ptr() + 4 * tr3.flat.flat_param.numel()
    assert all(lo <= p.data_ptr() < hi for p in tr3.model.parameters())
    f = _new_feed(pool)
    f.epoch = tr3.epoch + 1
    item = next(iter(f))
    torch.cuda.current_stream().wait_event(item[-1])
    for got, want in zip(item[:3], _batch(pool, dev, *plan[3])):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    tr3.fit(lambda epoch: _new_feed(pool), 2, ckpt_dir=ckpt)
    torch.cuda.synchronize()
    assert tr3.global_step == 6 and tr3.epoch == 1 and [e for e, _ in train.checkpoints(ckpt)] == [0, 1]
    diff = float((tr3.flat.flat_param.detach() - final).abs().max())
    print("two uninterrupted runs differ by at most %.3g, the resumed run from the uninterrupted by %.3g" % (allowance, diff))
    if allowance == 0.0:
        assert torch.equal(tr3.flat.flat_param.detach().view(torch.int32), final.view(torch.int32))
    else:
        assert diff <= allowance


def test_trainer_evaluates_without_touching_the_model(dev):
    pool = _pool(dev)
    tr = _trainer(pool, dev)
    before = _state(tr)
    r = tr.eval_one_epoch(feed.DeviceFeed(pool, BATCH, N_PTS, seed=SEED, augment=False))
    assert _same(_state(tr), before) and r.batches == 3 and np.isfinite(r.mean_loss) and r.seen > 0
    assert r.confusion.sum() == r.seen and 0.0 <= r.mean_iou <= 1.0


def test_trainer_steps_with_nesterov_momentum(dev):
    pool = _pool(dev)
    tr = _trainer(pool, dev, factory=lambda p: optim.FlatNesterov(p, lr=1e-3, momentum=0.9))
    before = tr.flat.flat_param.detach().clone()
    tr.train_step(_batch(pool, dev, 0, [3, 4, 5]) + (None,))
    r = tr.metrics.read()
    assert tr.global_step == 1 and r.batches == 1 and np.isfinite(r.loss_sum) and r.update_nonfinite == 0
    assert tr.opt.accum.any() and not torch.equal(before, tr.flat.flat_param.detach())


def test_trainer_sample_key_varies_the_inverse_density_sample(dev, monkeypatch):
    """the same batch twice under sample='IDS': the plans are keyed (seed, 0) and (seed, 1) and draw different samples"""
    from sph3d_gcn_amd import sph3gcn_util as s3g_util
    pool = _pool(dev)
    tr = _trainer(pool, dev, sample="IDS")
    seen, keyed = [], s3g_util.inverse_density_sample_keyed

    def spy(neursize, nn_dist, nn_count, seed, step, level=0):
        out = keyed(neursize, nn_dist, nn_count, seed, step, level=level)
        seen.append((seed, step, level, out.clone()))
        return out
    monkeypatch.setattr(s3g_util, "inverse_density_sample_keyed", spy)
    item = _batch(pool, dev, 0, [6, 7, 8]) + (None,)
    tr.train_step(item)
    tr.train_step(item)
    torch.cuda.synchronize()
    r = tr.metrics.read()
    assert r.batches == 2 and np.isfinite(r.loss_sum) and r.nonfinite == 0 and r.update_nonfinite == 0
    levels = len(tr.model.config.radius)
    assert [(s, t, l) for s, t, l, _ in seen] == [(SEED, t, l) for t in (0, 1) for l in range(levels)]
    assert not torch.equal(seen[0][3], seen[levels][3])            # the first level's sample of step 0 and of step 1
