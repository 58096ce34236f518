"""harness/train.py and the reference optimisers of harness/optim.py without a GPU: the schedule, the metrics statement against a
literal transcription of the reference's loops, the fp32 torch branch of the optimisers against the float64 statement under the
derived bound (tests/_train_ref.py), and the Trainer on the oracle-backed CPU ops — construction without a step, bit-exact
resume, pruning, the non-finite stop and the log lines."""
import os

import numpy as np
import pytest
import torch

import _train_ref as R
from oracle import torch_ops
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd.harness import feed, optim, s3dis_net, train


# ---- schedule ------------------------------------------------------------------------------------------------------------
def test_schedule_staircase_floor_and_first_step():
    kw = dict(base=1e-3, batch_size=16, decay_step=250000, decay_rate=0.7)
    assert train.learning_rate(0, **kw) == 1e-3                                  # the first step: exponent 0
    assert 15624 * 16 == 249984 and train.learning_rate(15624, **kw) == 1e-3     # exponent 0 at global_step * B = 249 984
    assert 15625 * 16 == 250000 and train.learning_rate(15625, **kw) == 1e-3 * 0.7 == 0.0007
    assert train.learning_rate(2 * 15625, **kw) == 1e-3 * 0.7 ** 2
    assert train.learning_rate(10 ** 9, **kw) == 1e-6                            # the floor far out
    assert train.learning_rate(15625 * 19, **kw) > 1e-6 and train.learning_rate(15625 * 20, **kw) == 1e-6   # 0.7^20 = 8e-4 of base
    s = train.Schedule.for_dataset("s3dis")
    assert s(15625) == 0.0007 and s.settings()["decay_step"] == 250000
    assert train.DEFAULTS["scannet"]["decay_step"] == 500000 and train.DEFAULTS["shapenet_onehot"]["decay_step"] == 320000
    assert train.DEFAULTS["s3dis"]["eps"] == 1e-4 and train.DEFAULTS["modelnet"]["eps"] == train.DEFAULTS["shapenet"]["eps"] == 1e-8
    assert train.DEFAULTS["s3dis"]["batch_size"] == 16 and train.DEFAULTS["modelnet"]["batch_size"] == 32
    with pytest.raises(ValueError):
        train.Schedule.for_dataset("shapenet")               # its decay_step is the category's, the caller's to give
    assert train.Schedule.for_dataset("shapenet", decay_step=36 * 500)(0) == 1e-3


# ---- the metrics statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C", [(4, 300, 13), (3, 64, 2), (1, 50, 21)])
def test_metrics_reference_equals_the_reference_loops(B, N, C):
    rng = np.random.RandomState(B * 1000 + C)
    logits, label, inner = R.metric_case(rng, B, N, C)
    if B > 1:
        assert not inner[B // 2].any()
    conf, cnt, loss = train.metrics_reference(logits, label, inner, np.array([0.5, 0.25], np.float32))
    correct, seen, seen_c, correct_c, union_c, acc_c, iou_c = R.literal_eval_counts(logits, label, inner, C)
    r = train.derive(conf, cnt, loss[0])
    # the reference counts a row with a label outside [0, C) as seen (never correct, in no class): here it is bad_label
    bad = int(((inner > 0) & ((label < 0) | (label >= C))).sum())
    assert bad >= 1 or not ((label < 0) | (label >= C))[inner > 0].any()
    assert r.seen + r.bad_label == seen and r.bad_label == bad and r.correct == correct
    assert conf.sum(axis=1).tolist() == [int(x) for x in seen_c] and np.diag(conf).tolist() == [int(x) for x in correct_c]
    # the reference's union counts a prediction of class l on a row whose label is outside [0, C); those rows are not in the matrix
    pred = np.argmax(logits, 2)
    stray = [(int(((pred == l) & (inner > 0) & ((label < 0) | (label >= C))).sum())) for l in range(C)]
    assert (conf.sum(axis=0) + conf.sum(axis=1) - np.diag(conf)).tolist() == [int(u) - s for u, s in zip(union_c, stray)]
    assert np.array_equal(r.class_acc, np.array(acc_c))
    if not any(stray):
        assert np.array_equal(r.class_iou, np.array(iou_c))
        assert r.mean_iou == float(np.mean(iou_c))
    assert r.mean_class_acc == float(np.mean(acc_c)) and r.accuracy == correct / float(r.seen)
    assert r.batches == 1 and r.loss_sum == 0.75 and r.mean_loss == 0.75
    nonfin = ~np.isfinite(logits).all(axis=2) & (inner > 0) & (label >= 0) & (label < C)
    assert r.nonfinite == int(nonfin.sum())


def test_metrics_reference_without_inner_and_nan_is_a_maximum():
    rng = np.random.RandomState(5)
    logits, label, _ = R.metric_case(rng, 2, 40, 5, with_inner=False)
    logits[0, 0] = [0.0, np.nan, 9.0, np.nan, 1.0]
    label[0, 0] = 1
    logits[0, 1] = [2.0, 7.0, 7.0, 1.0, 7.0]               # tied maxima: the first
    label[0, 1] = 1
    conf, cnt, loss = train.metrics_reference(logits, label, None)
    ones = np.ones_like(label)
    conf1, cnt1, _ = train.metrics_reference(logits, label, ones)
    assert np.array_equal(conf, conf1) and np.array_equal(cnt, cnt1) and loss[0] == 0.0
    only = train.metrics_reference(logits[:1, :2], label[:1, :2])[0]
    assert only[1, 1] == 2 and only.sum() == 2
    assert cnt[0] + cnt[2] == 80 and cnt[2] == 2 and cnt[3] >= 1
    # two calls accumulate into one state
    state = train.metrics_reference(logits, label, None, np.array([1.0], np.float32))
    train.metrics_reference(logits, label, None, np.array([2.0], np.float32), state)
    assert np.array_equal(state[0], 2 * conf) and state[1][4] == 2 and state[2][0] == 3.0


def test_train_metrics_on_cpu_tensors_uses_the_statement():
    rng = np.random.RandomState(9)
    logits, label, inner = R.metric_case(rng, 3, 100, 13)
    m = train.TrainMetrics(13, "cpu")
    for _ in range(2):
        m.add(torch.from_numpy(logits), torch.from_numpy(label), torch.from_numpy(inner), torch.tensor([0.5, 1.5]))
    state = train.metrics_reference(logits, label, inner, np.array([0.5, 1.5], np.float32))
    train.metrics_reference(logits, label, inner, np.array([0.5, 1.5], np.float32), state)
    r = m.read()
    assert np.array_equal(r.confusion, state[0]) and [r.seen, r.correct, r.bad_label, r.nonfinite, r.batches] == state[1].tolist()
    assert r.loss_sum == 4.0 and r.mean_loss == 2.0
    m.reset()
    assert m.read().batches == 0 and not m.read().confusion.any()
    with pytest.raises(_lib.Sph3dError):
        train.TrainMetrics(65, "cpu")


# ---- the optimiser statement ---------------------------------------------------------------------------------------------------
def _flat(p, g):
    fp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    fp.grad = torch.from_numpy(g.copy())
    return fp


@pytest.mark.parametrize("eps", [1e-4, 1e-8])
@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_tf_adam_fp32_branch_holds_the_float64_statement(eps, scale):
    rng = np.random.RandomState(3)
    n = 20000
    for draw in (R.why_inputs, R.wide_inputs):
        p, g = draw(rng, n)
        fp = _flat(p, g)
        opt = optim.FlatTFAdam(fp, lr=1e-3, eps=eps)
        opt.grad_scale = scale
        for step in range(1, 6):
            g = draw(rng, n)[1]
            fp.grad = torch.from_numpy(g.copy())
            before = [fp.detach().numpy().copy(), opt.m.numpy().copy(), opt.v.numpy().copy()]
            opt.step()
            assert opt.t == step
            want, bound = R.tf_adam_ref(before[0], g, before[1], before[2], 1e-3, 0.9, 0.999, eps, step, scale)
            for name, got, w, b in zip("pmv", (fp.detach().numpy(), opt.m.numpy(), opt.v.numpy()), want, bound):
                ratio, outside = R.worst(got, w, b)
                assert outside == 0, (draw.__name__, step, name, ratio)
            zero = (g == 0) & (before[1] == 0) & (before[2] == 0)
            assert np.array_equal(fp.detach().numpy()[zero], before[0][zero])
        assert int(opt.nonfinite) == 0


def test_nesterov_fp32_branch_holds_the_float64_statement():
    rng = np.random.RandomState(4)
    n = 20000
    for draw in (R.why_inputs, R.wide_inputs):
        p, g = draw(rng, n)
        fp = _flat(p, g)
        opt = optim.FlatNesterov(fp, lr=1e-3, momentum=0.9)
        opt.grad_scale = 0.125
        for step in range(1, 5):
            g = draw(rng, n)[1]
            fp.grad = torch.from_numpy(g.copy())
            before = [fp.detach().numpy().copy(), opt.accum.numpy().copy()]
            opt.step()
            want, bound = R.nesterov_ref(before[0], g, before[1], 1e-3, 0.9, 0.125)
            for name, got, w, b in zip("pa", (fp.detach().numpy(), opt.accum.numpy()), want, bound):
                ratio, outside = R.worst(got, w, b)
                assert outside == 0, (draw.__name__, step, name, ratio)


def test_the_bound_separates_the_two_adam_forms():
    """A condition on the BOUND: with eps = 1e-4, steps 1..10 and gradients N(0,1) 10^U(-6,-1), p ~ N(0, 0.1), the torch form
    (sph3d_adam_step's arithmetic, in float64, from the same state) lies outside the TF form's bound for at least half of the
    elements at every step.  A bound that the other kernel passed would prove nothing."""
    rng = np.random.RandomState(11)
    n = 50000
    p, g = R.why_inputs(rng, n)
    fp = _flat(p, g)
    opt = optim.FlatTFAdam(fp, lr=1e-3, eps=1e-4)
    for step in range(1, 11):
        g = R.why_inputs(rng, n)[1]
        fp.grad = torch.from_numpy(g.copy())
        state = (fp.detach().numpy().copy(), opt.m.numpy().copy(), opt.v.numpy().copy())
        want, bound = R.tf_adam_ref(state[0], g, state[1], state[2], 1e-3, 0.9, 0.999, 1e-4, step)
        other = torch_adam_ref = R.torch_adam_ref(state[0], g, state[1], state[2], 1e-3, 0.9, 0.999, 1e-4, step)[0]
        outside = float((np.abs(other - want[0]) > bound[0]).mean())
        print("step %d: torch form outside the TF bound for %.2f %% of the elements" % (step, 100 * outside))
        assert outside >= 0.5, (step, outside)
        opt.step()


def test_flat_tf_adam_surface_and_state_dict_round_trip():
    rng = np.random.RandomState(2)
    p, g = R.why_inputs(rng, 1000)
    g[7] = np.nan
    g[400] = np.inf
    fp = _flat(p, g)
    opt = optim.FlatTFAdam(fp, lr=1e-3, eps=1e-4)
    opt.step()
    assert int(opt.nonfinite) == 2 and np.isnan(fp.detach().numpy()[7])
    ok = np.ones(1000, bool)
    ok[[7, 400]] = False
    want, bound = R.tf_adam_ref(p, g, np.zeros_like(p), np.zeros_like(p), 1e-3, 0.9, 0.999, 1e-4, 1)
    assert R.worst(fp.detach().numpy()[ok], want[0][ok], bound[0][ok])[1] == 0
    for grp in opt.param_groups:
        grp["lr"] = 5e-4
    assert opt.lr == 5e-4
    sd = opt.state_dict()
    fp2 = _flat(p, g)
    other = optim.FlatTFAdam(fp2, lr=1.0, eps=1e-4)
    other.load_state_dict(sd)
    assert other.t == 1 and other.lr == 5e-4 and torch.equal(other.m[ok], opt.m[ok]) and torch.equal(other.v[ok], opt.v[ok])
    opt.zero_grad()
    assert not fp.grad.any()
    assert "not the reference's" in optim.FlatAdam.__doc__


# ---- the Trainer on the oracle ops ---------------------------------------------------------------------------------------------
N_PTS, BATCH, SEED = 1024, 2, 5


def _blocks():
    rng = np.random.RandomState(1)
    out = []
    for n in (1500, 1024, 900, 2000):
        b = np.empty((n, 8), np.float32)
        b[:, 0:3] = rng.rand(n, 3) * np.array([1.0, 1.0, 1.5])
        b[:, 3:6] = rng.rand(n, 3)
        b[:, 6] = rng.randint(0, 13, n)
        b[:, 7] = rng.randint(0, 2, n)
        out.append(b)
    return out


class HostFeed:
    """feed.DeviceFeed's batches from its numpy statement, as CPU tensors; no event"""

    def __init__(self, blocks, epoch=0, augment=True):
        self.blocks, self.epoch, self.augment = blocks, epoch, augment
        self.sizes = np.array([len(b) for b in blocks])

    def batch(self, step, ids):
        ref = feed.assemble_reference(self.sizes, ids, N_PTS, SEED, step, self.augment)
        pts, label, inner = feed.apply_reference(self.blocks, ids, ref)
        # (int64 labels: the CPU branch of s3dis_net.get_loss is F.cross_entropy, which takes no int32 targets)
        return torch.from_numpy(pts.astype(np.float32)), torch.from_numpy(label).long(), torch.from_numpy(inner), None

    def __iter__(self):
        plan = feed.epoch_plan(len(self.blocks), BATCH, SEED, self.epoch)
        self.epoch += 1
        for step, ids in plan:
            yield self.batch(step, ids)


def _trainer(blocks, log=None, **kw):
    model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(N_PTS), device=None, seed=3)
    prime = HostFeed(blocks).batch(0, np.array([0, 1]))[:3]
    return train.Trainer(model, model.loss, lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4),
                         train.Schedule(1e-3, BATCH, decay_step=4, decay_rate=0.7), 13, line=train.s3dis_line, prime=prime, seed=SEED,
                         log=(log.append if log is not None else (lambda s: None)), **kw)


def _state(tr):
    return {k: v.detach().clone() for k, v in tr.model.state_dict().items()}


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the uninterrupted four steps (two epochs of two batches, a checkpoint after each), and what was saved after two"""
    blocks = _blocks()
    ckpt = str(tmp_path_factory.mktemp("ckpt"))
    log = []
    with torch_ops.patched_util():
        tr = _trainer(blocks, log, log_every=2)
        losses = []
        inner_loss = tr.loss_fn
        tr.loss_fn = lambda *a: (lambda l: (losses.append(float(l.detach())), l)[1])(inner_loss(*a))
        fresh = _state(tr)
        tr.fit(lambda epoch: HostFeed(blocks), 1, ckpt_dir=ckpt)
        after_two = dict(model=_state(tr), m=tr.opt.m.clone(), v=tr.opt.v.clone(), t=tr.opt.t, lr=tr.opt.lr, step=tr.global_step,
                         epoch=tr.epoch)
        tr.fit(lambda epoch: HostFeed(blocks), 2, ckpt_dir=None)
    return dict(blocks=blocks, ckpt=ckpt, log=log, losses=losses, fresh=fresh, after_two=after_two, final=_state(tr),
                final_m=tr.opt.m.clone(), final_step=tr.global_step, final_lr=tr.opt.lr)


def test_construction_takes_no_step(runs):
    """the parameters equal those a fresh model creates in its first (training) forward, the moving statistics are the initial
    ones, nothing was counted, and the parameters are views of the flat buffer"""
    blocks = runs["blocks"]
    with torch_ops.patched_util():
        model = s3dis_net.SPH3DS3DIS(s3dis_net.small_config(N_PTS), device=None, seed=3)
        pts, label, inner, _ = HostFeed(blocks).batch(0, np.array([0, 1]))
        model(pts, is_training=True)
    created = {k: v.detach() for k, v in model.state_dict().items()}
    fresh = runs["fresh"]
    assert set(fresh) == set(created)
    n_stats = 0
    for k, v in fresh.items():
        if "moving_mean" in k:
            assert not v.any()
            n_stats += 1
        elif "moving_variance" in k:
            assert (v == 1).all()
            n_stats += 1
        else:
            assert torch.equal(v, created[k]), k
    assert n_stats >= 2 and any(not torch.equal(created[k], fresh[k]) for k in fresh if "moving" in k)


def test_four_steps_log_the_true_means(runs):
    assert runs["final_step"] == 4 and len(runs["losses"]) == 4
    log = runs["log"]
    assert log[0] == '**** EPOCH 000 ****' and log[1] == ' ---- batch: 002 ----'
    # accumulated in float64 from the fp32 loss of each step: the true mean of the two, not the reference's sum / 10
    assert log[2] == 'mean loss: %f' % ((runs["losses"][0] + runs["losses"][1]) / 2)
    assert log[6] == 'mean loss: %f' % ((runs["losses"][2] + runs["losses"][3]) / 2)
    assert log[3].startswith('accuracy: ') and 0.0 <= float(log[3].split()[1]) <= 1.0
    # the schedule ran: decay_step = 4 samples = 2 steps of B = 2
    assert runs["after_two"]["lr"] == 1e-3 and runs["final_lr"] == 1e-3 * 0.7
    assert not _same(runs["fresh"], runs["after_two"]["model"]) and not _same(runs["after_two"]["model"], runs["final"])


def test_resume_is_bit_exact_and_keeps_the_flat_views(runs):
    blocks, saved = runs["blocks"], runs["after_two"]
    assert train.latest_checkpoint(runs["ckpt"]) == os.path.join(runs["ckpt"], "model.ckpt-0.pt")
    with torch_ops.patched_util():
        tr = _trainer(blocks)
        tr.load(train.latest_checkpoint(runs["ckpt"]))
        assert _same(_state(tr), saved["model"])
        assert torch.equal(tr.opt.m, saved["m"]) and torch.equal(tr.opt.v, saved["v"])
        assert (tr.opt.t, tr.opt.lr, tr.global_step, tr.epoch) == (saved["t"], saved["lr"], saved["step"], saved["epoch"]) == (2, 1e-3, 2, 0)
        lo, hi = tr.flat.flat_param.data_ptr(), tr.flat.flat_param.data_ptr() + 4 * tr.flat.flat_param.numel()
        for p in tr.model.parameters():
            assert lo <= p.data_ptr() < hi and p.data.untyped_storage().data_ptr() == tr.flat.flat_param.data.untyped_storage().data_ptr()
        tr.fit(lambda epoch: HostFeed(blocks), 2, ckpt_dir=runs["ckpt"])          # loads the newest again, continues at epoch 1
        assert tr.global_step == 4 and tr.epoch == 1
        assert _same(_state(tr), runs["final"]) and torch.equal(tr.opt.m, runs["final_m"])
        assert [e for e, _p in train.checkpoints(runs["ckpt"])] == [0, 1]
        # max_to_keep prunes the oldest
        tr.max_to_keep = 2
        tr.save(runs["ckpt"], 2)
        assert [e for e, _p in train.checkpoints(runs["ckpt"])] == [1, 2]
        tr.max_to_keep = 1
        tr.save(runs["ckpt"], 7)
        assert [e for e, _p in train.checkpoints(runs["ckpt"])] == [7]


def test_a_planted_nan_stops_the_trainer_at_the_next_log_interval(runs):
    blocks = runs["blocks"]
    with torch_ops.patched_util():
        tr = _trainer(blocks, log_every=2)
        backward = tr.flat.backward

        def planted(loss):
            out = backward(loss)
            if tr.global_step == 0:
                tr.flat.flat[3] = float("nan")
            return out
        tr.flat.backward = planted
        with pytest.raises(_lib.Sph3dError, match=r"steps 0\.\.1"):
            tr.train_one_epoch(HostFeed(blocks))
        assert tr.global_step == 2            # the first step went through: the stop is at the log interval


def test_eval_one_epoch_changes_nothing_and_reports_the_reference_lines(runs):
    blocks = runs["blocks"]
    log = []
    with torch_ops.patched_util():
        tr = _trainer(blocks, log)
        before = _state(tr)
        r = tr.eval_one_epoch(HostFeed(blocks, augment=False))
        assert _same(_state(tr), before) and tr.global_step == 0
        state = None
        with torch.no_grad():
            for pts, label, inner, _ in HostFeed(blocks, augment=False):
                pred, _e = tr.model(pts, is_training=False)
                state = train.metrics_reference(pred.numpy(), label.numpy(), inner.numpy(), None, state)
    assert np.array_equal(r.confusion, state[0]) and [r.seen, r.correct] == state[1][:2].tolist() and r.batches == 2
    assert log[0].startswith('eval mean loss: ') and log[1] == 'eval overall accuracy: %f' % r.accuracy
    assert log[2] == 'eval avg class acc: %f' % r.mean_class_acc and log[-1] == 'eval mIoU of all classes: %f' % r.mean_iou
    assert len(log) == 4 + 13 and np.isfinite(r.mean_loss)
