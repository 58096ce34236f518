"""The guarded update on the device (csrc/train.hip: sph3d_train_update_guarded, sph3d_guard_restore) against harness/guard.py's
statement, bit for bit: the sum of squares and the count at every launch form, the state words from the device's own sum, the
update against sph3d_train_update when nothing triggers, the clipped update under tests/_train_ref.py's bounds, the EMA chain,
the skip; then the Trainer in deterministic mode over a DeviceFeed."""
import math

import numpy as np
import pytest
import torch

import _train_ref as R
from sph3d_gcn_amd import _lib
from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd.harness import feed, guard, optim, s3dis_net, train

pytestmark = pytest.mark.gpu

LR, B1, B2, MOM, EPS = 1e-3, 0.9, 0.999, 0.9, 1e-4
L = guard.LANES
SIZES = [1, 3, 4, 5, 255, 1023, L - 1, L, L + 1, 4 * L + 7, 2 ** 20 + 13]
THIRD = R.f32(1.0 / 3.0)


def _dev(a, dev, offset=0):
    """a device copy of `a` whose first element lies `offset` elements past a 16-byte boundary"""
    t = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
    assert t.data_ptr() % 16 == 0
    view = t[offset:offset + a.size]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


class Bufs:
    """p, g, the two slots, the EMA (or None), the state words, the workspace and a counter on the device"""

    def __init__(self, dev, p, offset=0, ema=False, g_offset=None):
        n = p.size
        self.n, self.dev, self.offset = n, dev, offset
        self.g_offset = offset if g_offset is None else g_offset
        self.p = _dev(p, dev, offset)
        self.s0, self.s1 = _dev(np.zeros(n, np.float32), dev, offset), _dev(np.zeros(n, np.float32), dev, offset)
        self.ema = _dev(p, dev, offset) if ema else None
        self.state = torch.from_numpy(guard.new_state()).to(dev)
        self.ws = torch.empty(_lib.lib().sph3d_train_guard_workspace(n), dtype=torch.uint8, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)

    def step(self, g, rule, scale=1.0, clip=None, skip=False, decay=None, lr=LR):
        gd = _dev(g, self.dev, self.g_offset)
        _lib.check(_lib.lib().sph3d_train_update_guarded(
            self.n, _lib.ptr(self.p), _lib.ptr(gd), _lib.ptr(self.s0), _lib.ptr(self.s1), _lib.ptr(self.ema), rule, lr,
            B1 if rule == 0 else MOM, B2, EPS, scale, clip if clip is not None else 0.0, 1 if skip else 0,
            decay if decay is not None else 0.0, _lib.ptr(self.state), _lib.ptr(self.counter), _lib.ptr(self.ws), self.ws.numel(),
            _lib.stream_ptr()))

    def words(self):
        return self.state.cpu().numpy().copy()

    def host(self):
        out = [self.p.cpu().numpy(), self.s0.cpu().numpy(), self.s1.cpu().numpy()]
        return out + ([self.ema.cpu().numpy()] if self.ema is not None else [])


def _same_double(a, b):
    """the same bits, or both NaN (IEEE 754 leaves a NaN's payload open; nothing reads S then)"""
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.int64) == np.float64(b).view(np.int64)


def _wide(rng, n):
    """magnitudes 1e-20 .. 1e10: the squares neither fit fp32 at the small end nor at the large one"""
    return (np.where(rng.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-20, 10, n)).astype(np.float32)


# ---- S and bad -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sum_cases():
    """one gradient per n and its statement per grad_scale, computed once"""
    rng = np.random.RandomState(61)
    cases = {}
    for n in SIZES:
        g = _wide(rng, n)
        cases[n] = (g, {s: guard.measure(g, s)[1:] for s in (1.0, 0.125, THIRD)})
    return cases


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_sum_of_squares_equals_the_statement_bit_for_bit(dev, sum_cases, offset):
    """offset 0: 16-byte loads; 1-3: scalar loads with the same lane mapping.  (Only the gradient's alignment matters.)"""
    for n in SIZES:
        g, want = sum_cases[n]
        b = Bufs(dev, np.zeros(n, np.float32), 0, g_offset=offset)
        for scale, (S, bad) in want.items():
            assert bad == 0 and np.isfinite(S) and S > 0
            b.step(g, 1, scale)
            w = guard.fields(b.words())
            assert w["bad"] == 0 and np.float64(w["S"]).view(np.int64) == np.float64(S).view(np.int64), (n, scale, w["S"], S)
            first = b.words()
            b.step(g, 1, scale)                                           # a second run: the same bits
            again = b.words()
            assert again[guard.S] == first[guard.S] and again[guard.BAD] == 0
    assert int(b.counter) == 0


@pytest.mark.parametrize("offset", [0, 3])
def test_nonfinite_elements_are_counted_wherever_they_lie(dev, offset):
    rng = np.random.RandomState(67)
    n = 4 * L + 7
    base = _wide(rng, n)
    places = {"first": [0], "last": [n - 1], "tail": [n - 2, n - 3], "lane boundary": [1023, 1024], "lane boundary, fifth trip": [4 * L - 1, 4 * L],
              "all": [0, 1023, 1024, L - 1, L, n - 5, n - 1]}
    b = Bufs(dev, np.zeros(n, np.float32), 0, g_offset=offset)
    total = 0
    for name, idx in places.items():
        for value in (np.nan, np.inf, -np.inf):
            g = base.copy()
            g[idx] = value
            _gg0, S, bad = guard.measure(g, 0.125)
            assert bad == len(idx)
            b.step(g, 1, 0.125, skip=True)
            first = b.words()
            w = guard.fields(first)
            assert w["bad"] == bad and w["flag"] == 0 and _same_double(w["S"], S), (name, value, w["S"], S)
            total += bad
            b.step(g, 1, 0.125, skip=True)
            again = b.words()
            assert again[guard.S] == first[guard.S] and again[guard.BAD] == bad     # (the same run twice: the same bits, a NaN's too)
            total += bad
    assert int(b.counter) == total and guard.fields(b.words())["applied"] == 0
    assert not b.p.any() and not b.s0.any()
    # an overflow of the SCALED element counts, an underflow does not
    g = base.copy()
    g[7] = 3e38
    b.step(g, 1, 2.0, skip=True)
    assert guard.fields(b.words())["bad"] == 1 == guard.measure(g, 2.0)[2]


# ---- the state words -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1], ids=["tf-adam", "nesterov"])
def test_state_words_equal_the_statement_from_the_devices_own_sum(dev, rule):
    rng = np.random.RandomState(71 + rule)
    n = 4099
    p0, _ = R.why_inputs(rng, n)
    b = Bufs(dev, p0, 0, ema=True)
    want = guard.new_state()
    counter = np.zeros(1, np.int64)
    clip, decay = 0.05, 0.99
    for step in range(12):
        g = R.why_inputs(rng, n)[1]
        if step in (3, 7):
            g[step] = np.nan if step == 3 else -np.inf
        if step == 5:
            g *= np.float32(1e-3)                                         # below the threshold: not clipped
        skip = step != 7                                                  # step 7: the NaN propagates and is counted
        lr = LR * 0.7 ** (step // 4)
        b.step(g, rule, THIRD, clip=clip, skip=skip, decay=decay, lr=lr)
        got = b.words()
        S_dev, bad_dev = float(got.view(np.float64)[guard.S]), int(got[guard.BAD])
        _gg0, S, bad = guard.measure(g, THIRD)
        assert bad_dev == bad and _same_double(S_dev, S)
        guard.decide(want, S_dev, bad_dev, rule, lr, B1 if rule == 0 else MOM, B2, clip, skip, decay, counter)
        for k, name in enumerate(guard.FIELDS):
            if name in ("S", "last_norm") and math.isnan(guard.fields(want)[name]):
                assert math.isnan(guard.fields(got)[name]), (step, name)
            else:
                assert got[k] == want[k], (step, name, guard.fields(got), guard.fields(want))
        assert not got[len(guard.FIELDS):].any()
    w = guard.fields(got)
    assert (w["applied"], w["skipped"]) == (11, 1) and 0 < w["clipped_steps"] < 11 and int(b.counter) == counter[0] == 2


# ---- the update ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-by-one"])
@pytest.mark.parametrize("rule", [0, 1], ids=["tf-adam", "nesterov"])
def test_nothing_triggering_equals_the_unguarded_update_bit_for_bit(dev, rule, offset):
    # the precondition, asserted on the CPU: the running powers round to the lr_t sph3d_train_update forms with pow()
    p1 = p2 = 1.0
    for t in range(1, 11):
        p1, p2 = p1 * R.f32(B1), p2 * R.f32(B2)
        assert guard.lr_t_from_powers(LR, p1, p2) == R.lr_t(LR, B1, B2, t)
    rng = np.random.RandomState(73 + rule)
    for n in (5, 4099):
        p0, _ = R.why_inputs(rng, n)
        a, b = Bufs(dev, p0, offset), Bufs(dev, p0, offset)
        for step in range(1, 11):
            g = (R.wide_inputs if step % 2 else R.why_inputs)(rng, n)[1]
            _lib.check(_lib.lib().sph3d_train_update(n, _lib.ptr(a.p), _lib.ptr(_dev(g, dev, offset)), _lib.ptr(a.s0), _lib.ptr(a.s1), rule,
                                                     LR, B1 if rule == 0 else MOM, B2, EPS, step, 0.125, None, _lib.stream_ptr()))
            b.step(g, rule, 0.125, clip=1e30, skip=True)
            for name, x, y in zip(("p", "slot0", "slot1"), a.host(), b.host()):
                assert np.array_equal(_bits(x), _bits(y)), (n, step, name)
        assert guard.stats(b.words())[:3] == (10, 0, 0)
        assert (not b.s1.any()) == (rule == 1)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-by-one"])
@pytest.mark.parametrize("rule", [0, 1], ids=["tf-adam", "nesterov"])
def test_clipped_steps_hold_the_float64_bounds_and_the_ema_chain(dev, rule, offset):
    """the bounds of tests/_train_ref.py with gg = fl32(c32 fl32(s g)) as the gradient; the EMA from the kernel's own p'"""
    rng = np.random.RandomState(79 + rule)
    n, clip, decay, scale = 4099, 0.25, 0.9, 0.125
    p0, _ = R.why_inputs(rng, n)
    b = Bufs(dev, p0, offset, ema=True)
    for step in range(1, 5):
        g = (rng.randn(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
        before = b.host()
        b.step(g, rule, scale, clip=clip, decay=decay)
        w = guard.fields(b.words())
        gg0, S, bad = guard.measure(g, scale)
        assert w["flag"] == 3 and w["clipped_steps"] == step and w["c32"] == R.f32(R.f32(clip) / (math.sqrt(S) + 1e-6)) < 1
        gg = np.float32(w["c32"]) * gg0
        assert math.sqrt(math.fsum((gg.astype(np.float64) ** 2).tolist())) <= clip * (1 + 2.0 ** -22)
        got = b.host()
        if rule == 0:
            want, bound = R.tf_adam_ref(before[0], gg, before[1], before[2], LR, B1, B2, EPS, step)
            assert w["lr_t"] == R.lr_t(LR, B1, B2, step)
        else:
            want, bound = R.nesterov_ref(before[0], gg, before[1], LR, MOM)
            assert w["lr_t"] == R.f32(LR) and not got[2].any()
        for name, x, y, e in zip("pmv", got, want, bound):
            ratio, outside = R.worst(x, y, e)
            assert outside == 0, (step, name, ratio)
        a = step - 1
        om = np.float32(w["om"])
        assert w["om"] == R.f32(1.0 - min(R.f32(decay), (1.0 + a) / (10.0 + a)))
        chain = before[3] - (before[3] - got[0]) * om                   # fp32, every operation rounded once
        assert chain.dtype == np.float32 and np.array_equal(_bits(got[3]), _bits(chain)), step
    assert not np.array_equal(got[3], got[0])
    # the whole step equals the statement bit for bit, too (rule, clip and EMA from the same state)
    host = [x.copy() for x in got]
    state = b.words()
    g = (rng.randn(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    b.step(g, rule, scale, clip=clip, decay=decay)
    guard.step(state, host[0], g, host[1], host[2] if rule == 0 else None, host[3], rule, LR, B1 if rule == 0 else MOM, B2, EPS, scale,
               clip, False, decay)
    assert np.array_equal(state, b.words())
    for name, x, y in zip(("p", "slot0", "slot1", "ema"), b.host(), host):
        assert np.array_equal(_bits(x), _bits(y)), name


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-by-one"])
@pytest.mark.parametrize("rule", [0, 1], ids=["tf-adam", "nesterov"])
def test_a_skipped_step_changes_nothing_and_the_next_is_as_if_it_never_was(dev, rule, offset):
    rng = np.random.RandomState(83 + rule)
    n = 4099
    p0, _ = R.why_inputs(rng, n)
    a, b = Bufs(dev, p0, offset, ema=True), Bufs(dev, p0, offset, ema=True)
    kw = dict(clip=0.5, skip=True, decay=0.99)
    grads = [R.why_inputs(rng, n)[1] for _ in range(4)]
    for g in grads[:2]:
        a.step(g, rule, **kw)
        b.step(g, rule, **kw)
    before, words = b.host(), guard.fields(b.words())
    for value, where in ((np.nan, 5), (np.inf, 1000), (-np.inf, n - 1)):   # the vector part's waves 0 and 3, the scalar tail
        bad = grads[2].copy()
        bad[where] = value
        b.step(bad, rule, **kw)
        for name, x, y in zip(("p", "slot0", "slot1", "ema"), before, b.host()):
            assert np.array_equal(_bits(x), _bits(y)), (value, name)
        w = guard.fields(b.words())
        assert w["flag"] == 0 and w["bad"] == 1
        for k in ("applied", "clipped_steps", "b1pow", "b2pow", "last_norm", "max_norm_seen", "lr_t", "c32", "om"):
            assert w[k] == words[k], k
    assert w["skipped"] == 3 and int(b.counter) == 3 and int(a.counter) == 0
    for g in grads[2:]:
        a.step(g, rule, **kw)
        b.step(g, rule, **kw)
        for name, x, y in zip(("p", "slot0", "slot1", "ema"), a.host(), b.host()):
            assert np.array_equal(_bits(x), _bits(y)), name
    wa, wb = guard.fields(a.words()), guard.fields(b.words())
    assert {k: v for k, v in wa.items() if k != "skipped"} == {k: v for k, v in wb.items() if k != "skipped"} and wa["applied"] == 4
    assert not np.array_equal(before[0], b.host()[0])


def test_restore_copies_only_after_a_skip_and_bad_requests_are_refused(dev):
    rng = np.random.RandomState(89)
    l = _lib.lib()
    for n in (1, 7, 1025):
        for offset in (0, 1):
            src, live = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
            s, d = _dev(src, dev, offset), _dev(live, dev, 0)
            state = torch.from_numpy(guard.new_state()).to(dev)
            for flag, want in ((1, live), (3, live), (0, src)):
                state[guard.FLAG] = flag
                _lib.check(l.sph3d_guard_restore(n, _lib.ptr(d), _lib.ptr(s), _lib.ptr(state), _lib.stream_ptr()))
                assert np.array_equal(_bits(d.cpu().numpy()), _bits(want)), (n, offset, flag)
    # through optim.Guard, after a real skipped step
    fp = torch.nn.Parameter(torch.zeros(64, device=dev))
    opt = optim.FlatTFAdam(fp, lr=LR, eps=EPS)
    opt.guard = optim.Guard(skip_nonfinite=True)
    keep, work = torch.ones(40, device=dev), torch.zeros(40, device=dev)
    fp.grad = torch.ones(64, device=dev)
    opt.step()
    opt.guard.restore(work, keep)
    assert not work.any() and opt.guard.read()[:2] == (1, 0)
    fp.grad[3] = float("inf")
    opt.step()
    opt.guard.restore(work, keep)
    assert bool((work == 1).all()) and opt.guard.read()[:2] == (1, 1) and int(opt.nonfinite) == 1
    # refused on the host, before any launch
    t = torch.zeros(8, dtype=torch.float32, device=dev)
    state = torch.from_numpy(guard.new_state()).to(dev)
    ws = torch.zeros(l.sph3d_train_guard_workspace(8), dtype=torch.uint8, device=dev)
    assert l.sph3d_train_guard_workspace(8) == l.sph3d_train_guard_workspace(1 << 22) == 256 * 16

    def call(n=8, p=t, g=t, s0=t, s1=t, ema=None, rule=0, decay=0.0, st=state, w=ws, wb=None, clip=0.0):
        return l.sph3d_train_update_guarded(n, _lib.ptr(p), _lib.ptr(g), _lib.ptr(s0), _lib.ptr(s1), _lib.ptr(ema), rule, LR, B1, B2, EPS,
                                            1.0, clip, 1, decay, _lib.ptr(st), None, _lib.ptr(w), w.numel() if wb is None and w is not None else (wb or 0),
                                            None)
    assert call(rule=2) == -1 and call(rule=-1) == -1 and call(n=-1) == -1
    assert call(p=None) == -1 and call(g=None) == -1 and call(s0=None) == -1 and call(s1=None) == -1 and call(st=None) == -1
    assert call(ema=t, decay=0.0) == -1 and call(ema=t, decay=1.0) == -1 and call(clip=float("nan")) == -1
    assert call(wb=ws.numel() - 1) == -2 and call(w=None) == -2
    with pytest.raises(ValueError):
        _lib.check(call(rule=2))
    g2, a2 = torch.zeros_like(t), torch.zeros_like(t)
    assert call(n=0) == 0 and call(rule=1, g=g2, s0=a2, s1=None) == 0      # (Nesterov needs no second slot)
    assert l.sph3d_guard_restore(8, None, _lib.ptr(t), _lib.ptr(state), None) == -1
    assert l.sph3d_guard_restore(8, _lib.ptr(t), None, _lib.ptr(state), None) == -1
    assert l.sph3d_guard_restore(8, _lib.ptr(t), _lib.ptr(t), None, None) == -1 and l.sph3d_guard_restore(-1, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert guard.stats(state.cpu().numpy())[:2] == (1, 0)                  # only the one accepted call with n > 0 ran
    with pytest.raises(ValueError):
        optim.FlatAdam(fp, guard=optim.Guard(clip_norm=1.0))


def test_flat_optimisers_issue_the_guarded_entry_and_equal_their_cpu_branch(dev):
    rng = np.random.RandomState(97)
    n = 4099
    p0, _ = R.why_inputs(rng, n)
    kw = dict(clip_norm=0.05, skip_nonfinite=True, ema_decay=0.99)
    for make in (lambda p: optim.FlatTFAdam(p, lr=LR, eps=EPS), lambda p: optim.FlatNesterov(p, lr=LR, momentum=MOM)):
        fd, fc = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dev)), torch.nn.Parameter(torch.from_numpy(p0.copy()))
        od, oc = make(fd), make(fc)
        od.guard, oc.guard = optim.Guard(**kw), optim.Guard(**kw)
        od.grad_scale = oc.grad_scale = 0.125
        for step in range(5):
            g = R.why_inputs(rng, n)[1] * np.float32(8.0)
            if step == 2:
                g[11] = np.nan
            fd.grad, fc.grad = torch.from_numpy(g.copy()).to(dev), torch.from_numpy(g.copy())
            od.step()
            oc.step()
        assert np.array_equal(od.guard.words()[1:], oc.guard.words()[1:]) and od.guard.read()[:2] == (4, 1)
        assert od.guard.read().clipped_steps > 0
        assert torch.equal(fd.detach().cpu().view(torch.int32), fc.detach().view(torch.int32))
        assert torch.equal(od.guard.ema.cpu().view(torch.int32), oc.guard.ema.view(torch.int32))
        for k in od.slots:
            assert torch.equal(od.state[k].cpu().view(torch.int32), oc.state[k].view(torch.int32))
        sd = od.state_dict()
        assert sd["step"] == 4 and int(od.nonfinite) == 1 == int(oc.nonfinite)


# ---- the Trainer over a DeviceFeed, deterministic mode ----------------------------------------------------------------------------
T_PTS, BATCH, SEED = 1024, 3, 21


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


def _coloured_input(points, config):
    """centred coordinates AND the colours.  The S3DIS net's own input is the reference's, coordinates + points[:, :, 6:]
    (models/SPH3D_s3dis.py:42), which a six-channel batch leaves empty: its colours never reach the model, and a NaN planted in
    one would test nothing."""
    xyz = points[:, :, 0:3]
    return torch.cat((s3dis_net.normalize_xyz(xyz) if config.normalize else xyz, points[:, :, 3:]), dim=2)


class ColouredS3DIS(s3dis_net.SPH3DS3DIS):
    def forward(self, points, is_training=True, graphs=None, points_ready=None, sample_key=(0, 0)):
        with s3g_util.variable_store(self.store):
            return s3dis_net.get_model(points, is_training, self.config, graphs=graphs, points_ready=points_ready,
                                       net_input=_coloured_input, sample_key=sample_key)


def _trainer(pool, dev, net=s3dis_net.SPH3DS3DIS, **kw):
    model = net(s3dis_net.small_config(T_PTS), device=dev, seed=3)
    prime = feed.assemble(pool.rows, pool.offsets, torch.from_numpy(np.asarray([0, 1, 2], np.int32)).to(dev), T_PTS, SEED, 0, True)
    return train.Trainer(model, model.loss, lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-4),
                         train.Schedule(1e-3, BATCH, decay_step=9, decay_rate=0.7), 13, prime=prime, seed=SEED, log=lambda s: None,
                         log_every=3, deterministic=True, **kw)


def _snapshot(tr):
    torch.cuda.synchronize()
    s = {"flat_param": tr.flat.flat_param.detach().clone(), "opt.m": tr.opt.m.clone(), "opt.v": tr.opt.v.clone()}
    if tr.guard is not None and tr.guard.ema is not None:
        s["ema"] = tr.guard.ema.clone()
    for k, v in tr.model.state_dict().items():
        s["model." + k] = v.detach().clone()
    return s


def _first_difference(a, b):
    assert set(a) == set(b)
    for k in a:
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            return k
    return None


def _items(pool, epoch=0):
    f = feed.DeviceFeed(pool, BATCH, T_PTS, seed=SEED, augment=True)
    f.epoch = epoch
    return f


def test_trainer_with_a_guard_that_never_triggers_ends_with_the_plain_bits(dev):
    pool = _pool(dev)
    plain, guarded = _trainer(pool, dev), _trainer(pool, dev, clip_norm=1e30, skip_nonfinite=True)
    assert plain.guard is None and guarded._buf_flat is not None
    for tr in (plain, guarded):
        f = _items(pool)
        for item in f:
            tr.train_step(item, f)
        assert tr.global_step == 3
    a, b = _snapshot(plain), _snapshot(guarded)
    assert _first_difference(a, b) is None, _first_difference(a, b)
    assert guarded.guard.read()[:3] == (3, 0, 0) and torch.isfinite(b["flat_param"]).all()
    assert guarded.metrics.read().update_nonfinite == 0


def test_trainer_skips_a_batch_with_a_nan_colour_and_goes_on(dev):
    pool = _pool(dev)
    tr = _trainer(pool, dev, net=ColouredS3DIS, clip_norm=1e30, skip_nonfinite=True, ema_decay=0.9)
    f = _items(pool)
    items = []
    for item in f:                                                        # copies that outlive the feed's two output sets
        torch.cuda.current_stream().wait_event(item[-1])
        items.append(tuple(t.clone() for t in item[:-1]) + (None,))
    torch.cuda.synchronize()
    tr.train_step(items[0])
    one = _snapshot(tr)
    pts = items[1][0].clone()
    pts[1, 17, 4] = float("nan")                                          # a colour channel: never the coordinates
    tr.train_step((pts,) + tuple(items[1][1:]))
    two = _snapshot(tr)
    assert _first_difference(one, two) is None, _first_difference(one, two)
    st = tr.guard.read()
    assert (st.applied, st.skipped, st.clipped_steps) == (1, 1, 0) and tr.global_step == 2 and math.isfinite(st.last_norm)
    assert any("moving" in k for k in two)
    tr.train_step(items[2])
    three = _snapshot(tr)
    st = tr.guard.read()
    assert (st.applied, st.skipped) == (2, 1) and all(torch.isfinite(v).all() for v in three.values())
    assert _first_difference(two, three) is not None and not torch.equal(three["ema"], three["flat_param"])
    r = tr.metrics.read()
    assert r.update_nonfinite > 0 and r.batches == 3 and math.isnan(r.mean_loss)    # what the data says; GuardStats says why
    tr._check(r, 0, 1)                                                    # one skipped step of the interval: the run goes on


def test_trainer_checkpoint_and_resume_with_guard_and_ema_are_bit_exact(dev, tmp_path):
    pool = _pool(dev)
    kw = dict(clip_norm=2.0, skip_nonfinite=True, ema_decay=0.9)
    ckpt = str(tmp_path)
    tr = _trainer(pool, dev, **kw)
    states = []
    for epoch in range(2):
        f = _items(pool, epoch)
        for item in f:
            tr.train_step(item, f)
        states.append(_snapshot(tr))
        tr.epoch = epoch
        if epoch == 0:
            tr.save(ckpt)
    words = tr.guard.words()
    tr2 = _trainer(pool, dev, **kw)
    state = tr2.load(train.latest_checkpoint(ckpt))
    assert state["optimizer"]["step"] == 3 and "ema" in state["optimizer"] and tr2.global_step == 3
    assert _first_difference(_snapshot(tr2), states[0]) is None
    tr2.fit(lambda epoch: feed.DeviceFeed(pool, BATCH, T_PTS, seed=SEED, augment=True), 2)
    assert tr2.global_step == 6
    assert _first_difference(_snapshot(tr2), states[1]) is None, _first_difference(_snapshot(tr2), states[1])
    assert np.array_equal(tr2.guard.words(), words) and tr2.guard.read().applied == 6
    # the averaged weights evaluate, and the live ones are back afterwards
    r = tr2.eval_one_epoch(feed.DeviceFeed(pool, BATCH, T_PTS, seed=SEED, augment=False))
    assert np.isfinite(r.mean_loss) and _first_difference(_snapshot(tr2), states[1]) is None
