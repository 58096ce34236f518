"""Deterministic mode on the ModelNet plan: the twin of section 7 of tests/test_gpu_determinism.py for the
classifier — odd channel counts (35, 67, 131: raw xyz concatenated at every level), a global convolution, and two dropout layers,
whose masks are keyed by (seed, step) when the Trainer runs in the mode.  Two fresh runs from one seed and a run resumed from a
checkpoint end with the same bits after every step.  Every comparison is of bit patterns; the switch is off afterwards."""
import numpy as np
import pytest
import torch

import sph3d_gcn_amd as pkg
from sph3d_gcn_amd import _lib, _tgraph
from sph3d_gcn_amd.harness import modelnet_net, objfeed, optim, synth, train

pytestmark = pytest.mark.gpu
T_PTS, BATCH, SEED, SHAPES = 1024, 3, 21, 9


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    pkg.set_deterministic(False)
    _tgraph.clear()
    yield
    pkg.set_deterministic(False)
    _tgraph.clear()
    assert _lib.lib().sph3d_get_deterministic() == 0


def _pool(dev):
    """nine synthetic shapes of 1024 to 2000 points, classes spread over the 40"""
    sizes = (1500, 1024, 1100, 2000, 1300, 1024, 1700, 1200, 1900)
    classes = [(7 * k) % 40 for k in range(SHAPES)]
    return objfeed.ShapePool.from_arrays([synth.modelnet_cloud(40 + k, n) for k, n in enumerate(sizes)], classes, classes, device=dev)


def _feed(pool):
    return objfeed.ObjectFeed(pool, BATCH, T_PTS, seed=SEED, dataset="modelnet")


def _trainer(pool, dev, deterministic=True, **kw):
    model = modelnet_net.SPH3DModelNet(modelnet_net.small_config(T_PTS), device=dev, seed=3)
    ids = torch.from_numpy(np.asarray([0, 1, 2], np.int32)).to(dev)
    points, label = objfeed.assemble(pool.rows, pool.offsets, ids, T_PTS, SEED, 0, 0)
    prime = (points, label, pool.category_dev[:3])
    # (modelnet_net.get_loss, not model.loss: the Trainer adds the 'losses' collection and the regularisers itself)
    return train.Trainer(model, modelnet_net.get_loss, lambda p: optim.FlatTFAdam(p, lr=1e-3, eps=1e-8),
                         train.Schedule(1e-3, BATCH, decay_step=9, decay_rate=0.7), 40, line=train.modelnet_line, prime=prime, seed=SEED,
                         log=lambda s: None, log_every=3, deterministic=deterministic, **kw)


def _snapshot(tr):
    torch.cuda.synchronize()
    s = {"flat_param": tr.flat.flat_param.detach().clone(), "opt.m": tr.opt.m.clone(), "opt.v": tr.opt.v.clone()}
    for k, v in tr.model.state_dict().items():
        if "moving" in k:
            s[k] = v.detach().clone()
    return s


def _first_difference(a, b):
    assert set(a) == set(b)
    for k in a:
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            return k
    return None


def _run(pool, dev, ckpt=None):
    """two epochs of three batches -> the state after every step (six snapshots); ckpt: a checkpoint is written after epoch 0"""
    tr = _trainer(pool, dev)
    assert tr.keyed_dropout, "in the mode the Trainer keys the model's dropout"
    states = []
    for epoch in range(2):
        f = _feed(pool)
        f.epoch = epoch
        for item in f:
            tr.train_step(item, f)
            states.append(_snapshot(tr))
        tr.epoch = epoch
        if ckpt is not None and epoch == 0:
            tr.save(ckpt)
    assert tr.global_step == 6 and not pkg.is_deterministic()
    return states


def test_modelnet_trainer_runs_from_one_seed_end_with_the_same_bits(dev, tmp_path):
    pool = _pool(dev)
    ckpt = str(tmp_path)
    a = _run(pool, dev, ckpt)
    b = _run(pool, dev)
    assert any("moving_mean" in k for k in a[-1]) and any("moving_variance" in k for k in a[-1])
    assert not torch.equal(a[0]["flat_param"], a[-1]["flat_param"]) and torch.isfinite(a[-1]["flat_param"]).all()
    for step, (sa, sb) in enumerate(zip(a, b)):
        assert _first_difference(sa, sb) is None, "two fresh runs differ after step %d in %s" % (step, _first_difference(sa, sb))
    # the resumed run: the checkpoint written after three steps, then fit() to the end of epoch 1
    tr = _trainer(pool, dev)
    tr.load(train.latest_checkpoint(ckpt))
    assert tr.global_step == 3 and _first_difference(_snapshot(tr), a[2]) is None
    tr.fit(lambda epoch: _feed(pool), 2)
    assert tr.global_step == 6 and not pkg.is_deterministic()
    assert _first_difference(_snapshot(tr), a[-1]) is None, "the resumed run differs in %s" % _first_difference(_snapshot(tr), a[-1])


def test_the_trainer_keys_dropout_where_asked(dev):
    pool = _pool(dev)
    assert not _trainer(pool, dev, keyed_dropout=False).keyed_dropout
    assert _trainer(pool, dev, keyed_dropout=None).keyed_dropout          # None follows `deterministic`
    # outside the mode, on request: a step runs and the parameters stay finite
    tr = _trainer(pool, dev, deterministic=False, keyed_dropout=True)
    assert tr.keyed_dropout and not tr.deterministic
    f = _feed(pool)
    tr.train_step(next(iter(f)), f)
    torch.cuda.synchronize()
    assert tr.global_step == 1 and torch.isfinite(tr.flat.flat_param).all() and not pkg.is_deterministic()
