"""Keyed dropout on the device (csrc/dropout.hip through tf_dropout.dropout_keyed) against its numpy statement
(harness/dropout.py), bit for bit, forward and backward; and through the ModelNet model, whose two dropout layers take the key."""
import numpy as np
import pytest
import torch

from sph3d_gcn_amd import tf_dropout
from sph3d_gcn_amd.harness import dropout as D
from sph3d_gcn_amd.harness import modelnet_net, synth

pytestmark = pytest.mark.gpu
KEY = (21, 5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _both(dev, x, rate, key, layer, row0=0, go=None):
    """-> (y, grad of x for grad_output go) from the device"""
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    y = tf_dropout.dropout_keyed(xt, rate, key, layer, row0)
    go = np.random.RandomState(7).randn(*x.shape).astype(np.float32) if go is None else go
    y.backward(torch.from_numpy(go).to(dev))
    torch.cuda.synchronize()
    return y.detach().cpu().numpy(), xt.grad.cpu().numpy(), go


@pytest.mark.parametrize("rate", [0.5, 0.3])
@pytest.mark.parametrize("shape", [(3, 512), (1, 1), (2, 7, 5), (3, 1027)], ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_equal_the_statement(dev, shape, rate):
    x = np.random.RandomState(sum(shape)).randn(*shape).astype(np.float32)
    for layer, row0 in ((0, 0), (1, 0), (0, 2), (15, 7)):
        y, gx, go = _both(dev, x, rate, KEY, layer, row0)
        np.testing.assert_array_equal(_bits(y), _bits(D.dropout_reference(x, rate, KEY, layer, row0)), err_msg="forward, layer %d row0 %d" % (layer, row0))
        np.testing.assert_array_equal(_bits(gx), _bits(D.dropout_reference(go, rate, KEY, layer, row0)), err_msg="backward, layer %d row0 %d" % (layer, row0))
    keep = D.keep_reference(shape, rate, KEY, 0)
    assert shape == (1, 1) or (keep.any() and not keep.all())


def test_row0_shifts_the_rows_on_the_device(dev):
    x = np.random.RandomState(3).randn(5, 1027).astype(np.float32)
    whole, _, _ = _both(dev, x, 0.5, KEY, 1)
    # rows 2..4 as a call of their own: a view at an address that is not 16-byte aligned (2 x 1027 floats in), so the scalar path
    xt = torch.from_numpy(x).to(dev)
    part = tf_dropout.dropout_keyed(xt[2:], 0.5, KEY, 1, row0=2)
    assert xt[2:].data_ptr() % 16 != 0
    np.testing.assert_array_equal(_bits(part.cpu().numpy()), _bits(whole[2:]))
    np.testing.assert_array_equal(_bits(whole), _bits(D.dropout_reference(x, 0.5, KEY, 1)))


def test_dropped_slots_are_plus_zero_whatever_x_holds(dev):
    x = np.random.RandomState(5).randn(3, 512).astype(np.float32)
    keep = D.keep_reference(x.shape, 0.5, KEY, 0)
    dropped = np.argwhere(~keep)
    for (b, i), v in zip(dropped[:6], (np.inf, -np.inf, np.nan, -0.0, -np.inf, np.nan)):
        x[b, i] = v
    kept = np.argwhere(keep)
    for (b, i), v in zip(kept[:3], (np.inf, np.nan, -0.0)):
        x[b, i] = v
    y, gx, go = _both(dev, x, 0.5, KEY, 0, go=x.copy())
    assert (_bits(y)[~keep] == 0).all() and (_bits(gx)[~keep] == 0).all(), "a dropped slot is +0.0, not 0 * x"
    np.testing.assert_array_equal(_bits(y), _bits(D.dropout_reference(x, 0.5, KEY, 0)))
    assert np.isinf(y[tuple(kept[0])]) and np.isnan(y[tuple(kept[1])]) and _bits(y)[tuple(kept[2])] == np.int32(-2 ** 31)


def test_rates_zero_and_one_and_bad_arguments(dev):
    xt = torch.randn(3, 8, device=dev)
    assert tf_dropout.dropout_keyed(xt, 0.0, KEY, 0) is xt
    assert (tf_dropout.dropout_keyed(xt, 1.0, KEY, 0).view(torch.int32) == 0).all()
    for bad in (dict(layer=16), dict(layer=-1), dict(rate=1.5), dict(rate=-0.1)):
        with pytest.raises(ValueError):
            tf_dropout.dropout_keyed(xt, bad.get("rate", 0.5), KEY, bad.get("layer", 0))
    with pytest.raises(ValueError):
        tf_dropout.dropout_keyed(xt.double(), 0.5, KEY, 0)
    with pytest.raises(ValueError):
        tf_dropout.dropout_keyed(xt, 0.5, KEY, 0, row0=2 ** 32)            # the entry's own check (SPH3D_EINVAL)


def test_the_modelnet_model_takes_the_key(dev):
    model = modelnet_net.SPH3DModelNet(modelnet_net.small_config(1024), device=dev, seed=3)
    pts = torch.from_numpy(synth.modelnet_batch(11, 2, 1024)[:, :, :3].copy()).to(dev)

    def logits(**kw):
        with torch.no_grad():
            out, _ = model(pts, **kw)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    a = logits(is_training=True, dropout_key=(21, 0))
    b = logits(is_training=True, dropout_key=(21, 0))
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="one key: the same logits")
    assert a.shape == (2, 40) and np.isfinite(a).all()
    c = logits(is_training=True, dropout_key=(21, 1))
    assert (_bits(a) != _bits(c)).any(), "another step: another mask"
    d = logits(is_training=True, dropout_key=(21, 0), dropout_row0=2)
    assert (_bits(a) != _bits(d)).any(), "other rows of the global batch: another mask"
    plain = logits(is_training=False)
    np.testing.assert_array_equal(_bits(logits(is_training=False, dropout_key=(21, 0))), _bits(plain), err_msg="inference ignores the key")
    with pytest.raises(ValueError, match="dropout_key"):
        model(pts, is_training=True, dropout_key=(21, 0), dropout_generator=torch.Generator().manual_seed(1))
