"""harness/objio.py:prepare_modelnet on the device: the ModelNet writer's farthest-point sampling, then its numpy lines."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import objio

pytestmark = pytest.mark.gpu


def test_prepare_modelnet_samples_centres_and_scales(dev):
    """a 300-row cloud to 256: the rows are xyz[idx] for the idx farthest_point_sample returned, centred on their float32 mean and
    divided by their largest norm as io/make_tfrecord_modelnet.py:93-95 states; the largest norm is 1 within one fp32 ulp"""
    import torch
    from sph3d_gcn_amd import tf_sample
    rng = np.random.RandomState(12)
    xyz = (rng.randn(300, 3) * [1.0, 0.5, 2.0] + [3.0, -1.0, 0.5]).astype(np.float32)
    normal = rng.randn(300, 3).astype(np.float32)
    got, got_normal, idx = objio.prepare_modelnet(xyz, normal, 256, device=dev)
    want_idx = tf_sample.farthest_point_sample(256, torch.from_numpy(xyz[None]).to(dev))[0].cpu().numpy()
    assert idx.dtype == np.int32 and np.array_equal(idx, want_idx) and idx[0] == 0 and np.unique(idx).shape[0] == 256
    rows = xyz[idx, :]
    rows = rows - np.mean(rows, axis=0)
    scale = np.sqrt(np.amax(np.sum(np.square(rows), axis=1)))
    rows /= scale
    assert got.dtype == np.float32 and got.shape == (256, 3) and np.array_equal(got.view(np.int32), rows.view(np.int32))
    assert np.array_equal(got_normal.view(np.int32), normal[idx].view(np.int32))
    largest = np.sqrt(np.amax(np.sum(np.square(got), axis=1)))                    # (the writer's own debug line, in float32)
    print("largest norm - 1 = %.3g (one ulp is %.3g)" % (float(largest) - 1.0, float(np.spacing(np.float32(1.0)))))
    assert abs(float(largest) - 1.0) <= float(np.spacing(np.float32(1.0)))
    # nothing to sample: the cloud is only centred and scaled; fewer points than asked for is refused, as the writer exits
    same, _n, none = objio.prepare_modelnet(xyz[:256], normal[:256], 256, device=dev)
    assert none is None and same.shape == (256, 3) and abs(float(np.sqrt(np.amax(np.sum(np.square(same), axis=1)))) - 1.0) <= float(np.spacing(np.float32(1.0)))
    with pytest.raises(ValueError):
        objio.prepare_modelnet(xyz[:100], normal[:100], 256, device=dev)
