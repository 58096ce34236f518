"""Keyed inverse-density sampling on the host: the -log of include/sph3d_log32.h over all of its arguments, the numpy statement
(harness/idsample.py) on its edge cases and its distribution, a CPU GraphPlan with config.sample == 'IDS' through the oracle ops,
and the C entry's validation, which answers before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _ids_cases
from oracle import torch_ops
from sph3d_gcn_amd import sph3gcn_util as s3g_util
from sph3d_gcn_amd import tf_sample
from sph3d_gcn_amd.harness import feed, idsample, s3dis_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_neglog32_over_all_arguments():
    """all u = k 2^-24, k = 1 .. 2^24: finite, sign bit clear, E(1) = +0, non-increasing in u, and within 2^-20 (relative) of the
    float64 -log(u) for k < 2^24.  The bound is derived: an error eps in E moves inclusion probabilities by a relative eps, and
    2^-20 is four orders below the 1 / sqrt(2 10^4) the distribution test below resolves.  Measured: 3.49 * 2^-24."""
    k = np.arange(1, 2 ** 24 + 1, dtype=np.int64)
    u = (k.astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    E = idsample.neglog32(u)
    assert E.dtype == np.float32
    bits = E.view(np.uint32)
    assert np.isfinite(E).all()
    assert not (bits >> np.uint32(31)).any()
    assert bits[-1] == 0
    assert (np.diff(E) <= 0).all()
    exact = -np.log(u[:-1].astype(np.float64))
    rel = np.abs(E[:-1].astype(np.float64) - exact) / exact
    print("neglog32: max relative error %.3f * 2^-24" % (rel.max() * 2.0 ** 24))
    assert rel.max() <= 2.0 ** -20


def test_coefficients_come_from_the_header():
    text = open(os.path.join(ROOT, "include", "sph3d_log32.h")).read()
    degree = int(re.search(r"#define\s+SPH3D_LOG32_DEGREE\s+(\d+)", text).group(1))
    c = idsample.neglog32_coefficients()
    assert c.dtype == np.float32 and len(c) == degree + 1
    assert np.array_equal(c, (2.0 / (2.0 * np.arange(degree + 1) + 1.0)).astype(np.float32))
    # the list is written once: the header's function body holds no other literal of them
    assert text.count("6.666666865e-01f") == 1


def _keys_of(d, c, out, seed, step, level):
    keys = idsample.ids_keys(d, c, seed, step, level)
    return np.take_along_axis(keys, out.astype(np.int64), axis=1)


@pytest.mark.parametrize("B,N,K,S", [(3, 200, 5, 200), (2, 777, 16, 100), (2, 64, 1, 7)])
def test_ids_reference_order_and_invalid_points(B, N, K, S):
    d, c = _ids_cases.graph_inputs(B, N, K, seed=N, nan_tail=False)
    out = idsample.ids_reference(d, c, S, 3, 9, 2)
    assert out.shape == (B, S) and out.dtype == np.int32
    w, valid = idsample.ids_weight(d, c)
    assert (~valid).mean() >= 0.1 and not valid[B - 1].any()
    assert (~valid[0] & (c[0] > 0)).any()                      # all-zero distances with a positive count
    assert np.isinf(w).any()                                   # a row with an inf distance
    for b in range(B):
        assert len(set(out[b].tolist())) == S and out[b].min() >= 0 and out[b].max() < N
    ks = _keys_of(d, c, out, 3, 9, 2)
    assert (ks[:, 1:] > ks[:, :-1]).all()                      # keys ascending (and distinct)
    for b in range(B):
        v = valid[b][out[b]]
        nv = int(min(S, valid[b].sum()))
        assert v[:nv].all() and not v[nv:].any()               # every invalid point after every valid one ..
        tail = out[b][nv:]
        assert np.array_equal(tail, np.flatnonzero(~valid[b])[:len(tail)])     # .. and in index order
    assert np.array_equal(out[B - 1], np.arange(S))            # the cloud with all counts 0
    # NaN in the slots >= count changes nothing
    d_nan = np.where(np.arange(K)[None, None, :] < c[:, :, None], d, np.float32(np.nan)).astype(np.float32)
    assert np.array_equal(idsample.ids_reference(d_nan, c, S, 3, 9, 2), out)
    # a pure function of its key: another seed, step or level is another sample
    full = idsample.ids_reference(d, c, S, 3, 9, 2)
    assert np.array_equal(full, out)
    if S < N:
        for other in ((4, 9, 2), (3, 10, 2), (3, 9, 1)):
            assert not np.array_equal(idsample.ids_reference(d, c, S, *other), out)


def test_ids_reference_rejects_bad_requests():
    d, c = _ids_cases.graph_inputs(1, 8, 2, seed=1, nan_tail=False)
    with pytest.raises(ValueError):
        idsample.ids_reference(d, c, 9, 0, 0, 0)
    with pytest.raises(ValueError):
        idsample.ids_reference(d, c, 4, 0, 0, 8)
    with pytest.raises(ValueError):
        tf_sample.inverse_density_sample_keyed(9, torch.from_numpy(d), torch.from_numpy(c), 0, 0)
    with pytest.raises(ValueError):
        tf_sample.inverse_density_sample_keyed(4, torch.from_numpy(d), torch.from_numpy(c), 0, 0, level=-1)
    assert feed.IDS == 8 and idsample.IDS == 8


def _chi2(counts, p):
    n = counts.sum()
    return float(((counts - n * p) ** 2 / (n * p)).sum())


def test_distribution_of_the_first_and_second_pick():
    """8 points with weights 1..8 (K = 1, count 1), B = 16 identical clouds, seed 11, steps 0..1249: 20 000 draws.  chi^2 of the
    first pick (S = 3, level 0) against p_i = i / 36 and of the second pick (S = 2, level 1) against
    sum_{i != j} p_i p_j / (1 - p_i), both below 24.32, the 0.999 quantile of chi^2 with 7 degrees of freedom."""
    B, N = 16, 8
    d = np.tile(np.arange(1, N + 1, dtype=np.float32).reshape(1, N, 1), (B, 1, 1))
    c = np.ones((B, N), dtype=np.int32)
    p = np.arange(1, N + 1, dtype=np.float64) / 36.0
    first = np.zeros(N)
    second = np.zeros(N)
    for step in range(1250):
        first += np.bincount(idsample.ids_reference(d, c, 3, 11, step, 0)[:, 0], minlength=N)
        second += np.bincount(idsample.ids_reference(d, c, 2, 11, step, 1)[:, 1], minlength=N)
    assert first.sum() == second.sum() == 20000
    p2 = np.array([sum(p[i] * p[j] / (1.0 - p[i]) for i in range(N) if i != j) for j in range(N)])
    assert abs(p2.sum() - 1.0) < 1e-12
    x1, x2 = _chi2(first, p), _chi2(second, p2)
    print("chi2 first pick %.2f, second pick %.2f" % (x1, x2))
    assert x1 < 24.32 and x2 < 24.32


def test_cpu_graph_plan_with_inverse_density_sampling():
    cfg = _ids_cases.ids_config()
    key = (5, 3)
    plan = _ids_cases.cpu_plan(key)
    L = len(cfg.radius)
    assert len(plan.indices) == L and len(plan.xyz_layers) == L + 1
    for l in range(L):
        g = plan.enc(l)
        want = idsample.ids_reference(g["intra_dst"].numpy(), g["intra_cnt"].numpy(), cfg.num_sample[l], key[0], key[1], l)
        assert np.array_equal(plan.indices[l][:, :, 1].numpy(), want)
        assert np.array_equal(plan.indices[l][:, :, 0].numpy(), np.repeat(np.arange(2)[:, None], cfg.num_sample[l], axis=1))
        src = plan.xyz_layers[l].numpy()
        assert np.array_equal(plan.xyz_layers[l + 1].numpy(), np.stack([src[b][want[b]] for b in range(2)]))
        assert np.array_equal(plan.pool(l)["inter_idx"].numpy(), np.stack([g["intra_idx"].numpy()[b][want[b]] for b in range(2)]))
    pts = torch.from_numpy(_ids_cases.plan_batch()[0])
    with torch_ops.patched_util():
        again = s3dis_net.GraphPlan(pts, cfg, sample_key=key)
        other = s3dis_net.GraphPlan(pts, cfg, sample_key=(5, 4))
        # build_graph with a key: the same sample as the plan's level 0
        _, _, _, ind = s3g_util.build_graph(pts[:, :, 0:3], cfg.radius[0], cfg.nn_uplimit[0], cfg.num_sample[0], sample_method='IDS',
                                            sample_key=key, level=0)
    for l in range(L):
        assert torch.equal(again.indices[l], plan.indices[l]) and torch.equal(again.xyz_layers[l + 1], plan.xyz_layers[l + 1])
        assert not torch.equal(other.indices[l], plan.indices[l])
    assert torch.equal(ind, plan.indices[0])


def test_host_validation_of_the_c_entry():
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    C = l.sph3d_ids_sample_chunk()
    assert C >= 1024 and C & (C - 1) == 0
    assert l.sph3d_ids_sample_workspace(4, C) == 0 and l.sph3d_ids_sample_workspace(4, C + 1) == 4 * 2 * C * 8
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args, word in (((1, 4, 2, 5, p, p, 0, 0, 0, p, None, 0, None), b"samples"),        # S > N
                       ((1, 4, 2, 2, p, p, 0, 0, 8, p, None, 0, None), b"level"),
                       ((1, 4, 0, 2, p, p, 0, 0, 0, p, None, 0, None), b"positive"),       # K = 0
                       ((1, 4, 2, 2, None, p, 0, 0, 0, p, None, 0, None), b"null")):
        rc = l.sph3d_ids_sample(*args)
        assert rc == -1 and word in l.sph3d_last_error(), (args, l.sph3d_last_error())
    rc = l.sph3d_ids_sample(1, C + 1, 2, 2, p, p, 0, 0, 0, p, None, 0, None)
    assert rc == -2 and b"workspace" in l.sph3d_last_error()                                # SPH3D_EWORKSPACE
    rc = l.sph3d_ids_sample(1, (1 << 20) + 1, 2, 2, p, p, 0, 0, 0, p, None, 0, None)
    assert rc == -4                                                                         # SPH3D_EUNSUPPORTED


def test_model_modules_pass_the_key_through():
    """config.sample == 'IDS' in the classification net (build_graph with a key on CPU tensors), both ShapeNet models and the
    facade model: one key gives one result, another key another"""
    import copy
    from sph3d_gcn_amd.harness import modelnet_net, ruemonge_net, shapenet_net, synth
    cpu = torch.device("cpu")

    def ids(cfg):
        cfg = copy.deepcopy(cfg)
        cfg.sample = 'IDS'
        return cfg

    xyz512 = torch.from_numpy(synth.modelnet_batch(20, 2, 512))
    nine = torch.from_numpy(np.concatenate([_ids_cases.plan_batch()[0], np.zeros((2, 1024, 3), np.float32)], axis=2)[:, :512].copy())
    cat = torch.tensor([1, 4])
    with torch_ops.patched_util():
        runs = [
            (modelnet_net.SPH3DModelNet(ids(modelnet_net.small_config(512)), device=cpu), (xyz512,), dict(is_training=False)),
            (shapenet_net.SPH3DShapeNet(3, ids(shapenet_net.small_config(512)), device=cpu), (xyz512,), dict(is_training=True)),
            (shapenet_net.SPH3DShapeNetOneHot(5, 16, ids(shapenet_net.small_config(512)), device=cpu), (xyz512, cat),
             dict(is_training=True)),
            (ruemonge_net.SPH3DRueMonge(ids(ruemonge_net.small_config(512)), device=cpu), (nine,), dict(is_training=True)),
        ]
        for model, args, kw in runs:
            # (gradients enabled, like the plumbing tests: the stand-ins have no one-kernel inference layer)
            a = model(*args, sample_key=(2, 7), **kw)[0].detach()
            b = model(*args, sample_key=(2, 7), **kw)[0].detach()
            c = model(*args, sample_key=(2, 8), **kw)[0].detach()
            assert torch.isfinite(a).all(), type(model).__name__
            assert torch.equal(a, b), type(model).__name__
            assert not torch.equal(a, c), type(model).__name__
