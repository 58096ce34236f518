"""k-NN un-pooling graphs through the model plans: small_config() with unpool_k = 3 and unpool_method = 'idw' on 2 x 1024 points.
Every decoder level's inter graph of the GraphPlan equals harness/knn.py's statement on the plan's own point sets, forward, loss
and backward run to finite values, and a config without the keyword (or with unpool_k = None) launches what it always did: the
same logits bit for bit from two plans built one after the other."""
import numpy as np
import pytest
import torch

from sph3d_gcn_amd.harness import knn, s3dis_net, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch(dev):
    xyz, label, inner = synth.s3dis_batch(0, 2, 1024, extent=(1.0, 1.0, 1.5))
    return torch.from_numpy(xyz).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(inner).to(dev)


def test_plan_with_unpool_k_builds_the_statements_graphs_and_trains(dev, batch):
    pts, label, inner = batch
    cfg = s3dis_net.small_config(1024)
    cfg.unpool_k, cfg.unpool_method = 3, 'idw'
    model = s3dis_net.SPH3DS3DIS(cfg, device=dev)
    plan = s3dis_net.build_graphs(pts, model.config)
    torch.cuda.synchronize()
    L = len(cfg.radius)
    sizes = [int(t.shape[1]) for t in plan.xyz_layers]
    assert sizes == [1024] + cfg.num_sample
    for l in range(L):
        g = plan.dec(l)
        coarse, fine = plan.xyz_layers[L - l].cpu().numpy(), plan.xyz_layers[L - 1 - l].cpu().numpy()
        want = knn.knn_reference(coarse, fine, 3, dist="squared")
        got = (g["inter_idx"].cpu().numpy(), g["inter_cnt"].cpu().numpy(), g["inter_dst"].cpu().numpy())
        assert got[0].shape == (2, fine.shape[1], 3) and (got[1] == 3).all()
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
        assert (got[2].view(np.uint32) == want[2].view(np.uint32)).all()
        # the coarse points are samples of the fine ones: each is its own nearest neighbour at d2 = 0
        assert (want[2][:, :, 0] == 0).sum() >= 2 * coarse.shape[1]
    pred, _ = model(pts, is_training=True, graphs=plan)
    loss = model.loss(pred, label, inner)
    loss.backward()
    torch.cuda.synchronize()
    assert pred.shape == (2, 1024, 13) and torch.isfinite(pred).all() and torch.isfinite(loss)
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)


def test_default_path_is_untouched_by_the_keyword(dev, batch):
    pts, _, _ = batch
    logits = []
    for unset in ("absent", "none"):
        cfg = s3dis_net.small_config(1024)
        assert not hasattr(cfg, "unpool_k")
        if unset == "none":
            cfg.unpool_k = None
        model = s3dis_net.SPH3DS3DIS(cfg, device=dev, seed=7)
        plan = s3dis_net.build_graphs(pts, model.config)
        for l in range(len(cfg.radius)):
            g = plan.dec(l)
            assert g["inter_idx"].shape[2] == cfg.nn_uplimit[len(cfg.radius) - 1 - l]          # the sphere search's rows
        with torch.no_grad():
            pred, _ = model(pts, is_training=False, graphs=plan)
        torch.cuda.synchronize()
        logits.append(pred.cpu().numpy())
    assert np.isfinite(logits[0]).all() and (logits[0].view(np.uint32) == logits[1].view(np.uint32)).all()
