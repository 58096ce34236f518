"""SPH3D_ruemonge2014 call pattern on s3g_util (torch restatement of models/SPH3D_ruemonge2014.py:11-123).

The facade-segmentation model is the S3DIS graph (harness/s3dis_net.py: the same encoder, decoder, fused logits tail and the same
three-stream GraphPlan) with three differences:
  1. normalize_xyz centres xy on the MEAN over the points, not on the bounding-box centre; z is kept
     (models/SPH3D_ruemonge2014.py:11-17);
  2. the input features are concat(norm_xyz, points[:, :, 3:]): nine channels — xyz, normal, rgb — into mlp1 (:40);
  3. the loss is the plain mean cross-entropy over all B * N points (:116-123).
The config is s3dis_config with num_cls = 7 (ruemonge2014_seg/ruemonge2014_config.py differs from s3dis_config.py in nothing else).
"""
import copy

import torch
import torch.nn.functional as F

from .. import sph3gcn_util as s3g_util, tf_loss
from . import s3dis_net
from .s3dis_net import GraphPlan  # noqa: F401

NUM_CLASSES = 7
INPUT_DIM = 9                           # train_ruemonge2014.py:159: xyz, normal, rgb


def ruemonge_config(num_input=8192):
    c = s3dis_net.s3dis_config(num_input)
    c.num_cls = NUM_CLASSES
    return c


def small_config(num_input=1024):
    """Reduced plan for tests (s3dis_net.small_config with the facades' seven classes)."""
    c = s3dis_net.small_config(num_input)
    c.num_cls = NUM_CLASSES
    return c


def normalize_xyz(points):
    """models/SPH3D_ruemonge2014.py:11-17"""
    center = points.mean(dim=1, keepdim=True)
    xy = points[:, :, 0:2] - center[:, :, 0:2]
    z = points[:, :, 2:]
    return torch.cat((xy, z), dim=2)


def net_input(points, config):
    """models/SPH3D_ruemonge2014.py:35-40: [B, N, 9] -> centred coordinates + normal + colour"""
    xyz = points[:, :, 0:3]
    norm_xyz = normalize_xyz(xyz) if config.normalize else xyz
    return torch.cat((norm_xyz, points[:, :, 3:]), dim=2)


def get_model(points, is_training, config=None, graphs=None, points_ready=None, sample_key=(0, 0)):
    """models/SPH3D_ruemonge2014.py:33-113: s3dis_net.get_model on the nine-channel input.  A plan handed in as `graphs` is
    GraphPlan(points, config, net_input=ruemonge_net.net_input)."""
    return s3dis_net.get_model(points, is_training, config, graphs=graphs, points_ready=points_ready, net_input=net_input,
                               sample_key=sample_key)


def get_loss(pred, label, end_points=None):
    """models/SPH3D_ruemonge2014.py:116-123: the mean cross-entropy over all B * N points.  On the device it is
    sph3d_masked_softmax_xent with an all-ones mask — the sum over the clouds of each cloud's mean — divided by B: every cloud has
    N points, so that is the global mean."""
    B, N, C = pred.shape
    if pred.is_cuda:
        ones = torch.ones((B, N), dtype=torch.float32, device=pred.device)
        return tf_loss.masked_softmax_xent(pred, label, ones).sum() / B
    return F.cross_entropy(pred.reshape(-1, C), label.long().reshape(-1))


class SPH3DRueMonge(torch.nn.Module):
    """Holds the VariableStore so parameters register with the optimiser; forward = get_model."""

    def __init__(self, config=None, device=None, seed=7):
        super().__init__()
        self.config = copy.deepcopy(config) if config is not None else ruemonge_config()
        self.store = s3g_util.VariableStore(device=device, seed=seed)

    def forward(self, points, is_training=True, graphs=None, points_ready=None, sample_key=(0, 0)):
        with s3g_util.variable_store(self.store):
            return get_model(points, is_training, self.config, graphs=graphs, points_ready=points_ready, sample_key=sample_key)

    def loss(self, pred, label):
        return get_loss(pred, label)
