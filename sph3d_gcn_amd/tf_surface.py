"""Surface normals on the device (csrc/normals.hip; include/sph3d.h states them, harness/normals.py is the numpy statement):
the eigenvector of the smallest eigenvalue of a neighbourhood's covariance, formed in float64 from order-free integer moments.

Registered as PyTorch custom ops ``sph3d::graph_normals`` / ``sph3d::ball_normals`` (no gradient), built the way tf_nnquery's
are.  Not in the reference: its facade line reads normals from the dataset's files.
"""
from typing import Optional, Tuple

import torch

from . import _lib

MAX_BALL_ROWS = 1 << 26


def _check(radius, min_count):
    if not (radius > 0 and radius < float("inf")):
        raise ValueError("normals: finite radius>0 required, got %r" % (radius,))
    if min_count < 3:
        raise ValueError("normals: min_count>=3 required, got %r" % (min_count,))


def _graph_normals_impl(database: torch.Tensor, query: torch.Tensor, nn_index: torch.Tensor, nn_count: torch.Tensor,
                        radius: float, toward: Optional[torch.Tensor], min_count: int,
                        want_moments: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    _lib.require_device(database, query, nn_index, nn_count)
    if database.dim() != 3 or database.shape[2] != 3:
        raise ValueError("Shape of database points requires to be (batch, npoint, 3)")
    if query.dim() != 3 or query.shape[2] != 3 or query.shape[0] != database.shape[0]:
        raise ValueError("Shape of query points requires to be (batch, mpoint, 3)")
    B, N, _ = database.shape
    M = query.shape[1]
    if nn_index.dim() != 3 or tuple(nn_index.shape[0:2]) != (B, M) or nn_index.shape[2] == 0 or tuple(nn_count.shape) != (B, M):
        raise ValueError("Shape of nn_index requires to be (batch, mpoint, nnsample>0), of nn_count (batch, mpoint)")
    _check(radius, min_count)
    K = nn_index.shape[2]
    database, query, nn_index, nn_count = _lib.f32(database), _lib.f32(query), _lib.i32(nn_index), _lib.i32(nn_count)
    dev = query.device
    if toward is not None:
        _lib.require_device(toward)
        if tuple(toward.shape) != (B, 3):
            raise ValueError("Shape of toward requires to be (batch, 3)")
        toward = _lib.f32(toward)
    normals = torch.empty((B, M, 3), dtype=torch.float32, device=dev)
    variation = torch.empty((B, M), dtype=torch.float32, device=dev)
    count = torch.empty((B, M), dtype=torch.int32, device=dev)
    moments = torch.empty((B, M, 10) if want_moments else (0,), dtype=torch.int64, device=dev)
    skipped = torch.zeros((1 if want_moments else 0,), dtype=torch.int64, device=dev)
    if B * M > 0:
        _lib.check(_lib.lib().sph3d_graph_normals(
            B, N, M, K, radius, min_count, _lib.ptr(database), _lib.ptr(query), _lib.ptr(nn_index), _lib.ptr(nn_count),
            _lib.ptr(toward), _lib.ptr(normals), _lib.ptr(variation), _lib.ptr(count),
            _lib.ptr(moments if want_moments else None), _lib.ptr(skipped if want_moments else None), _lib.stream_ptr()))
    return normals, variation, count, moments, skipped


_graph_normals = torch.library.custom_op("sph3d::graph_normals", mutates_args=())(_graph_normals_impl)


@_graph_normals.register_fake
def _(database, query, nn_index, nn_count, radius, toward, min_count, want_moments):
    B, M = query.shape[0], query.shape[1]
    return (query.new_empty((B, M, 3), dtype=torch.float32), query.new_empty((B, M), dtype=torch.float32),
            query.new_empty((B, M), dtype=torch.int32),
            query.new_empty((B, M, 10) if want_moments else (0,), dtype=torch.int64),
            query.new_empty((1 if want_moments else 0,), dtype=torch.int64))


def _ball_normals_impl(xyz: torch.Tensor, radius: float, toward: Optional[torch.Tensor], min_count: int,
                       want_moments: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    _lib.require_device(xyz)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("Shape of xyz requires to be (npoint, 3)")
    V = xyz.shape[0]
    if V > MAX_BALL_ROWS:
        raise ValueError("ball_normals: at most 2^26 rows, got %d" % V)
    _check(radius, min_count)
    xyz = _lib.f32(xyz)
    dev = xyz.device
    if toward is not None:
        _lib.require_device(toward)
        if tuple(toward.shape) != (3,):
            raise ValueError("Shape of toward requires to be (3,)")
        toward = _lib.f32(toward)
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    variation = torch.empty((V,), dtype=torch.float32, device=dev)
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    moments = torch.empty((V, 10) if want_moments else (0,), dtype=torch.int64, device=dev)
    if V > 0:
        l = _lib.lib()
        nbytes = l.sph3d_ball_normals_workspace(V)
        ws = _lib.scratch(nbytes, dev)
        _lib.check(l.sph3d_ball_normals(V, radius, min_count, _lib.ptr(xyz), _lib.ptr(toward), _lib.ptr(normals),
                                        _lib.ptr(variation), _lib.ptr(count), _lib.ptr(moments if want_moments else None),
                                        _lib.ptr(ws), nbytes, _lib.stream_ptr()))
    return normals, variation, count, moments


_ball_normals = torch.library.custom_op("sph3d::ball_normals", mutates_args=())(_ball_normals_impl)


@_ball_normals.register_fake
def _(xyz, radius, toward, min_count, want_moments):
    V = xyz.shape[0]
    return (xyz.new_empty((V, 3), dtype=torch.float32), xyz.new_empty((V,), dtype=torch.float32),
            xyz.new_empty((V,), dtype=torch.int32), xyz.new_empty((V, 10) if want_moments else (0,), dtype=torch.int64))


def graph_normals(database, query, nn_index, nn_count, radius, toward=None, min_count=3, want_moments=False):
    """Normals of the query points from the neighbours a graph lists (the first min(nn_count, K) entries of a row, as
    tf_nnquery's searches leave them in either radius mode).

    database  [B, N, >=3] fp32      query  [B, M, >=3] fp32      nn_index [B, M, K] int32      nn_count [B, M] int32
    radius    the scale of the quantisation (the search's radius); toward: None or [B, 3], the point a cloud's normals face
    returns   normals [B, M, 3] fp32 (zero for a row with fewer than min_count valid neighbours or a zero covariance trace),
              variation [B, M] fp32 = l0 / (l0 + l1 + l2), count [B, M] int32 = the valid neighbours;
              with want_moments also moments [B, M, 10] int64 and skipped [1] int64 (neighbours that were not valid).
    No gradient."""
    out = _graph_normals_impl(database[:, :, 0:3], query[:, :, 0:3], nn_index, nn_count, float(radius), toward, int(min_count),
                              bool(want_moments))
    return out if want_moments else out[0:3]


def ball_normals(xyz, radius, toward=None, min_count=3, want_moments=False):
    """Normals of a flat cloud from ALL points inside the ball of `radius` around each point (the point included), found
    through a cell grid on the device.

    xyz       [V, >=3] fp32, V <= 2^26          toward: None or [3]
    returns   normals [V, 3] fp32, variation [V] fp32, count [V] int32; with want_moments also moments [V, 10] int64.
    No gradient."""
    out = _ball_normals_impl(xyz[:, 0:3], float(radius), toward, int(min_count), bool(want_moments))
    return out if want_moments else out[0:3]
