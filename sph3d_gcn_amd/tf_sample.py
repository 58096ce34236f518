"""Point sampling — mirrors tf_ops/sampling/tf_sample.py:15-49.

``farthest_point_sample`` is the HIP kernel (custom op ``sph3d::farthest_point_sample``,
no gradient :24).  ``inverse_density_sample`` and ``random_sample`` were stock-TF one-liners in
the reference (:27-49) and are stock-torch one-liners here (RNG-dependent: parity is statistical).
``inverse_density_sample_keyed`` is inverse-density sampling as a pure function of the graph and a
(seed, step, level) key: a HIP kernel (custom op ``sph3d::inverse_density_sample``) that equals its
numpy statement (harness/idsample.py) bit for bit.
"""
import torch

from . import _lib


def _farthest_point_sample_impl(database: torch.Tensor, npoint: int) -> torch.Tensor:
    _lib.require_device(database)
    if npoint <= 0:
        raise ValueError("FarthestPointSample expects positive npoint")                     # tf_sample.cpp:35
    if database.dim() != 3 or database.shape[2] != 3:
        raise ValueError("FarthestPointSample expects (batch_size,num_points,3) inp shape")  # :40
    database = _lib.f32(database)
    b, n, _ = database.shape
    out = _lib.empty((b, npoint), torch.int32, database.device)
    l = _lib.lib()
    wsb = l.sph3d_farthest_point_sample_workspace(b, n, npoint)
    ws = _lib.scratch(wsb, database.device)
    _lib.check(l.sph3d_farthest_point_sample(b, n, npoint, _lib.ptr(database), _lib.ptr(out), _lib.ptr(ws), wsb,
                                             _lib.stream_ptr()))
    return out


_farthest_point_sample = torch.library.custom_op("sph3d::farthest_point_sample", mutates_args=())(_farthest_point_sample_impl)


@_farthest_point_sample.register_fake
def _(database, npoint):
    return database.new_empty((database.shape[0], npoint), dtype=torch.int32)


def farthest_point_sample(neursize, database):
    """Farthest-point sampling (public signature of tf_sample.py:15-23; note the argument order: count first).

    database [B, N, 3] fp32 -> [B, neursize] int32: index 0 first, then repeatedly the point farthest from the chosen set
    (ties: lower index within the reference's 1024-thread stride, then lower index).  No gradient.
    """
    return _farthest_point_sample_impl(database, int(neursize))


def inverse_density_sample(neursize, probability):
    '''Gumbel-max top-k over log(probability) (tf_sample.py:27-41): `neursize` DISTINCT points per cloud, point i drawn
    with weight probability[i] (build_graph passes the mean sqrt-distance to the neighbours, i.e. sparse regions are
    favoured).  Entries that are not positive and finite (a row whose neighbour count is 0 gives 0/0) get weight zero.'''
    probability = torch.where(torch.isfinite(probability) & (probability > 0), probability, torch.zeros_like(probability))
    logits = torch.log(probability)
    u = torch.rand_like(logits)
    z = -torch.log(-torch.log(u))
    _, neuron_index = torch.topk(logits + z, int(neursize), dim=-1)
    return neuron_index.int()


_IDS_LEVELS = 8
_U64_MASK = 0xffffffffffffffff


def _inverse_density_sample_impl(nn_dist: torch.Tensor, nn_count: torch.Tensor, nsample: int, seed: int, step: int,
                                 level: int) -> torch.Tensor:
    _lib.require_device(nn_dist, nn_count)
    if nn_dist.dim() != 3 or nn_count.dim() != 2 or tuple(nn_count.shape) != tuple(nn_dist.shape[:2]):
        raise ValueError("InverseDensitySample expects nn_dist (batch_size,num_points,nn_sample) and nn_count (batch_size,num_points)")
    nn_dist, nn_count = _lib.f32(nn_dist), _lib.i32(nn_count)
    b, n, k = nn_dist.shape
    out = _lib.empty((b, nsample), torch.int32, nn_dist.device)
    l = _lib.lib()
    wsb = l.sph3d_ids_sample_workspace(b, n)
    ws = _lib.scratch(wsb, nn_dist.device)
    _lib.check(l.sph3d_ids_sample(b, n, k, nsample, _lib.ptr(nn_dist), _lib.ptr(nn_count), seed & _U64_MASK, step & _U64_MASK, level,
                                  _lib.ptr(out), _lib.ptr(ws), wsb, _lib.stream_ptr()))
    return out


_inverse_density_sample = torch.library.custom_op("sph3d::inverse_density_sample", mutates_args=())(_inverse_density_sample_impl)


@_inverse_density_sample.register_fake
def _(nn_dist, nn_count, nsample, seed, step, level):
    return nn_dist.new_empty((nn_dist.shape[0], nsample), dtype=torch.int32)


def inverse_density_sample_keyed(neursize, nn_dist, nn_count, seed, step, level=0):
    """Inverse-density sampling as a pure function of (nn_dist, nn_count, seed, step, level) — the distribution of
    inverse_density_sample on the weights build_graph gives it (the mean distance to the neighbours), drawn from the feeds'
    counter-based numbers instead of the global generator, so that a batch's graph is a function of (seed, step).

    nn_dist [B, N, K] fp32, nn_count [B, N] int32 (an intra graph's) -> [B, neursize] int32, best first; points without a positive
    finite weight come last, by index.  level (0..7) separates the draws of a plan's levels.  On the HIP device: csrc/idsample.hip
    (custom op ``sph3d::inverse_density_sample``); on CPU tensors the numpy statement harness/idsample.ids_reference, which the
    kernel equals bit for bit.  No gradient."""
    neursize, seed, step, level = int(neursize), int(seed), int(step), int(level)
    if not 0 <= level < _IDS_LEVELS:
        raise ValueError("InverseDensitySample: level %d outside 0..%d" % (level, _IDS_LEVELS - 1))
    if neursize <= 0 or neursize > nn_dist.shape[1]:
        raise ValueError("InverseDensitySample: %d samples of %d points" % (neursize, nn_dist.shape[1]))
    if nn_dist.is_cuda:
        # (the custom op's integers are signed 64-bit words: the same 64 bits)
        wrap = lambda v: ((v & _U64_MASK) ^ (1 << 63)) - (1 << 63)
        return _inverse_density_sample_impl(nn_dist, nn_count, neursize, wrap(seed), wrap(step), level)
    from .harness import idsample
    return torch.from_numpy(idsample.ids_reference(nn_dist.detach().numpy(), nn_count.detach().numpy(), neursize, seed, step, level))


def random_sample(neursize, database):
    '''uniform sampling with replacement (tf_sample.py:44-49)'''
    batch_size, num_points = database.shape[0], database.shape[1]
    return torch.randint(0, num_points, (batch_size, int(neursize)), dtype=torch.int32, device=database.device)
