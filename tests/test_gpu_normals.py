"""Surface normals on the device (csrc/normals.hip through tf_surface) against the numpy statement (harness/normals.py): moments,
counts and the skipped total for equality, normals and variation within the derived bounds of tests/_normal_ref.py, on the
graphs the device searches return and on flat clouds; the estimated facade pool and one training step over it."""
import numpy as np
import pytest
import torch

import _normal_ref as nr
from sph3d_gcn_amd import _lib, tf_nnquery, tf_surface
from sph3d_gcn_amd.harness import facadefeed, normals as nrm, ruemonge_net, synth

pytestmark = pytest.mark.gpu

# (B, N, M, K), the family of the clouds and the search radius: the statement alone (CPU, on the search oracle's graphs in both
# radius modes) leaves no row of these out by the gap condition and none by the sign condition
GRAPH_CASES = [((2, 257, 257, 16), "sphere", 0.35), ((1, 1024, 300, 64), "box", 0.25), ((3, 64, 64, 3), "volume", 0.5),
               ((1, 300, 300, 200), "sphere", 0.6), ((2, 128, 128, 1), "volume", 0.3)]


def _clouds(shape, fam):
    B, N, M, _K = shape
    db = np.stack([nr.family(fam, N, 10 + b) for b in range(B)])
    return db, db[:, :M].copy()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_graph(dev, db, q, idx, cnt, radius, toward, what):
    """device graph_normals over (idx, cnt) against the statement, with and without the optional outputs -> stats"""
    ref = nrm.graph_normals_reference(db, q, idx, cnt, radius, toward, 3)
    tw = None if toward is None else _t(toward, dev)
    args = (_t(db, dev), _t(q, dev), _t(idx, dev), _t(cnt, dev), radius, tw, 3)
    normals, variation, count, moments, skipped = tf_surface.graph_normals(*args, want_moments=True)
    plain = tf_surface.graph_normals(*args)
    torch.cuda.synchronize()
    assert np.array_equal(moments.cpu().numpy(), ref.moments), what
    assert np.array_equal(count.cpu().numpy(), ref.count), what
    assert int(skipped.cpu()[0]) == ref.skipped, what
    assert len(plain) == 3 and all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                   for a, b in zip(plain, (normals, variation, count))), what
    return nr.check_rows(normals.cpu().numpy(), variation.cpu().numpy(), ref, q, None if toward is None else toward[:, None, :], what)


@pytest.mark.parametrize("mode", ["compat", "fixed"])
@pytest.mark.parametrize("shape,fam,radius", GRAPH_CASES)
def test_graph_form_on_the_device_searches_graphs(dev, shape, fam, radius, mode):
    B, N, M, K = shape
    db, q = _clouds(shape, fam)
    prev = tf_nnquery.get_radius_mode()
    tf_nnquery.set_radius_mode(mode)
    try:
        idx, cnt, _ = tf_nnquery.build_sphere_neighbor(_t(db, dev), _t(q, dev), radius, None, K)
    finally:
        tf_nnquery.set_radius_mode(prev)
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    toward = np.tile(np.array([[0.3, 0.2, 5.0]], np.float32), (B, 1)) + np.arange(B, dtype=np.float32)[:, None]
    for tw in (None, toward):
        stats = _check_graph(dev, db, q, idx, cnt, radius, tw, "%s %s toward=%s" % (shape, mode, tw is not None))
        if K == 1:
            assert stats["compared"] == 0                      # (one neighbour: every row is degenerate, and zero)
        else:
            assert stats["compared"] >= 0.95 * B * M


@pytest.mark.parametrize("B,M", [(0, 16), (1, 0)])
def test_graph_form_without_rows(dev, B, M):
    out = tf_surface.graph_normals(torch.zeros((B, 32, 3), device=dev), torch.zeros((B, M, 3), device=dev),
                                   torch.zeros((B, M, 4), dtype=torch.int32, device=dev),
                                   torch.zeros((B, M), dtype=torch.int32, device=dev), 0.1, None, 3, want_moments=True)
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in out] == [(B, M, 3), (B, M), (B, M), (B, M, 10), (1,)] and int(out[4][0]) == 0


def test_graph_form_hand_edits_and_null_outputs(dev):
    """counts edited to 0, 1, 2 and above K, a NaN coordinate in the database; then the C entry with every optional output
    null, and its counter accumulated on top of what it held"""
    shape, fam, radius = GRAPH_CASES[0]
    B, N, M, K = shape
    db, q = _clouds(shape, fam)
    idx, cnt, _ = tf_nnquery.build_sphere_neighbor(_t(db, dev), _t(q, dev), radius, None, K)
    idx, cnt = idx.cpu().numpy().copy(), cnt.cpu().numpy().copy()
    cnt[0, 0:4] = [0, 1, 2, K + 5]
    db[0, idx[0, 4, 0], 0] = np.nan
    q = db[:, :M].copy()
    toward = np.array([[0.0, 0.0, 4.0], [1.0, 1.0, -4.0]], np.float32)
    _check_graph(dev, db, q, idx, cnt, radius, toward, "hand edits")
    ref = nrm.graph_normals_reference(db, q, idx, cnt, radius, None, 3)
    assert ref.skipped > 0 and ref.count[0, 0] == 0 and ref.zero[0, 0:3].all()
    normals = torch.full((B, M, 3), 7.0, device=dev)
    counter = torch.tensor([1000], dtype=torch.int64, device=dev)
    args = [_t(a, dev) for a in (db, q, idx, cnt)]
    _lib.check(_lib.lib().sph3d_graph_normals(B, N, M, K, radius, 3, *[_lib.ptr(a) for a in args], None, _lib.ptr(normals), None,
                                              None, None, _lib.ptr(counter), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert int(counter[0]) == 1000 + ref.skipped
    nr.check_rows(normals.cpu().numpy(), None, ref, q, None, "null outputs")
    for bad in ((0.0, 3), (float("inf"), 3), (radius, 2)):
        with pytest.raises(ValueError):
            tf_surface.graph_normals(*args, bad[0], None, bad[1])
        rc = _lib.lib().sph3d_graph_normals(B, N, M, K, bad[0], bad[1], *[_lib.ptr(a) for a in args], None, _lib.ptr(normals), None,
                                            None, None, None, _lib.stream_ptr())
        assert rc == -1


# ---- ball form ---------------------------------------------------------------------------------------------------------------
def _ball_cloud(name):
    """-> (xyz [V, 3] fp32, radius)"""
    if name.startswith("v"):
        V = int(name[1:])
        fam, radius = {0: ("volume", 0.5), 1: ("volume", 0.5), 63: ("volume", 0.5), 64: ("volume", 0.5), 1000: ("sphere", 0.25),
                       20000: ("box", 0.05)}[V]
        return nr.family(fam, V, 20 + V % 7), radius
    if name == "identical":
        return np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (500, 1)), 0.1
    if name == "radius_beyond_cloud":
        return nr.family("volume", 1000, 4), 4.0
    if name == "crowded_cell":                       # 3000 points inside one cell of the grid, 1000 around them
        rng = np.random.RandomState(8)
        return np.concatenate([(0.5 + 0.004 * rng.rand(3000, 3)).astype(np.float32), nr.family("volume", 1000, 9)]), 0.05
    if name == "non_finite":
        xyz = nr.family("box", 1000, 6)
        xyz[3, 1], xyz[500, 0], xyz[501], xyz[999, 2] = np.nan, np.inf, [np.nan, np.inf, -np.inf], -np.inf
        return xyz, 0.2
    raise ValueError(name)


_BALL_MOMENTS = {}


def _ball_ref(name, toward):
    xyz, radius = _ball_cloud(name)
    if name not in _BALL_MOMENTS:                    # (brute force on the host: once per cloud, whatever `toward`)
        _BALL_MOMENTS[name] = nrm.ball_moments_reference(xyz, radius)
    m = _BALL_MOMENTS[name]
    n, v, f = nrm.normals_from_moments_reference(m, xyz, toward, 3, full=True)
    f.normals, f.variation, f.moments, f.count = n, v, m, m[:, 0].astype(np.int32)
    return xyz, radius, f


@pytest.mark.parametrize("name", ["v0", "v1", "v63", "v64", "v1000", "v20000", "identical", "radius_beyond_cloud", "crowded_cell",
                                  "non_finite"])
def test_ball_form(dev, name):
    for toward in (None, np.array([0.1, 0.2, 6.0], np.float32)):
        xyz, radius, ref = _ball_ref(name, toward)
        V = xyz.shape[0]
        tw = None if toward is None else _t(toward, dev)
        normals, variation, count, moments = tf_surface.ball_normals(_t(xyz, dev).reshape(V, 3), radius, tw, 3, want_moments=True)
        plain = tf_surface.ball_normals(_t(xyz, dev).reshape(V, 3), radius, tw, 3)
        torch.cuda.synchronize()
        what = "%s toward=%s" % (name, toward is not None)
        assert np.array_equal(moments.cpu().numpy(), ref.moments), what
        assert np.array_equal(count.cpu().numpy(), ref.count), what
        assert len(plain) == 3 and all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                       for a, b in zip(plain, (normals, variation, count))), what
        nr.check_rows(normals.cpu().numpy(), variation.cpu().numpy(), ref, xyz, toward, what)
        if name in ("radius_beyond_cloud", "identical"):
            assert (ref.count == V).all()
        if name == "identical":
            assert ref.zero.all()
        if name == "crowded_cell":
            assert ref.count.max() >= 3000
        if name == "non_finite":
            assert ref.count[[3, 500, 501, 999]].tolist() == [0, 0, 0, 0] and ref.zero[[3, 500, 501, 999]].all()


def test_ball_form_twice_is_bit_equal(dev):
    xyz, radius = _ball_cloud("v1000")
    tw = _t(np.array([0.1, 0.2, 6.0], np.float32), dev)
    a = tf_surface.ball_normals(_t(xyz, dev), radius, tw, 3, want_moments=True)
    b = tf_surface.ball_normals(_t(xyz, dev), radius, tw, 3, want_moments=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def test_ball_form_refuses_bad_requests(dev):
    xyz = torch.zeros((8, 3), device=dev)
    for radius, min_count in ((0.0, 3), (-1.0, 3), (float("nan"), 3), (0.1, 2)):
        with pytest.raises(ValueError):
            tf_surface.ball_normals(xyz, radius, None, min_count)
    l = _lib.lib()
    assert l.sph3d_ball_normals_workspace((1 << 26) + 1) == 0 and l.sph3d_ball_normals_workspace(1 << 20) > (1 << 20) * 16
    rc = l.sph3d_ball_normals((1 << 26) + 1, 0.1, 3, None, None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"2^26" in l.sph3d_last_error()


def test_registered_ops(dev):
    """torch.ops.sph3d.graph_normals / ball_normals go through the dispatcher, equal the public functions bit for bit, and
    their schema and fake registrations hold (torch.library.opcheck)"""
    xyz, radius = _ball_cloud("v1000")
    pts = _t(xyz, dev)
    tw = _t(np.array([0.1, 0.2, 6.0], np.float32), dev)
    want = tf_surface.ball_normals(pts, radius, tw, 3, want_moments=True)
    got = torch.ops.sph3d.ball_normals(pts, radius, tw, 3, True)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(got, want))
    db = pts[None, :512].contiguous()
    idx, cnt, _ = tf_nnquery.build_sphere_neighbor(db, db, radius, None, 16)
    want = tf_surface.graph_normals(db, db, idx, cnt, radius, None, 3, want_moments=True)
    got = torch.ops.sph3d.graph_normals(db, db, idx, cnt, radius, None, 3, True)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(got, want))
    for op, args in ((torch.ops.sph3d.ball_normals, (pts, radius, tw, 3, True)), (torch.ops.sph3d.ball_normals, (pts, radius, None, 3, False)),
                     (torch.ops.sph3d.graph_normals, (db, db, idx, cnt, radius, tw[None], 3, True)),
                     (torch.ops.sph3d.graph_normals, (db, db, idx, cnt, radius, None, 3, False))):
        torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))


# ---- pool and model ----------------------------------------------------------------------------------------------------------
def test_estimated_facade_pool_and_a_training_step(dev):
    """FacadePool.from_arrays_estimated equals per-facade ball_normals bit for bit, and the nine-channel model trains on it"""
    sizes, radius, N, B = (1500, 1100), 0.15, 1024, 2
    rng = np.random.RandomState(2)
    xyz = [synth.s3dis_batch(60 + k, 1, n, extent=(1.0, 1.0, 1.5))[0][0, :, 0:3].astype(np.float32) for k, n in enumerate(sizes)]
    rgb = [(rng.rand(n, 3) * 2 - 1).astype(np.float32) for n in sizes]
    label = [rng.randint(0, 7, n).astype(np.int32) for n in sizes]
    toward = torch.tensor([0.5, 0.5, 9.0], device=dev)
    pool = facadefeed.FacadePool.from_arrays_estimated(xyz, rgb, label, radius, toward, device=dev)
    assert tuple(pool.normals.shape) == (sum(sizes), 4) and pool.normals.dtype == torch.float32
    assert not pool.normals[:, 3].any() and torch.isfinite(pool.normals).all()
    lo = 0
    for x in xyz:
        want = tf_surface.ball_normals(_t(x, dev), radius, toward)[0]
        assert torch.equal(pool.normals[lo:lo + len(x), 0:3].view(torch.int32), want.view(torch.int32))
        length = want.double().pow(2).sum(dim=1).sqrt()
        zero = nrm.ball_normals_reference(x, radius, toward.cpu().numpy(), 3).zero
        assert np.array_equal((length == 0).cpu().numpy(), zero) and zero.mean() < 0.02
        assert ((length - 1).abs() <= 2.0 ** -23)[torch.from_numpy(~zero).to(dev)].all()
        lo += len(x)
    assert torch.equal(nrm.estimate_pool(pool.pool, radius, toward), pool.normals)
    bn, bv, bc = nrm.batch_normals(pool.rows[0:1024].reshape(1, 1024, 8), radius, 32)
    assert tuple(bn.shape) == (1, 1024, 3) and tuple(bv.shape) == (1, 1024) and torch.isfinite(bn).all()
    model = ruemonge_net.SPH3DRueMonge(ruemonge_net.small_config(N), device=dev, seed=3)
    f = facadefeed.FacadeFeed(pool, B, N, seed=5, repeat=2)
    pts, lab, ready = next(iter(f))
    pred, _ = model(pts, is_training=True, points_ready=ready)
    torch.cuda.current_stream().wait_event(ready)
    loss = model.loss(pred, lab)
    f.done(ready)
    loss.backward()
    torch.cuda.synchronize()
    assert pred.shape == (B, N, 7) and np.isfinite(float(loss.detach()))
    print("loss %r" % float(loss.detach()))
