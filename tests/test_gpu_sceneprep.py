"""csrc/prep.hip and the device half of harness/sceneprep.py against the numpy statement: voxel means as bit patterns, counts,
voxel_of_point, rectangle counts, the plan, block rows / offsets / index and the pool all EQUAL, no tolerance.  Every launch here
is an ordinary one; a grid that does not fit is refused through the header's flag, bad requests through status codes."""
import collections
import functools

import numpy as np
import pytest

from sph3d_gcn_amd.harness import feed, sceneprep as sp, scenemerge as sm, scenesynth

pytestmark = pytest.mark.gpu
F32 = np.float32


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _up(dev, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


@functools.lru_cache(maxsize=None)
def _room():
    """F = 60 000 on a 4 x 3.2 x 3 m synthetic room, A = 3 -> full cloud, colours, labels and the statement's voxel cloud"""
    full_xyz, full_label, _vx, _vl = scenesynth.synthetic_scene(11, 60000, extent=(4, 3.2, 3))
    rgb = (np.random.RandomState(0).rand(len(full_xyz), 3) * 255).astype(F32)
    return full_xyz, rgb, full_label, sp.voxel_reference(full_xyz, rgb, 0.03)


def _check_voxelize(dev, xyz, attr, h, name, **kw):
    want = sp.voxel_reference(xyz, attr, h, **kw)
    d_xyz, d_attr = _up(dev, xyz, attr)
    for mode in (sp.REDUCE_ATOMIC, sp.REDUCE_SORTED):
        vx, va, count, vop = sp.voxelize(d_xyz, d_attr, h, mode=mode, **kw)
        got = np.concatenate([vx.cpu().numpy(), va.cpu().numpy()], axis=1)
        assert _same_bits(got.view(np.int32), want[0].view(np.int32)), (name, mode)
        assert _same_bits(count.cpu().numpy(), want[1]) and _same_bits(vop.cpu().numpy(), want[2]), (name, mode)
    V, dropped, _n, _lo, _hi, _vop = sp.voxel_grid(d_xyz, d_attr, h, **kw)
    assert (V, dropped) == (len(want[0]), want[3]), name
    return want


def test_voxelize_a_room_and_the_same_room_shuffled(dev):
    full_xyz, rgb, _label, want = _room()
    got = _check_voxelize(dev, full_xyz, rgb, 0.03, "room")
    assert _same_bits(got[0], want[0]) and len(want[0]) > 40000 and want[1].max() >= 4
    perm = np.random.RandomState(1).permutation(len(full_xyz))
    shuffled = _check_voxelize(dev, full_xyz[perm], rgb[perm], 0.03, "shuffled")
    assert _same_bits(shuffled[0], want[0]) and _same_bits(shuffled[1], want[1])


def test_voxelize_small_clouds_one_cell_and_an_axis_of_one_cell(dev):
    rng = np.random.RandomState(2)
    for F in (1, 2, 63, 64, 65):
        _check_voxelize(dev, (rng.rand(F, 3) * 0.2).astype(F32), (rng.rand(F, 3) * 255).astype(F32), 0.03, "F=%d" % F)
    one = _check_voxelize(dev, (rng.rand(5000, 3) * 0.02 + 7).astype(F32), (rng.rand(5000, 3) * 255).astype(F32), 0.03, "one cell")
    assert len(one[0]) == 1 and one[1].tolist() == [5000]
    flat = (rng.rand(3000, 3) * np.array([2.0, 1.0, 0.09])).astype(F32)
    _check_voxelize(dev, flat, (rng.rand(3000, 1) * 9).astype(F32), 0.1, "n_z = 1")
    assert sp.grid_shape(flat.min(0), flat.max(0), F32(0.1), 1 << 20)[2] == 1
    # exact lattice points: on lo, on hi and on cell faces
    g = np.stack(np.meshgrid(np.arange(9), np.arange(5), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    xyz = np.concatenate([g * 0.25 - 1.0, g * 0.25 - 0.875]).astype(F32)
    _check_voxelize(dev, xyz, np.zeros((len(xyz), 0), F32), 0.25, "faces")


def test_voxelize_drops_non_finite_and_out_of_range_points(dev):
    rng = np.random.RandomState(3)
    xyz, attr = (rng.rand(4000, 3) * 2 - 1).astype(F32), (rng.rand(4000, 3) * 255).astype(F32)
    xyz[::97, 0] = np.nan
    xyz[5::97, 2] = np.inf
    attr[9::97, 1] = -np.inf
    attr[11::97, 2] = np.nan
    xyz[13::97, 1] = 2.0 ** 17 * 1.001
    attr[17::97, 0] = -2.0 ** 20
    want = _check_voxelize(dev, xyz, attr, 0.05, "dropped")
    assert want[3] == sum(len(range(k, 4000, 97)) for k in (0, 5, 9, 11, 13, 17)) and (want[2] == -1).sum() == want[3]
    d_xyz, d_attr = _up(dev, np.full((70, 3), np.nan, F32), np.zeros((70, 3), F32))
    with pytest.raises(ValueError):
        sp.voxelize(d_xyz, d_attr, 0.05)


def test_a_grid_beyond_max_cells_is_refused_by_the_flag(dev):
    """the table holds max_cells cells; a cloud that needs more raises the flag on the device, every later kernel of the call
    returns without touching a cell, and the harness raises"""
    import torch
    full_xyz, rgb, _label, want = _room()
    d_xyz, d_attr = _up(dev, full_xyz, rgb)
    nx, ny, nz = sp.grid_shape(full_xyz.min(0), full_xyz.max(0), F32(0.03), 1 << 26)
    for cells in (1000, nx * ny * nz - 1, nx * ny - 1):
        with pytest.raises(sp.GridTooLarge):
            sp.voxelize(d_xyz, d_attr, 0.03, max_cells=cells)
        with pytest.raises(sp.GridTooLarge):
            sp.voxel_reference(full_xyz, rgb, 0.03, max_cells=cells)
    with pytest.raises(sp.GridTooLarge):
        sp.voxelize(d_xyz, d_attr, 1e-30)
    vx, va, count, vop = sp.voxelize(d_xyz, d_attr, 0.03, max_cells=nx * ny * nz)           # the exact size fits
    assert _same_bits(vx.cpu().numpy(), want[0][:, 0:3])
    torch.cuda.synchronize()


def test_rectangle_counts_and_the_plan_on_the_branch_coverage_cloud(dev):
    for seed in (0, 1, 2):
        xyz = scenesynth.coverage_cloud(seed)
        lo, hi = xyz.min(axis=0), xyz.max(axis=0)
        want = sp.block_plan(lo[0:2], hi[0:2], lambda r: sp.rect_counts_reference(xyz, r), thresh=500)
        (d_xyz,) = _up(dev, xyz)
        asked = []

        def on_device(rects):
            asked.append(len(rects))
            return sp.rect_counts(d_xyz, rects).cpu().numpy()
        got = sp.block_plan(lo[0:2], hi[0:2], on_device, thresh=500)
        kinds = collections.Counter(k for k, _r in want)
        written = [r for k, r in want if k >= 0]
        assert set(kinds) == set(range(-1, 9)) and len(set(written)) < len(written) and asked == [81 * 9]
        assert got == want
        cand = sp.candidate_rects(lo[0:2], hi[0:2])
        both = np.concatenate([sp.rounded_rects(cand).reshape(-1, 4), sp.rounded_rects(cand, 0.3).reshape(-1, 4)])
        assert np.array_equal(sp.rect_counts(d_xyz, both).cpu().numpy(), sp.rect_counts_reference(xyz, both))
    many = np.tile(both, (4, 1))[:5000]                                      # more than one LDS tile of rectangles
    assert np.array_equal(sp.rect_counts(d_xyz, many).cpu().numpy(), sp.rect_counts_reference(xyz, many))


def _check_split(dev, xyz, rgb, label, thresh, name):
    blocks, index, plan = sp.split_reference(xyz, rgb, label, thresh=thresh)
    d = _up(dev, xyz, rgb, label)
    rows, offsets, sizes, idx, got = sp.split(*d, thresh=thresh, want_plan=True)
    assert got.plan == plan, name
    assert np.array_equal(sizes, [len(b) for b in blocks]) and np.array_equal(offsets.cpu().numpy(), np.concatenate(([0], np.cumsum(sizes))))
    assert _same_bits(rows.cpu().numpy().view(np.int32), np.concatenate(blocks).view(np.int32)), name
    assert _same_bits(idx.cpu().numpy(), np.concatenate(index)), name
    _r, _i, _o, mismatch = sp.fill_split(*d, got)
    assert int(mismatch.cpu()) == 0
    return blocks, index, plan, (rows, offsets, sizes, idx)


def test_split_on_the_coverage_cloud_and_the_pool_from_device(dev):
    xyz = scenesynth.coverage_cloud(0)
    rgb = np.random.RandomState(4).rand(len(xyz), 3).astype(F32)
    label = np.random.RandomState(5).randint(0, 13, len(xyz)).astype(np.int32)
    blocks, index, plan, (rows, offsets, sizes, idx) = _check_split(dev, xyz, rgb, label, 500, "coverage")
    written = [r for k, r in plan if k >= 0]
    assert len(blocks) == len(written) > len(set(written))                   # duplicates are kept
    sob = [0] * (len(blocks) // 2) + [3] * (len(blocks) - len(blocks) // 2)
    got = feed.BlockPool.from_device(rows, offsets, sizes, idx, sob)
    want = feed.BlockPool(blocks, dev, index, sob)
    assert got.rows.data_ptr() == rows.data_ptr() and got.device == want.device and len(got) == len(want)
    for name in ("rows", "offsets", "index"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and _same_bits(a.cpu().numpy(), b.cpu().numpy()), name
    assert np.array_equal(got.sizes, want.sizes) and np.array_equal(got.host_offsets, want.host_offsets)
    assert np.array_equal(got.scene_of_block, want.scene_of_block)
    with pytest.raises(ValueError):
        feed.BlockPool.from_device(rows, offsets, sizes, idx, sob[::-1])
    with pytest.raises(ValueError):
        feed.BlockPool.from_device(rows[1:], offsets, sizes, idx, sob)


@pytest.mark.parametrize("thresh", [2500, 6000])
def test_split_on_the_rooms_voxel_cloud(dev, thresh):
    _xyz, _rgb, full_label, (voxel, _count, _vop, _dropped) = _room()
    nx, nc, _c = sp.normalise_reference(voxel[:, 0:3], voxel[:, 3:6])
    label = (np.arange(len(nx)) % 13).astype(np.int32)
    d_xyz, d_rgb = _up(dev, np.ascontiguousarray(voxel[:, 0:3]), np.ascontiguousarray(voxel[:, 3:6]))
    got_xyz, got_rgb = sp.normalise(d_xyz, d_rgb)
    assert _same_bits(got_xyz.cpu().numpy().view(np.int32), nx.view(np.int32))
    assert _same_bits(got_rgb.cpu().numpy().view(np.int32), nc.view(np.int32))
    _blocks, _index, plan, _dev = _check_split(dev, nx, nc, label, thresh, "room")
    kinds = collections.Counter(k for k, _r in plan)
    assert kinds[0] > 0 and sum(v for k, v in kinds.items() if k > 0) > 0, sorted(kinds.items())    # kept AND merged squares
    print("thresh %d: %s" % (thresh, sorted(kinds.items())))


def test_entries_refuse_bad_requests_through_status_codes(dev):
    import torch
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    xyz = torch.zeros((10, 3), device=dev)
    i32 = torch.zeros((16,), dtype=torch.int32, device=dev)
    ws = torch.empty((l.sph3d_prep_voxel_grid_workspace(10, 64),), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr()
    grid = lambda F, A, h, cells, nbytes: l.sph3d_prep_voxel_grid(F, A, _lib.ptr(xyz), _lib.ptr(xyz), h, cells, _lib.ptr(i32),
                                                                  _lib.ptr(i32), _lib.ptr(ws), nbytes, st)
    assert grid(10, 3, 0.1, 64, ws.numel() - 1) == -1 and b"workspace" in l.sph3d_last_error()
    assert grid(10, 3, 0.0, 64, ws.numel()) == -1 and grid(10, 14, 0.1, 64, ws.numel()) == -1
    assert grid(0, 3, 0.1, 64, ws.numel()) == -1 and grid(10, 3, 0.1, (1 << 30) + 1, ws.numel()) == -1
    assert l.sph3d_prep_voxel_reduce(10, 3, 11, _lib.ptr(xyz), _lib.ptr(xyz), _lib.ptr(i32), 0, _lib.ptr(ws), _lib.ptr(i32), None, 0, st) == -1
    assert l.sph3d_prep_voxel_reduce(10, 3, 5, _lib.ptr(xyz), _lib.ptr(xyz), _lib.ptr(i32), 7, _lib.ptr(ws), _lib.ptr(i32), None, 0, st) == -1
    assert l.sph3d_prep_rect_count(10, 0, _lib.ptr(xyz), _lib.ptr(xyz), _lib.ptr(i32), st) == -1
    assert l.sph3d_prep_block_fill(10, 1, 4, _lib.ptr(xyz), _lib.ptr(xyz), _lib.ptr(i32), _lib.ptr(xyz), _lib.ptr(ws), _lib.ptr(xyz),
                                   _lib.ptr(i32), _lib.ptr(i32), None, 0, st) == -1
    assert l.sph3d_prep_box(10, None, _lib.ptr(i32), st) == -1
    with pytest.raises(_lib.Sph3dError):
        sp.voxelize(torch.zeros((4, 3)), torch.zeros((4, 3)))
    with pytest.raises(ValueError):
        sp.split(xyz, xyz, i32[:10], thresh=0)
    with pytest.raises(ValueError):
        sp.split(xyz, xyz, i32[:10], thresh=11)                              # no square holds that many points
    torch.cuda.synchronize()


class _Toy:
    """a cheap deterministic "network": a fixed [6, C] matrix on the points (the same function in every call)"""

    def __init__(self, C, dev, seed=0):
        import torch
        self.w = torch.from_numpy(np.random.RandomState(seed).randn(6, C).astype(F32)).to(dev)

    def __call__(self, points, label, inner):
        return (points.unsqueeze(-1) * self.w).sum(dim=2)


def test_prepare_scenes_then_evaluate_equals_the_host_preparation(dev):
    """two synthetic scenes: prepared on the device and evaluated, against the same scenes prepared by the statement on the host,
    pooled through BlockPool's host constructor and evaluated by the same device loop: pools, scenes, confusion matrices and
    counters equal"""
    C, N, seed, bs, h, thresh = 13, 1024, 5, 4, 0.05, 3000
    raw, blocks, index, sob, scenes = [], [], [], [], []
    for s, (n, ext) in enumerate([(20000, (3.0, 2.4, 2.0)), (12000, (2.4, 1.6, 2.0))]):
        fx, fl, _vx, _vl = scenesynth.synthetic_scene(30 + s, n, extent=ext, num_cls=C)
        rgb = (np.random.RandomState(s).rand(n, 3) * 255).astype(F32)
        raw.append((fx, rgb, fl))
        b, i, vx, vl = sp.prepare_scene_reference(fx, rgb, fl, h=h, thresh=thresh)
        blocks += b
        index += i
        sob += [s] * len(b)
        scenes.append(sm.Scene(vx, vl, fx, fl))
    pool, got_scenes = sp.prepare_scenes(raw, h=h, thresh=thresh, device=dev)
    want_pool = feed.BlockPool(blocks, dev, index, sob)
    assert _same_bits(pool.rows.cpu().numpy().view(np.int32), want_pool.rows.cpu().numpy().view(np.int32))
    assert _same_bits(pool.index.cpu().numpy(), want_pool.index.cpu().numpy())
    assert _same_bits(pool.offsets.cpu().numpy(), want_pool.offsets.cpu().numpy())
    assert np.array_equal(pool.scene_of_block, want_pool.scene_of_block) and np.array_equal(pool.sizes, want_pool.sizes)
    for a, b in zip(got_scenes, scenes):
        assert _same_bits(a.voxel_xyz.view(np.int32), b.voxel_xyz.view(np.int32)) and _same_bits(a.voxel_label, b.voxel_label)
        assert _same_bits(a.full_xyz, b.full_xyz) and _same_bits(a.full_label, b.full_label)
    got = sm.evaluate_scenes(_Toy(C, dev), pool, got_scenes, bs, N, seed, C)
    want = sm.evaluate_scenes(_Toy(C, dev), want_pool, scenes, bs, N, seed, C)
    assert np.array_equal(got.confusion_full, want.confusion_full) and np.array_equal(got.confusion_voxel, want.confusion_voxel)
    assert np.array_equal(got.block.confusion, want.block.confusion) and got.block.passes == want.block.passes
    assert got.unseen_rows == want.unseen_rows and got.skipped_rows == want.skipped_rows and got.out_of_scene == want.out_of_scene
    assert got.complete == want.complete and got.confusion_full.sum() == sum(len(r[0]) for r in raw)
    print("full mIoU %.4f voxel mIoU %.4f, %d blocks" % (got.full.miou, got.voxel.miou, len(pool)))
