"""harness/feed.py without a device: assemble_reference (the specification of the draws that csrc/feed.hip must reproduce bit for
bit), its statistics under fixed seeds, the transform against the reference's recorded results, the epoch plan, and the C
entry's declaration and host-side validation."""
import ctypes
import os
import re

import numpy as np
import pytest

from sph3d_gcn_amd.harness import feed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sph3d.h")
TAIL = 1e-6          # every chi-square statistic below must lie under the 1 - TAIL quantile of its distribution


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "blockio_ref.npz"))


# ---- the sample ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8192, 8193, 16384, 16385, 100000])
def test_enough_rows_gives_distinct_rows_in_range(n):
    N = 8192
    for step in range(3):
        r = feed.assemble_reference([n], [0, 0], N, seed=11, step=step, augment=True)
        assert r.index.shape == (2, N) and r.index.dtype == np.int32
        for b in range(2):
            assert r.index[b].min() >= 0 and r.index[b].max() < n
            assert np.unique(r.index[b]).size == N
    assert 4 ** feed.feistel_bits(n) < 4 * n and 4 ** feed.feistel_bits(n) >= n


def test_n_equal_num_point_is_a_permutation_and_not_the_identity():
    r = feed.assemble_reference([1024], [0], 1024, seed=5, step=0, augment=False)
    assert np.array_equal(np.sort(r.index[0]), np.arange(1024))
    assert (r.index[0] != np.arange(1024)).mean() > 0.99


@pytest.mark.parametrize("n", [1, 2, 500, 8191])
def test_too_few_rows_samples_with_replacement_in_range(n):
    r = feed.assemble_reference([n], [0], 8192, seed=3, step=9, augment=False)
    assert r.index.min() >= 0 and r.index.max() < n
    if n >= 500:
        assert np.unique(r.index[0]).size > 0.6 * min(n, 8192)        # 1 - 1/e of the rows of a block of about N rows, more of a small one


def test_pure_function_of_its_arguments():
    sizes = [3000, 700, 20000, 1024]
    ids = [2, 0, 1, 3, 0, 2, 1]
    a = feed.assemble_reference(sizes, ids, 1024, 77, 5, True)
    b = feed.assemble_reference(np.array(sizes), np.array(ids, dtype=np.int32), 1024, 77, 5, True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    other_step = feed.assemble_reference(sizes, ids, 1024, 77, 6, True)
    other_seed = feed.assemble_reference(sizes, ids, 1024, 78, 5, True)
    for o in (other_step, other_seed):
        for cloud in range(len(ids)):
            assert not np.array_equal(a.index[cloud], o.index[cloud])
        assert not np.array_equal(a.theta[:2], o.theta[:2]) and not np.array_equal(a.noise[2:4], o.noise[2:4])
    # the same block at two places of the batch: two different samples (clouds 1 and 4 are block 0, clouds 0 and 5 block 2)
    assert not np.array_equal(a.index[1], a.index[4]) and not np.array_equal(a.index[0], a.index[5])
    # augment = False: the same rows, no angles, no noise
    plain = feed.assemble_reference(sizes, ids, 1024, 77, 5, False)
    assert np.array_equal(plain.index, a.index) and not plain.kind.any() and not plain.noise.any()
    assert a.kind.tolist() == [1, 1, 2, 2, 0, 0, 0]                      # third = 7 // 3
    # a cloud's draws do not depend on the rest of the batch (only on its place b)
    solo = feed.assemble_reference(sizes, ids[:3], 1024, 77, 5, False)
    assert np.array_equal(solo.index, a.index[:3])


def test_rejects_what_the_host_path_rejects():
    with pytest.raises(ValueError, match="empty block"):
        feed.assemble_reference([10, 0], [1], 16, 0, 0, False)
    with pytest.raises(ValueError):
        feed.assemble_reference([10], [1], 16, 0, 0, False)
    with pytest.raises(ValueError):
        feed.assemble_reference([10], [0], 0, 0, 0, False)
    with pytest.raises(ValueError, match="empty block"):
        feed.BlockPool.from_blocks([np.zeros((5, 8), np.float32), np.zeros((0, 8), np.float32)])
    with pytest.raises(ValueError):
        feed.BlockPool.from_blocks([np.zeros((5, 6), np.float32)])


# ---- statistics, fixed seeds ---------------------------------------------------------------------------------------------
def _inclusion_chi2(n, N, steps, seed):
    """-> the statistic and its degrees of freedom.  Over `steps` independent samples of N of n rows the inclusion count of a
    row has mean S p and, with the hypergeometric covariance -p(1-p)/(n-1) between two rows of one sample, the quadratic form
    sum (c_i - S p)^2 (n-1) / (n S p (1-p)) is chi-square with n-1 degrees of freedom."""
    counts = np.zeros(n, dtype=np.int64)
    for step in range(steps):
        counts += np.bincount(feed.sample_without_replacement(feed.cloud_key(seed, step, step % 16), n, N), minlength=n)
    p = N / n
    return float(((counts - steps * p) ** 2).sum() * (n - 1) / (n * steps * p * (1 - p))), n - 1


@pytest.mark.parametrize("n,N,steps", [(1025, 1024, 4000), (1500, 1024, 2000), (2048, 1024, 2000), (2049, 1024, 2000),
                                       (5000, 1024, 2000), (12000, 8192, 2000)])
def test_inclusion_counts_follow_sampling_without_replacement(n, N, steps):
    """Statistic / degrees of freedom obtained (seed 2024), with the two bounds chi2.ppf(1e-6) / df and chi2.ppf(1 - 1e-6) / df:
    1024 of 1025 (4000 samples): 0.958 in [0.804, 1.224]; 1024 of 1500: 1.045 in [0.836, 1.183]; of 2048: 1.073 in
    [0.858, 1.156]; of 2049: 1.073 in [0.858, 1.156]; of 5000: 1.052 in [0.908, 1.098]; 8192 of 12000: 1.020 in [0.940, 1.063]."""
    from scipy.stats import chi2
    stat, df = _inclusion_chi2(n, N, steps, seed=2024)
    print("inclusion n=%d N=%d steps=%d: chi2/df = %.4f (bounds %.4f .. %.4f)" % (n, N, steps, stat / df, chi2.ppf(TAIL, df) / df,
                                                                                 chi2.ppf(1 - TAIL, df) / df))
    assert stat < chi2.ppf(1 - TAIL, df)
    assert stat > chi2.ppf(TAIL, df)          # nor more even than chance: a walk that visits rows in turn would be


@pytest.mark.parametrize("n", [8192, 8193, 16385, 100000])
@pytest.mark.parametrize("slot", [0, 8191])
def test_a_slot_is_uniform_over_the_block(n, slot):
    """Slot 0 seeds the farthest-point sampling and capped neighbour lists keep the lowest indices: the ORDER must be
    exchangeable, not only the set.  Histogram of one slot's row over 64 equal cells, 6400 keys; statistic obtained (63 degrees
    of freedom, bound chi2.ppf(1 - 1e-6, 63) = 131.4): slot 0: 64.8, 65.0, 50.8, 57.1; slot 8191: 50.3, 50.2, 54.2, 51.9 for
    n = 8192, 8193, 16385, 100000."""
    from scipy.stats import chi2
    steps = 6400
    rows = np.empty(steps, dtype=np.int64)
    for step in range(steps):
        ck = feed.cloud_key(99, step // 8, step % 8)
        # (slot j of the sample is a function of j alone: evaluate the one slot)
        rows[step] = _one_slot(ck, n, slot)
    edges = (np.arange(65) * n) // 64
    hist = np.histogram(rows, bins=edges)[0]
    expect = steps * np.diff(edges) / n
    stat = float(((hist - expect) ** 2 / expect).sum())
    print("slot %d of n=%d: chi2 = %.2f, bound %.2f" % (slot, n, stat, chi2.ppf(1 - TAIL, 63)))
    assert stat < chi2.ppf(1 - TAIL, 63)


def _one_slot(ck, n, slot):
    half = feed.feistel_bits(n)
    mask, sh = np.uint32((1 << half) - 1), np.uint32(half)
    rk = feed._hi(feed.draw(ck, feed.PERM, np.arange(feed.ROUNDS)))
    v = np.array([slot], dtype=np.uint32)
    with np.errstate(over="ignore"):
        while True:
            L, R = v >> sh, v & mask
            for t in range(feed.ROUNDS):
                L, R = R, L ^ (feed._fmix32(R ^ rk[t]) & mask)
            v = (L << sh) | R
            if v[0] < n:
                return int(v[0])


def test_one_slot_helper_is_the_sample():
    ck = feed.cloud_key(1, 2, 3)
    full = feed.sample_without_replacement(ck, 20000, 8192)
    assert [_one_slot(ck, 20000, s) for s in (0, 1, 4097, 8191)] == full[[0, 1, 4097, 8191]].tolist()


def test_sampling_with_replacement_is_uniform():
    """rows of a 500-row block over 200 keys x 8192 slots, 499 degrees of freedom: statistic obtained 455.4 (bound 663.8)"""
    from scipy.stats import chi2
    n, N, steps = 500, 8192, 200
    counts = np.zeros(n, dtype=np.int64)
    for step in range(steps):
        counts += np.bincount(feed.sample_with_replacement(feed.cloud_key(5, step, 0), n, N), minlength=n)
    expect = steps * N / n
    stat = float(((counts - expect) ** 2 / expect).sum())
    print("with replacement: chi2 = %.1f, bound %.1f" % (stat, chi2.ppf(1 - TAIL, n - 1)))
    assert stat < chi2.ppf(1 - TAIL, n - 1)


def test_jitter_noise_is_the_clipped_normal():
    """3 x 8192 x 40 = 983 040 draws.  Obtained: mean -9.9e-6 (standard error 9.7e-6: 1.0 s.e.), share at the clip 4.583 %
    against P(|z| > 2) = 4.550 % (s.e. 0.021 %: 1.6 s.e.), standard deviation 0.009608 against 0.009594 of the clipped normal."""
    from scipy.stats import norm
    noise = np.concatenate([feed.jitter_noise(feed.cloud_key(31, step, 4), 8192).ravel() for step in range(40)])
    m = noise.size
    assert np.abs(noise).max() <= feed.JITTER_CLIP
    p_clip = 2 * norm.sf(2.0)                                                       # 0.0455
    var_z = (1 - p_clip) - 4 * norm.pdf(2.0) + 4 * p_clip                           # E clip(z, +-2)^2
    se_mean = feed.JITTER_SIGMA * np.sqrt(var_z / m)
    share = float((np.abs(noise) >= feed.JITTER_CLIP).mean())
    se_share = np.sqrt(p_clip * (1 - p_clip) / m)
    print("jitter: mean %.3e (s.e. %.3e), clipped %.5f (expected %.5f, s.e. %.2e), std %.6f (expected %.6f)"
          % (noise.mean(), se_mean, share, p_clip, se_share, noise.std(), feed.JITTER_SIGMA * np.sqrt(var_z)))
    assert abs(noise.mean()) < 6 * se_mean
    assert abs(share - p_clip) < 6 * se_share
    # the variance of the squares, for the standard error of the second moment: E c^4 = int_{-2}^{2} z^4 phi + 16 p_clip
    m4 = 3 * (1 - p_clip) - 2 * (8 + 6) * norm.pdf(2.0) + 16 * p_clip
    se_var = feed.JITTER_SIGMA ** 2 * np.sqrt((m4 - var_z ** 2) / m)
    assert abs((noise ** 2).mean() - feed.JITTER_SIGMA ** 2 * var_z) < 6 * se_var
    # the three coordinates of a point and neighbouring points are uncorrelated (they share draws pairwise)
    xyz = noise.reshape(-1, 3)
    for a, b in ((xyz[:, 0], xyz[:, 1]), (xyz[:, 0], xyz[:, 2]), (xyz[:-1, 2], xyz[1:, 0])):
        assert abs(np.corrcoef(a, b)[0, 1]) < 6 / np.sqrt(a.size)


def test_angles_stay_inside_their_clips_and_cover_them():
    """20 000 clouds.  Obtained: theta histogram over 64 cells chi2 = 87.3 (bound 131.4); tilt angles: 0.275 % at the clip
    against P(|z| > 3) = 0.270 %, standard deviation 0.0598."""
    from scipy.stats import chi2, norm
    keys = [feed.cloud_key(8, s // 5, s % 5) for s in range(20000)]
    theta = np.array([feed.turn_angle(k) for k in keys])
    tilt = np.array([feed.tilt_angles(k) for k in keys])
    assert theta.min() >= 0.0 and theta.max() < 2 * np.pi
    assert np.abs(tilt).max() <= feed.ANGLE_CLIP
    hist = np.histogram(theta, bins=64, range=(0.0, 2 * np.pi))[0]
    stat = float(((hist - len(keys) / 64) ** 2 / (len(keys) / 64)).sum())
    share = float((np.abs(tilt) >= feed.ANGLE_CLIP).mean())
    p = 2 * norm.sf(3.0)
    print("theta chi2 = %.1f (bound %.1f); tilt clipped %.5f (expected %.5f), std %.5f" % (stat, chi2.ppf(1 - TAIL, 63), share, p, tilt.std()))
    assert stat < chi2.ppf(1 - TAIL, 63)
    assert abs(share - p) < 6 * np.sqrt(p * (1 - p) / tilt.size)
    assert abs(tilt.mean()) < 6 * feed.ANGLE_SIGMA / np.sqrt(tilt.size)


# ---- the transform against the reference's recorded results -------------------------------------------------------------------
def _within_parity_bound(got, want, src, extra=0.0):
    """README "Parity": 1e-5 per element against the sum of the magnitudes of that element's terms — |x| + |y| + |z| of the
    source row (a rotation mixes all three), plus `extra`"""
    bound = 1e-5 * (np.abs(src).sum(axis=-1, keepdims=True) + extra)
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    print("worst error / bound = %.4f" % float((err / bound).max()))
    assert (err <= bound).all()


def test_transform_reproduces_the_reference_results_from_the_reference_draws():
    """the numpy transform assemble_reference's results are applied with (feed.turn / tilt / jitter), fed the draws the stored
    seeds give, against the arrays the reference's own functions produced (tests/golden/blockio_ref.npz)"""
    g = _golden()
    xyz = g["xyz"]
    rng = np.random.RandomState(int(g["rotate_point_cloud_seed"]))
    got = np.stack([feed.turn(xyz[k], rng.uniform() * 2 * np.pi) for k in range(xyz.shape[0])])
    _within_parity_bound(got, g["rotate_point_cloud"], xyz)
    rng = np.random.RandomState(int(g["rotate_perturbation_point_cloud_seed"]))
    got = np.stack([feed.tilt(xyz[k], np.clip(feed.ANGLE_SIGMA * rng.randn(3), -feed.ANGLE_CLIP, feed.ANGLE_CLIP))
                    for k in range(xyz.shape[0])])
    _within_parity_bound(got, g["rotate_perturbation_point_cloud"], xyz)
    rng = np.random.RandomState(int(g["jitter_point_cloud_seed"]))
    noise = np.clip(feed.JITTER_SIGMA * rng.randn(*xyz.shape), -feed.JITTER_CLIP, feed.JITTER_CLIP)
    _within_parity_bound(feed.jitter(xyz, noise), g["jitter_point_cloud"], xyz, extra=feed.JITTER_CLIP)


def test_apply_reference_builds_the_batch_the_draws_describe():
    rng = np.random.RandomState(0)
    blocks = []
    for n in (300, 90, 150, 64):
        b = rng.rand(n, 8).astype(np.float32)
        b[:, 6] = rng.randint(0, 13, n)
        b[:, 7] = rng.randint(0, 2, n)
        blocks.append(b)
    ids = [3, 1, 0, 2, 1, 0]
    ref = feed.assemble_reference([len(b) for b in blocks], ids, 64, 4, 1, True)
    pts, label, inner = feed.apply_reference(blocks, ids, ref)
    assert ref.kind.tolist() == [1, 1, 2, 2, 0, 0]
    for b in range(6):
        rows = blocks[ids[b]][ref.index[b]]
        assert np.array_equal(pts[b, :, 3:6], rows[:, 3:6]) and np.array_equal(label[b], rows[:, 6].astype(np.int32))
        assert np.array_equal(inner[b], rows[:, 7].astype(np.int32))
        if ref.kind[b] == 0:
            assert np.array_equal(pts[b, :, 0:3], rows[:, 0:3])
        elif ref.kind[b] == 1:          # a rotation: lengths kept, z moved by the tilt only
            np.testing.assert_allclose(np.linalg.norm(pts[b, :, 0:3], axis=1), np.linalg.norm(rows[:, 0:3].astype(np.float64), axis=1), rtol=1e-12)
            assert not np.allclose(pts[b, :, 0:3], rows[:, 0:3])
        else:
            d = pts[b, :, 0:3] - rows[:, 0:3]
            assert np.abs(d).max() <= feed.JITTER_CLIP + 1e-12 and np.abs(d).min() > 0


# ---- the epoch plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 8])
def test_epoch_plan_covers_every_block_once_over_all_ranks(world):
    P, bs = 203, 16
    order = feed.epoch_order(P, 9, 0)
    assert np.array_equal(np.sort(order), np.arange(P))
    plans = [feed.epoch_plan(P, bs, 9, 0, rank, world) for rank in range(world)]
    seen = np.concatenate([ids for plan in plans for _step, ids in plan])
    assert np.array_equal(np.sort(seen), np.arange(P))
    # the batches of all ranks, by their step number, are the epoch's order cut into batches: the same order on every rank
    by_step = sorted(((s, ids) for plan in plans for s, ids in plan), key=lambda t: t[0])
    assert [s for s, _ in by_step] == list(range(13))
    assert np.array_equal(np.concatenate([ids for _, ids in by_step]), order)
    assert [len(ids) for _, ids in by_step] == [16] * 12 + [11]                   # the last, smaller batch is kept
    for rank, plan in enumerate(plans):
        assert [s for s, _ in plan] == list(range(rank, 13, world))
        assert all(ids.dtype == np.int32 for _, ids in plan)


def test_epoch_plan_changes_with_the_epoch_and_numbers_steps_across_epochs():
    a, b = feed.epoch_plan(50, 8, 3, 0), feed.epoch_plan(50, 8, 3, 1)
    assert not np.array_equal(np.concatenate([i for _, i in a]), np.concatenate([i for _, i in b]))
    assert [s for s, _ in a] == list(range(7)) and [s for s, _ in b] == list(range(7, 14))
    again = feed.epoch_plan(50, 8, 3, 1)
    assert all(np.array_equal(x[1], y[1]) for x, y in zip(b, again))
    assert not np.array_equal(feed.epoch_order(50, 4, 0), feed.epoch_order(50, 3, 0))
    assert feed.epoch_plan(5, 8, 3, 0, rank=1, world=2) == []                      # one batch, rank 1 has none this epoch
    with pytest.raises(ValueError):
        feed.epoch_plan(50, 8, 3, 0, rank=2, world=2)
    with pytest.raises(ValueError):
        feed.epoch_plan(0, 8, 3, 0)


# ---- the C entry -----------------------------------------------------------------------------------------------------------------
def test_feed_entry_is_declared_exported_and_bound():
    from sph3d_gcn_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sph3d_feed_assemble\s*\(", text)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "sph3d_feed_assemble")
    res, args = _lib.SIGNATURES["sph3d_feed_assemble"]
    assert res is ctypes.c_int and len(args) == 15
    assert args[7] is ctypes.c_ulonglong and args[8] is ctypes.c_ulonglong          # seed, step: 64 bits
    assert _lib.lib().sph3d_abi_version() == 2
    assert "feed.hip" in open(os.path.join(ROOT, "sph3d_gcn_amd", "csrc", "Makefile")).read()


def test_feed_entry_validates_on_the_host():
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p = (p + 15) & ~15
    ok = dict(B=1, N=1, P=1, T=1, rows=p, offsets=p, ids=p, seed=1, step=2, augment=1, points=p, label=p, inner=p, index=None)

    def call(**kw):
        a = dict(ok, **kw)
        return l.sph3d_feed_assemble(a["B"], a["N"], a["P"], a["T"], a["rows"], a["offsets"], a["ids"], a["seed"], a["step"],
                                     a["augment"], a["points"], a["label"], a["inner"], a["index"], None)

    for kw, text in ((dict(B=0), b"B>0"), (dict(B=-3), b"B>0"), (dict(N=0), b"num_point>0"), (dict(N=-1), b"num_point>0"),
                     (dict(P=0), b"empty pool"), (dict(T=0), b"empty pool"), (dict(augment=2), b"augment"),
                     (dict(rows=None), b"null input"), (dict(offsets=None), b"null input"), (dict(ids=None), b"null input"),
                     (dict(points=None), b"null output"), (dict(label=None), b"null output"), (dict(inner=None), b"null output"),
                     (dict(rows=p + 4), b"aligned"), (dict(B=1 << 20, N=1 << 20), b"too large")):
        rc = call(**kw)                                    # every one is rejected before any launch
        assert rc == -1 and text in l.sph3d_last_error(), (kw, l.sph3d_last_error())
    with pytest.raises(ValueError):
        _lib.check(-1)
    import torch
    with pytest.raises(_lib.Sph3dError):
        feed.assemble(torch.zeros(4, 8), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 4, 0, 0)
