"""harness/augment.py: the numpy statement of the augmentation stage (no GPU)."""
import numpy as np
import pytest

import _augment_cases as cases
import _augment_ref as aref
from sph3d_gcn_amd.harness import augment, feed


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_all_gates_off_is_the_identity():
    (p, label, inner), opts, _ = cases.CASES["a"]
    for o in (opts._replace(enable=0), opts._replace(prob=(0.0,) * 9)):
        q, l, i, rep = augment.apply_reference(p, label, inner, 3, 4, o)
        assert np.array_equal(_bits(q), _bits(p)) and np.array_equal(l, label) and np.array_equal(i, inner)
        assert not rep.gates.any() and rep.elastic_skipped == (0, 0) and rep.mixed_pairs == 0
    q, l, i, _ = augment.apply_reference(p, label, None, 3, 4, opts._replace(enable=0))
    assert i is None


def test_gates_are_a_pure_function_with_the_stated_frequencies():
    opts = augment.default_options("s3dis")
    B = 4096
    g = augment.gate_masks(11, 5, B, opts)
    assert np.array_equal(g, augment.gate_masks(11, 5, B, opts))
    assert not np.array_equal(g, augment.gate_masks(11, 6, B, opts)) and not np.array_equal(g, augment.gate_masks(12, 5, B, opts))
    # cloud b's gates do not depend on the batch around it (MIX: on the pair)
    assert np.array_equal(g[:100], augment.gate_masks(11, 5, 100, opts))
    for k, prob in enumerate(opts.prob):
        on = (g >> k & 1).astype(np.float64)
        n = B // 2 if k == 0 else B                         # MIX: one draw per pair
        freq = on[::2].mean() if k == 0 else on.mean()
        assert abs(freq - prob) <= 4 * np.sqrt(prob * (1 - prob) / n), (k, freq, prob)
    assert np.array_equal(g[0::2] & 1, g[1::2] & 1)
    assert augment.gate_masks(11, 5, 5, opts._replace(prob=(1.0,) * 9))[4] & augment.MIX == 0       # the unpaired last cloud
    assert augment.thresholds(opts._replace(prob=(0.0, 1.0, 0.5) + (0.0,) * 6))[:3] == [0, 1 << 32, 1 << 31]
    assert not (augment.gate_masks(1, 1, 64, opts._replace(enable=augment.FLIPX)) & ~augment.FLIPX).any()      # only enabled bits


@pytest.mark.parametrize("N", [8, 7, 2, 1])
def test_mix_exchanges_exactly_the_upper_slots(N):
    B, h = 5, N // 2
    rng = np.random.RandomState(N)
    p = rng.rand(B, N, 6).astype(np.float32)
    label = np.arange(B * N, dtype=np.int32).reshape(B, N)
    inner = -label
    opts = augment.default_options("s3dis", enable=augment.MIX)._replace(prob=(1.0,) * 9)
    q, l, i, rep = augment.apply_reference(p, label, inner, 1, 2, opts)
    assert rep.mixed_pairs == 2 and (rep.gates[:4] == augment.MIX).all() and rep.gates[4] == 0
    for a, b in ((0, 1), (2, 3)):
        assert np.array_equal(l[a, :h], label[a, :h]) and np.array_equal(l[a, h:], label[b, h:])
        assert np.array_equal(l[b, :h], label[b, :h]) and np.array_equal(l[b, h:], label[a, h:])
        assert np.array_equal(i, -l)
        assert np.array_equal(_bits(q[a, h:, 3:]), _bits(p[b, h:, 3:])) and np.array_equal(_bits(q[a, :h, 3:]), _bits(p[a, :h, 3:]))
        for src, dst, sl in ((a, a, slice(0, h)), (b, a, slice(h, N)), (b, b, slice(0, h)), (a, b, slice(h, N))):
            assert np.array_equal(q[dst, sl, 0:3], p[src, sl, 0:3].astype(np.float64) - augment.centre(p[src, :, 0:3].astype(np.float64)))
    assert np.array_equal(_bits(q[4]), _bits(p[4])) and np.array_equal(l[4], label[4])      # unpaired: untouched, not shifted


def test_blur_weights_sum_to_one_and_the_field_is_keyed_by_the_node():
    assert sum(augment.BLUR) ** 3 == 729 and augment.FIELD_UNIT == 729 << 20
    ones = np.ones((7, 8, 9, 3), dtype=np.int64)
    assert (augment.blur(augment.blur(augment.blur(ones, 0), 1), 2) == 729).all()
    ck = feed.cloud_key(5, 6, 7)
    raw = augment.raw_field(ck, 0, (-3, -2, 0), (6, 6, 6))
    assert raw.min() >= -(1 << 20) and raw.max() < 1 << 20
    # the same nodes from another box, and another pass / key give other noise
    assert np.array_equal(augment.raw_field(ck, 0, (-1, -1, 1), (2, 2, 2)), raw[2:4, 1:3, 1:3])
    assert not np.array_equal(augment.raw_field(ck, 1, (-3, -2, 0), (6, 6, 6)), raw)
    big, part = augment.lattice(ck, 0, (-4, -4, -4), (5, 5, 5)), augment.lattice(ck, 0, (-1, 0, 1), (2, 2, 2))
    assert np.array_equal(part, big[3:8, 4:8, 5:8])
    assert np.abs(big).max() < augment.FIELD_UNIT


def test_the_noise_at_a_point_does_not_depend_on_the_other_points():
    ck = feed.cloud_key(1, 2, 3)
    rng = np.random.RandomState(0)
    a = rng.rand(50, 3) * 2 - 1
    wide = np.concatenate([a, rng.rand(30, 3) * 6 - 3])
    for which, (g, mag) in enumerate(((0.2, 0.7), (0.8, 2.8))):
        da = augment.displacement(a, ck, which, g, mag, 1 << 20)
        dw = augment.displacement(wide, ck, which, g, mag, 1 << 20)
        assert np.array_equal(da, dw[:50])
        assert not np.array_equal(da, augment.displacement(a, feed.cloud_key(1, 2, 4), which, g, mag, 1 << 20))


def test_displacement_is_continuous_across_a_cell_face():
    ck = feed.cloud_key(9, 9, 0)
    g, mag = 0.25, 2.8
    base = np.array([[0.1, 0.3, 0.6], [-0.4, 0.2, 0.1], [0.3, -0.6, -0.2]])
    for axis in range(3):
        for plane in (-0.5, 0.0, 0.75):
            lo, hi = base.copy(), base.copy()
            lo[:, axis], hi[:, axis] = plane - 5e-7, plane + 5e-7
            d = augment.displacement(np.concatenate([lo, hi]), ck, 1, g, mag, 1 << 20)
            # the field's slope is at most (2 / 3) mag / g per axis: 1e-6 apart -> 7.5e-6 at the most
            assert np.abs(d[:3] - d[3:]).max() <= (2.0 / 3.0) * mag / g * 1e-6 * 1.001
            assert np.abs(d).max() > 1e-3
            assert (augment.cell_index(lo, g)[:, axis] + 1 == augment.cell_index(hi, g)[:, axis]).all()


def test_rms_displacement():
    """over 47^3 = 103823 points on nodes four cells apart (their 5-tap stencils share one raw node per axis: correlation 1 / 19):
    the rms per axis is mag * sqrt((19 / 81)^3 / 3) — uniform raw noise of variance 1 / 3 under three blurs of squared weight
    sum 19 / 81"""
    g, mag = 0.25, 2.8
    k = (np.arange(47) - 23) * 4
    xyz = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * g
    assert xyz.shape[0] >= 100000
    d = augment.displacement(xyz, feed.cloud_key(4, 2, 0), 1, g, mag, 1 << 24)
    want = mag * np.sqrt((19.0 / 81.0) ** 3 / 3.0)
    rms = np.sqrt((d * d).mean(axis=0))
    print("rms per axis %s, expected %.5f" % (rms, want))
    assert (np.abs(rms / want - 1) <= 0.03).all()
    assert abs(np.sqrt((d * d).mean()) / want - 1) <= 0.03
    # the default passes: about 4.6 cm and 18 cm
    assert abs(0.7 * np.sqrt((19.0 / 81.0) ** 3 / 3.0) - 0.046) < 0.001 and abs(want - 0.184) < 0.001


def test_elastic_skips_are_counted_and_leave_the_cloud_alone():
    (p, label, inner), opts, _ = cases.CASES["a_skip"]
    q, _, _, rep = augment.apply_reference(p, label, inner, 5, 1, opts._replace(enable=augment.ELASTIC))
    assert rep.elastic_skipped == (2, 2)
    assert np.array_equal(_bits(q[3:]), _bits(p[3:])) and not np.array_equal(_bits(q[:3]), _bits(p[:3]))
    tiny = augment.apply_reference(p, label, inner, 5, 1, opts._replace(enable=augment.ELASTIC, max_nodes=216))[3]
    assert tiny.elastic_skipped == (4, 4)                       # only the one-point cloud has a one-cell box


def test_the_gpu_cases_decide_every_skip_with_a_whole_node_to_spare():
    """what tests/test_gpu_augment.py relies on: a cell index that fp32 places one node off cannot change an elastic decision in
    any of its cases; the skip case skips exactly its last two clouds in both passes; and the cases reach both homes of the
    lattice (LDS and the workspace), negative cells, and every gate on and off"""
    homes, seen_on, seen_off, negative = set(), 0, 0, False
    for name, (batch, opts, keys) in cases.CASES.items():
        for seed, step in keys:
            rep = augment.apply_reference(*batch, seed, step, opts)[3]
            for b, which, ran, still in cases.margins(rep, opts.max_nodes):
                assert still, (name, seed, step, b, which, ran)
            for b, which, cmin, cmax in rep.boxes:
                if augment.box_ok(cmin, cmax, opts.max_nodes):
                    homes.add(int(np.prod(cmax - cmin + 6)) <= cases.LDS_NODES)
                    negative = negative or bool((cmin < 0).any())
            seen_on |= int(np.bitwise_or.reduce(rep.gates))
            seen_off |= int(np.bitwise_or.reduce(~rep.gates & opts.enable))
            if name == "a_skip":
                assert rep.elastic_skipped == (2, 2) and (rep.gates & augment.ELASTIC).all()
                assert [(b, w) for b, w, ran, _ in cases.margins(rep, opts.max_nodes) if not ran] == [(3, 0), (3, 1), (4, 0), (4, 1)]
            if name in ("c", "d"):
                assert rep.mixed_pairs == 1
    assert homes == {True, False} and negative
    assert seen_on == (1 << augment.NUM_GATES) - 1 and seen_off == (1 << augment.NUM_GATES) - 1


def test_flips_negate_exactly():
    (p, label, inner), opts, _ = cases.CASES["e"]
    o = opts._replace(enable=augment.FLIPX | augment.FLIPY, prob=(1.0,) * 9)
    q = augment.apply_reference(p, label, inner, 1, 1, o)[0]
    want = p.copy()
    want[..., [0, 1, 3, 4]] = -want[..., [0, 1, 3, 4]]
    assert np.array_equal(_bits(q), _bits(want))
    gates = augment.apply_reference(p, label, inner, 1, 1, opts._replace(enable=augment.FLIPX | augment.FLIPY))[3].gates
    assert set(gates.tolist()) <= {0, augment.FLIPX, augment.FLIPY, augment.FLIPX | augment.FLIPY}


def test_colours_stay_in_range_and_scaling_keeps_normals_unit():
    for name in ("a", "e"):
        (p, label, inner), opts, keys = cases.CASES[name]
        ro = opts.rgb_offset
        for rng_ in ((-1.0, 1.0), (0.0, 1.0)):
            src = p.copy()
            if rng_[0] == 0.0:
                src[..., ro:ro + 3] = (src[..., ro:ro + 3] + 1) / 2
            for seed, step in keys:
                q, _, _, rep = augment.apply_reference(src, label, inner, seed, step, opts._replace(rgb_range=rng_))
                assert q[..., ro:ro + 3].min() >= rng_[0] and q[..., ro:ro + 3].max() <= rng_[1]
                for b in np.nonzero(rep.gates & augment.CDROP)[0]:
                    assert (q[b, :, ro:ro + 3] == (rng_[0] + rng_[1]) / 2).all()
                if opts.normal_offset is not None:
                    assert np.abs(np.sqrt((q[..., 3:6] ** 2).sum(axis=2)) - 1).max() < 1e-6
    drop = augment.apply_reference(*cases.CASES["a"][0], 1, 1, cases.CASES["a"][1]._replace(enable=augment.CDROP, prob=(1.0,) * 9))[0]
    assert (drop[..., 3:6] == 0.0).all()


def test_a_colour_bit_without_colour_is_refused():
    p, label, inner = cases.small(2, 16, 3, 0)
    bad = augment.default_options("object")._replace(enable=augment.FLIPX | augment.CJITTER)
    with pytest.raises(ValueError, match="colour"):
        augment.apply_reference(p, label, inner, 1, 1, bad)
    with pytest.raises(ValueError):
        augment.apply_reference(p, label, inner, 1, 1, augment.default_options("s3dis"))          # rgb_offset 3 in 3 channels
    # and by the library, on the host, before any launch
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    prm = augment.params(augment.default_options("object"), 3)
    prm.enable = augment.CJITTER
    assert l.sph3d_augment_apply(2, 16, 3, 16, 16, None, 1, 1, prm, 16, 1 << 20, None, None) == -1
    assert b"colour" in l.sph3d_last_error()
    prm.enable = augment.FLIPX
    assert l.sph3d_augment_apply(2, 16, 4, 16, 16, None, 1, 1, prm, 16, 1 << 20, None, None) == -1 and b"C must be" in l.sph3d_last_error()
    prm.max_nodes = 100
    assert l.sph3d_augment_apply(2, 16, 3, 16, 16, None, 1, 1, prm, 16, 1 << 20, None, None) == -1 and b"max_nodes" in l.sph3d_last_error()
    prm.max_nodes = 4096
    assert l.sph3d_augment_apply(2, 16, 3, 16, 16, None, 1, 1, prm, 8, 1 << 20, None, None) == -1 and b"aligned" in l.sph3d_last_error()
    assert l.sph3d_augment_apply(2, 16, 3, 16, 16, None, 1, 1, prm, 16, 64, None, None) == -2          # SPH3D_EWORKSPACE
    assert l.sph3d_augment_workspace(2, 16, 4096) >= 2 * 9 * 4096 * 4


def test_the_bounded_evaluation_equals_the_statement():
    """tests/_augment_ref.py walks the kernel's operation order in float64; its values are the statement's, and an element no
    transform computes has a bound of zero"""
    for name, (batch, opts, keys) in cases.CASES.items():
        seed, step = keys[0]
        V, E, lab, inn, rep, want = aref.evaluate(*batch, seed, step, opts)
        assert np.allclose(V, want, rtol=1e-12, atol=1e-12), name
        assert (E >= 0).all() and np.isfinite(E).all(), name
        for b in np.nonzero(rep.gates == 0)[0]:
            assert not E[b].any()
    (p, label, inner), opts, _ = cases.CASES["a"]
    E = aref.evaluate(p, label, inner, 1, 1, opts._replace(enable=augment.FLIPX | augment.FLIPY, prob=(1.0,) * 9))[1]
    assert not E.any()
