"""Keyed dropout as harness/dropout.py states it (numpy, no GPU): a pure function of (seed, step, row, layer, element) built on
the feed's counter-based draws.  tests/test_gpu_dropout.py holds the kernel to this statement bit for bit."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import dropout as D
from sph3d_gcn_amd.harness import feed

SEED = 21


def _x(shape, seed=1):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


def test_the_mask_is_a_pure_function_of_its_arguments():
    shape = (5, 512)
    base = D.keep_reference(shape, 0.5, (SEED, 3), 0)
    np.testing.assert_array_equal(base, D.keep_reference(shape, 0.5, (SEED, 3), 0))
    for what, other in (("step", D.keep_reference(shape, 0.5, (SEED, 4), 0)), ("seed", D.keep_reference(shape, 0.5, (SEED + 1, 3), 0)),
                        ("layer", D.keep_reference(shape, 0.5, (SEED, 3), 1)), ("row0", D.keep_reference(shape, 0.5, (SEED, 3), 0, row0=1))):
        assert (other != base).mean() > 0.4, "another %s: about half of the elements change" % what       # 2560 fair coins: 0.5 +- 0.04 at 4 sigma
    assert (base[0] != base[1]).mean() > 0.35, "another row: another mask"
    # the statement is the draws of harness/feed.py, purpose 16 + layer, counter = the element's index inside its row
    ck = feed.cloud_key(SEED, 3, 2)
    np.testing.assert_array_equal(D.keep_reference(shape, 0.5, (SEED, 3), 1)[2],
                                  feed._hi(feed.draw(ck, 17, np.arange(512, dtype=np.uint64))) >= np.uint32(0x80000000))


def test_row0_shifts_the_rows():
    x = _x((5, 300))
    whole = D.dropout_reference(x, 0.5, (SEED, 7), 1)
    part = D.dropout_reference(x[2:], 0.5, (SEED, 7), 1, row0=2)
    np.testing.assert_array_equal(whole[2:].view(np.int32), part.view(np.int32))
    # trailing dimensions are one row: [B, 7, 5] is [B, 35]
    np.testing.assert_array_equal(D.keep_reference((3, 7, 5), 0.3, (SEED, 0), 0).reshape(3, 35), D.keep_reference((3, 35), 0.3, (SEED, 0), 0))


def test_rate_zero_keeps_everything_and_rate_one_nothing():
    x = _x((3, 512))
    np.testing.assert_array_equal(D.dropout_reference(x, 0.0, (SEED, 0), 0).view(np.int32), x.view(np.int32))
    assert D.keep_reference(x.shape, 0.0, (SEED, 0), 0).all()
    assert not D.keep_reference(x.shape, 1.0, (SEED, 0), 0).any()
    assert (D.dropout_reference(x, 1.0, (SEED, 0), 0).view(np.int32) == 0).all()


@pytest.mark.parametrize("layer,C", [(0, 512), (1, 256)])
def test_half_of_the_elements_survive_rate_one_half(layer, C):
    """the kept count of a [3, C] call is Binomial(3 C, 1/2): within 4 sigma of n / 2, sigma = sqrt(n) / 2, at every step"""
    n = 3 * C
    for step in range(6):
        kept = int(D.keep_reference((3, C), 0.5, (SEED, step), layer).sum())
        assert abs(kept - n / 2) <= 4 * np.sqrt(n) / 2, "step %d layer %d: %d of %d kept" % (step, layer, kept, n)


def test_kept_values_are_scaled_in_fp32_and_dropped_ones_are_plus_zero():
    x = _x((3, 512))
    x[0, :8] = [np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-45, 3e38, -3e38]
    keep = D.keep_reference(x.shape, 0.5, (SEED, 2), 0)
    y = D.dropout_reference(x, 0.5, (SEED, 2), 0)
    assert y.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        want = np.float32(x) * np.float32(2.0)
    np.testing.assert_array_equal(y[keep].view(np.int32), want[keep].view(np.int32))
    assert (y[~keep].view(np.int32) == 0).all()
    assert D.scale(0.5) == np.float32(2.0) and D.scale(0.3) == np.float32(1.0 / 0.7) and D.scale(0.3).dtype == np.float32


def test_thresholds():
    assert D.threshold(0.5) == 0x80000000
    assert D.threshold(0.25) == 0x40000000
    assert D.threshold(1e-10) == 1                         # ceil(0.43): any positive rate drops the all-zero word
    assert D.threshold(1.0) == 0xffffffff == D.threshold(1.0 - 1e-12)
    assert D.threshold(0.3) == int(np.ceil(0.3 * 2.0 ** 32)) == 1288490189


def test_arguments_outside_the_draws_range_are_refused():
    with pytest.raises(ValueError):
        D.keep_reference((2, 4), 0.5, (SEED, 0), 16)
    with pytest.raises(ValueError):
        D.keep_reference((2, 4), 0.5, (SEED, 0), -1)
    with pytest.raises(ValueError):
        D.keep_reference((2, 4), 0.5, (SEED, 0), 0, row0=2 ** 32 - 1)
