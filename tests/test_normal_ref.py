"""tests/_normal_ref.py's bounds are held to a condition themselves: the statement passes its own check, and an answer moved by
four fp32 ulps in one component, a flipped sign or a variation moved by four ulps fails it.  No GPU."""
import numpy as np
import pytest

import _normal_ref as nr
from sph3d_gcn_amd.harness import normals as nrm


@pytest.fixture(scope="module")
def case():
    xyz = nr.family("sphere", 1024, 3)[None]
    idx, cnt = nr.plain_graph(xyz, xyz, 0.25, 32)
    toward = np.zeros((1, 3), np.float32)
    ref = nrm.graph_normals_reference(xyz, xyz, idx, cnt, 0.25, toward, 3)
    return xyz, toward, ref


def test_the_statement_passes_its_own_check(case):
    xyz, toward, ref = case
    stats = nr.check_rows(ref.normals, ref.variation, ref, xyz, toward[:, None, :], "statement")
    assert stats["component"] == 0.0 and stats["variation"] == 0.0 and stats["compared"] > 900


def _compared_row(ref, xyz, toward):
    g = nr.relative_gap(ref.evals)[0]
    ok = ~ref.zero[0] & (g >= nr.GAP) & nr.sign_has_margin(ref, xyz, toward[:, None, :])[0]
    return int(np.nonzero(ok)[0][0])


def test_four_ulps_in_one_component_fail(case):
    xyz, toward, ref = case
    g = nr.relative_gap(ref.evals)[0]
    ok = ~ref.zero[0] & (g >= nr.GAP) & nr.sign_has_margin(ref, xyz, toward[:, None, :])[0]
    # the leading component (magnitude in [3^-1/2, 1], ulp 2^-24): four ulps are 2^-22, which the length check sees as well
    m = _compared_row(ref, xyz, toward)
    lead = int(np.argmax(np.abs(ref.normals[0, m])))
    # a component with magnitude in [1/4, 1/2) (ulp 2^-25): four ulps are 2^-23 and move the length by less than 2^-24, so it
    # is the component bound alone that refuses them
    mag = np.abs(ref.normals[0])
    rows, cols = np.nonzero(ok[:, None] & (mag >= 0.25) & (mag < 0.5))
    for row, col, match in ((m, lead, None), (int(rows[0]), int(cols[0]), "component")):
        for steps in (4, -4):
            moved = ref.normals.copy()
            moved[0, row, col] = (moved[0, row, col].view(np.int32) + np.int32(steps)).view(np.float32)
            with pytest.raises(AssertionError, match=match):
                nr.check_rows(moved, ref.variation, ref, xyz, toward[:, None, :], "moved")


def test_a_flipped_sign_fails(case):
    xyz, toward, ref = case
    m = _compared_row(ref, xyz, toward)
    moved = ref.normals.copy()
    moved[0, m] = -moved[0, m]
    with pytest.raises(AssertionError, match="component"):
        nr.check_rows(moved, ref.variation, ref, xyz, toward[:, None, :], "flipped")


def test_four_ulps_of_variation_fail(case):
    xyz, toward, ref = case
    m = int(np.argmax(ref.variation[0]))
    moved = ref.variation.copy()
    moved[0, m] = (moved[0, m].view(np.int32) + np.int32(4)).view(np.float32)
    with pytest.raises(AssertionError, match="variation"):
        nr.check_rows(ref.normals, moved, ref, xyz, toward[:, None, :], "moved")


def test_a_zero_row_that_is_not_zero_and_a_short_row_fail(case):
    xyz, toward, ref = case
    dead = np.nonzero(ref.zero[0])[0]
    live = np.nonzero(~ref.zero[0])[0]
    if len(dead):
        moved = ref.normals.copy()
        moved[0, dead[0], 2] = 1.0
        with pytest.raises(AssertionError, match="zeroes"):
            nr.check_rows(moved, ref.variation, ref, xyz, toward[:, None, :], "dead")
    moved = ref.normals.copy()
    moved[0, live[0]] *= np.float32(1.0 - 2.0 ** -21)
    with pytest.raises(AssertionError, match="unit"):
        nr.check_rows(moved, ref.variation, ref, xyz, toward[:, None, :], "short")


def test_the_caps_are_asserted():
    """a cloud of exact planes through three points each: every live row has l0 = 0 and l1 > 0 but K = 3 neighbourhoods on a
    line have no gap at all — the check must refuse an input where more than CAP of the rows is left out"""
    t = np.arange(64, dtype=np.float32)
    xyz = np.stack([t, 2 * t, -t], axis=1)[None]                 # all points on one line: every covariance has rank 1
    idx, cnt = nr.plain_graph(xyz, xyz, 10.0, 8)
    ref = nrm.graph_normals_reference(xyz, xyz, idx, cnt, 10.0, None, 3)
    assert not ref.zero.any()
    with pytest.raises(AssertionError, match="gap condition"):
        nr.check_rows(ref.normals, ref.variation, ref, xyz, None, "line")
