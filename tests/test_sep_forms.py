"""The one-kernel separable layer's launch choice, held on the host: the library's query sph3d_separable_conv3d_plan
(csrc/sepconv.hpp: sep_plan, which both entry points launch from) against tests/_sep_forms.py, the restatement of the launchers
as they stood before the choice was gathered into that one function — field for field, for inference and training, on every case
of tests/test_gpu_sep_forms.py and on a grid that crosses every boundary of the predicates and both thresholds of the general
kernel's tile-height ladder — and the older shape queries against the plan.  No device is touched."""
import ctypes

import pytest

import _sep_forms as S

N, K = 1000, 16
# (B, M): the empty launches, the partition's small geometries, and B M on both sides of 8192 and of 32768
GRID_BM = [(0, 107), (3, 0), (1, 40), (3, 107), (8, 1024), (1, 8191), (1, 8192), (3, 2731), (1, 32767), (1, 32768), (16, 2048)]
GRID_SHAPES = [s for s in S.SUPPORT_SWEEP if s[1] != 0]             # C = 0: test_query_validates


@pytest.fixture(scope="module")
def lib():
    from sph3d_gcn_amd import _lib
    return ctypes.CDLL(_lib.LIB_PATH)


@pytest.fixture(scope="module")
def query(lib):
    fn = lib.sph3d_separable_conv3d_plan
    fn.restype = ctypes.c_int
    out = (ctypes.c_int * len(S.FIELDS))()

    def q(*case):
        assert fn(*case, out) == 0, case
        return dict(zip(S.FIELDS, out))
    return q


def _inst(p):
    return (p["kernel"], p["R"], p["LPE"], p["RBK"] if p["kernel"] == S.GENERAL else p["KT"])


def test_plan_equals_the_old_launchers(query):
    seen = {0: set(), 1: set()}
    n = 0
    cases = [(B, N, M, F, C, r, K, Cout) for F, C, r, Cout in GRID_SHAPES for B, M in GRID_BM]
    cases += [(c.B, c.N, c.M, c.F, c.C, c.r, c.K, c.Cout) for c in S.ALL_CASES]
    for case in cases:
        for train in (0, 1):
            want = S.plan(train, *case)
            assert query(train, *case) == want, (train, case)
            seen[train].add(_inst(want))
            n += 1
    assert n == 2 * (len(GRID_SHAPES) * len(GRID_BM) + len(S.ALL_CASES)) and len(GRID_SHAPES) == 13 * 19 * 13
    # every instantiation the library contains is named by some plan, and no other is
    ring, small = {(S.RING,) + t for t in S.TRIPLES}, {(S.SMALL,) + t for t in S.TRIPLES}
    general = {(S.GENERAL,) + t for t in S.GENERAL_INSTS}
    assert seen[1] == ring | {(0, 0, 0, 0)}
    assert seen[0] == ring | small | general | {(0, 0, 0, 0)}
    assert len(ring) == len(small) == 5 and len(general) == 12


def test_plan_fields_hang_together(query):
    for F, C, r, Cout in GRID_SHAPES:
        for B, M in GRID_BM:
            for train in (0, 1):
                p = query(train, B, N, M, F, C, r, K, Cout)
                if p["kernel"] == S.UNSUPPORTED:
                    assert set(p.values()) == {0}
                    continue
                assert 0 < p["lds"] <= S.LDS and p["grid"] == (256 if train or (B and M) else 0)
                assert p["stats_blocks"] == (256 * p["G"] if train else 0)
                if p["kernel"] == S.RING:
                    assert 3 <= p["NB"] <= 8 and p["G"] * (Cout >> 4) == 16 and p["RBK"] == p["rbk_by_points"] == 0
                else:
                    assert not train and p["NB"] == p["G"] == 0
                    assert (p["KT"] == 0 and 1 <= p["RBK"] <= p["rbk_by_points"]) if p["kernel"] == S.GENERAL else p["RBK"] == 0


def test_shape_queries_read_the_plan(lib, query):
    for F, C, r, Cout in GRID_SHAPES:
        fused, train = lib.sph3d_separable_conv3d_fused_supported(N, F, C, r, K, Cout), lib.sph3d_separable_conv3d_train_supported(N, F, C, r, K, Cout)
        assert fused == int(S.fused_supported(N, F, C, r, K, Cout)) and train == int(S.sr_shape_ok(N, F, C, r, K, Cout))
        blocks = lib.sph3d_separable_conv3d_train_blocks(Cout)
        assert blocks == S.train_blocks(Cout)
        for B, M in GRID_BM:
            pi, pt = query(0, B, N, M, F, C, r, K, Cout), query(1, B, N, M, F, C, r, K, Cout)
            assert fused == int(pi["kernel"] != S.UNSUPPORTED) and train == int(pt["kernel"] != S.UNSUPPORTED)
            assert pt["stats_blocks"] == (blocks if train else 0)
    for Cout in range(0, 600, 8):
        assert lib.sph3d_separable_conv3d_train_blocks(Cout) == S.train_blocks(Cout)


def test_query_validates(lib):
    out = (ctypes.c_int * len(S.FIELDS))()
    p = ctypes.cast(out, ctypes.c_void_p)
    good = (0, 3, 150, 107, 33, 12, 2, 12, 64)
    assert lib.sph3d_separable_conv3d_plan(*good, p) == 0 and out[0] == S.RING
    assert lib.sph3d_separable_conv3d_plan(*good, None) == -1
    for i, bad in ((0, 2), (0, -1), (2, 0), (2, -5), (4, 0), (5, 0), (5, -4), (7, 0), (8, 0), (8, -16)):
        args = list(good)
        args[i] = bad
        assert lib.sph3d_separable_conv3d_plan(*args, p) == -1, args
    for F, C, r, Cout in S.SUPPORT_SWEEP:
        if C == 0:
            assert lib.sph3d_separable_conv3d_plan(0, 3, N, 107, F, C, r, K, Cout, p) == -1
    # r is no dimension: outside {1, 2} the shape is unsupported, not invalid
    assert lib.sph3d_separable_conv3d_plan(0, 3, 150, 107, 33, 12, 3, 12, 64, p) == 0 and tuple(out) == (0,) * len(S.FIELDS)
