"""Farthest-point sampling's launch choice, held on the host: the library's query sph3d_farthest_point_sample_plan
(csrc/fps_plan.hpp: fps_plan, which the entry launches from and the workspace query sizes from) against tests/_fps_forms.py, the
restatement of the launcher as it stood before the choice was gathered into that one function — field for field on a grid that
crosses every boundary of the rules, at the ends of the int range, and on every sampling case of the GPU suites, each of which
must have the plan its id names.  And what makes equality with the oracle on the GPU mean something: on every planted cloud of
the GPU list the float32 numpy statement of the sampling under the reference's tie rule equals the oracle, and under either
wrong rule it does not.  No device is touched."""
import ctypes
import itertools

import numpy as np
import pytest

import _fps_forms as S
import oracle

GRID_N = [1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 12288, 12289, 16384, 16385, 24576, 24577, 28672, 28673,
          65536, 131072, 262144]
GRID_B = [0, 1, 2, 3, 8, 9, 16, 17, 18, 19, 32, 33, 64, 65, 128, 129, S.INT_MAX]
GRID_M = [1, 2, 16384, 16385]

# every instantiation csrc/sample.hip contains: (kernel, P)
INSTANTIATIONS = ({(S.PLAIN, P) for P in (1, 2, 4, 8, 12, 16, 24)} | {(S.PRUNED, P) for P in (4, 8, 16)} | {(S.COOP, 0), (S.BIG, 0)})


@pytest.fixture(scope="module")
def lib():
    from sph3d_gcn_amd import _lib
    l = ctypes.CDLL(_lib.LIB_PATH)
    l.sph3d_farthest_point_sample_workspace.restype = ctypes.c_size_t
    l.sph3d_farthest_point_sample_workspace.argtypes = [ctypes.c_int] * 3
    l.sph3d_farthest_point_sample_plan.restype = ctypes.c_int
    l.sph3d_farthest_point_sample_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    l.sph3d_last_error.restype = ctypes.c_char_p
    return l


@pytest.fixture(scope="module")
def query(lib):
    out = (ctypes.c_longlong * (len(S.FIELDS) + 1))()
    ref = ctypes.addressof(out)

    def q(b, n, m):
        """-> the fields as a tuple, None for SPH3D_EINVAL"""
        out[len(S.FIELDS)] = -12345                      # (the query writes its fields and nothing behind them)
        rc = lib.sph3d_farthest_point_sample_plan(b, n, m, ref)
        assert rc in (0, -1) and out[len(S.FIELDS)] == -12345, (b, n, m)
        return tuple(out)[:len(S.FIELDS)] if rc == 0 else None
    return q


def _check(query, b, n, m):
    want = S.plan(b, n, m)
    want = None if isinstance(want, str) else tuple(want[f] for f in S.FIELDS)
    got = query(b, n, m)
    assert got == want, ((b, n, m), got and dict(zip(S.FIELDS, got)), want and dict(zip(S.FIELDS, want)))
    if got is None:
        return None
    p = dict(zip(S.FIELDS, got))
    # what every launch needs: workgroup counts an int, whole waves up to 1024 threads, offsets inside the workspace
    if p["kernel"] != S.NONE:
        assert 1 <= p["grid"] <= S.INT_MAX and p["block"] % 64 == 0 and 64 <= p["block"] <= 1024 and p["block"] >= min(n, 1024)
        assert (p["big_grid"] > 0) == (p["kernel"] in (S.COOP, S.BIG)) and p["big_grid"] <= 64
        assert (p["workspace_bytes"] > 0) == (p["kernel"] in (S.COOP, S.BIG))
    if p["kernel"] in (S.PLAIN, S.PRUNED):
        assert 1024 * p["P"] >= n and p["grid"] == b and p["G"] == 1
    if p["kernel"] == S.COOP:
        assert p["G"] * 4096 >= n > (p["G"] - 1) * 4096 and b * p["G"] <= 128 and p["G"] <= 64 and p["grid"] >= b * p["G"]
        assert p["off_err"] == 0 and p["off_slots"] == 256 and p["off_temp"] % 256 == 0
        assert p["off_slots"] + 8 * b * 2 * p["G"] <= p["off_temp"]
    if p["kernel"] in (S.COOP, S.BIG):
        assert p["off_temp"] + 4 * p["big_grid"] * n == p["workspace_bytes"] and p["big_grid"] == min(b, 64)
    return p


def test_plan_equals_the_old_launcher(lib, query):
    seen, kernels, count = set(), {}, 0
    for b, n, m in itertools.product(GRID_B, GRID_N, GRID_M):
        p = _check(query, b, n, m)
        assert p is not None
        # the workspace query is the plan's size, and the old function's
        assert lib.sph3d_farthest_point_sample_workspace(b, n, m) == p["workspace_bytes"] == S.workspace(b, n, m), (b, n, m)
        if p["kernel"] != S.NONE:
            seen.add((p["kernel"], p["P"]))
        kernels[p["kernel"]] = kernels.get(p["kernel"], 0) + 1
        count += 1
    assert count == 17 * 24 * 4
    assert seen == INSTANTIATIONS and len(INSTANTIATIONS) == 12          # every instantiation the file contains, and no other
    assert all(kernels[k] >= 24 for k in (S.NONE, S.PLAIN, S.PRUNED, S.COOP, S.BIG))


def test_the_choice_at_its_boundaries(query):
    """the rules in words, one assertion each (the grid above holds them to the old code; this says what they are)"""
    k = lambda b, n, m: (lambda p: (p[0], p[1]))(query(b, n, m))
    assert k(1, 2048, 2) == (S.PLAIN, 2) and k(1, 2049, 2) == (S.PRUNED, 4)             # kFpsPruneMin
    assert k(1, 16384, 2) == (S.PRUNED, 16) and k(1, 16385, 2) == (S.PLAIN, 24)
    # m == 1 inside the pruned range: the plain kernel, and the only way to its 4, 8, 12 and 16 point forms
    assert [k(2, n, 1) for n in (3000, 6000, 10000, 16384)] == [(S.PLAIN, 4), (S.PLAIN, 8), (S.PLAIN, 12), (S.PLAIN, 16)]
    assert k(1, 24576, 2) == (S.PLAIN, 24) and k(1, 24577, 2) == (S.COOP, 0)
    assert [query(1, n, 5)[2] for n in (1, 63, 64, 65, 1023, 1024)] == [64, 64, 64, 128, 1024, 1024]      # block
    f = lambda b, n: dict(zip(S.FIELDS, query(b, n, 2)))
    # co-operative while b G <= 128; XCD-local while ceil(b / 8) G <= 16
    assert f(18, 24577)["kernel"] == S.COOP and f(19, 24577)["kernel"] == S.BIG                             # G = 7: 126, 133
    assert f(2, 262144)["kernel"] == S.COOP and f(2, 262144)["G"] == 64 and f(3, 262144)["kernel"] == S.BIG
    assert (f(16, 32768)["xcd_local"], f(16, 32768)["grid"]) == (1, 128) and (f(16, 32769)["kernel"], f(14, 32769)["xcd_local"]) == (S.BIG, 0)
    assert (f(9, 24577)["xcd_local"], f(9, 24577)["grid"]) == (1, 112) and (f(9, 40000)["xcd_local"], f(9, 40000)["grid"]) == (0, 90)
    assert f(65, 24577)["grid"] == f(65, 24577)["big_grid"] == 64 and f(65, 24577)["workspace_bytes"] == 4 * 64 * 24577


def test_query_validates_in_the_entrys_order(lib, query):
    fn, err, ws = lib.sph3d_farthest_point_sample_plan, lib.sph3d_last_error, lib.sph3d_farthest_point_sample_workspace
    out = (ctypes.c_longlong * len(S.FIELDS))()
    p = ctypes.addressof(out)
    entry = lib.sph3d_farthest_point_sample
    entry.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]

    def both(b, n, m, message, want):
        """the query (even without `out`) and the entry itself (null pointers: nothing may be read or launched) answer alike"""
        assert S.plan(b, n, m) == want
        for call in (lambda: fn(b, n, m, p), lambda: fn(b, n, m, None), lambda: entry(b, n, m, None, None, None, 0, None)):
            assert call() == -1 and message in err(), (b, n, m, err())
        assert ws(b, n, m) == 0
    # npoint, then the shape (n, b), then the size: each with everything behind it wrong as well
    for m in (0, -1, -S.INT_MAX - 1):
        both(-1, 0, m, b"positive npoint", S.BAD_SAMPLES)
        both(1, 1 << 20, m, b"positive npoint", S.BAD_SAMPLES)
    for b, n in ((-1, 0), (1, 0), (1, -5), (-1, 1 << 20), (-S.INT_MAX - 1, 100), (3, -S.INT_MAX - 1)):
        both(b, n, 4, b"(batch_size,num_points,3) inp shape", S.BAD_SHAPE)
    for n in (262145, 1 << 20, S.INT_MAX):
        both(0, n, 4, b"exceeds the supported 262144 points", S.BAD_POINTS)
        both(S.INT_MAX, n, 4, b"exceeds the supported 262144 points", S.BAD_POINTS)
    # a valid call without `out`: the last thing looked at
    assert fn(2, 100, 4, None) == -1 and b"out is NULL" in err()
    assert fn(2, 100, 4, p) == 0 and tuple(out)[:4] == (S.PLAIN, 1, 128, 2)
    # an empty batch is valid and launches nothing (the entry returns before it looks at a pointer)
    assert query(0, 100, 4) == (0,) * len(S.FIELDS) and entry(0, 100, 4, None, None, None, 0, None) == 0
    assert query(0, 30000, 4) == tuple(256 if f == "workspace_bytes" else 0 for f in S.FIELDS)


def test_every_product_is_formed_in_64_bits(lib, query):
    ws = lib.sph3d_farthest_point_sample_workspace
    ends = (1, S.INT_MAX - 1, S.INT_MAX)
    for b, m in itertools.product(ends, ends):
        for n in (1, 24576, 24577, 131072, 262143, 262144):
            p = _check(query, b, n, m)
            assert ws(b, n, m) == p["workspace_bytes"] == S.workspace(b, n, m)
    # b G = 2^31 - 1 times 64 and the size 4 * 64 * 262144: neither is an `int` product, both are exact
    p = dict(zip(S.FIELDS, query(S.INT_MAX, 262144, S.INT_MAX)))
    assert (p["kernel"], p["grid"], p["workspace_bytes"], p["off_temp"]) == (S.BIG, 64, 1 << 26, 0)
    p = dict(zip(S.FIELDS, query(S.INT_MAX, 24576, 1)))
    assert (p["kernel"], p["P"], p["grid"], p["workspace_bytes"]) == (S.PLAIN, 24, S.INT_MAX, 0)
    # the ends of the int range in every argument: an answer, never a wrapped sum (n + 4095 at n = 2^31 - 1 is past an int)
    for b, n, m in itertools.product((-S.INT_MAX - 1, -1, 0, 1, S.INT_MAX), repeat=3):
        _check(query, b, n, m)
        if isinstance(S.plan(b, n, m), str):
            assert ws(b, n, m) == 0


# ---- the references -----------------------------------------------------------------------------------------------------------
PLANTED = [c for c in S.CASES if c[5] == "planted"]


def test_the_gpu_list_is_the_issues():
    assert len(S.CASES) == 27 and len({c[0] for c in S.CASES}) == 27 and len(PLANTED) == 12
    assert {c[0] for c in S.CASES if c[1]["kernel"] == S.COOP and c[7] != 2} == {"coop-local-eight-rotations"}
    # no size below the thresholds the kernels fix, and the tag-wrap chain passes round 16384 with m > n
    wrap = next(c for c in S.CASES if c[0] == "coop-tag-wrap-m-past-n")
    assert wrap[4] > 16400 and wrap[4] > wrap[3] >= 24577
    assert all(c[3] >= 24577 for c in S.CASES if c[1]["kernel"] in (S.COOP, S.BIG))


@pytest.mark.parametrize("case", PLANTED, ids=lambda c: c[0])
def test_numpy_statement_equals_the_oracle_and_the_wrong_rules_do_not(case):
    """With one point per thread (n <= 1024) the three rules are one function, and at n = 1025 thread 0 alone owns two points, one
    of them the first sample: "lowest_k" can differ from 1025 points on, "same_thread_higher_k" from 1026 on.  Below, the wrong
    rules must EQUAL the reference's (that is the proof that nothing is there to tell apart); from there on they must differ, on
    every cloud of the case."""
    _, _, b, n, m, _, span, _ = case
    pts = S.clouds(case)
    assert pts.shape == (b, n, 3) and pts.dtype == np.float32
    want = oracle.farthest_point_sample(m, pts)
    sites = S.planted_sites(n, span)
    for i in range(b):
        assert i == 0 or not np.array_equal(pts[i], pts[0])                      # clouds differ per cloud index
        ref = S.fps_numpy(pts[i], m, "ref")
        np.testing.assert_array_equal(ref, want[i])
        # every site is picked in rounds 1 .. len(sites), by one of its holders
        assert sorted(next(s for s in sites if k in s) for k in ref[1:1 + len(sites)]) == sorted(sites)
        for rule, first_n in (("lowest_k", 1025), ("same_thread_higher_k", 1026)):
            assert np.array_equal(S.fps_numpy(pts[i], m, rule), ref) == (n < first_n), (rule, i)


def test_numpy_statement_on_the_non_finite_clouds():
    """the picks there: 0, then the lowest thread among the three points that stay at 1e38, for ever"""
    for case in (c for c in S.CASES if c[5] == "nonfinite"):
        _, _, b, n, m, _, _, _ = case
        pts = S.clouds(case)
        with np.errstate(invalid="ignore", over="ignore"):
            want = oracle.farthest_point_sample(m, pts)
        assert np.isnan(pts).sum() == b and np.isposinf(pts).sum() == b and np.isneginf(pts).sum() == b
        for i in range(b):
            np.testing.assert_array_equal(S.fps_numpy(pts[i], m, "ref"), want[i])
            assert want[i].tolist() == [0] + [S.NONFINITE_AT[2]] * (m - 1)
            assert S.fps_numpy(pts[i], m, "lowest_k").tolist() == [0] + [S.NONFINITE_AT[0]] * (m - 1)


# ---- the GPU lists --------------------------------------------------------------------------------------------------------------
def _claims(query, b, n, m, claim):
    p = _check(query, b, n, m)
    assert {f: p[f] for f in claim} == claim, ((b, n, m), p)


def test_every_gpu_case_has_the_plan_it_names(query):
    import test_gpu_fps_prune
    import test_gpu_parity
    for name, claim, b, n, m, _, _, _ in S.CASES:
        _claims(query, b, n, m, claim)
    assert {(c[1]["kernel"], c[1]["P"]) for c in S.CASES} == INSTANTIATIONS       # the new list alone reaches all twelve
    assert len(test_gpu_fps_prune.CASES) == len(test_gpu_fps_prune.KERNELS) == 15
    for (_, b, n, m), (kernel, P) in zip(test_gpu_fps_prune.CASES, test_gpu_fps_prune.KERNELS):
        _claims(query, b, n, m, dict(kernel={"plain": S.PLAIN, "pruned": S.PRUNED}[kernel], P=P))
    parity = {3: (S.PLAIN, 1, 64), 100: (S.PLAIN, 1, 128), 1024: (S.PLAIN, 1, 1024), 2048: (S.PLAIN, 2, 1024), 1100: (S.PLAIN, 2, 1024),
              10000: (S.PRUNED, 16, 1024), 8192: (S.PRUNED, 8, 1024), 30000: (S.COOP, 0, 1024)}
    assert len(test_gpu_parity.FPS_CASES) == len(parity)
    for _, b, n, m in test_gpu_parity.FPS_CASES:
        _claims(query, b, n, m, dict(zip(("kernel", "P", "block"), parity[n])))
    # test_gpu_round3.test_fps_large_clouds_cooperative_kernel_bitexact: all four co-operative and XCD-local, ceil(b / 8) G <= 16
    for (b, n, m), G in zip([(1, 65536, 16384), (2, 30000, 2500), (1, 24577, 300), (3, 40000, 1000)], (16, 8, 7, 10)):
        _claims(query, b, n, m, _coop_claim(G))


def _coop_claim(G):
    return dict(kernel=S.COOP, G=G, xcd_local=1, grid=8 * G, repair=1)


def test_round3_parameters_are_the_ones_pinned_above():
    """(the four (B, n, m) are that test's parametrisation, read from its mark)"""
    import test_gpu_round3
    marks = [mk for mk in test_gpu_round3.test_fps_large_clouds_cooperative_kernel_bitexact.pytestmark if mk.name == "parametrize"]
    assert marks[0].args[1] == [(1, 65536, 16384), (2, 30000, 2500), (1, 24577, 300), (3, 40000, 1000)]
