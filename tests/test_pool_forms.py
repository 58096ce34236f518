"""Pooling and un-pooling on the host: the library's query sph3d_pool3d_plan (csrc/pool_plan.hpp: pool_plan, which every entry of
csrc/pool3d.hip launches from) against tests/_pool_forms.py, the launchers restated in Python — field for field, for every op, on a
grid that crosses every boundary of the rules and includes the ends of the int range — every refusal on the query and on the
entries themselves (with null pointers: they answer before they touch one), and the kernels the GPU tests' cases reach against
the full set.  No device is touched."""
import itertools
import os
import re

import pytest

import _pool_forms as S

INT_MAX, INT_MIN = S.INT_MAX, -S.INT_MAX - 1
# V = 1 | 4, the narrow limit 16, the pairs limit 128, passes of 64 and of 256 channels
GRID_C = [1, 3, 4, 16, 17, 124, 128, 129, 132, 256, 260, 516, 0, -4, INT_MAX, INT_MIN]
# the XCD spread (1, 2, 3-4, 5 and more clouds), the scatter's grid.y (65535), the new grid guard (2^31 - 7)
GRID_B = [0, 1, 2, 3, 5, 64, 65535, 65536, INT_MAX - 7, INT_MAX - 6, INT_MAX, -1, INT_MIN]
# 16 and 4 points per workgroup; B * points on both sides of 65536 (2 x 32767 | 32768, 1 x 65535 | 65536 | 65537); narrow: 4 * 65536
# sources (262144 | 262145) and 16 * 65536 rows (1048576 | 1048577)
GRID_N = [1, 2, 15, 16, 17, 100, 32767, 32768, 65535, 65536, 65537, 262144, 262145, 1048576, 1048577, INT_MAX, 0, -1, INT_MIN]
GRID_M = [0] + GRID_N


@pytest.fixture(scope="module")
def seen():
    return set()


def _check(seen, op, B, Nin, Mout, C, K=1, F=1):
    args = (op, B, Nin, Mout, C, K, F)
    want = S.plan(*args)
    got = S.query(*args)
    assert got == (S.STATUS[want] if isinstance(want, str) else want), (args, got, want)
    if isinstance(want, str):
        return want
    p = got
    seen |= S.instantiations(p)
    # what every launch needs, and what the kernels assume
    if p["kernel"] == S.NONE:
        assert all(p[f] == 0 for f in S.FIELDS if f != "zero_bytes"), args
        assert B == 0 or Mout == 0 and op in (S.FWD, S.MAX_GRAD, S.NARROW), args
        return p
    assert 1 <= p["grid"] <= INT_MAX and 1 <= p["grid_y"] <= 65535 and p["block"] == 256 and p["lds"] <= 64 * 1024, (args, p)
    points = Mout if op in (S.FWD, S.NARROW) else Nin
    if p["kernel"] in (S.GATHER_FWD_HALF, S.GATHER_FWD, S.GATHER_BWD_T, S.MAXPOOL_BWD_T, S.MAXPOOL_BWD_ROWS):
        assert p["parts"] * p["ppwg"] >= points > (p["parts"] - 1) * p["ppwg"] and p["ppwg"] in (4, 16), (args, p)
        assert p["grid"] == S.xcd_grid(B, p["parts"]) >= B * p["parts"] and p["grid"] % 8 == 0, (args, p)
    if p["V"]:
        assert p["V"] == (4 if C % 4 == 0 else 1) and (p["pairs"] or p["passes"] * 64 * p["V"] >= C > (p["passes"] - 1) * 64 * p["V"]), (args, p)
    if p["pairs"]:
        assert p["V"] == 4 and C <= 128 and p["kernel"] in (S.GATHER_FWD_HALF, S.GATHER_BWD_T_SPLIT), (args, p)
    if p["kernel"] == S.GATHER_BWD_T_SPLIT:
        assert p["grid"] == B * Nin <= 65536 and p["lds"] == 4 * 64 * p["V"] * 4, (args, p)
    if p["kernel"] == S.MAXPOOL_BWD:
        assert p["grid"] == min(p["blocks_wanted"], p["blocks_cap"]) and p["grid_y"] == B and p["grid"] * B <= 8192 + B, (args, p)
    if p["kernel"] in (S.NARROW_INTERP_FWD, S.NARROW_INTERP_BWD_T):
        assert C <= 16 and p["grid"] == min(-(-B * points // p["ppwg"]), 65536), (args, p)
    return p


def test_plan_equals_the_restatement(seen):
    n, refused = 0, {}
    for op, B, Nin, Mout, C in itertools.product(S.OPS, GRID_B, GRID_N, GRID_M, GRID_C):
        got = _check(seen, op, B, Nin, Mout, C, 1, 33)
        if isinstance(got, str):
            refused[got] = refused.get(got, 0) + 1
        n += 1
    assert n == 7 * len(GRID_B) * len(GRID_N) * len(GRID_M) * len(GRID_C)
    assert seen == S.INSTANTIATIONS and len(seen) == 21                    # every kernel csrc/pool3d.hip contains, and no other
    assert set(refused) == {S.BAD_DIMS, S.BAD_SEGMENTS, S.BAD_BATCH, S.WIDE, S.BAD_GRID} and all(v >= 10 for v in refused.values()), refused
    # K and F: read by the ops that have them, and by no other
    for op in S.OPS:
        for K, F in itertools.product((1, 0, -1, INT_MAX, INT_MIN), repeat=2):
            got = _check(seen, op, 3, 100, 300, 8, K, F)
            assert (got == S.BAD_DIMS) == ((op in (S.FWD, S.NARROW) and K <= 0) or (op == S.MAX_GRAD_ROWS and F <= 0)), (op, K, F)
    for op in (-1, 7, INT_MAX, INT_MIN):
        assert _check(seen, op, 3, 100, 300, 8) == S.BAD_OP


def test_plan_at_every_boundary(seen):
    kernel = lambda *a, **k: _check(seen, *a, **k)["kernel"]
    field = lambda f, *a, **k: _check(seen, *a, **k)[f]
    for C in GRID_C[:12]:
        # points per workgroup: B * points against 65536
        for B, n, ppwg in ((2, 32767, 4), (2, 32768, 16), (1, 65535, 4), (1, 65536, 16), (1, 65537, 16), (64, 1023, 4), (64, 1024, 16)):
            assert field("ppwg", S.FWD, B, 7, n, C) == field("ppwg", S.MAX_GRAD_T, B, n, 7, C) == ppwg
            assert field("ppwg", S.MAX_GRAD_ROWS, B, n, 7, C, F=33) == ppwg
        # the split gather: Mout against 2 Nin, B Nin against 65536
        for B, Nin in ((1, 1), (2, 100), (3, 21845), (1, 65536), (2, 32768), (64, 1024)):
            assert kernel(S.SUM_GRAD_T, B, Nin, 2 * Nin - 1, C) == S.GATHER_BWD_T and kernel(S.SUM_GRAD_T, B, Nin, 2 * Nin, C) == S.GATHER_BWD_T_SPLIT
        for B, Nin in ((1, 65537), (2, 32769), (3, 21846), (64, 1025), (65536, 2)):
            assert kernel(S.SUM_GRAD_T, B, Nin, 2 * Nin, C) == kernel(S.SUM_GRAD_T, B, Nin, 8 * Nin, C) == S.GATHER_BWD_T
        # the scatter: M C on both sides of 256 * cap
        for B, cap in ((1, 8192), (64, 128), (3, 2731), (8192, 1), (65535, 1)):
            for M in (max(256 * cap // C, 1), 256 * cap // C + 1, 256 * cap // C + 2):
                p = _check(seen, S.MAX_GRAD, B, 9, M, C)
                assert (p["blocks_wanted"], p["blocks_cap"]) == (-(-M * C // 256), cap) and p["grid"] == min(p["blocks_wanted"], cap)
                assert p["zero_bytes"] == 4 * B * 9 * C
    assert _check(seen, S.MAX_GRAD, 65536, 9, 1, 4) == S.BAD_BATCH and kernel(S.MAX_GRAD, 65536, 9, 0, 4) == S.NONE
    assert field("zero_bytes", S.MAX_GRAD, 65536, 9, 0, 4) == 4 * 65536 * 9 * 4 and field("zero_bytes", S.MAX_GRAD, INT_MAX, INT_MAX, 0, INT_MAX) == S.HUGE
    # narrow rows: 16 * 65536 rows, 4 * 65536 sources
    for C in (1, 13, 16):
        assert [field("grid", S.NARROW, 1, 5, (1 << 20) + d, C) for d in (-16, -15, 0, 1)] == [65535, 65536, 65536, 65536]
        assert [field("grid", S.NARROW_GRAD_T, 1, (1 << 18) + d, 5, C) for d in (-4, -3, 0, 1)] == [65535, 65536, 65536, 65536]
        assert [field("grid", S.NARROW, 64, 5, (1 << 14) + d, C) for d in (-1, 0, 1)] == [65532, 65536, 65536]
        assert [field("grid", S.NARROW_GRAD_T, 64, (1 << 12) + d, 5, C) for d in (-1, 0, 1)] == [65520, 65536, 65536]
    assert _check(seen, S.NARROW, 2, 5, 100, 17) == _check(seen, S.NARROW_GRAD_T, 2, 5, 100, 17) == S.WIDE
    # N F against 2^31 - 1
    for N, F in ((INT_MAX, 1), (1 << 30, 2), (65536, 32768), (46341, 46341), (1, INT_MAX)):
        assert _check(seen, S.MAX_GRAD_ROWS, 1, N, 7, 8, F=F) == S.BAD_SEGMENTS
    for N, F in ((INT_MAX - 1, 1), ((1 << 30) - 1, 2), (65535, 32768), (46340, 46341), (1, INT_MAX - 1)):
        assert kernel(S.MAX_GRAD_ROWS, 1, N, 7, 8, F=F) == S.MAXPOOL_BWD_ROWS
    # the grid guard: from 2^31 - 7 clouds of one point (8 * ceil(B / 8) workgroups)
    for op, a in ((S.FWD, (7, 1)), (S.SUM_GRAD_T, (1, 1)), (S.MAX_GRAD_T, (1, 7)), (S.MAX_GRAD_ROWS, (1, 7))):
        assert _check(seen, op, INT_MAX - 6, *a, 4) == S.BAD_GRID and field("grid", op, INT_MAX - 7, *a, 4) == INT_MAX - 7
        assert _check(seen, op, 1 << 27, *[257 if v == 1 else v for v in a], 4) == S.BAD_GRID           # 2^27 * ceil(257 / 16) = 2^31 + 2^27
    assert field("grid", S.FWD, 1 << 27, 7, 240, 4) == 15 << 27 and _check(seen, S.FWD, 1 << 27, 7, 241, 4) == S.BAD_GRID


def test_smallest_launch_the_grid_guard_refuses():
    """DESIGN.md quotes it: B * Mout = 2 147 483 641, 2^31 - 7 clouds of one point.  For each row count, the first B that is
    refused (the grid grows with B), and the smallest product among them"""
    best = None
    for Mout in range(1, 4097):
        lo, hi = 0, INT_MAX + 1                     # lo is accepted, hi refused (or no int)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if S.plan(S.FWD, mid, 1, Mout, 4) == S.BAD_GRID:
                hi = mid
            else:
                lo = mid
        if hi <= INT_MAX and (best is None or hi * Mout < best[0]):
            best = (hi * Mout, hi, Mout)
    assert best == (2147483641, INT_MAX - 6, 1)
    # rows beyond that list: B * Mout >= 2^31 - 7 needs B > 2^19, where every cloud's parts are whole workgroups of 16 points
    assert S.plan(S.FWD, (INT_MAX - 6) // 4097 + 1, 1, 4097, 4)["grid"] < INT_MAX


def test_kernels_in_the_source_are_the_ones_the_plans_reach():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sph3d_gcn_amd", "csrc", "pool3d.hip")).read()
    defined = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src))
    assert defined == {i[0] for i in S.INSTANTIATIONS}
    # and the launch rules stand in pool_plan.hpp alone: no threshold outside the kernels' bodies
    host = src[src.index("// ---- the host side"):]
    assert not re.search(r"65536|65535|8192|% 4|<= 128|<= 16\b|kPtsPerWG", host)


def test_plan_query_writes_its_fields_and_nothing_behind_them():
    import ctypes
    from sph3d_gcn_amd import _lib
    fn = ctypes.CDLL(_lib.LIB_PATH).sph3d_pool3d_plan
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.c_void_p]
    n = len(S.FIELDS)
    assert n == 13
    out = (ctypes.c_longlong * (n + 4))(*([0x5a5a5a5a5a5a5a5a] * (n + 4)))
    want = tuple(S.plan(S.SUM_GRAD_T, 2, 40, 500, 260).values())
    assert fn(S.SUM_GRAD_T, 2, 40, 500, 260, 0, 0, ctypes.addressof(out)) == 0
    assert tuple(out)[:n] == want and tuple(out)[n:] == (0x5a5a5a5a5a5a5a5a,) * 4
    # a refusal writes nothing
    assert fn(S.NARROW, 2, 40, 500, 17, 8, 0, ctypes.addressof(out)) == -4 and tuple(out)[:n] == want
    assert fn(S.SUM_GRAD_T, 2, 40, 500, 260, 0, 0, None) == -1


def test_query_and_entries_refuse_alike():
    """every refusal, on the query and on the entry with null pointers: nothing may be read or launched before the answer"""
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    err = l.sph3d_last_error
    big = INT_MAX - 6

    def refused(call, status, text):
        assert call() == status and text in err(), (status, text, err())

    def both(op, B, Nin, Mout, C, K, F, entries, status, text):
        want = S.plan(op, B, Nin, Mout, C, K, F)
        assert isinstance(want, str) and S.STATUS[want] == status, (op, B, Nin, Mout, C, K, F, want)
        refused(lambda: l.sph3d_pool3d_plan(op, B, Nin, Mout, C, K, F, None), status, text)
        for e in entries:
            refused(lambda: e(B, Nin, Mout, C, K, F), status, text)

    # (the un-pooling entries name the rows N and the sources M)
    forward = [lambda B, Nin, Mout, C, K, F: l.sph3d_max_pool3d(B, Nin, Mout, C, K, None, None, None, None, None, None),
               lambda B, Nin, Mout, C, K, F: l.sph3d_avg_pool3d(B, Nin, Mout, C, K, None, None, None, None, None),
               lambda B, Nin, Mout, C, K, F: l.sph3d_mean_interpolate(B, Mout, Nin, C, K, None, None, None, None, None),
               lambda B, Nin, Mout, C, K, F: l.sph3d_weighted_interpolate(B, Mout, Nin, C, K, None, None, None, None, None, None)]
    sum_grad = [lambda B, Nin, Mout, C, K, F: l.sph3d_scatter_grad_t(B, Nin, Mout, C, None, None, None, None, None, None)]
    wrappers = [lambda B, Nin, Mout, C, K, F: l.sph3d_avg_pool3d_grad(B, Nin, Mout, C, K, None, None, None, None, None, 0, None),
                lambda B, Nin, Mout, C, K, F: l.sph3d_mean_interpolate_grad(B, Mout, Nin, C, K, None, None, None, None, None, 0, None),
                lambda B, Nin, Mout, C, K, F: l.sph3d_weighted_interpolate_grad(B, Mout, Nin, C, K, None, None, None, None, None, None, 0, None)]
    scatter = [lambda B, Nin, Mout, C, K, F: l.sph3d_max_pool3d_grad(B, Nin, Mout, C, None, None, None, None)]
    max_t = [lambda B, Nin, Mout, C, K, F: l.sph3d_max_pool3d_grad_t(B, Nin, Mout, C, *[None] * 8)]
    rows = [lambda B, Nin, Mout, C, K, F: l.sph3d_max_pool3d_grad_rows(B, Nin, Mout, C, F, *[None] * 10)]
    narrow = [lambda B, Nin, Mout, C, K, F: l.sph3d_interpolate_narrow(B, Mout, Nin, C, K, *[None] * 7)]
    narrow_grad = [lambda B, Nin, Mout, C, K, F: l.sph3d_interpolate_narrow_grad_t(B, Nin, Mout, C, *[None] * 6)]
    of = {S.FWD: forward, S.SUM_GRAD_T: sum_grad, S.MAX_GRAD: scatter, S.MAX_GRAD_T: max_t, S.MAX_GRAD_ROWS: rows, S.NARROW: narrow,
          S.NARROW_GRAD_T: narrow_grad}
    for op, entries in of.items():
        for B, Nin, Mout, C in ((-1, 8, 8, 8), (2, 0, 8, 8), (2, 8, -1, 8), (2, 8, 8, 0), (INT_MIN, INT_MIN, INT_MIN, INT_MIN)):
            both(op, B, Nin, Mout, C, 3, 3, entries, -1, b"bad dims")
        if op in (S.FWD, S.NARROW):
            both(op, 2, 8, 8, 8, 0, 3, entries, -1, b"bad dims")
    for e in wrappers:                      # (they check their own dimensions, K among them, in front of their workspace)
        for B, Nin, Mout, C, K in ((-1, 8, 8, 8, 3), (2, 0, 8, 8, 3), (2, 8, -1, 8, 3), (2, 8, 8, 0, 3), (2, 8, 8, 8, 0)):
            refused(lambda: e(B, Nin, Mout, C, K, 0), -1, b"bad dims")
        refused(lambda: e(2, 8, 8, 8, 3, 0), -2, b"workspace")
    both(S.MAX_GRAD_ROWS, 2, 0, 8, 8, 0, 0, rows, -1, b"F=0")
    both(S.MAX_GRAD_ROWS, 2, 65536, 8, 8, 0, 32768, rows, -1, b"index range")
    both(S.MAX_GRAD, 65536, 8, 8, 8, 0, 0, scatter, -1, b"second dimension")
    both(S.NARROW, 2, 8, 8, 17, 3, 0, narrow, -4, b"interpolate_narrow: rows of at most 16 channels")
    both(S.NARROW_GRAD_T, 2, 8, 8, 17, 0, 0, narrow_grad, -4, b"interpolate_narrow_grad_t: rows of at most 16 channels")
    # in the entries' order: the dimensions, then the segments; the dimensions, then the width
    both(S.MAX_GRAD_ROWS, -1, 65536, 8, 8, 0, 32768, rows, -1, b"bad dims")
    both(S.NARROW, 2, 8, 8, 17, 0, 0, narrow, -1, b"bad dims")
    # the new guard
    for op in (S.FWD, S.SUM_GRAD_T, S.MAX_GRAD_T, S.MAX_GRAD_ROWS):
        both(op, big, 1, 1, 4, 1, 1, of[op], -1, b"2^31 - 1 workgroups")
    # empty calls are valid and launch nothing, null pointers and all
    for op, entries in of.items():
        assert S.query(op, 0, 8, 8, 8, 3, 3) == dict.fromkeys(S.FIELDS, 0)
        assert all(e(0, 8, 8, 8, 3, 3) == 0 for e in entries), op
    for e in forward + narrow:
        assert e(3, 8, 0, 8, 3, 3) == 0
    assert all(e(0, 8, 8, 8, 3, 0) == 0 for e in wrappers)


def test_gpu_cases_reach_every_kernel():
    """the parametrize lists of the GPU tests, imported: the union of the kernels their library calls launch is every kernel of
    csrc/pool3d.hip — a form no device test reaches fails here"""
    import test_gpu_pool_forms as G
    import test_gpu_pool_rows as R
    import test_gpu_unpool_logits as L
    seen = set()
    for op, B, Nin, Mout, C, K, modes in G.plan_cases():
        seen |= S.instantiations(_check(set(), op, B, Nin, Mout, C, K), modes=modes)
    assert {i[0] for i in S.INSTANTIATIONS - seen} == {"maxpool_bwd_rows", "narrow_interp_fwd", "narrow_interp_bwd_t"}
    for op, B, Nin, Mout, C, F in R.plan_cases():
        seen |= S.instantiations(_check(set(), op, B, Nin, Mout, C, 1, F))
    for B, Nf, Mc, C, K in L.plan_cases():                      # (mean and weighted, forward and backward)
        seen |= S.instantiations(_check(set(), S.NARROW, B, Mc, Nf, C, K)) | S.instantiations(_check(set(), S.NARROW_GRAD_T, B, Mc, Nf, C))
    assert seen == S.INSTANTIATIONS
    # and the forms the cases are there for: both points-per-workgroup values of every gather, every body of the split gather
    forms = {(op, p["kernel"], p["V"], p["pairs"], min(p["passes"], 3), p["ppwg"])
             for op, p in [(c[0], S.query(*c[:6])) for c in G.plan_cases()] + [(c[0], S.query(*c[:5], 1, c[5])) for c in R.plan_cases()]}
    for kernel, ops in ((S.GATHER_FWD_HALF, (S.FWD,)), (S.GATHER_FWD, (S.FWD,)), (S.MAXPOOL_BWD_T, (S.MAX_GRAD_T,)), (S.MAXPOOL_BWD_ROWS, (S.MAX_GRAD_ROWS,))):
        assert {(f[2], f[5]) for f in forms if f[1] == kernel} >= ({(4, 4), (4, 16)} if kernel == S.GATHER_FWD_HALF else {(4, 4), (4, 16), (1, 4), (1, 16)})
    assert {f[2:5] for f in forms if f[1] == S.GATHER_BWD_T_SPLIT} == {(4, 1, 1), (4, 0, 1), (4, 0, 2), (4, 0, 3), (1, 0, 1), (1, 0, 2), (1, 0, 3)}
