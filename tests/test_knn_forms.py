"""The k-nearest-neighbour search on the host: the library's query sph3d_build_nearest_neighbor_plan (csrc/knn_plan.hpp: knn_plan,
which the entry launches from) against tests/_knn_forms.py, the launcher restated in Python — field for field, on a grid that
crosses every boundary of the rules and includes the ends of the int range in every argument — the workspace query against the
plan, the validation order of the query and of the entry, the plan of every GPU case; and the numpy statement harness/knn.py
itself against exact integers (a lattice, where most rows tie at the k-th place) and against float64.  No device is touched."""
import ctypes
import itertools

import numpy as np
import pytest

import _knn_forms as S
import _knn_ref as R

INT_MAX, INT_MIN = S.INT_MAX, -S.INT_MAX - 1
GRID_K = [1, 2, 63, 64, 65, 0, -1, INT_MAX, INT_MIN]
# the wave, the tile (1024) and AUTO's threshold (2048), 128 = 2 * kNn1MinCells (the cell count leaves its floor), the build's 64 parts of
# 256 points, the cell cap 2 * 2^21
GRID_N = [1, 2, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385, 65536,
          (1 << 22) - 1, 1 << 22, (1 << 22) + 2, INT_MAX, 0, -1, INT_MIN]
GRID_B = [0, 1, 2, 255, 256, 257, 511, 512, 513, 1 << 14, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, INT_MAX, -1, INT_MIN]
GRID_M = [0, 1, 3, 4, 5, 2048, 8192, (1 << 22) - 3, 1 << 22, (1 << 22) + 1, INT_MAX, -1, INT_MIN]
GRID_RADIUS = [float("inf"), 0.15]
MODES = [S.MODE_AUTO, S.MODE_SCAN, S.MODE_GRID]


@pytest.fixture(scope="module")
def lib():
    from sph3d_gcn_amd import _lib
    l = ctypes.CDLL(_lib.LIB_PATH)
    l.sph3d_build_nearest_neighbor_workspace.restype = ctypes.c_size_t
    l.sph3d_build_nearest_neighbor_workspace.argtypes = [ctypes.c_int] * 5
    l.sph3d_build_nearest_neighbor_plan.restype = ctypes.c_int
    l.sph3d_build_nearest_neighbor_plan.argtypes = [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    l.sph3d_build_nearest_neighbor.restype = ctypes.c_int
    l.sph3d_build_nearest_neighbor.argtypes = ([ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6 +
                                               [ctypes.c_size_t, ctypes.c_void_p])
    l.sph3d_last_error.restype = ctypes.c_char_p
    return l


@pytest.fixture(scope="module")
def query(lib):
    out = (ctypes.c_longlong * len(S.FIELDS))()
    ref = ctypes.addressof(out)

    def q(*args):
        """-> the fields as a tuple, or the status of a refusal"""
        rc = lib.sph3d_build_nearest_neighbor_plan(*args, ref)
        assert rc in (0, -1, -4), args
        return tuple(out) if rc == 0 else rc
    return q


def _check(query, seen, B, N, M, k, radius, mode):
    args = (B, N, M, k, radius, mode)
    want = S.plan(*args)
    if isinstance(want, str):
        want = -4 if want == S.BIG_K else -1
    else:
        want = tuple(want[f] for f in S.FIELDS)
    got = query(*args)
    assert got == want, (args, got, want)
    if isinstance(got, tuple):
        p = dict(zip(S.FIELDS, got))
        seen |= S.instantiations(p)
        # what every launch needs: workgroup counts and LDS a launch can have, offsets in order and 16-byte aligned, a grid's cells
        # inside their slots, and bytes that are the exact 64-bit sums
        assert max(p["scan_grid"], p["search_grid"], p["build_grid"], p["setup_grid"], p["prefix_grid"]) <= S.MAX_GRID
        assert max(p["scan_lds"], p["search_lds"]) <= 64 * 1024 and max(p["block"], p["build_block"], p["prefix_block"]) <= 1024
        assert (p["form"] == S.NONE) == (B == 0 or M == 0) and (p["workspace_bytes"] > 0) == (p["form"] == S.GRID) == bool(p["fallback"])
        if p["form"] != S.NONE:
            assert p["groups"] * p["queries"] >= M > (p["groups"] - 1) * p["queries"] and (p["queries"], p["block"]) == (4, 256)
        if p["form"] == S.GRID:
            assert 0 == p["off_hdr"] < p["off_cells"] < p["off_points"] < p["workspace_bytes"] < 1 << 62
            assert all(p[f] % 16 == 0 for f in ("off_cells", "off_points", "cell_stride", "point_stride", "hdr_stride"))
            assert p["off_cells"] - p["off_hdr"] == B * p["hdr_stride"] and p["off_points"] - p["off_cells"] == B * p["cell_stride"]
            assert p["workspace_bytes"] - p["off_points"] == B * p["point_stride"] == 16 * B * N
            assert 4 * (p["cells"] + 1) <= p["cell_stride"] and S.MIN_CELLS <= p["cells"] <= p["cell_cap"] == S.MAX_CELLS
            assert 1 <= p["build_parts"] <= S.BUILD_PARTS and (p["build_parts"] - 1) * p["build_block"] < N
    return got


def test_plan_equals_the_restatement(query):
    seen, n, forms, refused = set(), 0, {0: 0, 1: 0, 2: 0}, 0
    for B, N, M, k in itertools.product(GRID_B, GRID_N, GRID_M, GRID_K):
        for radius, mode in itertools.product(GRID_RADIUS, MODES):
            got = _check(query, seen, B, N, M, k, radius, mode)
            if isinstance(got, tuple):
                forms[got[0]] += 1
            else:
                refused += 1
            n += 1
    assert n == len(GRID_B) * len(GRID_N) * len(GRID_M) * len(GRID_K) * 6
    assert seen == S.INSTANTIATIONS and len(seen) == 9          # every kernel csrc/knn.hip contains, and no other
    assert all(v > 1000 for v in forms.values()) and refused > 1000
    # the ends of the int range together: refused in 64-bit arithmetic, never a wrapped product
    assert query(INT_MAX, INT_MAX, INT_MAX, 64, 1.0, S.MODE_GRID) == -1
    p = dict(zip(S.FIELDS, query(512, INT_MAX, INT_MAX, 64, 1.0, S.MODE_GRID)))
    assert p["workspace_bytes"] == 512 * (256 + 16 * INT_MAX + (4 * (S.MAX_CELLS + 1) + 255) // 256 * 256) and p["search_grid"] == S.MAX_GRID


def test_kernels_in_the_source_are_the_ones_the_plans_reach():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sph3d_gcn_amd", "csrc", "knn.hip")).read()
    defined = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src))
    assert defined == {i[0] for i in S.INSTANTIATIONS}


def test_workspace_query_reads_the_plan(lib, query):
    ws = lib.sph3d_build_nearest_neighbor_workspace
    for B, N, M, k, mode in itertools.product(GRID_B, GRID_N, GRID_M[:8] + GRID_M[-3:], (1, 64, 65, 0), MODES + [3, -1]):
        want = S.plan(B, N, M, k, np.inf, mode)
        assert ws(B, N, M, k, mode) == (0 if isinstance(want, str) else want["workspace_bytes"]), (B, N, M, k, mode)
        for radius in GRID_RADIUS:
            got = query(B, N, M, k, radius, mode)
            assert isinstance(got, tuple) == (not isinstance(want, str))
            if isinstance(got, tuple):
                assert got[S.FIELDS.index("workspace_bytes")] == ws(B, N, M, k, mode)


def test_plan_query_writes_its_fields_and_nothing_behind_them(lib):
    out = (ctypes.c_longlong * (len(S.FIELDS) + 4))(*([0x5a5a5a5a5a5a5a5a] * (len(S.FIELDS) + 4)))
    assert lib.sph3d_build_nearest_neighbor_plan(3, 4096, 4096, 16, 0.5, S.MODE_AUTO, ctypes.addressof(out)) == 0
    assert tuple(out)[:len(S.FIELDS)] == tuple(S.plan(3, 4096, 4096, 16, 0.5, S.MODE_AUTO).values())
    assert tuple(out)[len(S.FIELDS):] == (0x5a5a5a5a5a5a5a5a,) * 4
    # a refusal writes nothing
    assert lib.sph3d_build_nearest_neighbor_plan(3, 4096, 4096, 65, 0.5, S.MODE_AUTO, ctypes.addressof(out)) == -4
    assert tuple(out)[:len(S.FIELDS)] == tuple(S.plan(3, 4096, 4096, 16, 0.5, S.MODE_AUTO).values())


def test_query_and_entry_validate_alike_and_in_order(lib, query):
    fn, err, entry = lib.sph3d_build_nearest_neighbor_plan, lib.sph3d_last_error, lib.sph3d_build_nearest_neighbor
    out = (ctypes.c_longlong * len(S.FIELDS))()
    p = ctypes.addressof(out)
    nulls = [None] * 6 + [0, None]

    def both(B, N, M, k, radius, mode, status, text):
        # (the entry with null pointers: nothing may be read or launched before the answer)
        assert fn(B, N, M, k, radius, mode, p) == status and text in err(), (B, N, M, k, radius, mode, err())
        assert entry(B, N, M, k, radius, mode, 0, *nulls) == status and text in err(), (B, N, M, k, radius, mode, err())

    assert fn(2, 128, 128, 16, 0.5, S.MODE_AUTO, p) == 0 and out[0] == S.SCAN
    assert fn(2, 128, 128, 16, 0.5, S.MODE_AUTO, None) == -1 and b"out is NULL" in err()
    # k, then radius, then the dimensions, then the mode: every later argument is bad as well
    for k in (0, -3, INT_MIN):
        both(-1, 0, -1, k, -1.0, 7, -1, b"k>=1")
    for k in (65, 1000, INT_MAX):
        both(-1, 0, -1, k, -1.0, 7, -4, b"k<=64")
    for radius in (0.0, -1.0, float("nan"), float("-inf")):
        both(-1, 0, -1, 64, radius, 7, -1, b"radius>0")
        assert S.plan(-1, 0, -1, 64, radius, 7) == S.BAD_RADIUS
    for B, N, M in ((-1, 128, 128), (3, 0, 128), (3, -2, 128), (3, 128, -1), (INT_MAX, INT_MAX, 1), (INT_MAX, 1, INT_MAX)):
        both(B, N, M, 16, 0.5, 7, -1, b"bad dims")
    for mode in (3, -1):
        both(2, 128, 128, 16, 0.5, mode, -1, b"mode")
    # the entry alone: dist, then (for a call that launches) the pointers and the workspace
    assert entry(2, 128, 128, 16, 0.5, S.MODE_AUTO, 2, *nulls) == -1 and b"dist" in err()
    assert entry(2, 128, 128, 16, 0.5, S.MODE_AUTO, 0, *nulls) == -1 and b"null pointer" in err()
    one = ctypes.c_void_p(4096)             # never dereferenced: the workspace is refused on the host
    assert entry(2, 4096, 128, 16, 0.5, S.MODE_AUTO, 0, one, one, one, one, one, None, 0, None) == -2 and b"workspace" in err()
    # an empty call is valid and launches nothing, null pointers and all; an infinite radius is "no radius"
    assert query(0, 128, 128, 16, 0.5, S.MODE_GRID) == (0,) * len(S.FIELDS) == query(3, 128, 0, 16, 0.5, S.MODE_GRID)
    assert entry(0, 128, 128, 16, 0.5, S.MODE_GRID, 0, *nulls) == 0 == entry(3, 128, 0, 16, 0.5, S.MODE_GRID, 1, *nulls)
    assert query(3, 4096, 4096, 16, float("inf"), S.MODE_AUTO)[0] == S.GRID


def test_plan_of_every_gpu_case(query):
    """each case of tests/test_gpu_knn.py has the plan its id names, in AUTO; SCAN and GRID force either form at any size; together
    they reach every kernel of the file"""
    seen = set()
    for name in R.CASES:
        db, q, k, radius = R.case(name)
        B, N, M = db.shape[0], db.shape[1], q.shape[1]
        r = np.inf if radius is None else radius
        assert _check(query, seen, B, N, M, k, r, S.MODE_AUTO)[0] == R.FORM_OF_ID[name.rsplit("-", 1)[1]], name
        assert _check(query, seen, B, N, M, k, r, S.MODE_SCAN)[0] == S.SCAN and _check(query, seen, B, N, M, k, r, S.MODE_GRID)[0] == S.GRID
    assert seen == S.INSTANTIATIONS
    sizes = {R.case(n)[0].shape[1] for n in R.CASES}
    assert {1, 2, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049} <= sizes and {S.SCAN_MAX - 1, S.SCAN_MAX, S.SCAN_MAX + 1} <= sizes


def test_statement_against_exact_integers_on_the_lattice():
    """12^3 lattice at spacing 0.25, 600 queries, k = 16: every float32 operation of the statement is exact there, so it must give
    the order computed in integers with ties by index — and most rows tie exactly at the k-th place, so a wrong tie rule fails"""
    from sph3d_gcn_amd.harness import knn
    db, q, P8, Q8 = R.lattice()
    assert db.shape == (1, 1728, 3) and q.shape == (1, 600, 3)
    assert (db.astype(np.float64) * 8 == P8).all() and (q.astype(np.float64) * 8 == Q8).all()
    want_idx, want_d64, tie = R.integer_order(P8, Q8, R.LATTICE_K)
    print("rows with a tie at the k-th place: %d of %d" % (tie.sum(), len(tie)))
    assert tie.sum() >= 400
    for dist in ("squared", "root"):
        idx, cnt, dst = knn.knn_reference(db, q, R.LATTICE_K, None, dist)
        assert (cnt == R.LATTICE_K).all() and (idx[0] == want_idx).all()
        d2 = (want_d64 / 64.0).astype(np.float32)
        want = d2 if dist == "squared" else np.sqrt(np.sqrt(d2))
        assert (dst[0].view(np.uint32) == want.view(np.uint32)).all()
    assert (R.expected("lattice-scan", "squared")[0][0] == want_idx).all()


def test_statement_against_float64_on_the_uniform_clouds():
    from sph3d_gcn_amd.harness import knn
    db, q = R.uniform_database(), R.radius_queries()
    idx, cnt, _ = knn.knn_reference(db, q, 16)
    differ = rows = 0
    for b in range(2):
        want, clear = R.float64_order(db[b], q[b], 16)
        rows += int(clear.sum())
        differ += int((idx[b][clear] != want[clear]).any(axis=1).sum())
    print("float64 rows without a tie: %d, rows that differ: %d" % (rows, differ))
    assert (cnt == 16).all() and rows >= 1300 and differ == 0


def test_statement_edges():
    from sph3d_gcn_amd.harness import knn
    db = np.array([[[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 0, np.inf], [1, 0, 0]]], np.float32)
    q = np.array([[[0.9, 0, 0], [np.nan, 0, 0], [10, 0, 0]]], np.float32)
    idx, cnt, dst = knn.knn_reference(db, q, 4, dist="squared")
    assert cnt.tolist() == [[3, 0, 3]] and idx[0].tolist() == [[1, 4, 0, 0], [0, 0, 0, 0], [1, 4, 0, 0]]
    assert dst[0, 1].tolist() == [0, 0, 0, 0] and dst[0, 0, 3] == 0 and dst[0, 0, 0] == np.float32(np.float32(0.9) - 1) ** 2
    idx, cnt, dst = knn.knn_reference(db, q, 4, radius=0.5)
    assert cnt.tolist() == [[2, 0, 0]] and idx[0, 0].tolist() == [1, 4, 0, 0]
    assert dst[0, 0, 0] == np.sqrt(np.sqrt(np.float32(np.float32(0.9) - 1) ** 2, dtype=np.float32), dtype=np.float32)
    assert [knn.knn_reference(db, q, 4, radius=r)[1].tolist() for r in (None, np.inf)] == [[[3, 0, 3]]] * 2
    for bad in (dict(k=0), dict(k=65), dict(k=3, radius=0.0), dict(k=3, radius=np.nan), dict(k=3, dist="euclid")):
        with pytest.raises(ValueError):
            knn.knn_reference(db, q, **bad)
