"""The range search's launch choice, held on the host: the library's query sph3d_build_sphere_neighbor_plan (csrc/nn_plan.hpp:
nn_plan, which every search entry point launches from) against tests/_nn_forms.py, the restatement of the launchers as they
stood before the choice was gathered into that one function — field for field, in both radius modes, with each state of the
front's memory, with and without the fused output pass, on a grid that crosses every boundary of the rules (batches past 32
clouds, ragged M, the 64-position cap and K = 256 / 257 among them, which no device test reaches), on every case of the GPU case
lists and on the levels of the model configurations — and the workspace query against the plan.  No device is touched."""
import ctypes
import itertools

import numpy as np
import pytest

import _nn_forms as S

GRID_N = [1, 128, 700, 1023, 1024, 1025, 2048, 4096, 12288, 12289, 65536, 65537]
GRID_M = [0, 1, 63, 64, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 5 * 1024 - 1, 5 * 1024, 5 * 1024 + 1, 65536, 65537]
GRID_B = [0, 1, 2, 3, 16, 32, 33, 64, 65]
GRID_K = [1, 160, 161, 256, 257, 320, 321, 640, 641]       # 160 / 320 / 640: the last K with deferred hit lists at CPW 4 / 2 / 1
GRID_RADIUS = [0.02, 0.03, 0.11, 0.5, 0.1]                  # 1, 2, 5 and 8 positions inside kGridReach; 0.1: r_4 against 3 r_0 in float
# (fixed, fuse_wanted, memory): every radius goes through the first four, the rest through radius 0.1
MODES = [(0, 1, S.MEM_CALLER), (1, 1, S.MEM_CALLER), (0, 0, S.MEM_LIBRARY), (1, 0, S.MEM_LIBRARY)]
MORE_MODES = [m for m in itertools.product((0, 1), (0, 1), (S.MEM_NONE, S.MEM_CALLER, S.MEM_LIBRARY)) if m not in MODES]

INSTANTIATIONS = ({("nnquery_sphere_kernel", cpw, multi, defer, fuse) for cpw, multi in ((1, 0), (2, 0), (4, 0), (1, 1))
                   for defer, fuse in ((0, 0), (1, 0), (1, 1))}
                  | {(k, fuse) for k in ("nngrid_search_kernel", "nndense_kernel") for fuse in (0, 1)}
                  | {("nngrid_build_kernel",), ("nngrid_qorder_kernel",), ("nnsmall_prepare_kernel",), ("gated_zero_kernel",)})


@pytest.fixture(scope="module")
def lib():
    from sph3d_gcn_amd import _lib
    l = ctypes.CDLL(_lib.LIB_PATH)
    l.sph3d_build_sphere_neighbor_workspace.restype = ctypes.c_size_t
    l.sph3d_last_error.restype = ctypes.c_char_p
    return l


@pytest.fixture(scope="module")
def query(lib):
    fn = lib.sph3d_build_sphere_neighbor_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    out = (ctypes.c_longlong * len(S.FIELDS))()
    ref = ctypes.addressof(out)

    def q(*args):
        """-> the fields as a tuple, None for SPH3D_EINVAL"""
        rc = fn(*args, ref)
        assert rc in (0, -1), args
        return tuple(out) if rc == 0 else None
    return q


def _instantiations(p):
    """the kernel instantiations a plan launches"""
    p = dict(zip(S.FIELDS, p))
    if p["chain_grid"] == 0:
        return set()
    out = {("nnquery_sphere_kernel", p["CPW"], p["MULTI"], p["DEFER"], p["fused"])}
    if p["front"] == S.GRID:
        out |= {("nngrid_build_kernel",), ("nngrid_qorder_kernel",), ("nngrid_search_kernel", p["fused"])}
    if p["front"] == S.SMALL:
        out.add(("nnsmall_prepare_kernel",))
    if p["dense_grid"]:
        out.add(("nndense_kernel", p["fused"]))
    if p["clear_counts"]:
        out.add(("gated_zero_kernel",))
    return out


def _check(query, seen, fixed, B, N, M, K, radius, fuse, memory):
    args = (fixed, B, N, M, K, radius, fuse, memory)
    want = S.plan(*args)
    want = None if isinstance(want, str) else tuple(want[f] for f in S.FIELDS)
    got = query(*args)
    assert got == want, (args, got and dict(zip(S.FIELDS, got)), want and dict(zip(S.FIELDS, want)))
    if got is not None:
        p = dict(zip(S.FIELDS, got))
        seen |= _instantiations(got)
        # what every launch needs: LDS inside 160 KiB, workgroup counts an int, a front only with memory
        assert max(p["build_lds"], p["search_lds"], p["dense_lds"], p["chain_lds"]) <= S.LDS
        assert max(p["build_grid"], p["order_grid"], p["search_grid"], p["dense_grid"], p["chain_grid"]) <= S.INT_MAX
        assert memory != S.MEM_NONE or p["front"] == S.NONE
        assert (p["grid_done"] == 1 << 20) == (p["front"] != S.NONE) and (p["workspace_bytes"] > 0) == (p["front"] != S.NONE)
        assert p["fused"] == (fuse and p["DEFER"]) and (p["CPW"] == 1 or not p["MULTI"])
    return got


def test_the_radii_of_the_grid_put_1_2_5_and_8_positions_inside_the_reach():
    assert [S.positions(r, S.GRID_MAX_POS) for r in GRID_RADIUS[:4]] == [1, 2, 5, 8]


def test_plan_equals_the_old_launchers(query):
    seen, n, fronts = set(), 0, {}
    for B, N, M, K in itertools.product(GRID_B, GRID_N, GRID_M, GRID_K):
        for radius, mode in itertools.chain(itertools.product(GRID_RADIUS, MODES), itertools.product([0.1], MORE_MODES)):
            fixed, fuse, memory = mode
            p = _check(query, seen, fixed, B, N, M, K, radius, fuse, memory)
            fronts[p[0]] = fronts.get(p[0], 0) + 1
            n += 1
    assert n == 9 * 12 * 16 * 9 * (5 * 4 + 8)
    assert seen == INSTANTIATIONS and len(INSTANTIATIONS) == 20         # every instantiation the two files contain, and no other
    assert all(fronts[f] > 1000 for f in (S.NONE, S.GRID, S.SMALL))


def _gpu_cases():
    """(fixed, B, N, M, K, radius, fuse_wanted) of the GPU tests"""
    import test_gpu_nngrid, test_gpu_nnsmall, test_gpu_parity
    from sph3d_gcn_amd.harness import modelnet_net, ruemonge_net, s3dis_net, shapenet_net
    for _, B, N, M, radius, K in test_gpu_nngrid.GRID_CASES + test_gpu_parity.NN_CASES:
        for fuse in (0, 1):
            yield 0, B, N, N if M is None else M, K, radius, fuse
    # the cases test_gpu_nngrid, test_gpu_boundary and test_gpu_tgraph state inside their tests
    for fixed, B, N, M, K, radius in ((0, 2, 2048, 2500, 16, 0.05), (0, 40, 2048, 2048, 8, 0.08), (0, 70, 2048, 2048, 64, 0.2),
                                      (0, 40, 4096, 1024, 32, 0.1), (0, 33, 2100, 2100, 8, 0.08), (0, 2, 1000, 1000, 16, 0.1),
                                      (0, 2, 2048, 2048, 32, 0.3), (1, 2, 4096, 4096, 32, 0.1), (1, 2, 4096, 3000, 32, 0.1),
                                      (0, 2, 4096, 4096, 16, 0.05), (0, 2, 4096, 4096, 16, 0.03), (0, 4, 4096, 4096, 64, 0.1),
                                      (0, 4, 4096, 4096, 32, 0.07), (0, 2, 4096, 4096, 32, 0.1), (0, 4, 8192, 8192, 32, 0.1),
                                      (0, 2, 300, 300, 16, 0.2), (0, 2, 300, 500, 24, 0.15), (0, 2, 2048, 2048, 16, 0.07)):
        for fuse in (0, 1):
            yield fixed, B, N, M, K, radius, fuse
    nb = test_gpu_nnsmall.B
    for (N, K), radius in test_gpu_nnsmall.INTRA_RADIUS.items():
        for fuse in (0, 1):
            yield 0, nb, N, N, K, radius, fuse
    for (N, M, radius), K, fixed in itertools.product(test_gpu_nnsmall.INTER, (8, 64, 1024), (0, 1)):
        for B in (nb, 2, 33):
            yield fixed, B, N, M, K, radius, 1
    # the levels of the model configurations: intra graph, pooling graph and un-pooling graph of each
    for cfg in (s3dis_net.s3dis_config(), s3dis_net.scannet_config(), shapenet_net.shapenet_config(), modelnet_net.modelnet_config(),
                ruemonge_net.ruemonge_config(), s3dis_net.small_config(), modelnet_net.small_config()):
        N = cfg.num_input
        for l, radius in enumerate(cfg.radius):
            for B, fixed in itertools.product((1, 2, 4, 16, 32), (0, 1)):
                yield fixed, B, N, N, cfg.nn_uplimit[l], radius, 1
                yield fixed, B, N, cfg.num_sample[l], cfg.nn_uplimit[l], radius, 1
                yield fixed, B, cfg.num_sample[l], N, cfg.nn_uplimit[l], radius, 0
            N = cfg.num_sample[l]


def test_plan_of_every_gpu_case_and_model_level(query):
    seen, n = set(), 0
    for fixed, B, N, M, K, radius, fuse in _gpu_cases():
        for memory in (S.MEM_NONE, S.MEM_CALLER, S.MEM_LIBRARY):
            assert _check(query, seen, fixed, B, N, M, K, radius, fuse, memory) is not None
            n += 1
    assert n > 2000 and {i for i in INSTANTIATIONS if i[0] != "nnquery_sphere_kernel"} <= seen


def test_the_grid_takes_1024_points_where_both_shape_tests_hold(query):
    for B, fixed in itertools.product((3, 16, 32), (0, 1)):
        assert S.small_shape(B, 1024, 4096)
        p = dict(zip(S.FIELDS, query(fixed, B, 1024, 4096, 16, 0.1, 0, S.MEM_CALLER)))
        assert p["front"] == S.GRID and p["workspace_bytes"] == S.grid_bytes(B, 1024, 4096)[0]
        assert query(fixed, B, 1024, 4095, 16, 0.1, 0, S.MEM_CALLER)[0] == S.SMALL          # below 2^22 pairs: the small clouds' scan
        assert query(fixed, 2, 1024, 4095, 16, 0.1, 0, S.MEM_CALLER)[0] == S.NONE


def test_workspace_query_reads_the_plan(lib, query):
    ws = lib.sph3d_build_sphere_neighbor_workspace
    for B, N, M in itertools.product(GRID_B + [-1], GRID_N + [0, -1], GRID_M + [-1]):
        have = ws(B, N, M)
        assert have == S.workspace_bytes(B, N, M), (B, N, M)
        for K, radius, fixed, memory in itertools.product((1, 256, 257), (0.02, 0.5), (0, 1), (S.MEM_CALLER, S.MEM_LIBRARY)):
            p = query(fixed, B, N, M, K, radius, 0, memory)
            if p is not None:
                p = dict(zip(S.FIELDS, p))
                assert have >= p["workspace_bytes"] and (p["front"] == S.NONE or have == p["workspace_bytes"]), (B, N, M, K, fixed)
        if B > 0 and N > 0 and M > 0:
            assert have == query(1, B, N, M, 1, 1.0, 0, S.MEM_CALLER)[16]


def test_a_batch_whose_launch_is_past_an_int_is_the_chain_kernels(lib, query):
    """fixed mode takes any number of clouds: from 131 065 clouds of 65 536 queries the search launch of the grid would be 2^31
    workgroups, which xcd_grid() formed in an `int`.  The plan has no front there, and the workspace query says 0"""
    ws = lib.sph3d_build_sphere_neighbor_workspace
    B = 131064
    assert S.xcd_grid(B, 65536 // 4) <= S.INT_MAX < S.xcd_grid(B + 1, 65536 // 4)
    p = dict(zip(S.FIELDS, query(1, B, 1024, 65536, 8, 0.1, 0, S.MEM_CALLER)))
    assert p["front"] == S.GRID and p["search_grid"] == S.xcd_grid(B, 65536 // 4) and ws(B, 1024, 65536) == p["workspace_bytes"]
    for b in (B + 1, 1 << 20, S.INT_MAX):
        p = dict(zip(S.FIELDS, query(1, b, 1024, 65536, 8, 0.1, 0, S.MEM_CALLER)))
        assert p["front"] == S.NONE and (p["CPW"], p["chain_grid"]) == (4, 32 * 16) and ws(b, 1024, 65536) == 0
        assert tuple(p.values()) == tuple(S.plan(1, b, 1024, 65536, 8, 0.1, 0, S.MEM_CALLER).values())
    # the ends of the int range elsewhere: nothing but the chain kernel, in 64-bit arithmetic
    p = dict(zip(S.FIELDS, query(0, S.INT_MAX, S.INT_MAX, S.INT_MAX, S.INT_MAX, 0.1, 1, S.MEM_LIBRARY)))
    assert (p["front"], p["CPW"], p["MULTI"], p["DEFER"], p["fused"], p["chunkN"]) == (S.NONE, 1, 1, 0, 0, 12288)


def test_query_validates_in_the_entry_points_order(lib, query):
    fn, err = lib.sph3d_build_sphere_neighbor_plan, lib.sph3d_last_error
    out = (ctypes.c_longlong * len(S.FIELDS))()
    p = ctypes.addressof(out)
    good = (0, 3, 128, 128, 16, 0.5, 0, S.MEM_CALLER)
    assert fn(*good, p) == 0 and out[0] == S.SMALL
    assert fn(*good, None) == -1
    for i, bad in ((0, -1), (0, 2), (6, -1), (6, 2), (7, -1), (7, 3)):
        args = list(good)
        args[i] = bad
        assert fn(*args, p) == -1 and b"bad argument" in err(), args
    # radius, then nn_sample, then the dimensions — as sph3d_build_sphere_neighbor answers them
    for radius in (0.0, -1.0, float("nan")):
        assert fn(0, -1, 0, -1, 0, radius, 0, S.MEM_CALLER, p) == -1 and b"radius>0" in err()
        assert S.plan(0, -1, 0, -1, 0, radius, 0, S.MEM_CALLER) == S.BAD_RADIUS
    for K in (0, -3):
        assert fn(0, -1, 0, -1, K, 0.5, 0, S.MEM_CALLER, p) == -1 and b"nn_sample>0" in err()
    for B, N, M in ((-1, 128, 128), (3, 0, 128), (3, -2, 128), (3, 128, -1)):
        assert fn(0, B, N, M, 16, 0.5, 0, S.MEM_CALLER, p) == -1 and b"bad dims" in err()
    # the entry points themselves: the same statuses before anything is launched (null pointers: nothing may be read)
    search = lib.sph3d_build_sphere_neighbor
    search.argtypes = [ctypes.c_int] * 4 + [ctypes.c_float] + [ctypes.c_void_p] * 6
    assert search(-1, 0, -1, 0, 0.0, *([None] * 6)) == -1 and b"radius>0" in err()
    assert search(-1, 0, -1, 0, 0.5, *([None] * 6)) == -1 and b"nn_sample>0" in err()
    assert search(-1, 0, -1, 16, 0.5, *([None] * 6)) == -1 and b"bad dims" in err()
    # an empty call is valid and launches nothing; an infinite radius is a radius
    assert query(0, 0, 128, 128, 16, 0.5, 1, S.MEM_CALLER) == (0,) * len(S.FIELDS) == query(0, 3, 128, 0, 16, 0.5, 1, S.MEM_CALLER)
    assert query(0, 3, 4096, 8192, 16, float("inf"), 0, S.MEM_CALLER)[:2] == (S.GRID, 8)
    assert query(0, 3, 4096, 4096, 16, float(np.float32(1e-45)), 0, S.MEM_CALLER)[:2] == (S.GRID, 1)
