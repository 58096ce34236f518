"""The host side of the range search as it stood before csrc/nn_plan.hpp gathered it: sphere_neighbor() of csrc/nnquery.hip (the
chain kernel's choice), nngrid_search(), nnsmall_search(), launch_dense(), search_memory() and nngrid_workspace_bytes() of
csrc/nngrid.hip, restated function by function in Python.  tests/test_nn_forms.py holds the library's query
sph3d_build_sphere_neighbor_plan to plan() below, field for field.  Python integers do not overflow: where the old code's `int`
arithmetic would have, plan() says what the arithmetic means."""
import numpy as np

FIELDS = ("front", "npos", "nq", "nslices", "parts", "W", "build_lds", "search_lds", "build_grid", "order_grid", "search_grid", "j0",
          "dparts", "dense_lds", "dense_grid", "prepare_block", "workspace_bytes", "off_flag", "off_radii", "off_hdr", "off_cells",
          "off_points", "off_order", "CPW", "MULTI", "DEFER", "chunkN", "groups", "chain_grid", "chain_lds", "grid_done", "fused",
          "clear_counts")
NONE, GRID, SMALL = 0, 1, 2                              # front
MEM_NONE, MEM_CALLER, MEM_LIBRARY = 0, 1, 2              # memory
BAD_RADIUS, BAD_SAMPLE, BAD_DIMS = "radius", "nn_sample", "dims"

REF_GRID, REF_BLOCK = 32, 1024                           # common.hpp
WAVES_PER_WG, MAX_CHUNK, THR_TABLE = 16, 12288, 64       # nnquery.hip
GRID_MAX_CELLS, GRID_MAX_K, GRID_MAX_POS, GRID_REACH, MAX_POSITIONS, DENSE_Q, SMALL_MIN_CLOUDS = 8192, 256, 8, 3, 64, 4, 3    # nngrid.hip
SIZEOF_GRID_HDR = 32
LDS = 160 * 1024
INT_MAX = (1 << 31) - 1


def xcd_grid(B, parts):
    """common.hpp"""
    ls = 0 if B >= 5 else (1 if B >= 3 else (2 if B == 2 else 3))
    s, cpr = 1 << ls, 8 >> ls
    return 8 * ((B + cpr - 1) // cpr) * ((parts + s - 1) >> ls)


def hits_bytes(CPW, K):
    b = 4 * WAVES_PER_WG * CPW * K
    return b if b <= 40 * 1024 else 0


def positions(radius, limit):
    """nngrid_search's loop: chain positions whose radius stays <= 3 r_0, at most `limit`; float32, the sum in double"""
    radius = np.float32(radius)
    npos, rk = 1, radius
    with np.errstate(all="ignore"):
        while npos < limit:
            rk = np.float32(np.float64(rk) + 0.05)
            if not rk <= np.float32(GRID_REACH) * radius:
                break
            npos += 1
    return npos


def grid_bytes(B, N, M):
    """-> total, (cell starts, points, query order): the offsets nngrid_search forms"""
    hdr = 1024 + SIZEOF_GRID_HDR * B
    cs = 4 * B * (GRID_MAX_CELLS + 1)
    a16 = lambda v: (v + 15) & ~15
    return a16(hdr) + a16(cs) + 16 * B * N + 4 * B * M, (a16(hdr), a16(hdr) + a16(cs), a16(hdr) + a16(cs) + 16 * B * N)


def small_shape(B, N, M):
    return SMALL_MIN_CLOUDS <= B <= REF_GRID and 1 <= N <= 1024 and 1 <= M <= MAX_POSITIONS * REF_BLOCK


def small_bytes(B):
    return (1024 + SIZEOF_GRID_HDR * B + 15) & ~15


def workspace_bytes(B, N, M):
    """nngrid_workspace_bytes"""
    if B <= 0 or N <= 0 or M <= 0:
        return 0
    if N < 1024 or N > 65536 or M < 64 or M > MAX_POSITIONS * REF_BLOCK or N * M < (1 << 22):
        return small_bytes(B) if small_shape(B, N, M) else 0
    return grid_bytes(B, N, M)[0]


def dense(p, B, M, K, j0):
    """launch_dense"""
    p["dparts"] = (M - j0 + 4 * DENSE_Q - 1) // (4 * DENSE_Q)
    p["dense_lds"] = 4 * 4 * DENSE_Q * K
    p["dense_grid"] = xcd_grid(B, p["dparts"])


def grid_search(p, fixed, B, N, M, K, radius, memory):
    """nngrid_search -> it launched"""
    if (N < 1024 or N > 65536 or M < 64 or M > MAX_POSITIONS * REF_BLOCK or N * M < (1 << 22) or K > GRID_MAX_K or
            (not fixed and B > REF_GRID and ((M >= REF_BLOCK and M % REF_BLOCK != 0) or
                                             ((B + REF_GRID - 1) // REF_GRID) * ((M + REF_BLOCK - 1) // REF_BLOCK) > MAX_POSITIONS))):
        return False
    npos = 1
    if not fixed:
        npos = min(positions(radius, GRID_MAX_POS), ((B + REF_GRID - 1) // REF_GRID) * ((M + REF_BLOCK - 1) // REF_BLOCK))
    if memory == MEM_NONE:
        return False
    total, (cells, points, order) = grid_bytes(B, N, M)
    nq = M if fixed else min(M, npos * REF_BLOCK)
    W = ((N + 31) // 32 + 15) & ~15
    p.update(front=GRID, npos=npos, nq=nq, nslices=(nq + REF_BLOCK - 1) // REF_BLOCK, parts=(nq + 3) // 4, W=W,
             build_lds=4 * GRID_MAX_CELLS, search_lds=4 * W * 4 + 4 * 64 * 8 + 4 * K * 2, workspace_bytes=total, off_radii=64,
             off_hdr=1024, off_cells=cells, off_points=points, off_order=order)
    p.update(build_grid=B, order_grid=B * p["nslices"], search_grid=xcd_grid(B, p["parts"]))
    j0 = M
    if not fixed:
        S = (M + REF_BLOCK - 1) // REF_BLOCK
        sl = max(0, min(S, npos - ((B - 1) // REF_GRID) * S))
        j0 = min(sl * REF_BLOCK, M)
    p["j0"] = j0
    if j0 < M:
        dense(p, B, M, K, j0)
    return True


def small_search(p, fixed, B, N, M, K, memory):
    """nnsmall_search -> it launched"""
    if not small_shape(B, N, M) or K > GRID_MAX_K or memory == MEM_NONE:
        return False
    p.update(front=SMALL, workspace_bytes=small_bytes(B), off_radii=64, off_hdr=1024, prepare_block=64 * min(B, 16))
    dense(p, B, M, K, 0)
    return True


def plan(fixed, B, N, M, K, radius, fuse_wanted, memory):
    """sphere_neighbor -> the fields, or why the call is SPH3D_EINVAL"""
    if not np.float32(radius) > 0:
        return BAD_RADIUS
    if not K > 0:
        return BAD_SAMPLE
    if not (B >= 0 and N > 0 and M >= 0):
        return BAD_DIMS
    p = dict.fromkeys(FIELDS, 0)
    if B == 0 or M == 0:
        return p
    chains = min(B, REF_GRID) * min(M, REF_BLOCK)
    cpw = 4 if chains >= 256 * WAVES_PER_WG * 4 else (2 if chains >= 256 * WAVES_PER_WG * 2 else 1)
    hb = hits_bytes(cpw, K)
    max_chunk = min(((LDS - THR_TABLE * 4 - hb) // 12) & ~127, MAX_CHUNK)
    chunk = min(N, max_chunk)
    multi = N > chunk
    if multi:
        hb = hits_bytes(1, K)
        chunk = min(((LDS - THR_TABLE * 4 - hb) // 12) & ~127, MAX_CHUNK)
    fused = bool(fuse_wanted) and hb != 0
    launched = grid_search(p, fixed, B, N, M, K, radius, memory) or small_search(p, fixed, B, N, M, K, memory)
    if launched and max(p["order_grid"], p["search_grid"], p["dense_grid"]) > INT_MAX:
        # the old code held these in an `int` and would have asked for a launch that cannot be made: the plan leaves such a call
        # (131 072 clouds or more) to the chain kernel
        p = dict.fromkeys(FIELDS, 0)
        launched = False
    if launched:
        p["grid_done"] = 1 << 20
        p["clear_counts"] = B * N + 1 if fused else 0           # (the launch covers B N F + F counters)
    # launch_sphere of the instantiation SPH3D_NN picks: multi first, then cpw
    CPW = 1 if multi else cpw
    nt = min(M, REF_BLOCK)
    groups = (nt + WAVES_PER_WG * CPW - 1) // (WAVES_PER_WG * CPW)
    p.update(CPW=CPW, MULTI=int(multi), DEFER=int(hb != 0), chunkN=chunk, groups=groups, chain_grid=min(B, REF_GRID) * groups,
             chain_lds=3 * ((chunk + 127) & ~127) * 4 + hb + THR_TABLE * 4, fused=int(fused))
    return p
