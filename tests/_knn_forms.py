"""The host side of the k-nearest-neighbour search, restated in Python: what sph3d_build_nearest_neighbor launches for a call
(csrc/knn_plan.hpp: knn_plan).  tests/test_knn_forms.py holds the library's query sph3d_build_nearest_neighbor_plan to plan()
below, field for field.  Python integers do not overflow: every product here is the exact one."""
import numpy as np

FIELDS = ("form", "queries", "block", "groups", "scan_grid", "scan_lds", "search_grid", "search_lds", "fallback", "cells", "cell_cap",
          "build_block", "build_parts", "build_grid", "setup_grid", "prefix_block", "prefix_grid", "workspace_bytes", "off_hdr",
          "off_cells", "off_points", "hdr_stride", "cell_stride", "point_stride")
NONE, SCAN, GRID = 0, 1, 2                               # form
MODE_AUTO, MODE_SCAN, MODE_GRID = 0, 1, 2                # mode
BAD_K, BIG_K, BAD_RADIUS, BAD_DIMS, BAD_MODE = "k", "k > 64", "radius", "dims", "mode"

MAX_K, QUERIES, BLOCK, TILE, SCAN_MAX = 64, 4, 256, 1024, 2048
MAX_GRID, MAX_ELEMS = 1 << 20, 1 << 40
MIN_CELLS, MAX_CELLS, HDR_BYTES = 64, 1 << 21, 256       # nn1grid.hpp
BUILD_BLOCK, BUILD_PARTS, PREFIX_BLOCK = 256, 64, 1024
LDS = 160 * 1024
INT_MAX = (1 << 31) - 1

# the kernels of csrc/knn.hip as a plan launches them ("gated": knn_scan_kernel behind the grid search, per cloud on the device flag)
INSTANTIATIONS = {("knn_scan_kernel", "all"), ("knn_scan_kernel", "gated"), ("knn_grid_kernel",), ("knn_init_kernel",),
                  ("knn_bbox_kernel",), ("knn_setup_kernel",), ("knn_sort_kernel", 0), ("knn_sort_kernel", 1), ("knn_prefix_kernel",)}


def cell_cap(n):
    return min(max(n // 2, MIN_CELLS), MAX_CELLS)


def plan(B, N, M, k, radius, mode):
    """-> the fields, or why the call is refused (BIG_K: SPH3D_EUNSUPPORTED, the others SPH3D_EINVAL)"""
    if not k >= 1:
        return BAD_K
    if not k <= MAX_K:
        return BIG_K
    if not np.float32(radius) > 0:
        return BAD_RADIUS
    if not (B >= 0 and N >= 1 and M >= 0):
        return BAD_DIMS
    if not (B * N <= MAX_ELEMS and B * M <= MAX_ELEMS):
        return BAD_DIMS
    if mode not in (MODE_AUTO, MODE_SCAN, MODE_GRID):
        return BAD_MODE
    p = dict.fromkeys(FIELDS, 0)
    if B == 0 or M == 0:
        return p
    groups = -(-M // QUERIES)
    p.update(queries=QUERIES, block=BLOCK, groups=groups, scan_lds=3 * 4 * TILE, scan_grid=min(B * groups, MAX_GRID))
    if mode == MODE_SCAN or (mode == MODE_AUTO and N <= SCAN_MAX):
        p["form"] = SCAN
        return p
    cells = cell_cap(N)
    parts = min(-(-N // BUILD_BLOCK), BUILD_PARTS)
    cell_stride = (4 * (cells + 1) + 255) // 256 * 256
    p.update(form=GRID, search_grid=p["scan_grid"], fallback=1, cells=cells, cell_cap=MAX_CELLS, build_block=BUILD_BLOCK,
             build_parts=parts, build_grid=min(B * parts, MAX_GRID), setup_grid=min(-(-B // BUILD_BLOCK), MAX_GRID),
             prefix_block=PREFIX_BLOCK, prefix_grid=min(B, MAX_GRID), hdr_stride=HDR_BYTES, cell_stride=cell_stride,
             point_stride=16 * N, off_hdr=0, off_cells=HDR_BYTES * B, off_points=HDR_BYTES * B + cell_stride * B)
    p["workspace_bytes"] = p["off_points"] + 16 * N * B
    return p


def instantiations(p):
    """the kernels a plan (a dict of FIELDS) launches"""
    if p["form"] == NONE:
        return set()
    if p["form"] == SCAN:
        return {("knn_scan_kernel", "all")}
    return INSTANTIATIONS - {("knn_scan_kernel", "all")}
