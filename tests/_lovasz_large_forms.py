"""The launcher of sph3d_lovasz_softmax_large restated in Python (csrc/lovasz_plan.hpp: lovasz_large_plan): what the host decides
for a call, field by field, in Python's unbounded integers.  tests/test_lovasz_large.py holds the library's plan query to it.
No library, no torch."""

FIELDS = ("tile_log2", "tile", "runs", "npad", "passes", "mtile", "mtiles", "slab", "slabs", "probs_grid", "count_grid", "sort_lds",
          "merge_lds", "grad_grid", "key_bufs", "workspace_bytes", "off_keys0", "off_keys1", "off_tilecnt", "off_partial",
          "off_count", "off_bad", "cap")

MAX_N = 1 << 20
MAX_C = 1024
TILE_LOG2 = (10, 14)            # forced run lengths
DEFAULT_TILE_LOG2 = 12
MERGE_TILE = 1024
COUNT_ROWS = 4096
WS_CAP = 128 << 20
EINVAL, EUNSUPPORTED = -1, -4


def plan(B, N, C, tile_log2=0, slab=0):
    """-> dict of FIELDS, or the status of the refusal (in the entry's order)"""
    if not (B >= 0 and N > 0 and C > 0):
        return EINVAL
    if not (B * N * C <= 1 << 40 and B * C <= 0x7fffffff and B <= 65535):
        return EINVAL
    if N > MAX_N or C > MAX_C:
        return EUNSUPPORTED
    if not (tile_log2 == 0 or TILE_LOG2[0] <= tile_log2 <= TILE_LOG2[1]):
        return EINVAL
    if not (0 <= slab <= C):
        return EINVAL
    p = dict.fromkeys(FIELDS, 0)
    if B == 0:
        return p
    p["tile_log2"] = tile_log2 or DEFAULT_TILE_LOG2
    tile = p["tile"] = 1 << p["tile_log2"]
    runs = p["runs"] = -(-N // tile)
    npad = p["npad"] = runs * tile
    p["passes"] = (runs - 1).bit_length()
    p["mtile"] = MERGE_TILE
    mtiles = p["mtiles"] = npad // MERGE_TILE
    bufs = p["key_bufs"] = 2 if p["passes"] else 1
    fixed = 4 * B * C + 4 * B
    per_class = B * (bufs * 8 * npad + 8 * mtiles)
    if slab == 0:
        room = WS_CAP - fixed - 255
        slab = min(C, max(1, room // per_class if room > 0 else 0))
    p["slab"] = slab
    p["slabs"] = -(-C // slab)
    p["probs_grid"] = -(-B * N // 256)
    p["count_grid"] = -(-N // COUNT_ROWS)
    p["sort_lds"] = 8 * tile
    p["merge_lds"] = 8 * MERGE_TILE
    p["grad_grid"] = -(-N // 1024)
    keys, words = 8 * slab * B * npad, 4 * slab * B * mtiles
    p["off_keys0"] = 0
    p["off_keys1"] = keys if bufs == 2 else 0
    p["off_tilecnt"] = bufs * keys
    p["off_partial"] = p["off_tilecnt"] + words
    p["off_count"] = p["off_partial"] + words
    p["off_bad"] = p["off_count"] + 4 * B * C
    p["workspace_bytes"] = (p["off_bad"] + 4 * B + 255) & ~255
    p["cap"] = WS_CAP
    return p
