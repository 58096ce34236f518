"""The launchers' rules of csrc/gemm.hip, restated: which kernel, tile, k-step, guard, exchange and slab split a pointwise product
takes.  Copied launcher by launcher from the host code as it stood BEFORE the choice was gathered into one plan function
(launch_gemm / launch_gemm_tiles, nn_stats_tile + sph3d_pointwise_gemm_bnstats, tn_plan + sph3d_pointwise_gemm_tn), so that it
states what the code did, not what the plan function says.  Plain Python: no torch, no library; tests/test_gemm_forms.py holds the
library's host-only query (sph3d_pointwise_gemm_plan) to it, tests/test_gpu_gemm_forms.py runs FORM_CASES.

Dimensions are those of the C ABI: (R, Cin, Cout) as passed to sph3d_pointwise_gemm (NN: trans_w = 0, NT: trans_w = 1 — there
"Cin" is the reduced dimension and W is stored [Cout, Cin]), sph3d_pointwise_gemm_bnstats (NNS) and sph3d_pointwise_gemm_tn (TN)."""
NN, NT, NNS, TN = 0, 1, 2, 3
NAMES = ("NN", "NT", "NNS", "TN")
F32, SPLIT = 0, 1
# the order in which sph3d_pointwise_gemm_plan writes its output
FIELDS = ("pipe", "bm", "bn", "bk", "guard", "stats", "xs", "nsplit", "kchunk", "reduce", "grid", "stats_blocks")

BM, BKS, BKL = 128, 16, 32
K_MIN_TILES = 512
K_XS_CAP, K_XS_MAX_WGS, K_XS_MAX_TG, K_XS_FLAGS = 4, 1024, 384, 4096
K_TN_XS_ROWS, K_TN_XS_CAP = 2048, 8


def gemm_grid(tiles_m, tiles_n, nsplit=0):
    if nsplit > 0:
        return ((nsplit + 7) // 8) * 8 * tiles_m * tiles_n
    return ((tiles_m + 7) // 8) * 8 * tiles_n


def xs_splits(Tg, Kd, bk, cap):
    ns = K_XS_MAX_WGS // (Tg if Tg > 0 else 1)
    if Tg > K_XS_MAX_TG:
        ns = 1
    ns = min(ns, cap)
    while ns > 1 and (Kd % (bk * ns) != 0 or Kd // ns < 256):
        ns -= 1
    return max(ns, 1)


def xs_buffer(exchange_ok, ntile):
    """the stream's exchange buffer: none for more tiles than arrival counters, else whatever the stream can supply"""
    return bool(exchange_ok) and ntile <= K_XS_FLAGS


def _form(pipe, bm, bn, bk, guard, grid, stats=0, xs=1, nsplit=1, kchunk=0, reduce=0, stats_blocks=0):
    return dict(pipe=pipe, bm=bm, bn=bn, bk=bk, guard=int(guard), stats=stats, xs=xs, nsplit=nsplit, kchunk=kchunk, reduce=reduce,
                grid=grid, stats_blocks=stats_blocks)


def launch_gemm_tiles(bkm, guard, M, N, Kd, mode, exchange_ok):
    """launch_gemm_tiles<AK = true, BKM, GUARD>"""
    def ntiles(bm, bn):
        return ((M + bm - 1) // bm) * ((N + bn - 1) // bn)

    def tile(pipe, bm, bn, bk):
        return _form(pipe, bm, bn, bk, guard, gemm_grid((M + bm - 1) // bm, (N + bn - 1) // bn))

    big = N > 64 and ntiles(128, 128) >= K_MIN_TILES
    if guard:
        if mode and Kd >= 16 and N >= 32:
            if big:
                return tile(SPLIT, 128, 128, 16)
            if not bkm and N <= 64 and ntiles(128, 64) >= K_MIN_TILES:
                return tile(SPLIT, 128, 64, 16)
            return tile(SPLIT, 64, 64, 16)
    else:
        if mode:
            if big:
                return tile(SPLIT, 128, 128, 16)
            if not bkm and N <= 64 and ntiles(128, 64) >= K_MIN_TILES:
                return tile(SPLIT, 128, 64, 16)
            if Kd % 32 == 0:
                Tg = gemm_grid(M // 64, N // 64)
                ns = xs_splits(Tg, Kd, 32, K_XS_CAP)
                if ns > 1 and xs_buffer(exchange_ok, (M // 64) * (N // 64)):
                    return _form(SPLIT, 64, 64, 32, 0, Tg * ns, xs=ns, kchunk=Kd // ns)
                return tile(SPLIT, 64, 64, 32)
            return tile(SPLIT, 64, 64, 16)
    if bkm and not big:
        return tile(F32, 64, 64, BKS)
    if big:
        return tile(F32, 128, 128, BKS)
    if N <= 64 and ntiles(128, 64) >= K_MIN_TILES:
        return tile(F32, 128, 64, BKS)
    return tile(F32, 64, 64, BKS)


def launch_gemm(bkm, M, N, Kd, lda, ldb, ldc, aligned, mode, exchange_ok):
    whole = (M % 128 == 0 and N % 64 == 0 and (N <= 64 or N % 128 == 0) and Kd % BKS == 0
             and lda % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0 and aligned)
    return launch_gemm_tiles(bkm, not whole, M, N, Kd, mode, exchange_ok)


def pointwise_gemm(R, Cin, Cout, trans_w, aligned, mode, exchange_ok):
    """sph3d_pointwise_gemm"""
    if trans_w:
        return launch_gemm(True, R, Cout, Cin, Cin, Cin, Cout, aligned, mode, exchange_ok)
    return launch_gemm(False, R, Cout, Cin, Cin, Cout, Cout, aligned, mode, exchange_ok)


def nn_stats_tile(M, N, Kd):
    """-> (row blocks, bm, bn); 0 blocks: the shape does not qualify"""
    whole = M % 128 == 0 and N % 64 == 0 and (N <= 64 or N % 128 == 0) and Kd % BKS == 0 and Kd % 4 == 0 and N % 4 == 0
    if not whole:
        return 0, 0, 0

    def ntiles(a, b):
        return ((M + a - 1) // a) * ((N + b - 1) // b)
    if N > 64 and ntiles(128, 128) >= K_MIN_TILES:
        bm, bn = 128, 128
    elif ntiles(128, 64) >= K_MIN_TILES:
        bm, bn = 128, 64
    else:
        bm, bn = 64, 64
    return 2 * (M // bm), bm, bn


def bnstats_blocks(R, Cin, Cout):
    """sph3d_pointwise_gemm_bnstats_blocks"""
    return nn_stats_tile(R, Cout, Cin)[0] if R > 0 and Cin > 0 and Cout > 0 else 0


def pointwise_gemm_bnstats(R, Cin, Cout, aligned, mode, exchange_ok):
    """sph3d_pointwise_gemm_bnstats; grid 0: SPH3D_EUNSUPPORTED, nothing is launched"""
    nblk, bm, bn = nn_stats_tile(R, Cout, Cin)
    if nblk == 0 or not aligned:
        return _form(0, 0, 0, 0, 0, 0, stats=1, stats_blocks=nblk)
    tiles = gemm_grid(R // bm, Cout // bn)
    if mode:
        if bm == 128:
            return _form(SPLIT, 128, bn, 16, 0, tiles, stats=1, stats_blocks=nblk)
        if Cin % 32 == 0:
            ns = xs_splits(tiles, Cin, 32, K_XS_CAP)
            if ns > 1 and xs_buffer(exchange_ok, (R // 64) * (Cout // 64)):
                return _form(SPLIT, 64, 64, 32, 0, tiles * ns, stats=1, xs=ns, kchunk=Cin // ns, stats_blocks=nblk)
            return _form(SPLIT, 64, 64, 32, 0, tiles, stats=1, stats_blocks=nblk)
        return _form(SPLIT, 64, 64, 16, 0, tiles, stats=1, stats_blocks=nblk)
    return _form(F32, bm, bn, BKS, 0, tiles, stats=1, stats_blocks=nblk)


def tn_plan(R, Cin, Cout):
    """-> (bn, tiles, nsplit, kchunk)"""
    bn = 128 if Cout > 64 else 64
    tiles = ((Cin + BM - 1) // BM) * ((Cout + bn - 1) // bn)
    target = 256 if (R <= 12288 and tiles <= 16) else 512
    want = (target + tiles - 1) // tiles
    maxsplit = (R + 255) // 256
    nsplit = max(min(want, maxsplit), 1)
    kchunk = (R + nsplit - 1) // nsplit
    kchunk = ((kchunk + BKL - 1) // BKL) * BKL
    nsplit = (R + kchunk - 1) // kchunk
    return bn, tiles, nsplit, kchunk


def tn_workspace(R, Cin, Cout):
    """sph3d_pointwise_gemm_tn_workspace"""
    nsplit = tn_plan(R, Cin, Cout)[2]
    return 4 * nsplit * Cin * Cout if nsplit > 1 else 0


def pointwise_gemm_tn(R, Cin, Cout, aligned, mode, exchange_ok):
    """sph3d_pointwise_gemm_tn (every pointer — X, dY, dW, the workspace — aligned, or not)"""
    bn, tiles, nsplit, kchunk = tn_plan(R, Cin, Cout)
    whole = Cin % 128 == 0 and Cout % bn == 0 and R % kchunk == 0 and aligned
    if mode and R <= K_TN_XS_ROWS and Cin % 64 == 0 and Cout % 64 == 0 and R % 32 == 0 and aligned:
        Tg = gemm_grid(Cin // 64, Cout // 64)
        ns = xs_splits(Tg, R, 32, K_TN_XS_CAP)
        if ns > 1 and xs_buffer(exchange_ok, (Cin // 64) * (Cout // 64)):
            return _form(SPLIT, 64, 64, 32, 0, Tg * ns, xs=ns, kchunk=R // ns)
    slab = dict(grid=gemm_grid(tiles, 1, nsplit), nsplit=nsplit, kchunk=kchunk, reduce=int(nsplit > 1))
    if whole and mode:
        return _form(SPLIT, 128, bn, 16, 0, **slab)
    if not whole and mode and Cin >= 32 and Cout >= 32:
        return _form(SPLIT, 128, bn, 16, 1, **slab)
    if whole:
        return _form(F32, 128, bn, BKS, 0, **slab)
    return _form(F32, 128, bn, BKL, 1, **slab)


def tag(product, f):
    """the name of a launch form: product, pipe, tile, and what else the launch does"""
    if f["grid"] == 0:
        return NAMES[product] + " none"
    return "%s %s %dx%dx%d%s%s%s" % (NAMES[product], "split" if f["pipe"] == SPLIT else "f32", f["bm"], f["bn"], f["bk"],
                                     " guard" if f["guard"] else "", " xs%d" % f["xs"] if f["xs"] > 1 else "",
                                     " +reduce" if f["reduce"] else "")


def form(product, R, Cin, Cout, aligned, mode, exchange_ok):
    """-> the fields of FIELDS and "tag" """
    if product == NN:
        f = pointwise_gemm(R, Cin, Cout, 0, aligned, mode, exchange_ok)
    elif product == NT:
        f = pointwise_gemm(R, Cin, Cout, 1, aligned, mode, exchange_ok)
    elif product == NNS:
        f = pointwise_gemm_bnstats(R, Cin, Cout, aligned, mode, exchange_ok)
    else:
        f = pointwise_gemm_tn(R, Cin, Cout, aligned, mode, exchange_ok)
    f["tag"] = tag(product, f)
    return f


# ---- the grid on which the query is held to the restatement, and on which the forms are counted ---------------------------------
GRID_R = (1, 31, 32, 64, 100, 128, 256, 777, 1000, 1024, 2048, 2080, 4096, 4100, 6144, 12288, 12289, 32768, 65536, 80000, 131072,
          320000)
GRID_C = (3, 13, 16, 31, 32, 33, 35, 48, 64, 67, 70, 96, 128, 131, 144, 192, 256, 262, 384, 512, 1024, 2048)


def grid():
    for product in (NN, NT, NNS, TN):
        for R in GRID_R:
            for Cin in GRID_C:
                for Cout in GRID_C:
                    for aligned in (0, 1):
                        for mode in (0, 1):
                            for exchange_ok in (0, 1):
                                yield product, R, Cin, Cout, aligned, mode, exchange_ok


# ---- the case list -----------------------------------------------------------------------------------------------------------------
# For every form (tag) the grid reaches, the smallest shape that reaches it: (tag, product, R, Cin, Cout, aligned, mode, exchange_ok).
# Every form is reachable with aligned operands and a stream that supplies the exchange buffer: misaligned operands take the guarded
# forms that ragged dimensions take, and a stream without a buffer takes a form without the exchange — the same tile and k-step
# (NN, NT, NNS) or the slab plan (TN) — that other shapes reach anyway.  Whole 128 x 128 tiles need 512 of them (kMinTiles): 8.4 M
# outputs, the list's largest operand; the 128 x 64 forms need 65536 rows (65409 ragged), the guarded 128 x 128 ones 32641 x 129.
# Off the grid the exchange also runs with other split counts (3 at Cin = 768; 2 .. 8 for TN): the same kernels, another argument.
FORM_CASES = [
    ("NN f32 128x128x16", NN, 4096, 16, 2048, 1, 0, 1),
    ("NN f32 128x128x16 guard", NN, 32641, 3, 129, 1, 1, 1),
    ("NN f32 128x64x16", NN, 65536, 16, 64, 1, 0, 1),
    ("NN f32 128x64x16 guard", NN, 65409, 3, 3, 1, 1, 1),
    ("NN f32 64x64x16", NN, 128, 16, 64, 1, 0, 1),
    ("NN f32 64x64x16 guard", NN, 1, 3, 3, 1, 1, 1),
    ("NN split 128x128x16", NN, 4096, 16, 2048, 1, 1, 1),
    ("NN split 128x128x16 guard", NN, 32641, 16, 129, 1, 1, 1),
    ("NN split 128x64x16", NN, 65536, 16, 64, 1, 1, 1),
    ("NN split 128x64x16 guard", NN, 65409, 16, 32, 1, 1, 1),
    ("NN split 64x64x16", NN, 128, 16, 64, 1, 1, 1),
    ("NN split 64x64x16 guard", NN, 1, 16, 32, 1, 1, 1),
    ("NN split 64x64x32", NN, 128, 32, 64, 1, 1, 1),
    ("NN split 64x64x32 xs2", NN, 128, 512, 64, 1, 1, 1),
    ("NN split 64x64x32 xs4", NN, 128, 1024, 64, 1, 1, 1),
    ("NT f32 128x128x16", NT, 4096, 16, 2048, 1, 0, 1),
    ("NT f32 128x128x16 guard", NT, 32641, 3, 129, 1, 1, 1),
    ("NT f32 64x64x16", NT, 128, 16, 64, 1, 0, 1),
    ("NT f32 64x64x16 guard", NT, 1, 3, 3, 1, 1, 1),
    ("NT split 128x128x16", NT, 4096, 16, 2048, 1, 1, 1),
    ("NT split 128x128x16 guard", NT, 32641, 16, 129, 1, 1, 1),
    ("NT split 64x64x16", NT, 128, 16, 64, 1, 1, 1),
    ("NT split 64x64x16 guard", NT, 1, 16, 32, 1, 1, 1),
    ("NT split 64x64x32", NT, 128, 32, 64, 1, 1, 1),
    ("NT split 64x64x32 xs2", NT, 128, 512, 64, 1, 1, 1),
    ("NT split 64x64x32 xs4", NT, 128, 1024, 64, 1, 1, 1),
    ("NNS none", NNS, 1, 3, 3, 1, 1, 1),
    ("NNS f32 128x128x16", NNS, 4096, 16, 2048, 1, 0, 1),
    ("NNS f32 128x64x16", NNS, 2048, 16, 2048, 1, 0, 1),
    ("NNS f32 64x64x16", NNS, 128, 16, 64, 1, 0, 1),
    ("NNS split 128x128x16", NNS, 4096, 16, 2048, 1, 1, 1),
    ("NNS split 128x64x16", NNS, 2048, 16, 2048, 1, 1, 1),
    ("NNS split 64x64x16", NNS, 128, 16, 64, 1, 1, 1),
    ("NNS split 64x64x32", NNS, 128, 32, 64, 1, 1, 1),
    ("NNS split 64x64x32 xs2", NNS, 128, 512, 64, 1, 1, 1),
    ("NNS split 64x64x32 xs4", NNS, 128, 1024, 64, 1, 1, 1),
    ("TN f32 128x128x16", TN, 32, 128, 128, 1, 0, 1),
    ("TN f32 128x128x16 +reduce", TN, 320, 128, 128, 1, 0, 1),
    ("TN f32 128x128x32 guard", TN, 1, 3, 65, 1, 1, 1),
    ("TN f32 128x128x32 guard +reduce", TN, 257, 3, 65, 1, 1, 1),
    ("TN f32 128x64x16", TN, 32, 128, 64, 1, 0, 1),
    ("TN f32 128x64x16 +reduce", TN, 320, 128, 64, 1, 0, 1),
    ("TN f32 128x64x32 guard", TN, 1, 3, 3, 1, 1, 1),
    ("TN f32 128x64x32 guard +reduce", TN, 257, 3, 3, 1, 1, 1),
    ("TN split 128x128x16", TN, 32, 128, 128, 1, 1, 1),
    ("TN split 128x128x16 +reduce", TN, 320, 128, 128, 1, 1, 1),
    ("TN split 128x128x16 guard", TN, 1, 32, 65, 1, 1, 1),
    ("TN split 128x128x16 guard +reduce", TN, 257, 32, 65, 1, 1, 1),
    ("TN split 128x64x16", TN, 32, 128, 64, 1, 1, 1),
    ("TN split 128x64x16 +reduce", TN, 320, 128, 64, 1, 1, 1),
    ("TN split 128x64x16 guard", TN, 1, 32, 32, 1, 1, 1),
    ("TN split 128x64x16 guard +reduce", TN, 257, 32, 32, 1, 1, 1),
    ("TN split 64x64x32 xs4", TN, 1024, 64, 64, 1, 1, 1),
    ("TN split 64x64x32 xs8", TN, 2048, 64, 64, 1, 1, 1),
]
