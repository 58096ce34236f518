// lovasz_plan.hpp — everything the host decides about a Lovasz-softmax call that sorts in global memory (lovasz.hip:
// sph3d_lovasz_softmax_large), stated once: lovasz_large_plan().  The entry launches what the plan says,
// sph3d_lovasz_softmax_large_workspace reads its size from it, and sph3d_lovasz_softmax_large_plan reports it field by field
// (tests/test_lovasz_large.py holds that report to tests/_lovasz_large_forms.py, the launcher restated in Python).  Plain C++ in
// 64-bit integers: nothing of HIP is included, no global and no environment is read, so a host program can compile it alone
// (tools/lovasz_plan_sweep.cpp, built with the sanitizers).
//
// A (class, block) pair is a SEGMENT of npad = runs * tile keys (the rows past N are zero keys, below every valid key):
//   run sort   one workgroup per (run, class, block) sorts `tile` keys in LDS and writes them to key buffer 0
//   merge      `passes` = ceil(log2(runs)) launches; pass p merges neighbouring runs of tile << p keys (the last one may be
//              shorter or alone) from one key buffer into the other, a workgroup per output tile of kLovMergeTile keys
//   finish     the foreground count of every output tile, then one pass over the sorted keys that takes its exclusive prefix
//              from those counts, and one wave per segment that adds the tiles' partial sums
// Classes go through these launches `slab` at a time, so the key buffers hold slab * B segments, not C * B.
#pragma once

namespace sph3d {

constexpr int kLovLargeMaxN = 1 << 20;      // U, U - 1 and G - F stay exactly convertible to fp32 factors of one rounded product
constexpr int kLovLargeMaxC = 1024;         // the label histogram of the count kernel (static LDS), as kLovMaxC
constexpr int kLovMinTileLog2 = 10, kLovMaxTileLog2 = 14;
// The run length by default: 4096 keys are 32 KB.  A CU holds 2048 threads, i.e. two of the 1024-thread sort workgroups, and
// both fit its 160 KB of LDS with room to spare (64 KB); no launch has to raise the 64 KB a kernel gets without asking.  16384
// keys (128 KB, what lovasz_sort_kernel takes) leave ONE workgroup per CU, whose barriers then idle the CU, and the bitonic
// network's log2(tile)^2 / 2 stages grow where a merge pass costs one read and one write of the keys whatever the run length.
constexpr int kLovDefaultTileLog2 = 12;
constexpr int kLovMergeTile = 1024;         // keys of an output tile of the merge, the tile count and the finish (<= every tile)
constexpr int kLovSortBlock = 1024, kLovMergeBlock = 256, kLovCountRows = 4096;
// The workspace cap.  At 16 x 65536 x 21 a class takes 16 segments of 65536 keys in two buffers, 16 MB, all classes 336 MB, next
// to the call's own probs and coef of 88 MB each.  128 MB hold 7 classes there: three slabs of 7 classes, each 1792 sort
// workgroups and 7168 merge workgroups per launch on 256 CUs, so a slab loses nothing to a short grid, and the workspace stays
// below what the caller already spends on probs and coef.  A call whose single class exceeds the cap runs with slab 1.
constexpr long long kLovWsCap = 128LL << 20;
constexpr long long kLovMaxElems = 1LL << 40;       // B N C, as sph3d_lovasz_softmax

enum { kLovOk = 0, kLovBadDims, kLovBadSize, kLovBigN, kLovBigC, kLovBadTile, kLovBadSlab };       // LovaszPlan::bad

struct LovaszPlan {         // (the order of sph3d_lovasz_softmax_large_plan's output, up to `bad`)
    long long tile_log2, tile;          // keys of a sorted run (0: B == 0, nothing is launched and every field is 0)
    long long runs, npad;               // runs per segment, ceil(N / tile), and keys per segment, runs * tile
    long long passes;                   // merge launches per slab, ceil(log2(runs))
    long long mtile, mtiles;            // keys of an output tile, and output tiles per segment, npad / mtile
    long long slab, slabs;              // classes per pass, and passes over the classes, ceil(C / slab)
    long long probs_grid;               // lovasz_probs_kernel: workgroups of 256 rows
    long long count_grid;               // lovasz_large_count_kernel: workgroups of kLovCountRows rows per block (grid count_grid x B)
    long long sort_lds, merge_lds;      // bytes: dynamic LDS of the run sort, static LDS of the merge
    long long grad_grid;                // lovasz_large_grad_kernel with dlogits: workgroups of 1024 rows per block
    long long key_bufs;                 // 1: one run per segment, nothing is merged; 2 otherwise
    long long workspace_bytes;          // device memory the call needs and the byte offsets into it:
    long long off_keys0, off_keys1;     // keys [slab][B][npad] uint64, twice (off_keys1 == off_keys0 if key_bufs == 1)
    long long off_tilecnt, off_partial; // foreground count int32 and partial sum fp32 of every output tile [slab][B][mtiles]
    long long off_count, off_bad;       // G [B][C] int32 and the bad flag [B] int32 (one zero fill covers both)
    long long cap;                      // kLovWsCap
    int bad;                            // (not reported)
};

static inline LovaszPlan lovasz_large_plan(int B_, int N_, int C_, int tile_log2, int slab_)
{
    LovaszPlan p = {};
    const long long B = B_, N = N_, C = C_;         // (every product below: in 64 bits)
    if (!(B >= 0 && N > 0 && C > 0)) { p.bad = kLovBadDims; return p; }
    // (in this order: B C < 2^31 keeps the triple product inside 64 bits)
    if (!(B <= 65535 && B * C <= 0x7fffffffLL && B * C * N <= kLovMaxElems)) { p.bad = kLovBadSize; return p; }
    if (!(N <= kLovLargeMaxN)) { p.bad = kLovBigN; return p; }
    if (!(C <= kLovLargeMaxC)) { p.bad = kLovBigC; return p; }
    if (!(tile_log2 == 0 || (tile_log2 >= kLovMinTileLog2 && tile_log2 <= kLovMaxTileLog2))) { p.bad = kLovBadTile; return p; }
    if (!(slab_ >= 0 && slab_ <= C)) { p.bad = kLovBadSlab; return p; }
    if (B == 0) return p;
    p.tile_log2 = tile_log2 ? tile_log2 : kLovDefaultTileLog2;
    p.tile = 1LL << p.tile_log2;
    p.runs = (N + p.tile - 1) / p.tile;
    p.npad = p.runs * p.tile;
    while ((1LL << p.passes) < p.runs) p.passes++;
    p.mtile = kLovMergeTile;
    p.mtiles = p.npad / kLovMergeTile;
    p.key_bufs = p.passes > 0 ? 2 : 1;
    const long long fixed = 4 * B * C + 4 * B;                                       // G and the bad flags
    const long long per_class = B * (p.key_bufs * 8 * p.npad + 8 * p.mtiles);        // keys, tile counts and partial sums
    if (slab_ > 0) {
        p.slab = slab_;
    } else {
        p.slab = (kLovWsCap - fixed - 255) / per_class;
        if (p.slab < 1) p.slab = 1;
        if (p.slab > C) p.slab = C;
    }
    p.slabs = (C + p.slab - 1) / p.slab;
    p.probs_grid = (B * N + 255) / 256;
    p.count_grid = (N + kLovCountRows - 1) / kLovCountRows;
    p.sort_lds = 8 * p.tile;
    p.merge_lds = 8 * kLovMergeTile;
    p.grad_grid = (N + 1023) / 1024;
    const long long keys = 8 * p.slab * B * p.npad, words = 4 * p.slab * B * p.mtiles;
    p.off_keys0 = 0;
    p.off_keys1 = p.key_bufs == 2 ? keys : 0;
    p.off_tilecnt = p.key_bufs * keys;
    p.off_partial = p.off_tilecnt + words;
    p.off_count = p.off_partial + words;
    p.off_bad = p.off_count + 4 * B * C;
    p.workspace_bytes = (p.off_bad + 4 * B + 255) & ~255LL;
    p.cap = kLovWsCap;
    return p;
}

}  // namespace sph3d
