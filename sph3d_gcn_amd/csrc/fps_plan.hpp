// fps_plan.hpp — everything the host decides about a farthest-point sampling call (sample.hip), stated once: fps_plan().
// sph3d_farthest_point_sample launches what the plan says, sph3d_farthest_point_sample_workspace reads its size from it, and
// sph3d_farthest_point_sample_plan reports it field by field (tests/test_fps_forms.py holds that report to tests/_fps_forms.py, the
// launcher restated in Python as it stood before the choice was gathered here).  Plain C++ in 64-bit integers: nothing of HIP is
// included, no global and no environment is read, so a host program can compile it alone (tools/fps_plan_sweep.cpp, built with the
// sanitizers).  What is NOT here: which XCD an XCD-local co-operative launch starts on (a counter of the launcher's that advances
// once per launch) and the forced time-out of the test hook.
#pragma once

namespace sph3d {

constexpr int kFpsRefBlock = 1024;          // common.hpp's kRefBlock: thread t of the reference owns points t, t + 1024, ... (sample.hip asserts it)
constexpr int kFpsMaxPoints = 1024 * 256;   // the tie rule's k >> 10 travels in 8 bits
constexpr int kFpsMaxRegPoints = 24;        // points per thread that fps_reg_kernel holds in registers
// cloud sizes the pruned kernel takes when more than one sample is asked for (at 2048 points it only ties with the plain kernel:
// 0.620 vs 0.614 us per round)
constexpr int kFpsPruneMin = 2049, kFpsPruneMax = 16384;
constexpr int kFpsCoopPts = 1024 * 4;       // points per workgroup of the co-operative kernel (sample.hip: kCoopPts)
constexpr int kFpsCoopMaxGroups = 64;       // workgroups per cloud: one lane of wave 0 polls each
constexpr int kFpsCoopMaxBlocks = 128;      // b * G workgroups that must be resident at once (half of the 256 CUs)
constexpr int kFpsCoopXcdBlocks = 16;       // ceil(b / 8) * G up to which a cloud's workgroups share an XCD (half of its 32 CUs)
constexpr int kFpsBigGrid = 64;             // workgroups of fps_big_kernel; cloud i + 64 is workgroup i's next one
constexpr long long kFpsSlotsOffset = 256;  // the co-operative kernel's granules behind its error word

enum { kFpsNone = 0, kFpsPlain, kFpsPruned, kFpsCoop, kFpsBig };                  // FpsPlan::kernel
enum { kFpsOk = 0, kFpsBadSamples, kFpsBadShape, kFpsBadPoints };                 // FpsPlan::bad: why the entry answers SPH3D_EINVAL

struct FpsPlan {            // (the order of sph3d_farthest_point_sample_plan's output, up to `bad`)
    long long kernel;                   // kFpsNone: b == 0, nothing is launched
    long long P;                        // fps_reg_kernel<P> / fps_prune_kernel<P, 16>: points per thread / lane; 0 for the other two
    long long block, grid;              // threads per workgroup, workgroups of the first launch
    long long G;                        // workgroups per cloud (1 but for the co-operative kernel)
    long long xcd_local;                // co-operative: a cloud's G workgroups on one XCD (the grid is 8 ceil(b / 8) G, the surplus leaves)
    long long repair;                   // co-operative: fps_big_kernel is queued behind it, gated on the error word
    long long big_grid;                 // workgroups of fps_big_kernel (as the repair pass or alone), 0 where it is not launched
    long long workspace_bytes;          // device memory the call needs, and the byte offsets into it:
    long long off_err, off_slots, off_temp;         // error word, granules [b][2][G] (co-operative), running distances [big_grid][n]
    int bad;                            // (not reported)
};

static inline FpsPlan fps_plan(int b_, int n_, int m_)
{
    FpsPlan p = {};
    const long long b = b_, n = n_, m = m_;                  // (every product below: in 64 bits)
    if (!(m > 0)) { p.bad = kFpsBadSamples; return p; }                         // tf_sample.cpp:35
    if (!(b >= 0 && n > 0)) { p.bad = kFpsBadShape; return p; }
    if (!(n <= kFpsMaxPoints)) { p.bad = kFpsBadPoints; return p; }
    const long long need = (n + kFpsRefBlock - 1) / kFpsRefBlock;               // points per thread of the reference's mapping
    const long long rows = b < kFpsBigGrid ? b : kFpsBigGrid;
    long long G = 0;
    if (need > kFpsMaxRegPoints) {
        // ---- beyond the registers of one workgroup: the co-operative kernel while all b * G workgroups can be resident, with the
        // running distances of its repair pass behind its own memory; fps_big_kernel alone otherwise
        const long long g = (n + kFpsCoopPts - 1) / kFpsCoopPts;
        if (g <= kFpsCoopMaxGroups && b * g <= kFpsCoopMaxBlocks) G = g;
        if (G) p.off_temp = (kFpsSlotsOffset + 8 * b * 2 * G + 255) & ~255LL;
        p.workspace_bytes = p.off_temp + 4 * rows * n;
    }
    if (b == 0) {                       // (a co-operative shape still answers its 256-byte head, as the size query always did)
        p.off_temp = 0;
        return p;
    }
    p.block = kFpsRefBlock;
    p.grid = b;
    p.G = 1;
    if (n >= kFpsPruneMin && n <= kFpsPruneMax && m > 1) {
        p.kernel = kFpsPruned;
        p.P = need <= 4 ? 4 : (need <= 8 ? 8 : 16);
    } else if (need <= kFpsMaxRegPoints) {
        p.kernel = kFpsPlain;
        p.P = need <= 2 ? need : (need <= 4 ? 4 : (need <= 8 ? 8 : (need <= 12 ? 12 : (need <= 16 ? 16 : 24))));
        if (n < kFpsRefBlock) p.block = (n + 63) / 64 * 64;
    } else if (G) {
        const long long rounds8 = (b + 7) / 8;
        p.kernel = kFpsCoop;
        p.G = G;
        // all workgroups of a cloud on one XCD while they take at most half of its 32 CUs (one 1024-thread workgroup per CU);
        // 32 per XCD measured slower than spread: 2.88 vs 2.46 us per round at 131 072 points
        p.xcd_local = rounds8 * G <= kFpsCoopXcdBlocks;
        p.grid = p.xcd_local ? 8 * rounds8 * G : b * G;
        p.repair = 1;
        p.big_grid = rows;
        p.off_slots = kFpsSlotsOffset;
    } else {
        p.kernel = kFpsBig;
        p.grid = p.big_grid = rows;
    }
    return p;
}

}  // namespace sph3d
