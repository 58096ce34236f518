"""The launchers' rules of csrc/conv3d.hip, restated (copied from the launchers: which kernel, which plan, which table a call takes),
and the case lists of tests/test_gpu_conv_forms.py that are chosen by those rules.  Plain Python: no torch, no library, so the
CPU test of the case lists' coverage (tests/test_conv_ref.py) and the GPU tests share one statement."""
import os

from _conv_ref import reduce_depth

# ---- the launchers' rules (conv3d.hip) -----------------------------------------------------------------------------------------
K_SLICE, K_COMPACT_BINS, K_HUB_WG, K_BWD_POINTS_PER_WG, K_BWD_WAVES, K_BWD_FILL_WG = 256, 17, 1024, 64, 4, 128


def dims_ok(F, C, r):
    """conv_dims_ok: the filter table slice fits LDS"""
    return F * min(C * r, K_SLICE) * 4 <= 160 * 1024


def fwd_form(N, F, C, r):
    """sph3d_depthwise_conv3d"""
    vec = C % 4 == 0 and r in (1, 2)
    multi_ok = vec and N <= (1 << 24) and F <= 254 and N * C * 4 + 1024 < (1 << 32)
    if multi_ok and C <= 128:
        return "dwconv_fwd_multi<%d,%d>" % (r, 32 if C > 64 else 16)
    if vec and N * C + 256 < (1 << 32):
        return "dwconv_fwd_row<%d>" % r
    return "dwconv_fwd_generic"


def vec_plan(F, CR, r):
    """-> V, channels per lane; 0: dwconv_bwd_t_generic"""
    if r not in (1, 2):
        return 0
    if F <= 33 and CR % 4 == 0:
        return 4
    if F <= 65 and CR % 2 == 0:
        return 2
    return 0


def bwd_parts(V, CR):
    """run_bwd_t_vec: PARTS"""
    return 1 if V == 2 else 4 if CR <= 64 else 2 if CR <= 128 else 1


def bwd_plan(B, N, nslices, wg_per_cu):
    """-> (parts, W, slabs)"""
    g = B & 7
    g = 8 if g == 0 else (g & -g)
    parts = 8 // g
    if parts > N:
        parts = 1
    items_per_xcd = (B * parts + 7) // 8
    src = items_per_xcd * ((N + parts - 1) // parts)
    w_work = (src + K_BWD_POINTS_PER_WG - 1) // K_BWD_POINTS_PER_WG
    w_fill = max((K_BWD_FILL_WG if wg_per_cu >= 4 else 64) // max(nslices, 1), 1)
    w_min = (src + 2 * K_BWD_WAVES - 1) // (2 * K_BWD_WAVES)
    w = max(min(w_fill, w_min), w_work)
    W = max(1, min(w, 32 * wg_per_cu))
    return parts, W, 8 * W


def bwd_layout(B, N, F, C, r):
    V = vec_plan(F, C * r, r)
    if not V:
        return dict(V=0, bytes=0)
    nslices = (C * r + 64 * V - 1) // (64 * V)
    full, compact = bwd_plan(B, N, nslices, 3), bwd_plan(B, N, nslices, 4)
    hub_list_offset = 4 * (max(full[2], compact[2]) + K_HUB_WG) * F * C * r
    return dict(V=V, nslices=nslices, full=full, compact=compact, hub_list_offset=hub_list_offset,
                bytes=hub_list_offset + 4 * (B * N + 4))


def hub_min_n():
    return int(os.environ.get("SPH3D_BWD_HUB_MIN_N", 32768))


def hub_threshold():
    return max(int(os.environ.get("SPH3D_BWD_HUB_T", 1024)), 1)


def grad_form(B, N, M, F, C, r, active_given, A):
    """sph3d_depthwise_conv3d_grad_t, launch_bwd_t_vec and the kernels' own choice between the two tables -> a dict; "tag" names
    the launch form.  With active_bins given for a V = 4 shape the launcher starts BOTH the compact and the full instantiation
    (the host cannot read the count without a sync) and each returns at once unless the count is in its range: "compact" /
    "full" names the one that does the work.  "hub" stands for the pair of launches HUB = 1 (sweep) and HUB = 2 (hub kernel)."""
    L = bwd_layout(B, N, F, C, r)
    if not (L["V"] and M * C * r + 256 < (1 << 32)):
        return dict(kernel="generic", V=0, hub=False, depth=B * ((N + 63) // 64), tag="bwd generic")
    V, MAXF = L["V"], (33 if L["V"] == 4 else 65)
    compact_launch = active_given and V == 4 and MAXF > K_COMPACT_BINS and F <= 63           # the compact condition (host)
    compact = compact_launch and A <= K_COMPACT_BINS                                           # ... and on the device
    hub = V == 4 and N >= hub_min_n()                                                          # the hub condition
    plan = L["compact"] if compact else L["full"]
    slabs = plan[2] + (K_HUB_WG if hub else 0)                                                 # what reduce_filter_partials reads
    parts = bwd_parts(V, C * r)
    return dict(kernel="vec", V=V, PARTS=parts, compact=compact, hub=hub, plan=plan, slabs=slabs, depth=reduce_depth(slabs),
                tag="bwd R%d V%d PARTS%d %s%s" % (r, V, parts, "compact" if compact else "full", " hub" if hub else ""))


def cat_ok(F, Ca, Cb, r):
    C = Ca + Cb
    return (Ca > 0 and Cb > 0 and r in (1, 2) and C % 4 == 0 and C > 128 and (Ca * r) % K_SLICE == 0
            and vec_plan(F, C * r, r) == 4)


# ---- the case lists ------------------------------------------------------------------------------------------------------------------
FWD_CASES = ([("dwconv_fwd_multi<%d,16>" % r, C, r, 33) for C in (4, 60, 64) for r in (1, 2)]
             + [("dwconv_fwd_multi<%d,32>" % r, C, r, 33) for C in (68, 128) for r in (1, 2)]
             + [("dwconv_fwd_multi<2,16>", 64, 2, 254), ("dwconv_fwd_row<2>", 64, 2, 255)]
             + [("dwconv_fwd_row<2>", 132, 2, 33), ("dwconv_fwd_row<2>", 256, 2, 33), ("dwconv_fwd_row<1>", 260, 1, 33)]
             + [("dwconv_fwd_generic", C, r, 33) for C in (3, 35, 67) for r in (1, 2)]
             + [("dwconv_fwd_generic", 6, 4, 33), ("dwconv_fwd_generic", 100, 3, 33)])

#            C, r -> C r in {4, 64} (PARTS 4), {68, 128} (PARTS 2), {132, 256, 512} (PARTS 1)
PLAN_CASES = [(2, 2, 4), (32, 2, 4), (4, 1, 4), (64, 1, 4), (34, 2, 2), (64, 2, 2), (68, 1, 2), (128, 1, 2),
              (66, 2, 1), (128, 2, 1), (256, 2, 1), (132, 1, 1), (256, 1, 1), (512, 1, 1)]

V2_CASES = [(6, 1, 33), (3, 2, 33), (8, 2, 34), (64, 1, 34), (8, 1, 49), (64, 2, 49), (4, 2, 65), (130, 1, 65)]

HUB_CASES = [(8, 2, 4), (16, 1, 4), (34, 2, 2), (128, 1, 2), (66, 2, 1), (132, 1, 1)]
