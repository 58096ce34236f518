"""The host rules of the depthwise convolution and its gradient, restated, and the case lists of tests/test_gpu_conv_forms.py and
tests/test_gpu_conv_odd.py that are chosen by those rules.  The rule functions are copied from the launchers of csrc/conv3d.hip
as they stood before the choice was gathered into one function (csrc/conv_plan.hpp: conv_plan, which every entry point launches
from); plan() puts them together in the order the entry points applied them, and tests/test_conv_forms.py holds the library's
query (sph3d_depthwise_conv3d_plan) to it field for field.  Three clauses are not the old launchers' and are marked (new): the LDS
clause of the forward choice, and two that turn integer overflow in the old launchers into SPH3D_EINVAL.  Python integers do not
overflow, so this is the exact statement.  Plain Python: no torch, no library, so the CPU tests and the GPU tests share it."""
import os

from _conv_ref import reduce_depth

# ---- the launchers' rules (conv3d.hip) -----------------------------------------------------------------------------------------
K_SLICE, K_COMPACT_BINS, K_HUB_WG, K_BWD_POINTS_PER_WG, K_BWD_WAVES, K_BWD_FILL_WG = 256, 17, 1024, 64, 4, 128
LDS, INT_MAX = 160 * 1024, (1 << 31) - 1


def dims_ok(F, C, r):
    """conv_dims_ok: the filter table slice fits LDS"""
    return F * min(C * r, K_SLICE) * 4 <= LDS


def xcd_grid(B, parts):
    """common.hpp: workgroups of a launch that deals `parts` parts of each of B clouds to the 8 XCDs"""
    ls = 0 if B >= 5 else 1 if B >= 3 else 2 if B == 2 else 3
    s, cpr = 1 << ls, 8 >> ls
    return 8 * ((B + cpr - 1) // cpr) * ((parts + s - 1) >> ls)


def fwd_lds(kernel, F, C, r):
    """dynamic LDS bytes of the three forward launches (multi, row: + the zero row of the padding slots)"""
    if kernel == FWD_MULTI:
        return (F + 1) * (128 if C > 64 else 64) * r * 4
    return (F + (kernel == FWD_ROW)) * min(C * r, K_SLICE) * 4


def fwd_kernel(N, F, C, r):
    """sph3d_depthwise_conv3d"""
    vec = C % 4 == 0 and r in (1, 2)
    multi_ok = vec and N <= (1 << 24) and F <= 254 and N * C * 4 + 1024 < (1 << 32)
    if multi_ok and C <= 128 and fwd_lds(FWD_MULTI, F, C, r) <= LDS:           # (new) the LDS clause
        return FWD_MULTI
    if vec and N * C + 256 < (1 << 32) and fwd_lds(FWD_ROW, F, C, r) <= LDS:   # (new) the LDS clause
        return FWD_ROW
    return FWD_GENERIC


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


def odd_layout(B, N, F, C, r):
    """the odd-width gradient's plan (deterministic mode) -> dict(T=0) for a shape it does not serve, else T, nslices,
    plan = (parts, W, slabs), bytes"""
    if r != 1 or C % 2 == 0 or F > 65:
        return dict(T=0, bytes=0)
    tmax = 4 if F <= 33 else 2
    T = min((C + 63) // 64, tmax)
    nslices = (C + 64 * T - 1) // (64 * T)
    plan = bwd_plan(B, N, nslices, 3)
    return dict(T=T, MAXF=33 if F <= 33 else 65, nslices=nslices, plan=plan, bytes=4 * plan[2] * F * C)


def hub_min_n():
    return int(os.environ.get("SPH3D_BWD_HUB_MIN_N", 32768))


def hub_threshold():
    return max(int(os.environ.get("SPH3D_BWD_HUB_T", 1024)), 1)


def cat_ok(F, Ca, Cb, r):
    C = Ca + Cb
    return (Ca > 0 and Cb > 0 and r in (1, 2) and C % 4 == 0 and C > 128 and (Ca * r) % K_SLICE == 0
            and vec_plan(F, C * r, r) == 4)


# ---- the plan: the rules above in the order the entry points applied them ------------------------------------------------------
# the order in which sph3d_depthwise_conv3d_plan writes its output, the values of `kernel` and of `op`
FIELDS = ("kernel", "R", "LPE", "V", "MAXF", "PARTS", "nslices", "compact_launch", "hub", "hub_threshold", "full_parts", "full_W",
          "full_slabs", "compact_parts", "compact_W", "compact_slabs", "reduce_slabs", "reduce_slabs_compact", "lds", "grid",
          "hub_list_offset", "workspace_bytes")
NONE, FWD_MULTI, FWD_ROW, FWD_GENERIC, BWD_VEC, BWD_ODD, BWD_GENERIC, REFUSED = range(8)
FWD, FWD_CAT, GRAD_T, GRAD_T_CAT = range(4)


def plan(op, B, N, M, F, Ca, Cb, r, K, deterministic, active_given, hub_n=None, hub_t=None):
    """what the entry point `op` does with these dimensions -> a dict of FIELDS, or None where it answers SPH3D_EINVAL.  kernel
    REFUSED: SPH3D_EUNSUPPORTED; NONE: nothing is launched.  hub_n, hub_t: the hub hooks' values (None: the environment's)"""
    grad, cat = op in (GRAD_T, GRAD_T_CAT), op in (FWD_CAT, GRAD_T_CAT)
    C = Ca + Cb
    CR = C * r
    if not (B >= 0 and N > 0 and M >= 0 and F > 0 and C > 0 and r > 0 and (grad or K > 0)):
        return None
    if CR > INT_MAX:                                                              # (new) C r is an int in every kernel
        return None
    if not dims_ok(F, C, r):
        return None
    p = dict.fromkeys(FIELDS, 0)
    if cat and not (cat_ok(F, Ca, Cb, r) and (M * CR if grad else N * C) + 256 < (1 << 32)):
        return dict(p, kernel=REFUSED)
    if not grad:
        kernel = FWD_ROW if cat else fwd_kernel(N, F, C, r)
        nslices = 1 if kernel == FWD_MULTI else (CR + K_SLICE - 1) // K_SLICE
        grid = xcd_grid(B, ((M + 31) // 32) * nslices)
        if grid > INT_MAX:                                                        # (new) the grid is an int
            return None
        if B == 0 or M == 0:
            return p
        return dict(p, kernel=kernel, R=r, LPE=(32 if C > 64 else 16) if kernel == FWD_MULTI else 0, nslices=nslices,
                    lds=fwd_lds(kernel, F, C, r), grid=grid)
    L = bwd_layout(B, N, F, C, r)
    if L["V"] and M * CR + 256 < (1 << 32):
        V = L["V"]
        MAXF = 33 if V == 4 else 65
        compact_launch = bool(active_given) and V == 4 and MAXF > K_COMPACT_BINS and F <= 63      # the compact condition
        hub = V == 4 and not deterministic and N >= (hub_min_n() if hub_n is None else hub_n)    # the hub condition
        hub_slabs = K_HUB_WG if hub else 0
        full, compact = L["full"], L["compact"]
        p.update(kernel=BWD_VEC, R=r, V=V, MAXF=MAXF, PARTS=bwd_parts(V, CR), nslices=L["nslices"], compact_launch=int(compact_launch),
                 hub=int(hub), hub_threshold=(hub_threshold() if hub_t is None else hub_t) if hub else 0,
                 full_parts=full[0], full_W=full[1], full_slabs=full[2], compact_parts=compact[0], compact_W=compact[1],
                 compact_slabs=compact[2], reduce_slabs=full[2] + hub_slabs,
                 reduce_slabs_compact=(compact[2] if compact_launch else 0) + hub_slabs, lds=F * min(CR, 64 * V) * 4,
                 grid=full[2] * L["nslices"], hub_list_offset=L["hub_list_offset"], workspace_bytes=L["bytes"])
    elif deterministic:
        O = odd_layout(B, N, F, C, r)
        if not (O["T"] and M * CR + 256 < (1 << 32)):
            return dict(p, kernel=REFUSED if B > 0 else NONE)
        t = O["plan"]
        p.update(kernel=BWD_ODD, R=1, V=O["T"], MAXF=O["MAXF"], PARTS=1, nslices=O["nslices"], full_parts=t[0], full_W=t[1],
                 full_slabs=t[2], reduce_slabs=t[2], lds=F * 64 * O["T"] * 4, grid=t[2] * O["nslices"], workspace_bytes=O["bytes"])
    else:
        if r > 256:
            return None if B > 0 else p
        sliceC = min(max(256 // r, 1), C)
        nslices = (C + sliceC - 1) // sliceC
        p.update(kernel=BWD_GENERIC, R=r, nslices=nslices, lds=F * sliceC * r * 4, grid=xcd_grid(B, ((N + 63) // 64) * nslices))
    if p["grid"] > INT_MAX:                                                       # (new) the grid is an int
        return None
    if B == 0:
        return dict(dict.fromkeys(FIELDS, 0), workspace_bytes=p["workspace_bytes"])
    return p


def fwd_form(N, F, C, r):
    """sph3d_depthwise_conv3d -> the instantiation's name"""
    p = plan(FWD, 1, N, 1, F, C, 0, r, 1, False, False)
    return {FWD_MULTI: "dwconv_fwd_multi<%d,%d>" % (r, p["LPE"]), FWD_ROW: "dwconv_fwd_row<%d>" % r, FWD_GENERIC: "dwconv_fwd_generic"}[p["kernel"]]


def grad_form(B, N, M, F, C, r, active_given, A):
    """sph3d_depthwise_conv3d_grad_t with deterministic mode off, and the kernels' own choice between the two tables -> a dict;
    "tag" names the launch form.  With active_bins given for a V = 4 shape the launcher starts BOTH the compact and the full
    instantiation (the host cannot read the count without a sync) and each returns at once unless the count is in its range:
    "compact" / "full" names the one that does the work.  "hub" stands for the pair of launches HUB = 1 (sweep) and HUB = 2 (hub
    kernel)."""
    p = plan(GRAD_T, B, N, M, F, C, 0, r, 1, False, active_given)
    if p["kernel"] != BWD_VEC:
        assert p["kernel"] == BWD_GENERIC
        return dict(kernel="generic", V=0, hub=False, depth=B * ((N + 63) // 64), tag="bwd generic")
    compact = bool(p["compact_launch"]) and A <= K_COMPACT_BINS                                # ... and on the device
    t = "compact" if compact else "full"
    slabs = p["reduce_slabs_compact"] if compact else p["reduce_slabs"]                         # what reduce_filter_partials reads
    return dict(kernel="vec", V=p["V"], PARTS=p["PARTS"], compact=compact, hub=bool(p["hub"]),
                plan=(p[t + "_parts"], p[t + "_W"], p[t + "_slabs"]), slabs=slabs, depth=reduce_depth(slabs),
                tag="bwd R%d V%d PARTS%d %s%s" % (r, p["V"], p["PARTS"], t, " hub" if p["hub"] else ""))


def odd_form(B, N, M, F, C, r, deterministic):
    """sph3d_depthwise_conv3d_grad_t for a shape without a vec_plan -> a dict like grad_form's: kernel "odd" (mode on, served),
    "generic" (mode off: no workspace) or "refused" (mode on, not served); bytes: what the workspace query answers"""
    assert vec_plan(F, C * r, r) == 0, "the vector kernels take this shape in and out of the mode"
    p = plan(GRAD_T, B, N, M, F, C, 0, r, 1, deterministic, True)
    nbytes = plan(GRAD_T, B, N, 0, F, C, 0, r, 1, deterministic, True)["workspace_bytes"]
    if p["kernel"] == BWD_GENERIC:
        return dict(kernel="generic", bytes=nbytes, depth=B * ((N + 63) // 64), tag="bwd generic")
    if p["kernel"] == REFUSED:
        return dict(kernel="refused", bytes=nbytes)
    assert p["kernel"] == BWD_ODD
    slabs = p["reduce_slabs"]
    return dict(kernel="odd", T=p["V"], MAXF=p["MAXF"], nslices=p["nslices"], plan=(p["full_parts"], p["full_W"], p["full_slabs"]),
                slabs=slabs, depth=reduce_depth(slabs), bytes=nbytes, tag="bwd odd T%d MAXF%d slices%d" % (p["V"], p["MAXF"], p["nslices"]))


# ---- the case lists ------------------------------------------------------------------------------------------------------------------
FWD_CASES = ([("dwconv_fwd_multi<%d,16>" % r, C, r, 33) for C in (4, 60, 64) for r in (1, 2)]
             + [("dwconv_fwd_multi<%d,32>" % r, C, r, 33) for C in (68, 128) for r in (1, 2)]
             + [("dwconv_fwd_multi<2,16>", 64, 2, 254), ("dwconv_fwd_row<2>", 64, 2, 255)]
             # 160 bins: the multi kernel's table, (F + 1) x 128 r floats whatever C is, passes 160 KiB; the row kernel's fits
             + [("dwconv_fwd_row<2>", 68, 2, 160), ("dwconv_fwd_row<2>", 124, 2, 160)]
             + [("dwconv_fwd_row<2>", 132, 2, 33), ("dwconv_fwd_row<2>", 256, 2, 33), ("dwconv_fwd_row<1>", 260, 1, 33)]
             + [("dwconv_fwd_generic", C, r, 33) for C in (3, 35, 67) for r in (1, 2)]
             + [("dwconv_fwd_generic", 6, 4, 33), ("dwconv_fwd_generic", 100, 3, 33)])

#            C, r -> C r in {4, 64} (PARTS 4), {68, 128} (PARTS 2), {132, 256, 512} (PARTS 1)
PLAN_CASES = [(2, 2, 4), (32, 2, 4), (4, 1, 4), (64, 1, 4), (34, 2, 2), (64, 2, 2), (68, 1, 2), (128, 1, 2),
              (66, 2, 1), (128, 2, 1), (256, 2, 1), (132, 1, 1), (256, 1, 1), (512, 1, 1)]

V2_CASES = [(6, 1, 33), (3, 2, 33), (8, 2, 34), (64, 1, 34), (8, 1, 49), (64, 2, 49), (4, 2, 65), (130, 1, 65)]

HUB_CASES = [(8, 2, 4), (16, 1, 4), (34, 2, 2), (128, 1, 2), (66, 2, 1), (132, 1, 1)]

# odd widths (r = 1): T = 1, 1, 1, 1, 2, 2, 3, 4 and 4 with a second slice of one channel
ODD_CHANNELS = [1, 3, 35, 63, 65, 67, 131, 255, 257]
