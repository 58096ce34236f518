"""The launch plan of the odd-width conv gradient (csrc/conv3d.hip: odd_layout, run_bwd_t_odd, dwconv_bwd_t_odd), restated: which
shapes it serves in deterministic mode, T channels per lane, the channel slices, the slabs reduce_filter_partials adds and the
workspace bytes.  Plain Python, copied from the launcher; tests/test_gpu_conv_odd.py compares the bytes with the library's answer
and takes the reduce depth of its float64 bound from here."""
from _conv_forms import bwd_plan, vec_plan
from _conv_ref import reduce_depth


def odd_layout(B, N, F, C, r):
    """-> dict(T=0) for a shape the plan does not serve, else T, nslices, plan = (parts, W, slabs), bytes"""
    if r != 1 or C % 2 == 0 or F > 65:
        return dict(T=0, bytes=0)
    tmax = 4 if F <= 33 else 2
    T = min((C + 63) // 64, tmax)
    nslices = (C + 64 * T - 1) // (64 * T)
    plan = bwd_plan(B, N, nslices, 3)
    return dict(T=T, MAXF=33 if F <= 33 else 65, nslices=nslices, plan=plan, bytes=4 * plan[2] * F * C)


def odd_form(B, N, M, F, C, r, deterministic):
    """sph3d_depthwise_conv3d_grad_t for a shape without a vec_plan -> a dict like _conv_forms.grad_form's: kernel "odd" (mode on,
    served), "generic" (mode off: no workspace) or "refused" (mode on, not served)"""
    assert vec_plan(F, C * r, r) == 0, "the vector kernels take this shape in and out of the mode"
    L = odd_layout(B, N, F, C, r)
    if not deterministic:
        return dict(kernel="generic", bytes=0, depth=B * ((N + 63) // 64), tag="bwd generic")
    if not (L["T"] and M * C * r + 256 < (1 << 32)):
        return dict(kernel="refused", bytes=L["bytes"])
    slabs = L["plan"][2]
    return dict(kernel="odd", T=L["T"], MAXF=L["MAXF"], nslices=L["nslices"], plan=L["plan"], slabs=slabs, depth=reduce_depth(slabs),
                bytes=L["bytes"], tag="bwd odd T%d MAXF%d slices%d" % (L["T"], L["MAXF"], L["nslices"]))
