"""The host side of pooling and un-pooling, restated in Python: what the entry points of csrc/pool3d.hip launch for a call, as
their launchers stood before the choice was gathered in csrc/pool_plan.hpp (pool_plan).  tests/test_pool_forms.py holds the
library's query sph3d_pool3d_plan to plan() below, field for field; the GPU tests read the form a case reaches from that query
(query() and the *_form functions at the end) and assert it.  Python integers do not overflow: every product here is the exact one."""
import ctypes

FIELDS = ("kernel", "V", "pairs", "passes", "ppwg", "parts", "grid", "grid_y", "block", "lds", "zero_bytes", "blocks_wanted", "blocks_cap")
FWD, SUM_GRAD_T, MAX_GRAD, MAX_GRAD_T, MAX_GRAD_ROWS, NARROW, NARROW_GRAD_T = range(7)                 # op
OPS = (FWD, SUM_GRAD_T, MAX_GRAD, MAX_GRAD_T, MAX_GRAD_ROWS, NARROW, NARROW_GRAD_T)
(NONE, GATHER_FWD_HALF, GATHER_FWD, GATHER_BWD_T, GATHER_BWD_T_SPLIT, MAXPOOL_BWD, MAXPOOL_BWD_T, MAXPOOL_BWD_ROWS, NARROW_INTERP_FWD,
 NARROW_INTERP_BWD_T) = range(10)                                                                      # kernel
BAD_OP, BAD_DIMS, BAD_SEGMENTS, BAD_BATCH, WIDE, BAD_GRID = "op", "dims", "N F", "batch", "C > 16", "grid"
STATUS = {BAD_OP: -1, BAD_DIMS: -1, BAD_SEGMENTS: -1, BAD_BATCH: -1, WIDE: -4, BAD_GRID: -1}         # SPH3D_EINVAL, SPH3D_EUNSUPPORTED

INT_MAX = (1 << 31) - 1
HUGE = 1 << 62                      # conv_plan.hpp: products of dimensions are held there
MODES = ("max", "avg", "weighted")

# every kernel instantiation csrc/pool3d.hip launches
INSTANTIATIONS = ({("gather_fwd_half", m) for m in MODES} | {("gather_fwd", m, v) for m in MODES for v in (4, 1)} |
                  {(k, v) for k in ("gather_bwd_t", "gather_bwd_t_split", "maxpool_bwd_t", "maxpool_bwd_rows") for v in (4, 1)} |
                  {("maxpool_bwd",), ("narrow_interp_fwd", True), ("narrow_interp_fwd", False), ("narrow_interp_bwd_t",)})


def xcd_grid(B, parts):
    """common.hpp: workgroups of a launch that deals `parts` parts of each of B clouds to the 8 XCDs"""
    ls = 0 if B >= 5 else 1 if B >= 3 else 2 if B == 2 else 3
    return 8 * -(-B // (8 >> ls)) * ((parts + (1 << ls) - 1) >> ls)


def _mul(a, b):
    return HUGE if b != 0 and a > HUGE // b else a * b


def _launch_fwd(p, B, Nin, Mout, C, K):
    if not (B >= 0 and Nin > 0 and Mout >= 0 and C > 0 and K > 0):
        return BAD_DIMS
    if B == 0 or Mout == 0:
        return p
    ppwg = 16 if B * Mout >= 65536 else 4
    mblocks = (Mout + ppwg - 1) // ppwg
    p.update(ppwg=ppwg, parts=mblocks, grid=xcd_grid(B, mblocks), grid_y=1, block=256)
    if C % 4 == 0 and C <= 128:
        p.update(kernel=GATHER_FWD_HALF, V=4, pairs=1, passes=1)
    elif C % 4 == 0:
        p.update(kernel=GATHER_FWD, V=4, passes=-(-C // 256))
    else:
        p.update(kernel=GATHER_FWD, V=1, passes=-(-C // 64))
    return p


def _launch_bwd_t(p, B, Nin, Mout, C):
    if not (B >= 0 and Nin > 0 and Mout >= 0 and C > 0):
        return BAD_DIMS
    if B == 0:
        return p
    V = 4 if C % 4 == 0 else 1
    p.update(V=V, passes=-(-C // (64 * V)), grid_y=1, block=256)
    if B * Nin <= 65536 and Mout >= 2 * Nin:
        p.update(kernel=GATHER_BWD_T_SPLIT, pairs=int(V == 4 and C <= 128), ppwg=1, parts=Nin, grid=B * Nin, lds=4 * 64 * V * 4)
    else:
        nblocks = (Nin + 15) // 16
        p.update(kernel=GATHER_BWD_T, ppwg=16, parts=nblocks, grid=xcd_grid(B, nblocks))
    return p


def _max_grad(p, B, N, M, C):
    if not (B >= 0 and N > 0 and M >= 0 and C > 0):
        return BAD_DIMS
    if B == 0:
        return p
    p["zero_bytes"] = _mul(_mul(4 * B, N), C)
    per_b = M * C
    if per_b == 0:
        return p
    if not B <= 65535:
        return BAD_BATCH
    blocks = (per_b + 255) // 256
    cap = max((8192 + B - 1) // B, 1)
    p.update(kernel=MAXPOOL_BWD, blocks_wanted=blocks, blocks_cap=cap, parts=min(blocks, cap), grid=min(blocks, cap), grid_y=B, block=256)
    return p


def _max_grad_gather(p, kernel, B, N, M, C, F):
    if not (B >= 0 and N > 0 and M >= 0 and C > 0 and (kernel == MAXPOOL_BWD_T or F > 0)):
        return BAD_DIMS
    if kernel == MAXPOOL_BWD_ROWS and not N * F < 0x7fffffff:
        return BAD_SEGMENTS
    if B == 0:
        return p
    ppwg = 16 if B * N >= 65536 else 4
    nblocks = (N + ppwg - 1) // ppwg
    V = 4 if C % 4 == 0 else 1
    p.update(kernel=kernel, V=V, passes=-(-C // (64 * V)), ppwg=ppwg, parts=nblocks, grid=xcd_grid(B, nblocks), grid_y=1, block=256)
    return p


def _narrow(p, forward, B, Nin, Mout, C, K):
    """forward: the entry names the Mout rows N and the Nin sources M"""
    if not (B >= 0 and Mout >= 0 and Nin > 0 and C > 0 and (K > 0 or not forward)):
        return BAD_DIMS
    if C > 16:
        return WIDE
    items, per = (B * Mout, 16) if forward else (B * Nin, 4)
    if items == 0:                  # (the gradient: B == 0, Nin is positive)
        return p
    p.update(kernel=NARROW_INTERP_FWD if forward else NARROW_INTERP_BWD_T, passes=1, ppwg=per, grid=min((items + per - 1) // per, 65536),
             grid_y=1, block=256)
    return p


def plan(op, B, Nin, Mout, C, K=1, F=1):
    """-> the fields, or why the call is refused (STATUS)"""
    p = dict.fromkeys(FIELDS, 0)
    if op == FWD:
        p = _launch_fwd(p, B, Nin, Mout, C, K)
    elif op == SUM_GRAD_T:
        p = _launch_bwd_t(p, B, Nin, Mout, C)
    elif op == MAX_GRAD:
        p = _max_grad(p, B, Nin, Mout, C)
    elif op in (MAX_GRAD_T, MAX_GRAD_ROWS):
        p = _max_grad_gather(p, MAXPOOL_BWD_T if op == MAX_GRAD_T else MAXPOOL_BWD_ROWS, B, Nin, Mout, C, F)
    elif op in (NARROW, NARROW_GRAD_T):
        p = _narrow(p, op == NARROW, B, Nin, Mout, C, K)
    else:
        return BAD_OP
    # the one rule the launchers did not have: a grid.x that is no int is refused, where it used to wrap
    if not isinstance(p, str) and p["grid"] > INT_MAX:
        return BAD_GRID
    return p


def instantiations(p, modes=MODES, weighted=(True, False)):
    """the kernels a plan (a dict of FIELDS) launches; modes: of the forward entries called with it; weighted: narrow calls with
    (True) and without (False) a weight array"""
    k, V = p["kernel"], p["V"]
    if k == NONE:
        return set()
    if k == GATHER_FWD_HALF:
        return {("gather_fwd_half", m) for m in modes}
    if k == GATHER_FWD:
        return {("gather_fwd", m, V) for m in modes}
    if k == NARROW_INTERP_FWD:
        return {("narrow_interp_fwd", w) for w in weighted}
    if k in (MAXPOOL_BWD, NARROW_INTERP_BWD_T):
        return {("maxpool_bwd" if k == MAXPOOL_BWD else "narrow_interp_bwd_t",)}
    return {({GATHER_BWD_T: "gather_bwd_t", GATHER_BWD_T_SPLIT: "gather_bwd_t_split", MAXPOOL_BWD_T: "maxpool_bwd_t",
              MAXPOOL_BWD_ROWS: "maxpool_bwd_rows"}[k], V)}


# ---- the library's answer ------------------------------------------------------------------------------------------------------
_fn = []


def query(op, B, Nin, Mout, C, K=1, F=1):
    """sph3d_pool3d_plan -> the fields as a dict, or the status of a refusal.  No device is touched."""
    if not _fn:
        from sph3d_gcn_amd import _lib
        fn = ctypes.CDLL(_lib.LIB_PATH).sph3d_pool3d_plan
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.c_void_p]
        _fn.append(fn)
    out = (ctypes.c_longlong * len(FIELDS))()
    rc = _fn[0](op, B, Nin, Mout, C, K, F, ctypes.addressof(out))
    assert rc in (0, -1, -4), (op, B, Nin, Mout, C, K, F, rc)
    return dict(zip(FIELDS, out)) if rc == 0 else rc


def fwd_form(B, Mout, C):
    """-> (kernel, points per workgroup) of the forward entries"""
    p = query(FWD, B, 1, Mout, C)
    return ("gather_fwd_half" if p["kernel"] == GATHER_FWD_HALF else "gather_fwd<%d>" % p["V"]), p["ppwg"]


def bwd_t_form(B, Nin, Mout, C):
    p = query(SUM_GRAD_T, B, Nin, Mout, C)
    if p["kernel"] == GATHER_BWD_T_SPLIT:
        return "split pairs" if p["pairs"] else "split<%d> %d passes" % (p["V"], p["passes"])
    assert p["kernel"] == GATHER_BWD_T
    return "gather_bwd_t<%d>" % p["V"]


def scatter_blocks(B, M, C):
    """-> (blocks the elements ask for, the cap)"""
    p = query(MAX_GRAD, B, 1, M, C)
    assert p["kernel"] == MAXPOOL_BWD and p["grid"] == min(p["blocks_wanted"], p["blocks_cap"]) and p["grid_y"] == B
    return p["blocks_wanted"], p["blocks_cap"]


def max_t_form(B, N, C):
    p = query(MAX_GRAD_T, B, N, 1, C)
    assert p["kernel"] == MAXPOOL_BWD_T
    return "maxpool_bwd_t<%d>" % p["V"], p["ppwg"]


def max_rows_form(B, N, C, F):
    p = query(MAX_GRAD_ROWS, B, N, 1, C, F=F)
    assert p["kernel"] == MAXPOOL_BWD_ROWS
    return "maxpool_bwd_rows<%d>" % p["V"], p["ppwg"]
