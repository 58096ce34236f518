"""The launchers' rules of csrc/sepring.hip and csrc/sepconv.hip, restated (copied from the launchers as they stood before the
choice was gathered into csrc/sepconv.hpp: sep_plan — which of the three one-kernel separable layers a call takes, which
instantiation, which ring depth or tile height, and how the 256 workgroups share the row blocks or tiles), and the case lists of
tests/test_gpu_sep_forms.py that are chosen by those rules.  Plain Python: no torch, no library, so the CPU test of the case lists'
coverage (tests/test_sep_ref.py) and the GPU tests share one statement; tests/test_sep_forms.py holds the library's host-only
query (sph3d_separable_conv3d_plan) to plan() below, field for field.

  sepconv_ring_kernel<R, LPE, KT, TRAIN>   sepring.hip   tag "ring<R,LPE,KT> NBn Gg wrapw"   (training: "train<R,LPE,KT> ...")
      NB ring slots, G = 16 / (Cout / 16) wave groups, w = how often the busiest workgroup comes back to a slot it has used
  sepconv_fused_kernel<R, LPE, KT>         sepconv.hip   tag "small<R,LPE,KT>"
  sepconv_general_kernel<R, LPE, RBK>      sepconv.hip   tag "general<R,LPE,RBK> slicesn"
"""
from collections import namedtuple

LDS = 160 * 1024
WORKGROUPS, WAVES, SR_ROWS, SC_TILE = 256, 16, 16, 32


# ---- sepring.hip -------------------------------------------------------------------------------------------------------------------
def lpe_of(C):
    return 16 if C <= 64 else 32


def sr_filter_floats(F, C, r):
    return (F + 1) * 4 * lpe_of(C) * r


def sr_ktp(C, r):
    KT = (C * r + 15) // 16
    return 4 if KT <= 4 else (8 if KT <= 8 else 16)


def sr_ring_depth(F, C, r):
    """as many 16-point row blocks as fit beside the filter table (at most 8); 0: fewer than three"""
    rb = 4 * SR_ROWS * (sr_ktp(C, r) * 16 + 4)
    fixed = 4 * sr_filter_floats(F, C, r) + 256
    if fixed + 3 * rb > LDS:
        return 0
    return min((LDS - fixed) // rb, 8)


def _common_ok(N, F, C, r, K):
    return r in (1, 2) and C % 4 == 0 and C >= 4 and F <= 254 and N <= (1 << 24) and K > 0 and N * C * 4 + 1024 < (1 << 32)


def sr_shape_ok(N, F, C, r, K, Cout):
    return (_common_ok(N, F, C, r, K) and C <= 128 and C * r <= 256 and Cout in (16, 32, 64, 128, 256)
            and sr_ring_depth(F, C, r) >= 3)


# ---- sepconv.hip -------------------------------------------------------------------------------------------------------------------
def sc_small_lds(F, C, r):
    return 4 * ((F + 1) * 4 * lpe_of(C) * r + 2 * SC_TILE * (sr_ktp(C, r) * 16 + 4))


def sc_shape_ok(N, F, C, r, K, Cout):
    return (_common_ok(N, F, C, r, K) and sc_small_lds(F, C, r) <= LDS and C <= 128 and C * r <= 256
            and Cout % 16 == 0 and 16 <= Cout <= 128)


def sc_general_lds(F, C, r, rbk):
    lpe = lpe_of(C)
    return 4 * ((F + 1) * 4 * lpe * r + 16 * rbk * (4 * lpe * r + 4))


def sc_general_ok(N, F, C, r, K, Cout):
    return (_common_ok(N, F, C, r, K) and sc_general_lds(F, C, r, 1) <= LDS and (C <= 128 or (C % 128 == 0 and C <= 4096))
            and Cout % 16 == 0 and 16 <= Cout <= 512)


def general_rbk(B, M, F, C, r):
    """sc_launch_general: -> (tile height by point count, tile height after the LDS step-down)"""
    pts = B * M
    by_points = 4 if pts >= 64 * 512 else (2 if pts >= 32 * 256 else 1)
    rbk = by_points
    while rbk > 1 and sc_general_lds(F, C, r, rbk) > LDS:
        rbk >>= 1
    return by_points, rbk


def fused_supported(N, F, C, r, K, Cout):
    """sph3d_separable_conv3d_fused_supported"""
    return sc_shape_ok(N, F, C, r, K, Cout) or sc_general_ok(N, F, C, r, K, Cout)


# ---- the workgroup partition (the same lines in all three kernels) ------------------------------------------------------------------
def partition(B, per_cloud):
    """-> one list per workgroup (blockIdx.x = 0 .. 255) of its units (cloud b, unit index inside the cloud); a unit is a 16-point
    row block (ring) or a tile (small: 32 points, general: 16 RBK points), per_cloud of them in a cloud"""
    WPX = WORKGROUPS >> 3
    affine = (B & 7) == 0
    out = []
    for blk in range(WORKGROUPS):
        xcd, wi = blk & 7, blk >> 3
        if affine:
            total, part, parts = (B >> 3) * per_cloud, wi, WPX
        else:
            total, part, parts = B * per_cloud, xcd * WPX + wi, 8 * WPX
        j_begin, j_end = total * part // parts, total * (part + 1) // parts
        units = []
        for j in range(j_begin, j_end):
            cl, u = divmod(j, per_cloud)
            units.append((xcd + 8 * cl if affine else cl, u))
        out.append(units)
    return out


def wave_groups(Cout):
    return WAVES // (Cout >> 4)


# the order in which sph3d_separable_conv3d_plan writes its output; kernel: 0 unsupported, 1 ring, 2 small, 3 general
FIELDS = ("kernel", "R", "LPE", "KT", "RBK", "rbk_by_points", "NB", "G", "lds", "grid", "stats_blocks")
UNSUPPORTED, RING, SMALL, GENERAL = range(4)


def plan(train, B, N, M, F, C, r, K, Cout):
    """what sph3d_separable_conv3d_train (train = 1) or sph3d_separable_conv3d_fused (0) launches -> a dict of FIELDS (all 0:
    SPH3D_EUNSUPPORTED; grid 0: nothing is launched).  No partition(): cheap enough for a grid of shapes"""
    p = dict.fromkeys(FIELDS, 0)
    ring, small = sr_shape_ok(N, F, C, r, K, Cout), sc_shape_ok(N, F, C, r, K, Cout)
    if not ring if train else not (small or sc_general_ok(N, F, C, r, K, Cout)):
        return p
    p.update(R=r, LPE=lpe_of(C), grid=WORKGROUPS if train or (B > 0 and M > 0) else 0)
    if ring:
        NB, KT = sr_ring_depth(F, C, r), sr_ktp(C, r)
        p.update(kernel=RING, KT=KT, NB=NB, G=wave_groups(Cout), stats_blocks=train_blocks(Cout) if train else 0,
                 lds=4 * (sr_filter_floats(F, C, r) + NB * SR_ROWS * (KT * 16 + 4)) + 4 * (2 + 2 * NB))
    elif small:
        p.update(kernel=SMALL, KT=sr_ktp(C, r), lds=sc_small_lds(F, C, r))
    else:
        by_points, rbk = general_rbk(B, M, F, C, r)
        p.update(kernel=GENERAL, RBK=rbk, rbk_by_points=by_points, lds=sc_general_lds(F, C, r, rbk))
    return p


def _ring_form(kind, p, B, M):
    NB, G = p["NB"], p["G"]
    per_wg = [len(u) for u in partition(B, (M + SR_ROWS - 1) // SR_ROWS)]
    nrb_max = max(per_wg)
    wrap = max(nrb_max - 1, 0) // NB
    inst = (p["R"], p["LPE"], p["KT"])
    return dict(kernel=kind, inst=inst, NB=NB, G=G, nrb_max=nrb_max, wrap=wrap, idle=per_wg.count(0), units=sum(per_wg),
                affine=(B & 7) == 0, tag="%s<%d,%d,%d> NB%d G%d wrap%d" % ((kind,) + inst + (NB, G, wrap)))


def infer_form(B, N, M, F, C, r, K, Cout):
    """sph3d_separable_conv3d_fused -> a dict; "tag" names the launch form ("unsupported": SPH3D_EUNSUPPORTED, "empty": nothing is
    launched)"""
    p = plan(0, B, N, M, F, C, r, K, Cout)
    if p["kernel"] == UNSUPPORTED:
        return dict(kernel="unsupported", tag="unsupported")
    if p["grid"] == 0:
        return dict(kernel="empty", tag="empty")
    if p["kernel"] == RING:
        return _ring_form("ring", p, B, M)
    affine = (B & 7) == 0
    if p["kernel"] == GENERAL:
        rbk, lpe = p["RBK"], p["LPE"]
        per_wg = [len(u) for u in partition(B, (M + 16 * rbk - 1) // (16 * rbk))]
        nslices = (C + 4 * lpe - 1) // (4 * lpe)
        return dict(kernel="general", inst=(r, lpe, rbk), rbk=rbk, rbk_by_points=p["rbk_by_points"], nslices=nslices, ncb=Cout >> 4,
                    partial_slice=C % (4 * lpe) != 0, idle=per_wg.count(0), units=sum(per_wg), affine=affine,
                    tag="general<%d,%d,%d> slices%d" % (r, lpe, rbk, nslices))
    per_wg = [len(u) for u in partition(B, (M + SC_TILE - 1) // SC_TILE)]
    inst = (p["R"], p["LPE"], p["KT"])
    return dict(kernel="small", inst=inst, idle=per_wg.count(0), units=sum(per_wg), affine=affine, tag="small<%d,%d,%d>" % inst)


def train_form(B, N, M, F, C, r, K, Cout):
    """sph3d_separable_conv3d_train: the ring kernel or SPH3D_EUNSUPPORTED; B = 0 or M = 0 still launch (all-zero partial rows)"""
    p = plan(1, B, N, M, F, C, r, K, Cout)
    if p["kernel"] == UNSUPPORTED:
        return dict(kernel="unsupported", tag="unsupported")
    return _ring_form("train", p, B, M)


def train_blocks(Cout):
    """sph3d_separable_conv3d_train_blocks: rows of the partial statistics"""
    if Cout < 16 or Cout > 256 or Cout & (Cout - 1):
        return 0
    return WORKGROUPS * wave_groups(Cout)


# ---- the reachable instantiations -------------------------------------------------------------------------------------------------
# (R, LPE, KT) of the ring and the small kernel: LPE follows C (16: C <= 64), KT the padded C r / 16
TRIPLES = {(1, 16, 4): (4, 64, 1), (2, 16, 4): (4, 32, 2), (2, 16, 8): (36, 64, 2), (1, 32, 8): (68, 128, 1),
           (2, 32, 16): (68, 128, 2)}                                  # -> (smallest C, largest C, r)
GENERAL_INSTS = [(R, lpe, rbk) for R in (1, 2) for lpe in (16, 32) for rbk in (1, 2, 4)]
# the triples no (C, r) yields, which the library does not contain: C <= 64 gives C r <= 128 (KT <= 8), and r = 1 with C <= 64
# gives KT <= 4; C >= 68 gives KT >= 5 (r = 1: <= 8) and, r = 2, KT >= 9
UNREACHED_TRIPLES = [(1, 16, 8), (1, 16, 16), (2, 16, 16), (1, 32, 4), (1, 32, 16), (2, 32, 4), (2, 32, 8)]


def reachable_triples():
    """every (R, LPE, KT) some supported (C, r) gives: computed, to hold TRIPLES to the rules"""
    got = {}
    for r in (1, 2):
        for C in range(4, 129, 4):
            if C * r <= 256:
                t = (r, lpe_of(C), sr_ktp(C, r))
                lo, hi, _ = got.get(t, (C, C, r))
                got[t] = (min(lo, C), max(hi, C), r)
    return got


# ---- the case lists --------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "kind B N M F C r K Cout tag")            # kind: "infer" | "train"; tag: the form the case is meant for


def case_id(c):
    return "%s-B%d-M%d-F%d-C%d-r%d-K%d-Co%d" % (c.kind, c.B, c.M, c.F, c.C, c.r, c.K, c.Cout)


def form_of(c):
    return (infer_form if c.kind == "infer" else train_form)(c.B, c.N, c.M, c.F, c.C, c.r, c.K, c.Cout)


def _mk(kind, B, N, M, F, C, r, K, Cout):
    c = Case(kind, B, N, M, F, C, r, K, Cout, None)
    return c._replace(tag=form_of(c)["tag"])


SMALL_GEOM = (3, 150, 107, 33, 12)                                    # B, N, M, F, K: 321 points, M = 6 * 16 + 11 < N


def _small(kind, C, r, Cout, F=None):
    B, N, M, F0, K = SMALL_GEOM
    return _mk(kind, B, N, M, F0 if F is None else F, C, r, K, Cout)


# every reachable form at a small shape: the smallest and the largest C of the form
RING_FORM_CASES = [_small(kind, C, r, Cout) for kind in ("infer", "train") for (lo, hi, r) in TRIPLES.values()
                   for C, Cout in ((lo, 16), (lo, 256), (hi, 64))]
SMALL_FORM_CASES = [_small("infer", C, r, Cout) for (lo, hi, r) in TRIPLES.values() for C, Cout in ((lo, 48), (lo, 112), (hi, 96))]
GENERAL_FORM_CASES = [_small("infer", C, r, Cout) for r in (1, 2)
                      for C, Cout in ((4, 144), (4, 512), (64, 272), (68, 144), (68, 512), (128, 272), (256, 16))]

# ring slot reuse: (2,32,16) beside 100 bins has three slots; 28672 points are seven row blocks per workgroup (epochs 0..2), with
# more wave groups than slots (Cout = 16) and with one (Cout = 256), not affine (B = 7) and affine (B = 8); and one form with eight
# slots whose workgroups get ten or eleven row blocks
RING_REUSE_CASES = ([_mk(kind, B, M + 64, M, 100, 68, 2, 8, Cout) for kind in ("infer", "train") for B, M in ((7, 4096), (8, 3584))
                     for Cout in (16, 256)]
                    + [_mk(kind, 5, 8300, 8200, 33, 8, 1, 8, 64) for kind in ("infer", "train")])

# the general kernel's tile height by point count (both LPE, both R; the narrowest input of the form), lowered by LDS beside 120
# and 130 bins (which also is the step from the ring to the general kernel at F >= 111), two and three slices, a partial slice
GENERAL_RBK_CASES = [_mk("infer", 3, M + 40, M, 33, C, r, 8, 144) for r in (1, 2) for C in (8, 68) for M in (2739, 10925)]
GENERAL_LDS_CASES = [_mk("infer", 3, 10965, 10925, F, 68, 2, 8, 64) for F in (120, 130)]
GENERAL_SLICE_CASES = [_small("infer", C, r, Cout) for C, r, Cout in ((256, 2, 144), (384, 1, 272), (384, 2, 512), (100, 1, 144),
                                                                      (36, 2, 144), (100, 2, 272))]

# the partition: B in {1, 3, 8, 9, 16}; B = 1, M = 40 is three row blocks in the whole launch; B = 16, M = 600 gives a workgroup two
# or three row blocks of one cloud or of two
PARTITION_GEOMS = [(1, 40), (3, 107), (8, 75), (9, 257), (16, 600)]
PARTITION_CASES = [_mk(kind, B, M + 24, M, 33, 16, 2, 12, Cout) for B, M in PARTITION_GEOMS
                   for kind, Cout in (("infer", 32), ("train", 32), ("infer", 48), ("infer", 144))]

# counts above 64: the second and third trip of the kt loop
K130_CASES = [_mk(kind, 2, 160, 43, 33, C, r, 130, Cout)
              for kind, C, r, Cout in (("infer", 64, 2, 128), ("train", 128, 1, 64), ("infer", 32, 2, 96), ("infer", 128, 2, 144))]

# one form per kernel for out-of-range bin ids and for a non-finite input
EDGE_CASES = [_small(kind, C, r, Cout) for kind, C, r, Cout in (("infer", 36, 2, 64), ("train", 68, 1, 32), ("infer", 64, 1, 80),
                                                                ("infer", 100, 2, 272))]

ALL_CASES = (RING_FORM_CASES + SMALL_FORM_CASES + GENERAL_FORM_CASES + RING_REUSE_CASES + GENERAL_RBK_CASES + GENERAL_LDS_CASES
             + GENERAL_SLICE_CASES + PARTITION_CASES + K130_CASES + EDGE_CASES)

# (F, C, r, Cout) around every boundary of the predicates: C 64 | 68 (LPE), 128 | 132 | 256 (slices), C r 256, the ring's Cout set,
# the small kernel's Cout <= 128, the general kernel's Cout <= 512, F 93 | 94 (ring depth 4 | 3), 110 | 111 (ring | general),
# 142 | 143 (general | nothing), 254 | 255, r = 3, C not a multiple of 4
SUPPORT_SWEEP = [(F, C, r, Cout)
                 for F in (1, 33, 93, 94, 110, 111, 120, 130, 142, 143, 200, 254, 255)
                 for C, r in ((4, 1), (4, 2), (6, 1), (32, 2), (36, 2), (64, 1), (64, 2), (68, 1), (68, 2), (128, 1), (128, 2), (132, 1),
                              (192, 2), (256, 1), (256, 2), (384, 1), (4096, 1), (4224, 1), (64, 3), (0, 1))
                 for Cout in (8, 16, 24, 32, 48, 64, 112, 128, 144, 256, 272, 512, 528)]
