"""Farthest-point sampling without a device: the host side of csrc/sample.hip as it stood before csrc/fps_plan.hpp gathered it
(sph3d_farthest_point_sample, sph3d_farthest_point_sample_workspace, coop_groups, coop_slot_bytes), restated in Python integers;
the sampling itself in float32 numpy under the reference's tie rule and under two wrong ones; and the clouds and the case list that
tests/test_fps_forms.py (CPU) and tests/test_gpu_fps_forms.py share.  Python integers do not overflow: where the old code's `int`
arithmetic would have, plan() says what the arithmetic means."""
import numpy as np

FIELDS = ("kernel", "P", "block", "grid", "G", "xcd_local", "repair", "big_grid", "workspace_bytes", "off_err", "off_slots", "off_temp")
NONE, PLAIN, PRUNED, COOP, BIG = range(5)                # kernel
BAD_SAMPLES, BAD_SHAPE, BAD_POINTS = "npoint", "shape", "points"

REF_BLOCK = 1024                                         # common.hpp
MAX_REG_POINTS, BIG_GRID, PRUNE_MIN, COOP_PTS = 24, 64, 2049, 4096         # sample.hip
INT_MAX = (1 << 31) - 1


def coop_groups(b, n):
    G = (n + COOP_PTS - 1) // COOP_PTS
    return G if G <= 64 and b * G <= 128 else 0


def coop_slot_bytes(b, G):
    return (256 + 8 * b * 2 * G + 255) & ~255


def workspace(b, n, m):
    """sph3d_farthest_point_sample_workspace, for arguments the entry accepts"""
    if n <= REF_BLOCK * MAX_REG_POINTS:
        return 0
    G = coop_groups(b, n)
    big = 4 * min(b, BIG_GRID) * n
    return coop_slot_bytes(b, G) + big if G else big


def plan(b, n, m):
    """sph3d_farthest_point_sample -> the fields, or why the call is SPH3D_EINVAL"""
    if not m > 0:
        return BAD_SAMPLES
    if not (b >= 0 and n > 0):
        return BAD_SHAPE
    if not n <= REF_BLOCK * 256:
        return BAD_POINTS
    p = dict.fromkeys(FIELDS, 0)
    p["workspace_bytes"] = workspace(b, n, m)
    if b == 0:
        return p
    P = (n + REF_BLOCK - 1) // REF_BLOCK
    bs = (n + 63) // 64 * 64 if n < REF_BLOCK else REF_BLOCK
    p.update(grid=b, G=1)
    if n >= PRUNE_MIN and n > REF_BLOCK and n <= 16384 and m > 1:
        p.update(kernel=PRUNED, block=REF_BLOCK, P=4 if P <= 4 else (8 if P <= 8 else 16))
    elif P <= MAX_REG_POINTS:
        p.update(kernel=PLAIN, block=bs, P=next(q for q in (1, 2, 4, 8, 12, 16, 24) if P <= q))
    else:
        G = coop_groups(b, n)
        g = min(b, BIG_GRID)
        if G:
            head = coop_slot_bytes(b, G)
            rounds8 = (b + 7) // 8
            xcd_local = int(rounds8 * G <= 16)
            p.update(kernel=COOP, block=REF_BLOCK, G=G, xcd_local=xcd_local, grid=8 * rounds8 * G if xcd_local else b * G, repair=1,
                     big_grid=g, off_slots=256, off_temp=head)
        else:
            p.update(kernel=BIG, block=REF_BLOCK, grid=g, big_grid=g)
    return p


# ---- the sampling ------------------------------------------------------------------------------------------------------------
RULES = ("ref", "lowest_k", "same_thread_higher_k")


def fps_numpy(pts, m, rule="ref"):
    """pts [n, 3] float32 -> m indices.  The kernels' expression order, d = (dx*dx + dy*dy) + dz*dz rounded per operation, the
    running distance d < td ? d : td from 1e38, the arg-max by strict > from -1 (so a NaN distance changes nothing).  Among the
    points at the maximum:
      "ref"                    the reference's: lower k mod 1024 (its thread), then lower k (tf_sample_gpu.cu:49,56-66)
      "lowest_k"               wrong: the lowest index whatever its thread
      "same_thread_higher_k"   wrong: the right thread, but its HIGHER k (the granule's 255 - q field dropped or inverted)"""
    assert rule in RULES
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    n = pts.shape[0]
    x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
    td = np.full(n, 1e38, np.float32)
    out = np.zeros(m, np.int32)
    old = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(1, m):
            dx, dy, dz = x - x[old], y - y[old], z - z[old]
            d = (dx * dx + dy * dy) + dz * dz
            td = np.where(d < td, d, td)
            ks = np.flatnonzero(td == td.max())              # (td holds no NaN and is >= 0: the strict > from -1 takes it)
            if rule == "lowest_k":
                old = ks[0]
            else:
                t = ks % REF_BLOCK
                same = ks[t == t.min()]
                old = same[0] if rule == "ref" else same[-1]
            out[j] = old
    return out


# ---- the clouds --------------------------------------------------------------------------------------------------------------
def uniform(n, seed):
    return np.random.RandomState(seed).rand(n, 3).astype(np.float32)


def planted_sites(n, span):
    """the index sets that hold one outlier site each (indices past the cloud's end dropped, sites without a holder too)"""
    sites = [(100, 100 + span),                 # same thread (span a multiple of 1024), another workgroup or k >> 10
             (200, 200 + 1024),                 # same thread, next register
             (1023, 1024),                      # the lower thread id at the higher k
             (2000, 900 + span),                # ... again, further apart
             (10 + span, 10),                   # same thread, the higher index named first
             (300, 300 + 1024, 300 + span)]     # three holders: registers and workgroups at once
    out = []
    for s in sites:
        s = tuple(dict.fromkeys(k for k in s if 0 < k < n))
        if s:
            out.append(s)
    assert len({k for s in out for k in s}) == sum(len(s) for s in out)
    return out


def planted(n, seed, span):
    """A random cloud in the unit cube plus six outlier sites at distance 5 .. 5.5 from its centre along the six axis directions
    (which site gets which direction depends on the seed).  Each site is held by several points with the SAME coordinates
    (planted_sites), so the round that picks the site — one of the first six: every site is further from everything picked so far
    than any point of the cube — is decided by the tie rule alone, and each field of the rule decides one of them."""
    rng = np.random.RandomState(seed)
    pts = rng.rand(n, 3).astype(np.float32)
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)[rng.permutation(6)]
    for i, holders in enumerate(planted_sites(n, span)):
        pts[list(holders)] = np.float32(0.5) + dirs[i] * np.float32(5.0 + 0.1 * i)
    return pts


NONFINITE_AT = (700 + 1024 * 1, 500 + 1024 * 5, 300 + 1024 * 9)      # NaN, +inf, -inf: three threads, three 4096-blocks


def nonfinite(n, seed):
    """A random cloud with one NaN, one +inf and one -inf coordinate (the axis depends on the seed).  None of the three is ever
    lowered from 1e38, so round 1 is a three-way tie between different threads (and workgroups of the co-operative kernel), and
    whichever wins is the sample of every later round: a non-finite sample lowers nothing."""
    rng = np.random.RandomState(seed)
    pts = rng.rand(n, 3).astype(np.float32)
    assert n > max(NONFINITE_AT)
    for k, v in zip(NONFINITE_AT, (np.nan, np.inf, -np.inf)):
        pts[k, rng.randint(3)] = v
    return pts


# ---- the GPU case list (tests/test_gpu_fps_forms.py); every case names the plan it must have --------------------------------------
def _plain(P, block=REF_BLOCK):
    return dict(kernel=PLAIN, P=P, block=block)


def _coop(G, xcd_local):
    return dict(kernel=COOP, P=0, G=G, xcd_local=xcd_local, repair=1)


# (id, plan fields it claims, b, n, m, cloud kind, span, launches)
CASES = [
    ("plain1-one-point", _plain(1, 64), 2, 1, 3, "uniform", 0, 2),
    ("plain1-n63-every-point", _plain(1, 64), 2, 63, 63, "uniform", 0, 2),
    ("plain1-n64-every-point", _plain(1, 64), 2, 64, 64, "uniform", 0, 2),
    ("plain1-n65-every-point", _plain(1, 128), 2, 65, 65, "uniform", 0, 2),
    ("plain1-n1023-planted", _plain(1, 1024), 3, 1023, 200, "planted", 512, 2),
    ("plain2-n1025-planted", _plain(2), 2, 1025, 200, "planted", 1024, 2),
    ("plain2-n2048-planted", _plain(2), 2, 2048, 200, "planted", 1024, 2),
    ("plain4-m1", _plain(4), 2, 3000, 1, "uniform", 0, 2),
    ("plain8-m1", _plain(8), 2, 6000, 1, "uniform", 0, 2),
    ("plain12-m1", _plain(12), 2, 10000, 1, "uniform", 0, 2),
    ("plain16-m1", _plain(16), 2, 16384, 1, "uniform", 0, 2),
    ("plain24-planted", _plain(24), 2, 20000, 300, "planted", 8192, 2),
    ("plain24-full-nonfinite", _plain(24), 1, 24576, 100, "nonfinite", 0, 2),
    ("plain24-m-past-n", _plain(24), 1, 16385, 16390, "uniform", 0, 2),
    ("pruned4-n2049", dict(kernel=PRUNED, P=4), 1, 2049, 200, "uniform", 0, 2),
    ("pruned8-n4097", dict(kernel=PRUNED, P=8), 1, 4097, 200, "uniform", 0, 2),
    ("pruned16-n8193", dict(kernel=PRUNED, P=16), 1, 8193, 200, "uniform", 0, 2),
    ("coop-local-eight-rotations", _coop(8, 1), 1, 30000, 64, "planted", 4096, 8),
    ("coop-local-two-rounds-of-eight", dict(_coop(7, 1), grid=112), 9, 24577, 48, "planted", 4096 * 5, 2),
    ("coop-local-cap", dict(_coop(8, 1), grid=128), 16, 32768, 24, "planted", 4096 * 7, 2),
    ("coop-spread", dict(_coop(10, 0), grid=90), 9, 40000, 48, "planted", 4096, 2),
    ("coop-spread-G64", dict(_coop(64, 0), grid=128), 2, 262144, 24, "planted", 4096 * 40, 2),
    ("coop-nonfinite", _coop(7, 1), 2, 28672, 100, "nonfinite", 0, 2),
    ("coop-tag-wrap-m-past-n", _coop(7, 1), 1, 24577, 24580, "uniform", 0, 2),
    ("big-alone", dict(kernel=BIG, P=0, grid=19, big_grid=19, repair=0), 19, 24577, 32, "planted", 4096 * 5, 2),
    ("big-grid-stride", dict(kernel=BIG, P=0, grid=64, big_grid=64, repair=0), 65, 24577, 12, "planted", 4096 * 5, 2),
    ("big-widest-key", dict(kernel=BIG, P=0, grid=3, big_grid=3, repair=0), 3, 262144, 12, "planted", 1024 * 250, 2),
]


def clouds(case):
    """-> [b, n, 3] float32; every cloud of a batch differs"""
    name, _, b, n, m, kind, span, _ = case
    seed = 1000 * (1 + [c[0] for c in CASES].index(name))
    if kind == "planted":
        return np.stack([planted(n, seed + i, span) for i in range(b)])
    if kind == "nonfinite":
        return np.stack([nonfinite(n, seed + i) for i in range(b)])
    return np.stack([uniform(n, seed + i) for i in range(b)])
