"""The depthwise convolution's launch choice, held on the host: the library's query sph3d_depthwise_conv3d_plan (csrc/conv_plan.hpp:
conv_plan, which every entry point of csrc/conv3d.hip launches from) against tests/_conv_forms.py, the restatement of the launchers
as they stood before the choice was gathered into that one function — field for field, for the four ops, in and out of
deterministic mode, with and without active_bins, with the hub hooks at their defaults and set, on every case of the GPU case
lists and on a grid that crosses every boundary of the rules, the 32-bit offset guards among them (which no device test reaches) —
and the older shape queries against the plan.  No device is touched."""
import ctypes
import itertools

import pytest

import _conv_forms as S

K, M = 16, 107
GRID_C = [3, 4, 6, 35, 60, 64, 67, 68, 124, 128, 131, 132, 256, 257, 260, 512]      # (257: the odd-width kernel at T = 4, two slices)
GRID_R = [1, 2, 3, 4]
GRID_F = [1, 17, 18, 33, 34, 49, 63, 64, 65, 66, 159, 160, 161, 164, 165, 254, 255]
GRID_B = [0, 1, 3, 8, 9, 16]
GRID_N = [1, 7, 128, 768, 8192, 32767, 32768]
HOOKS = [None, (1, 8), (8192, 1)]                      # SPH3D_BWD_HUB_MIN_N, SPH3D_BWD_HUB_T: unset; set


@pytest.fixture(scope="module")
def lib():
    from sph3d_gcn_amd import _lib
    return ctypes.CDLL(_lib.LIB_PATH)


@pytest.fixture(scope="module")
def query(lib):
    fn = lib.sph3d_depthwise_conv3d_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 11 + [ctypes.c_void_p]
    out = (ctypes.c_longlong * len(S.FIELDS))()
    ref = ctypes.addressof(out)

    def q(*args):
        """-> the fields as a tuple, None for SPH3D_EINVAL"""
        rc = fn(*args, ref)
        assert rc in (0, -1), args
        return tuple(out) if rc == 0 else None
    return q


def _want(*args, **kw):
    p = S.plan(*args, **kw)
    return None if p is None else tuple(p[f] for f in S.FIELDS)


def _hooks(monkeypatch, h):
    for name, v in zip(("SPH3D_BWD_HUB_MIN_N", "SPH3D_BWD_HUB_T"), h or (None, None)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _splits(C):
    """(Ca, Cb) of a two-input call over C channels: slices inside one input and not, and an empty second input"""
    return [(Ca, C - Ca) for Ca in sorted({4, 64, 128, 256, C - 4, C}) if 0 < Ca <= C]


def _instantiations(p):
    """the kernel instantiations a plan launches"""
    p = dict(zip(S.FIELDS, p))
    k = p["kernel"]
    if k == S.FWD_MULTI:
        return {("dwconv_fwd_multi", p["R"], p["LPE"])}
    if k == S.FWD_ROW:
        return {("dwconv_fwd_row", p["R"])}
    if k == S.BWD_ODD:
        return {("dwconv_bwd_t_odd", p["V"], p["MAXF"])}
    if k == S.BWD_VEC:
        tables = [(S.K_COMPACT_BINS, 1)] * p["compact_launch"] + [(p["MAXF"], 0)]
        return {("dwconv_bwd_t_vec", p["R"], p["V"], mf, p["PARTS"], ct, hub) for mf, ct in tables for hub in ((1, 2) if p["hub"] else (0,))}
    return {S.FWD_GENERIC: {("dwconv_fwd_generic",)}, S.BWD_GENERIC: {("dwconv_bwd_t_generic",)}}.get(k, set())


INSTANTIATIONS = ({("dwconv_fwd_multi", r, lpe) for r in (1, 2) for lpe in (16, 32)} | {("dwconv_fwd_row", r) for r in (1, 2)}
                  | {("dwconv_fwd_generic",), ("dwconv_bwd_t_generic",)}
                  | {("dwconv_bwd_t_vec", r, 4, mf, parts, ct, hub) for r in (1, 2) for parts in (1, 2, 4) for mf, ct in ((17, 1), (33, 0))
                     for hub in (0, 1, 2)}
                  | {("dwconv_bwd_t_vec", r, 2, 65, 1, 0, 0) for r in (1, 2)}
                  | {("dwconv_bwd_t_odd", t, 33) for t in (1, 2, 3, 4)} | {("dwconv_bwd_t_odd", t, 65) for t in (1, 2)})


def _check(query, seen, op, B, N, M_, F, Ca, Cb, r, det, active):
    args = (op, B, N, M_, F, Ca, Cb, r, K, det, active)
    got, want = query(*args), _want(*args)
    assert got == want, (args, got and dict(zip(S.FIELDS, got)), want and dict(zip(S.FIELDS, want)))
    if got is not None:
        seen |= _instantiations(got)
    return got


def test_plan_equals_the_old_launchers(query, monkeypatch):
    seen, n = set(), 0
    for hooks in HOOKS:
        _hooks(monkeypatch, hooks)
        for C, r, F, B, N in itertools.product(GRID_C, GRID_R, GRID_F, GRID_B, GRID_N):
            for det, active in itertools.product((0, 1), (0, 1)):
                _check(query, seen, S.GRAD_T, B, N, M, F, C, 0, r, det, active)
                n += 1
            if hooks is None:                       # the forward reads neither the mode, nor active_bins, nor the hooks: below
                _check(query, seen, S.FWD, B, N, M, F, C, 0, r, 0, 0)
                n += 1
    assert n == (3 * 4 + 1) * 16 * 4 * 17 * 6 * 7
    assert seen == INSTANTIATIONS and len(INSTANTIATIONS) == 52          # every instantiation the library contains, and no other


def test_plan_of_the_two_input_ops_and_of_empty_launches(query, monkeypatch):
    seen = set()
    for hooks in HOOKS:
        _hooks(monkeypatch, hooks)
        for C, r, F in itertools.product(GRID_C, GRID_R, GRID_F):
            for (B, N), (det, active) in itertools.product(((0, 128), (3, 768), (8, 32768)), itertools.product((0, 1), (0, 1))):
                for Ca, Cb in _splits(C):
                    _check(query, seen, S.FWD_CAT, B, N, M, F, Ca, Cb, r, det, active)
                    _check(query, seen, S.GRAD_T_CAT, B, N, M, F, Ca, Cb, r, det, active)
                # the forward's answer is the same in every mode, with every flag and hook
                assert _check(query, seen, S.FWD, B, N, M, F, C, 0, r, det, active) == query(S.FWD, B, N, M, F, C, 0, r, K, 0, 0)
                # no output point: the forward launches nothing, the gradient still writes its zeros
                fwd = _check(query, seen, S.FWD, B, N, 0, F, C, 0, r, det, active)
                assert fwd is None or fwd == (0,) * len(S.FIELDS)
                _check(query, seen, S.GRAD_T, B, N, 0, F, C, 0, r, det, active)
    assert ("dwconv_fwd_row", 1) in seen and ("dwconv_bwd_t_vec", 2, 4, 17, 1, 1, 2) in seen


def _gpu_cases():
    """(op, B, N, M, F, Ca, Cb, r) of the GPU tests' case lists at their geometries"""
    for _, C, r, F in S.FWD_CASES:
        for B, M_, _K in ((1, 33, 70), (3, 31, 200), (9, 1, 70)):
            yield S.FWD, B, 40, M_, F, C, 0, r
    for C, r, _ in S.PLAN_CASES:
        yield S.GRAD_T, 2, 40, 250, 33, C, 0, r
    for C, r, F in S.V2_CASES + [(3, 1, 33), (5, 3, 33), (64, 2, 66), (100, 3, 17)]:
        yield S.GRAD_T, 2, 70, 150, F, C, 0, r
    for C, r, _ in S.HUB_CASES:
        yield S.GRAD_T, 2, 200, 2000, 33, C, 0, r
    for Ca, Cb, r in ((128, 4, 2), (128, 128, 2), (256, 128, 1), (64, 64, 2)):
        yield S.FWD_CAT, 3, 40, 31, 33, Ca, Cb, r
        yield S.GRAD_T_CAT, 2, 40, 250, 33, Ca, Cb, r
    for C in S.ODD_CHANNELS:
        for F in (33, 49, 65, 66):
            yield S.GRAD_T, 3, 300, 77, F, C, 0, 1
    for B in (1, 2, 3, 4, 5, 8, 9, 16):
        for N in (1, 5, 8, 63, 64, 65, 300):
            for C, r in ((4, 2), (34, 2), (132, 1), (6, 1), (3, 1)):
                yield S.GRAD_T, B, N, N + 5, 33, C, 0, r


def test_plan_of_every_gpu_case(query, monkeypatch):
    seen = set()
    for hooks in HOOKS:
        _hooks(monkeypatch, hooks)
        for case in _gpu_cases():
            for det, active in itertools.product((0, 1), (0, 1)):
                assert _check(query, seen, *case, det, active) is not None
    assert seen == INSTANTIATIONS                   # the GPU case lists reach every instantiation too


def test_the_two_forward_shapes_that_took_a_table_past_lds(query):
    """C r in (136, 248] at 160 bins: the multi kernel's table is (F + 1) x 128 r floats whatever C is, 164 864 B at r = 2; the
    first kernel whose table fits is the row kernel (87 584 B and 159 712 B); at C = 128 only the generic kernel's fits"""
    for C, lds in ((68, 87584), (124, 159712)):
        p = dict(zip(S.FIELDS, query(S.FWD, 3, 40, 31, 160, C, 0, 2, K, 0, 0)))
        assert (p["kernel"], p["R"], p["lds"]) == (S.FWD_ROW, 2, lds) and S.fwd_lds(S.FWD_MULTI, 160, C, 2) == 164864 > S.LDS
    p = dict(zip(S.FIELDS, query(S.FWD, 3, 40, 31, 160, 128, 0, 2, K, 0, 0)))
    assert (p["kernel"], p["lds"]) == (S.FWD_GENERIC, 160 * 256 * 4) and p["lds"] == S.LDS
    assert query(S.FWD, 3, 40, 31, 161, 128, 0, 2, K, 0, 0) is None                 # no kernel's table fits: SPH3D_EINVAL
    # the row kernel's own edge: F SL 4 = 160 KiB is the generic kernel's table, one row less than the row kernel needs
    p = dict(zip(S.FIELDS, query(S.FWD, 3, 40, 31, 160, 132, 0, 2, K, 0, 0)))
    assert p["kernel"] == S.FWD_GENERIC and (159 + 1) * 256 * 4 == S.LDS
    assert dict(zip(S.FIELDS, query(S.FWD, 3, 40, 31, 159, 132, 0, 2, K, 0, 0)))["kernel"] == S.FWD_ROW


def _around(limit, per, add):
    """the n that are an int with n * per + add one below, at and above `limit` (just below and above, if `limit` is not met)"""
    n, rest = divmod(limit - add, per)
    return [v for v in ([n - 1, n, n + 1] if rest == 0 else [n, n + 1]) if v < (1 << 31)]


def test_plan_at_the_32_bit_edges(query, monkeypatch):
    """neighbour ids of 24 bits, byte and element offsets into a cloud's input (forward), element offsets into a cloud's grad_output
    rows (gradient): the fall-backs no device test can afford to reach"""
    seen, two32 = set(), 1 << 32
    kernels = {}
    for hooks in (None, (1, 8)):
        _hooks(monkeypatch, hooks)
        for C, r in ((4, 1), (4, 2), (64, 2), (128, 1), (128, 2), (256, 1), (256, 2), (3, 1), (35, 2), (6, 1)):
            ns = [(1 << 24), (1 << 24) + 1] + _around(two32, 4 * C, 1024) + _around(two32, C, 256)
            for N in ns:
                for B, F in ((1, 33), (3, 65), (16, 159)):
                    p = _check(query, seen, S.FWD, B, N, M, F, C, 0, r, 0, 0)
                    kernels.setdefault((C, r, N <= 1 << 24, N * C * 4 + 1024 < two32, N * C + 256 < two32), set()).add(p[0])
                    _check(query, seen, S.GRAD_T, B, N, M, F, C, 0, r, 0, 1)
            for M_ in _around(two32, C * r, 256):
                for (B, N, F), (det, active) in itertools.product(((1, 128, 33), (3, 7, 65), (16, 768, 17)), itertools.product((0, 1), (0, 1))):
                    _check(query, seen, S.GRAD_T, B, N, M_, F, C, 0, r, det, active)
                    _check(query, seen, S.FWD, B, N, M_, F, C, 0, r, det, active)
        for Ca, Cb, r in ((128, 128, 2), (256, 128, 1), (128, 4, 2)):
            C = Ca + Cb
            for N in _around(two32, C, 256):
                _check(query, seen, S.FWD_CAT, 3, N, M, 33, Ca, Cb, r, 0, 0)
            CR = C * r
            for M_ in _around(two32, CR, 256):
                for det in (0, 1):
                    _check(query, seen, S.GRAD_T_CAT, 3, 128, M_, 33, Ca, Cb, r, det, 1)
    # each guard moved the forward choice: multi -> row at the 24-bit and byte-offset edges, row -> generic at the element-offset edge
    assert kernels[(64, 2, True, True, True)] == {S.FWD_MULTI} and kernels[(64, 2, True, False, True)] == {S.FWD_ROW}
    assert kernels[(4, 1, False, True, True)] == {S.FWD_ROW}
    assert kernels[(256, 2, True, False, True)] == {S.FWD_ROW} and kernels[(256, 2, False, False, False)] == {S.FWD_GENERIC}
    # ... and the gradient's: the vector and odd-width kernels up to M C r + 256 < 2^32, then the generic one or, in the mode, none
    for C, r, inside, outside in ((128, 2, S.BWD_VEC, S.BWD_GENERIC), (3, 1, S.BWD_GENERIC, S.BWD_GENERIC)):
        below, at, _ = _around(two32, C * r, 256)
        assert query(S.GRAD_T, 1, 128, below, 33, C, 0, r, K, 0, 1)[0] == inside and query(S.GRAD_T, 1, 128, at, 33, C, 0, r, K, 0, 1)[0] == outside
        assert query(S.GRAD_T, 1, 128, below, 33, C, 0, r, K, 1, 1)[0] == (S.BWD_VEC if C == 128 else S.BWD_ODD)
        assert query(S.GRAD_T, 1, 128, at, 33, C, 0, r, K, 1, 1)[0] == S.REFUSED


def test_shape_queries_read_the_plan(lib, query):
    ws_t, ws = lib.sph3d_depthwise_conv3d_grad_t_workspace, lib.sph3d_depthwise_conv3d_grad_workspace
    ws_t.restype = ws.restype = ctypes.c_size_t
    assert lib.sph3d_get_deterministic() == 0
    try:
        for det in (0, 1):
            lib.sph3d_set_deterministic(det)
            for C, r, F in itertools.product(GRID_C, GRID_R, GRID_F):
                for B, N in ((0, 128), (1, 7), (3, 768), (8, 8192), (16, 32768)):
                    p = S.plan(S.GRAD_T, B, N, 0, F, C, 0, r, 1, det, True)
                    if p is None:
                        continue
                    assert ws_t(B, N, F, C, r) == p["workspace_bytes"] == query(S.GRAD_T, B, N, 0, F, C, 0, r, K, -1, 1)[-1]
                    # (C = 5, r = 3, F = 1: the generic kernel's shape in and out of the mode: the transposed graph's bytes alone;
                    # they do not depend on the channels)
                    assert ws(B, N, M, F, C, r, K) - ws(B, N, M, F, 5, 3, K) == p["workspace_bytes"]
                    # with a plan that launches, the bytes are the query's at the call's own M
                    at_m = S.plan(S.GRAD_T, B, N, M, F, C, 0, r, 1, det, True)
                    assert at_m["kernel"] == S.REFUSED or at_m["workspace_bytes"] == p["workspace_bytes"]
    finally:
        lib.sph3d_set_deterministic(0)
    for C, r, F in itertools.product(GRID_C + [384, 1024], GRID_R, GRID_F):
        for Ca, Cb in _splits(C):
            want = S.plan(S.FWD_CAT, 1, 1, 1, F, Ca, Cb, r, 1, False, False)
            want = want is not None and want["kernel"] != S.REFUSED
            assert lib.sph3d_depthwise_conv3d_cat_supported(F, Ca, Cb, r) == int(want) == int(S.cat_ok(F, Ca, Cb, r) and S.dims_ok(F, C, r))
            for op in (S.FWD_CAT, S.GRAD_T_CAT):
                got = query(op, 3, 768, M, F, Ca, Cb, r, K, 0, 1)
                assert (got is not None and got[0] != S.REFUSED) == want and (got is None or got[0] in (S.FWD_ROW, S.BWD_VEC, S.REFUSED))


def test_query_validates(lib, query):
    fn = lib.sph3d_depthwise_conv3d_plan
    out = (ctypes.c_longlong * len(S.FIELDS))()
    p = ctypes.addressof(out)
    good = (S.GRAD_T, 3, 150, 107, 33, 12, 0, 2, 12, 0, 1)
    assert fn(*good, p) == 0 and out[0] == S.BWD_VEC
    assert fn(*good, None) == -1
    #  op; B, N, M, F, Ca; Cb with one input; r; the flags
    for i, bad in ((0, -1), (0, 4), (1, -1), (2, 0), (2, -5), (3, -1), (4, 0), (5, 0), (5, -4), (6, 4), (7, 0), (7, -2), (9, -2), (9, 2),
                   (10, -1), (10, 2)):
        args = list(good)
        args[i] = bad
        assert fn(*args, p) == -1, args
    # K: the forward ops have one, the gradients ignore it
    assert fn(S.FWD, 3, 150, 107, 33, 12, 0, 2, 0, 0, 0, p) == -1 and fn(S.FWD_CAT, 3, 150, 107, 33, 128, 128, 2, 0, 0, 0, p) == -1
    assert fn(S.GRAD_T, 3, 150, 107, 33, 12, 0, 2, 0, 0, 0, p) == 0 and fn(S.GRAD_T, 3, 150, 107, 33, 12, 0, 2, -7, 0, 0, p) == 0
    # the filter table slice must fit LDS: F min(C r, 256) floats
    assert fn(S.FWD, 3, 150, 107, 640, 64, 0, 1, 12, 0, 0, p) == 0 and fn(S.FWD, 3, 150, 107, 641, 64, 0, 1, 12, 0, 0, p) == -1
    err = lib.sph3d_last_error
    err.restype = ctypes.c_char_p
    assert fn(S.GRAD_T, 3, 150, 107, 641, 64, 0, 1, 12, 0, 0, p) == -1 and b"does not fit LDS" in err()
    # depth multipliers above 256: the generic gradient rejects them; the mode refuses first; an empty batch launches nothing
    assert fn(S.GRAD_T, 3, 150, 107, 1, 1, 0, 300, 1, 0, 0, p) == -1 and b"depth multiplier" in err()
    assert fn(S.GRAD_T, 3, 150, 107, 1, 1, 0, 300, 1, 1, 0, p) == 0 and tuple(out) == (S.REFUSED,) + (0,) * (len(S.FIELDS) - 1)
    assert fn(S.GRAD_T, 0, 150, 107, 1, 1, 0, 300, 1, 0, 0, p) == 0 and tuple(out) == (0,) * len(S.FIELDS)
    # a shape is not invalid for being unsupported
    assert fn(S.FWD_CAT, 3, 150, 107, 33, 64, 64, 2, 12, 0, 0, p) == 0 and tuple(out) == (S.REFUSED,) + (0,) * (len(S.FIELDS) - 1)
    # C r and the grid are ints
    assert fn(S.FWD, 1, 1, 1, 1, 1 << 20, 0, 1 << 12, 1, 0, 0, p) == -1 and fn(S.FWD, 1, 1, 1, 1, 1 << 20, 0, 1 << 10, 1, 0, 0, p) == 0
    assert fn(S.FWD, 16, 8, (1 << 31) - 1, 1, 3, 0, 1, 1, 0, 0, p) == 0 and out[19] == 1 << 30
    assert fn(S.FWD, 64, 8, (1 << 31) - 1, 1, 3, 0, 1, 1, 0, 0, p) == -1 and b"workgroups" in err()
    # the one-call gradient has a K and checks it before it sizes its transposed graph; it launches nothing here
    grad = lib.sph3d_depthwise_conv3d_grad
    assert grad(3, 150, 107, 33, 12, 2, 0, *([None] * 8), None, ctypes.c_size_t(0), None) == -1 and b"K=0" in err()
    assert grad(3, 150, 107, 641, 64, 1, 16, *([None] * 8), None, ctypes.c_size_t(0), None) == -1 and b"does not fit LDS" in err()
    assert grad(3, 150, 107, 33, 12, 2, 16, *([None] * 8), None, ctypes.c_size_t(0), None) == -2 and b"workspace 0 B" in err()
