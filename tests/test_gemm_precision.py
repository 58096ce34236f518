"""float32 matmul precision of the pointwise products, without a GPU: the statement of the three levels (tests/_gemm_precision_ref.py)
against hand-computed bit patterns and its two error constants, the process-wide C entry (sph3d_pointwise_gemm_pieces) and the
Python interface (sph3d_gcn_amd.set_float32_matmul_precision and friends).  The kernels themselves: tests/test_gpu_gemm_precision.py."""
import ctypes

import numpy as np
import pytest
import torch

import _gemm_forms as G
import _gemm_precision_ref as P
import sph3d_gcn_amd as pkg
from sph3d_gcn_amd import _lib, tf_gemm

PIECES_AT_IMPORT = _lib.lib().sph3d_pointwise_gemm_pieces(0)


@pytest.fixture(autouse=True)
def _default_level_around_every_test():
    _lib.lib().sph3d_pointwise_gemm_pieces(3)
    yield
    _lib.lib().sph3d_pointwise_gemm_pieces(3)


def _f(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)


def _bits(a):
    return [int(v) for v in np.asarray(a, dtype=np.float32).reshape(-1).view(np.uint32)]


def _pieces_bits(x, level):
    return [_bits(p)[0] for p in P.pieces(np.asarray(x, dtype=np.float32).reshape(1), level)]


# ---- the statement against hand-computed patterns ---------------------------------------------------------------------------------
def test_pieces_of_one_value_with_a_bit_in_each_piece():
    x = _f(0x3f802008)                                   # 1 + 2^-10 + 2^-20
    assert float(x[0]) == 1.0 + 2.0 ** -10 + 2.0 ** -20
    assert _pieces_bits(x, "high") == _bits([1.0, 2.0 ** -10])
    assert _pieces_bits(x, "medium") == _bits([1.0])
    assert _pieces_bits(x, "highest") == _bits([1.0, 2.0 ** -10, 2.0 ** -20])


def test_pieces_ties_round_to_even():
    # 1 + 2^-8 lies half way between the bf16 neighbours 1 (even mantissa) and 1 + 2^-7: down; what is left is the second piece
    x = _f(0x3f808000)
    assert _pieces_bits(x, "medium") == [0x3f800000]
    assert _pieces_bits(x, "high") == [0x3f800000, 0x3b800000]                  # (1, 2^-8)
    # 1 + 2^-7 + 2^-8 lies half way between 1 + 2^-7 (odd) and 1 + 2^-6 (even): up; the second piece is negative
    x = _f(0x3f818000)
    assert _pieces_bits(x, "medium") == [0x3f820000]
    assert _pieces_bits(x, "high") == [0x3f820000, 0xbb800000]                  # (1 + 2^-6, -2^-8)
    # a tie in the SECOND piece: x - h = 2^-9 (1 + 2^-8) -> 2^-9
    x = _f(0x3f804040)
    assert _pieces_bits(x, "high") == [0x3f800000, 0x3b000000]
    # just below and just above a tie
    assert _pieces_bits(_f(0x3f807fff), "medium") == [0x3f800000] and _pieces_bits(_f(0x3f808001), "medium") == [0x3f810000]


def test_pieces_of_the_largest_finite_value():
    x = _f(0x7f7fffff)
    assert _pieces_bits(x, "medium") == [0x7f800000]                            # rounds to +inf
    h, m, l = P.pieces(x, "highest")
    assert np.isfinite([h[0], m[0], l[0]]).all()
    assert float(h[0]) + float(m[0]) + float(l[0]) == float(x[0])              # exact (float64 holds the three pieces' sum)
    assert _bits(h) == [0x7f7f0000]


def test_pieces_of_signed_zeros():
    assert _pieces_bits(_f(0x00000000), "medium") == [0x00000000]
    assert _pieces_bits(_f(0x80000000), "medium") == [0x80000000]
    assert _pieces_bits(_f(0x00000000), "high") == [0x00000000, 0x00000000]
    assert _pieces_bits(_f(0x80000000), "high") == [0x80000000, 0x00000000]    # (-0) - (-0) = +0


def test_pieces_of_a_negative_value():
    x = _f(0xc0490fdb)                                                          # -3.14159274...
    # low half 0x0fdb is below the tie 0x8000: h = 0xc0490000 = -3.140625; x - h = -4059 * 2^-22, 4059 = 253.6875 * 16 -> 254 * 16
    assert _pieces_bits(x, "medium") == [0xc0490000] and float(_f(0xc0490000)[0]) == -3.140625
    assert _pieces_bits(x, "high") == _bits([-3.140625, -4064.0 * 2.0 ** -22])
    x = _f(0xbf802008)
    assert _pieces_bits(x, "high") == _bits([-1.0, -(2.0 ** -10)]) and _pieces_bits(x, "medium") == _bits([-1.0])


def test_pieces_are_bf16_numbers_and_unknown_levels_raise():
    x = np.random.RandomState(0).randn(4096).astype(np.float32) * np.exp2(np.random.RandomState(1).randint(-20, 20, 4096)).astype(np.float32)
    for level in P.LEVELS:
        ps = P.pieces(x, level)
        assert len(ps) == P.PIECES[level]
        for p in ps:
            assert (p.view(np.uint32) & 0xffff == 0).all()
    h, m, l = P.pieces(x, "highest")
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    with pytest.raises(ValueError):
        P.pieces(x, "low")


# ---- the constants -------------------------------------------------------------------------------------------------------------------
def _spread(shape, rs):
    """tests/test_gpu_gemm_split.py's row operands: ~12 binades, both signs"""
    return (rs.randn(*shape) * np.exp2(rs.randint(-6, 6, shape))).astype(np.float32)


def _under_a_tie(shape, level, rs):
    """positive operands whose LAST kept piece sits just under a rounding tie (the rounding error is as large as it gets, and of one
    sign, so that nothing cancels in a sum): medium — low half 0x7fff; high — x - h = 2^14 + 2^7 j + 63 units in the last place"""
    hi = rs.randint(0, 32, shape).astype(np.uint32) << 16
    low = np.uint32(0x7fff) if level == "medium" else (np.uint32(1 << 14) | (rs.randint(0, 128, shape).astype(np.uint32) << 7) | np.uint32(0x3f))
    return ((rs.randint(121, 133, shape).astype(np.uint32) << 23) | hi | low).view(np.float32)


def _statement_error(x, w, level):
    x, w = torch.from_numpy(x), torch.from_numpy(w)
    exact, mag = x.double() @ w.double(), x.double().abs() @ w.double().abs()
    return float(((P.statement(P.pieces(x, level), P.pieces(w, level), level) - exact).abs() / mag).max())


@pytest.mark.parametrize("level", ["high", "medium"])
def test_statement_error_is_within_its_constant_and_not_fp32_sized(level):
    """the float64 evaluation of the statement against the exact product, per element over the summed term magnitudes: within the
    level's constant on both operand distributions, and above the 1e-5 that "highest" is held to.  (Signed operands over many binades
    let the roundings cancel — "high" then reaches 9.2e-6 — so the operands under a tie, 2.6e-5, are what tells "high" from "highest";
    "medium": 4.3e-3 and 7.5e-3.)"""
    rs = np.random.RandomState(5)
    K = 64
    e_spread = _statement_error(_spread((256, K), rs), (rs.randn(K, 32) / K ** 0.5).astype(np.float32), level)
    e_tie = _statement_error(_under_a_tie((256, K), level, rs), _under_a_tie((K, 32), level, rs), level)
    print("%s: statement error / term magnitudes: spread operands %.3g, operands under a tie %.3g, constant %.3g"
          % (level, e_spread, e_tie, P.C_LEVEL[level]))
    assert e_spread <= P.C_LEVEL[level] and e_tie <= P.C_LEVEL[level]
    assert max(e_spread, e_tie) > 1e-5                   # the level is really another one: not the fp32-sized error of "highest"
    e3 = _statement_error(_spread((256, K), rs), (rs.randn(K, 32) / K ** 0.5).astype(np.float32), "highest")
    assert e3 <= 4e-7


def test_constants():
    assert P.C_HIGH == 3 * 2.0 ** -16 * (1 + 2.0 ** -7) and P.C_MEDIUM == 2.0 ** -7 + 2.0 ** -16
    # the derivation's sums: high (1 + 2^-8)^2 + 1 + (1 + 2^-16) in units of 2^-16; medium 2 d + d^2 at d = 2^-8
    assert 2.0 ** -16 * ((1 + 2.0 ** -8) ** 2 + 1 + (1 + 2.0 ** -16)) <= P.C_HIGH
    assert 2 * 2.0 ** -8 + 2.0 ** -16 == P.C_MEDIUM


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_default_round_trip_and_query():
    l = _lib.lib()
    assert PIECES_AT_IMPORT == 3
    assert _lib.SIGNATURES["sph3d_pointwise_gemm_pieces"] == (ctypes.c_int, [ctypes.c_int])
    assert l.sph3d_pointwise_gemm_pieces(0) == 3
    assert l.sph3d_pointwise_gemm_pieces(2) == 3 and l.sph3d_pointwise_gemm_pieces(0) == 2
    assert l.sph3d_pointwise_gemm_pieces(1) == 2 and l.sph3d_pointwise_gemm_pieces(-1) == 1
    for other in (0, 4, -1, -3, 7, 1 << 20):
        assert l.sph3d_pointwise_gemm_pieces(other) == 1                       # values outside {1, 2, 3} change nothing
    assert l.sph3d_pointwise_gemm_pieces(3) == 1 and l.sph3d_pointwise_gemm_pieces(0) == 3


def test_mode_plan_and_workspace_answer_the_same_at_every_piece_count():
    l = _lib.lib()

    def answers():
        out = [l.sph3d_pointwise_gemm_mode(-1)]
        buf = (ctypes.c_int * len(G.FIELDS))()
        for _, product, R, Ci, Co, aligned, _, xok in G.FORM_CASES:
            for mode in (-1, 0, 1):
                assert l.sph3d_pointwise_gemm_plan(product, R, Ci, Co, aligned, mode, xok, ctypes.cast(buf, ctypes.c_void_p)) == 0
                out.append(tuple(buf))
            out.append(l.sph3d_pointwise_gemm_bnstats_blocks(R, Ci, Co))
            out.append(l._cdll.sph3d_pointwise_gemm_tn_workspace(R, Ci, Co))   # (the library's answer, not the binding's memo)
        return out

    want = answers()
    for pieces in (2, 1, 3):
        l.sph3d_pointwise_gemm_pieces(pieces)
        assert answers() == want
    assert l.sph3d_pointwise_gemm_mode(-1) in (0, 1)


# ---- the Python interface ------------------------------------------------------------------------------------------------------------
def test_python_levels_map_to_pieces():
    l = _lib.lib()
    assert pkg.set_float32_matmul_precision is tf_gemm.set_float32_matmul_precision
    assert pkg.get_float32_matmul_precision is tf_gemm.get_float32_matmul_precision
    assert pkg.float32_matmul_precision is tf_gemm.float32_matmul_precision
    assert pkg.get_float32_matmul_precision() == "highest"
    assert pkg.set_float32_matmul_precision("high") == "highest" and l.sph3d_pointwise_gemm_pieces(0) == 2
    assert pkg.get_float32_matmul_precision() == "high"
    assert pkg.set_float32_matmul_precision("medium") == "high" and l.sph3d_pointwise_gemm_pieces(0) == 1
    assert pkg.set_float32_matmul_precision("highest") == "medium" and l.sph3d_pointwise_gemm_pieces(0) == 3
    for pieces, level in ((1, "medium"), (2, "high"), (3, "highest")):
        l.sph3d_pointwise_gemm_pieces(pieces)
        assert pkg.get_float32_matmul_precision() == level


def test_python_unknown_level_raises_and_changes_nothing():
    pkg.set_float32_matmul_precision("high")
    for bad in ("low", "HIGH", "", None, 2):
        with pytest.raises(ValueError):
            pkg.set_float32_matmul_precision(bad)
        with pytest.raises(ValueError):
            with pkg.float32_matmul_precision(bad):
                pass
    assert pkg.get_float32_matmul_precision() == "high"


def test_context_manager_restores_also_on_an_exception():
    pkg.set_float32_matmul_precision("high")
    with pkg.float32_matmul_precision("medium"):
        assert pkg.get_float32_matmul_precision() == "medium"
        with pkg.float32_matmul_precision("highest"):
            assert pkg.get_float32_matmul_precision() == "highest"
        assert pkg.get_float32_matmul_precision() == "medium"
    assert pkg.get_float32_matmul_precision() == "high"
    with pytest.raises(RuntimeError):
        with pkg.float32_matmul_precision("medium"):
            raise RuntimeError("inside")
    assert pkg.get_float32_matmul_precision() == "high"


def test_torch_global_is_not_read():
    prev = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("medium")
        assert pkg.get_float32_matmul_precision() == "highest" and _lib.lib().sph3d_pointwise_gemm_pieces(0) == 3
    finally:
        torch.set_float32_matmul_precision(prev)


def test_trainer_takes_a_level():
    import inspect
    from sph3d_gcn_amd.harness import train
    assert inspect.signature(train.Trainer.__init__).parameters["matmul_precision"].default is None
