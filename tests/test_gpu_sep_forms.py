"""The one-kernel separable layer (csrc/sepring.hip: sepconv_ring_kernel, inference and training; csrc/sepconv.hip:
sepconv_fused_kernel and sepconv_general_kernel) per element against float64 (tests/_sep_ref.py), at every launch form, through
the C ABI.

sph3d_separable_conv3d_fused picks one of three kernels and an instantiation from the dimensions; every case restates the rule
that selects its form as an assertion — the functions of tests/_sep_forms.py are copied from the launchers as they stood before
csrc/sepconv.hpp: sep_plan — and every call asserts that the library's own plan for it (sph3d_separable_conv3d_plan) is that
form: kernel, instantiation, ring depth, wave groups.  The two predicates the library can be asked about are compared with its
answer over a sweep that crosses each boundary.  Outputs are
pre-filled with NaN, the statistics partials included (an idle workgroup's row that is not written shows); after every ring launch
sph3d_separable_conv3d_ring_failures() must be 0.  Graphs come from make_graph (rows of count 0, 1, 2, K - 1 and K in every cloud),
bin ids are synthetic, data differ per cloud.  The checks print the used fraction of each derived bound behind a [form] tag:
DESIGN.md §2 quotes the maxima.

Left out on purpose: the ring's spin limit and abort flag (they are for a broken launch), the 32-bit-offset limits (N C near
2^32, N above 2^24) and neighbour ids outside [0, N)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _conv_ref import clamp_bins, make_values
from _sep_forms import (EDGE_CASES, FIELDS, GENERAL_FORM_CASES, GENERAL_LDS_CASES, GENERAL_RBK_CASES, GENERAL_SLICE_CASES, K130_CASES,
                        PARTITION_CASES, RING_FORM_CASES, RING_REUSE_CASES, SMALL_FORM_CASES, SUPPORT_SWEEP, case_id, form_of,
                        fused_supported, infer_form, sr_shape_ok, train_blocks, train_form)
from _sep_ref import SepRef, check_infer, check_train, make_inputs
from sph3d_gcn_amd import _lib

pytestmark = pytest.mark.gpu
P, S = _lib.ptr, _lib.stream_ptr
OK, EUNSUPPORTED = 0, -4


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _shape(c):
    return (c.B, c.N, c.M, c.F, c.C, c.r, c.K, c.Cout)


@functools.lru_cache(maxsize=2)
def _data(shape):
    """inputs and the float64 statement of a shape: computed once, shared by the inference and the training case of the shape (the
    lists are run in shape order), never changed"""
    return make_inputs(*shape)


def _out(t, dev):
    """address of an output; a zero-sized one still gets an address that is not NULL"""
    return P(t) if t.numel() else P(torch.zeros(1, dtype=torch.float32, device=dev))


def _assert_library_plan(c, train):
    """what the library launches for the case is the form the restated rules give: kernel, instantiation, ring depth, wave groups"""
    out = (ctypes.c_int * len(FIELDS))()
    assert _lib.lib().sph3d_separable_conv3d_plan(train, *_shape(c), ctypes.cast(out, ctypes.c_void_p)) == OK
    p, form = dict(zip(FIELDS, out)), (train_form if train else infer_form)(*_shape(c))
    if form["kernel"] in ("unsupported", "empty"):
        assert (p["kernel"] == 0) == (form["kernel"] == "unsupported") and p["grid"] == 0, (p, form)
        return
    assert p["kernel"] == {"ring": 1, "train": 1, "small": 2, "general": 3}[form["kernel"]] and p["grid"] == 256, (p, form)
    assert (p["R"], p["LPE"], p["RBK"] if form["kernel"] == "general" else p["KT"]) == form["inst"], (p, form)
    assert (p["NB"], p["G"]) == (form.get("NB", 0), form.get("G", 0)), (p, form)


def _infer(dev, c, d, tail, bins=None, x=None, expect=OK):
    """sph3d_separable_conv3d_fused into a NaN-filled output -> [B, M, Cout]"""
    _assert_library_plan(c, 0)
    with_bias, act, bn = {"none": (0, 0, 0), "bias": (1, 0, 0), "bias+elu+bn": (1, 1, 1)}[tail]
    l = _lib.lib()
    args = [_t(d["idx"], dev), _t(d["cnt"], dev), _t(d["bins"] if bins is None else bins, dev), _t(d["x"] if x is None else x, dev),
            _t(d["w_dw"], dev), _t(d["W"], dev), _t(d["bias"], dev) if with_bias else None, _t(d["scale"], dev) if bn else None,
            _t(d["shift"], dev) if bn else None]
    out = _nan((c.B, c.M, c.Cout), dev)
    rc = l.sph3d_separable_conv3d_fused(c.B, c.N, c.M, c.F, c.C, c.r, c.K, c.Cout, act, *[P(a) for a in args], P(out), S())
    assert rc == expect, "sph3d_separable_conv3d_fused returned %d: %s" % (rc, l.sph3d_last_error().decode("utf-8", "replace"))
    torch.cuda.synchronize()
    assert l.sph3d_separable_conv3d_ring_failures() == 0
    return _n(out)


def _train(dev, c, d, with_bias, bins=None, x=None):
    """sph3d_separable_conv3d_train into NaN-filled outputs -> (depthwise [B, M, C r], y [B, M, Cout], partial [nblk, 2, Cout])"""
    _assert_library_plan(c, 1)
    l = _lib.lib()
    nblk = l.sph3d_separable_conv3d_train_blocks(c.Cout)
    assert nblk == train_blocks(c.Cout)
    args = [_t(d["idx"], dev), _t(d["cnt"], dev), _t(d["bins"] if bins is None else bins, dev), _t(d["x"] if x is None else x, dev),
            _t(d["w_dw"], dev), _t(d["W"], dev), _t(d["bias"], dev) if with_bias else None]
    dw, y, partial = _nan((c.B, c.M, c.C * c.r), dev), _nan((c.B, c.M, c.Cout), dev), _nan((nblk, 2, c.Cout), dev)
    _lib.check(l.sph3d_separable_conv3d_train(c.B, c.N, c.M, c.F, c.C, c.r, c.K, c.Cout, *[P(a) for a in args], _out(dw, dev), _out(y, dev),
                                              P(partial), S()))
    torch.cuda.synchronize()
    assert l.sph3d_separable_conv3d_ring_failures() == 0
    return _n(dw), _n(y), _n(partial)


def _run_case(dev, c, tails=("none", "bias+elu+bn")):
    """one case: the form the rules give must be the one the case is meant for, then the call(s) and the per-element checks"""
    form = form_of(c)
    assert form["tag"] == c.tag, "the rules give %s, the case is meant for %s" % (form["tag"], c.tag)
    d = _data(_shape(c))
    what = "[%s] %s" % (form["tag"], case_id(c))
    if c.kind == "infer":
        for tail in tails:
            check_infer(_infer(dev, c, d, tail), d["ref"], tail, d["bias"], d["scale"], d["shift"], what)
    else:
        for with_bias in (False, True):
            bias = d["bias"] if with_bias else None
            check_train(*_train(dev, c, d, with_bias), d["ref"], bias, form, what + (" bias" if with_bias else " nobias"))
    return form


def _by_shape(cases):
    return sorted(cases, key=lambda c: (_shape(c), c.kind))


def _params(cases):
    cases = _by_shape(cases)
    return dict(argvalues=cases, ids=[case_id(c) for c in cases])


# ---- every reachable form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_params(RING_FORM_CASES))
def test_ring_forms(dev, c):
    form = _run_case(dev, c)
    assert form["kernel"] in ("ring", "train") and form["NB"] >= 7 and form["idle"] > 0 and c.M % 16 and c.M < c.N


@pytest.mark.parametrize("c", **_params(SMALL_FORM_CASES))
def test_small_kernel_forms(dev, c):
    form = _run_case(dev, c)
    assert form["kernel"] == "small" and c.M % 32 and not sr_shape_ok(c.N, c.F, c.C, c.r, c.K, c.Cout)


@pytest.mark.parametrize("c", **_params(GENERAL_FORM_CASES + GENERAL_SLICE_CASES))
def test_general_kernel_forms(dev, c):
    form = _run_case(dev, c)
    assert form["kernel"] == "general" and form["rbk"] == 1 and c.M % 16


# ---- the ring comes back to its slots ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_params(RING_REUSE_CASES))
def test_ring_slot_reuse(dev, c):
    """more row blocks per workgroup than ring slots: the `consumed` wait, the epochs of `filled`, and a slot overwritten while the
    other column blocks' owners may still be reading it — in numbers, per element"""
    form = form_of(c)
    assert form["nrb_max"] > form["NB"] and form["wrap"] >= 1
    if form["NB"] == 3:
        assert form["nrb_max"] == 7 and form["wrap"] == 2 and form["affine"] == (c.B == 8) and form["G"] in (1, 16)
    else:
        assert form["NB"] == 8 and c.B * c.M >= 40960
    _run_case(dev, c)


# ---- the general kernel's tile heights ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_params(GENERAL_RBK_CASES + GENERAL_LDS_CASES))
def test_general_kernel_tile_heights(dev, c):
    form = form_of(c)
    assert form["kernel"] == "general" and c.M % (16 * form["rbk_by_points"])
    if c.F > 110:                                      # many bins: no ring, no small kernel, and a lower tile than the points ask for
        assert form["rbk_by_points"] == 4 and form["rbk"] == {120: 2, 130: 1}[c.F] and c.Cout in (16, 32, 64, 128, 256)
    else:
        assert form["rbk"] == form["rbk_by_points"] == (4 if c.B * c.M >= 32768 else 2)
    _run_case(dev, c)


# ---- the partition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_params(PARTITION_CASES))
def test_partition(dev, c):
    form = _run_case(dev, c)
    assert form["affine"] == (c.B % 8 == 0)
    if (c.B, c.M) == (1, 40) and form["kernel"] in ("ring", "train"):
        assert form["units"] == 3 and form["idle"] == 253


# ---- counts above 64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_params(K130_CASES))
def test_counts_above_64(dev, c):
    d = _data(_shape(c))
    assert c.K == 130 and (d["cnt"] == 130).any() and (d["cnt"] == 129).any() and ((d["cnt"] > 64) & (d["cnt"] < 128)).any()
    _run_case(dev, c)


# ---- live bin ids out of range are clamped -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_params(EDGE_CASES))
def test_out_of_range_bin_ids(dev, c):
    form = form_of(c)
    assert form["tag"] == c.tag
    d = _data(_shape(c))
    rng = np.random.RandomState(5)
    live = np.arange(c.K)[None, None, :] < d["cnt"][:, :, None]
    bad = d["bins"].copy()
    sel = live & (rng.rand(*bad.shape) < 0.3)
    bad[sel] = rng.choice([-1, -1000, c.F, c.F + 1, 250, 255, 256, 2 ** 24, 2 ** 31 - 1, -2 ** 31], size=int(sel.sum())).astype(np.int32)
    assert sel.sum() > 50 and (bad[live] < 0).any() and (bad[live] >= c.F).any()
    ref = SepRef(d["x"], d["w_dw"], d["W"], d["idx"], d["cnt"], clamp_bins(bad, c.F).astype(np.int32))
    what = "[%s] bad bin ids, %s" % (form["tag"], case_id(c))
    if c.kind == "infer":
        check_infer(_infer(dev, c, d, "bias+elu+bn", bins=bad), ref, "bias+elu+bn", d["bias"], d["scale"], d["shift"], what)
    else:
        check_train(*_train(dev, c, d, True, bins=bad), ref, d["bias"], form, what)


# ---- one non-finite input ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_params(EDGE_CASES))
def test_one_non_finite_input(dev, c):
    """x[1, n, c] = NaN: the rows of cloud 1 whose neighbourhood names n are non-finite, every other row is finite and within its
    bound (a NaN must not travel through a ring slot, a tile row, a padding slot or the zero filter row)"""
    form = form_of(c)
    d = _data(_shape(c))
    live = np.arange(c.K)[None, None, :] < d["cnt"][:, :, None]
    n = int(np.bincount(d["idx"][1][live[1]], minlength=c.N).argmax())
    names = np.zeros((c.B, c.M), bool)
    names[1] = ((d["idx"][1] == n) & live[1]).any(axis=1)
    assert 3 <= names.sum() < c.M
    x = d["x"].copy()
    x[1, n, c.C // 2] = np.nan
    what = "[%s] one NaN input, %s" % (form["tag"], case_id(c))
    if c.kind == "infer":
        out = _infer(dev, c, d, "bias+elu+bn", x=x)
        check_infer(out, d["ref"], "bias+elu+bn", d["bias"], d["scale"], d["shift"], what, rows=~names)
        assert not np.isfinite(out[names]).any(), "a row that names the NaN point has a finite output"
    else:
        dw, y, partial = _train(dev, c, d, True, x=x)
        check_train(dw, y, partial, d["ref"], d["bias"], form, what, rows=~names)
        assert not np.isfinite(y[names]).any() and not np.isfinite(dw[names]).all(axis=1).any()
        assert not np.isfinite(partial.astype(np.float64).sum(0)).any()           # every column's sums hold a NaN row


# ---- contracts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M", [(0, 50), (3, 0), (0, 0)])
def test_empty_launches(dev, B, M):
    """B = 0 and M = 0 return OK; inference writes nothing, training writes all-zero partial rows (no point is claimed, so nothing
    divides by the zero row-block count)"""
    c = EDGE_CASES[0]._replace(B=B, M=M)
    assert infer_form(*_shape(c))["tag"] == "empty"
    form = train_form(*_shape(c))
    assert form["kernel"] == "train" and form["units"] == 0 and form["idle"] == 256
    rng = np.random.RandomState(1)
    d = dict(idx=np.zeros((B, M, c.K), np.int32), cnt=np.zeros((B, M), np.int32), bins=np.zeros((B, M, c.K), np.int32),
             x=make_values(rng, (max(B, 1), c.N, c.C))[:B], w_dw=make_values(rng, (c.F, c.C, c.r)),
             W=make_values(rng, (c.C * c.r, c.Cout)), bias=rng.randn(c.Cout).astype(np.float32),
             scale=rng.randn(c.Cout).astype(np.float32), shift=rng.randn(c.Cout).astype(np.float32))
    assert _infer(dev, c, d, "bias+elu+bn").shape == (B, M, c.Cout)
    dw, y, partial = _train(dev, c._replace(kind="train"), d, True)
    assert partial.shape == (train_blocks(c.Cout), 2, c.Cout) and (partial.view(np.int32) == 0).all()


def test_supported_predicates_equal_the_restated_rules():
    l = _lib.lib()
    N, K = 1000, 16
    seen = set()
    for F, C, r, Cout in SUPPORT_SWEEP:
        want_f, want_t = fused_supported(N, F, C, r, K, Cout), sr_shape_ok(N, F, C, r, K, Cout)
        assert l.sph3d_separable_conv3d_fused_supported(N, F, C, r, K, Cout) == int(want_f), (F, C, r, Cout)
        assert l.sph3d_separable_conv3d_train_supported(N, F, C, r, K, Cout) == int(want_t), (F, C, r, Cout)
        seen.add((want_f, want_t))
    assert seen == {(True, True), (True, False), (False, False)}
    for n, k in (((1 << 24) + 1, K), (1 << 24, K), ((1 << 24) - 5, K), (N, 0)):       # N above 2^24, N C at 2^32, below it, K = 0
        assert l.sph3d_separable_conv3d_fused_supported(n, 33, 64, 2, k, 128) == int(fused_supported(n, 33, 64, 2, k, 128))
        assert l.sph3d_separable_conv3d_train_supported(n, 33, 64, 2, k, 128) == int(sr_shape_ok(n, 33, 64, 2, k, 128))


def test_143_bins_beside_256_depthwise_channels_are_unsupported(dev):
    c = EDGE_CASES[0]._replace(F=143, C=128, r=2, Cout=64)
    assert infer_form(*_shape(c))["tag"] == "unsupported" and train_form(*_shape(c))["tag"] == "unsupported"
    assert infer_form(*_shape(c._replace(F=142)))["tag"].startswith("general<2,32,1>")
    d = _data(_shape(c))
    out = _infer(dev, c, d, "none", expect=EUNSUPPORTED)
    assert np.isnan(out).all()
    l = _lib.lib()
    bufs = [_t(d[k], dev) for k in ("idx", "cnt", "bins", "x", "w_dw", "W")]
    dw, y, partial = _nan((c.B, c.M, 256), dev), _nan((c.B, c.M, c.Cout), dev), _nan((train_blocks(c.Cout), 2, c.Cout), dev)
    rc = l.sph3d_separable_conv3d_train(c.B, c.N, c.M, c.F, c.C, c.r, c.K, c.Cout, *[P(a) for a in bufs], None, P(dw), P(y), P(partial), S())
    assert rc == EUNSUPPORTED
