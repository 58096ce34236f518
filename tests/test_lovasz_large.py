"""The Lovasz-softmax loss with the sort in global memory, without a device: the library's plan query
(sph3d_lovasz_softmax_large_plan; csrc/lovasz_plan.hpp: lovasz_large_plan, which the entry launches from) against
tests/_lovasz_large_forms.py, the launcher restated in Python, field for field; the workspace query against the plan; the order of
the refusals; the unchanged limits of the existing entry; and scope="batch" of the statement (harness/lovasz.py) against the
reference on the reshaped arrays and against the paper's own form written out here."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _lovasz_large_forms as S
import _lovasz_large_ref as RL
import _lovasz_ref as R
from sph3d_gcn_amd import _lib, tf_loss
from sph3d_gcn_amd.harness import lovasz

GRID_N = [1, 1023, 1024, 1025, 16384, 16385, 40000, 65536, 1 << 20]
GRID_C = [1, 2, 13, 21, 1024]
GRID_B = [0, 1, 4, 16]
GRID_TILE = [0, 10, 14]
GRID_SLAB = [0, 1, 5]


@pytest.fixture(scope="module")
def query():
    l = _lib.lib()
    out = (ctypes.c_longlong * len(S.FIELDS))()
    ref = ctypes.addressof(out)

    def q(*args):
        """-> the fields as a dict, or the status of a refusal"""
        rc = l.sph3d_lovasz_softmax_large_plan(*args, ref)
        return dict(zip(S.FIELDS, out)) if rc == 0 else rc
    return q


def test_plan_equals_the_restated_launcher(query):
    l = _lib.lib()
    seen_passes, seen_slabs, refused = set(), set(), 0
    for N, C, B, t, slab in itertools.product(GRID_N, GRID_C, GRID_B, GRID_TILE, GRID_SLAB):
        args = (B, N, C, t, slab)
        want, got = S.plan(*args), query(*args)
        assert got == want, (args, got, want)
        if not isinstance(got, dict):
            assert got == S.EINVAL and (slab > C or B * N * C > 1 << 40), args
            refused += 1
            continue
        p = got
        if B == 0:
            assert not any(p.values())
            continue
        # what every launch needs: grids and LDS a launch can have, a partition of the classes, runs that cover the rows, offsets in
        # order, aligned for what they hold, and bytes that are the exact sums
        assert p["tile"] == 1 << p["tile_log2"] and p["tile_log2"] == (t or S.DEFAULT_TILE_LOG2)
        assert (p["runs"] - 1) * p["tile"] < N <= p["npad"] == p["runs"] * p["tile"] and p["runs"] <= 1024
        assert 1 << p["passes"] >= p["runs"] and (p["passes"] == 0 or 1 << (p["passes"] - 1) < p["runs"])
        assert p["mtile"] == 1024 <= p["tile"] and p["mtiles"] * 1024 == p["npad"] and p["mtiles"] <= 1024
        assert 1 <= p["slab"] <= C and (p["slabs"] - 1) * p["slab"] < C <= p["slabs"] * p["slab"] and p["slab"] <= 65535
        assert p["sort_lds"] == 8 * p["tile"] <= 128 << 10 and p["merge_lds"] == 8192
        assert p["probs_grid"] * 256 >= B * N and p["count_grid"] * 4096 >= N and p["grad_grid"] * 1024 >= N
        assert p["key_bufs"] == (2 if p["passes"] else 1)
        keys = 8 * p["slab"] * B * p["npad"]
        assert p["off_keys0"] == 0 and p["off_keys1"] == (keys if p["passes"] else 0) and p["off_tilecnt"] == p["key_bufs"] * keys
        assert p["off_partial"] - p["off_tilecnt"] == p["off_count"] - p["off_partial"] == 4 * p["slab"] * B * p["mtiles"]
        assert p["off_bad"] - p["off_count"] == 4 * B * C and 0 <= p["workspace_bytes"] - p["off_bad"] - 4 * B < 256
        assert p["off_keys1"] % 8 == 0 and all(p[f] % 4 == 0 for f in ("off_tilecnt", "off_partial", "off_count", "off_bad"))
        assert p["workspace_bytes"] % 256 == 0 and p["cap"] == S.WS_CAP
        if slab == 0:
            # the plan's slab: under the cap, and the largest that is; one class where even one does not fit
            assert p["workspace_bytes"] <= S.WS_CAP or p["slab"] == 1
            if p["slab"] < C:
                more = S.plan(B, N, C, t, p["slab"] + 1)
                assert more["off_bad"] + 4 * B + 255 > S.WS_CAP
            if t == 0:
                assert l.sph3d_lovasz_softmax_large_workspace(B, N, C) == p["workspace_bytes"]
        seen_passes.add(p["passes"])
        seen_slabs.add(p["slabs"] > 1)
    assert seen_passes >= {0, 1, 2, 3, 4, 8, 10} and seen_slabs == {False, True} and refused > 0
    # the case the cap is derived from: seven classes at a time, in three passes
    p = query(16, 65536, 21, 0, 0)
    assert (p["tile"], p["runs"], p["passes"], p["slab"], p["slabs"]) == (4096, 16, 4, 7, 3) and p["workspace_bytes"] <= S.WS_CAP
    assert l.sph3d_lovasz_softmax_large_workspace(0, 8, 4) == 0 and l.sph3d_lovasz_softmax_large_workspace(1, (1 << 20) + 1, 4) == 0


def test_refusals_come_before_any_pointer(query):
    l = _lib.lib()
    null = [None] * 3 + [-1] + [None] * 6 + [None, 0]

    def entry(B, N, C, tile_log2=0, slab=0):
        return l.sph3d_lovasz_softmax_large(B, N, C, *null, tile_log2, slab, None)
    for args, rc, text in (((4, (1 << 20) + 1, 13), -4, b"not covered"), ((4, 4096, 1025), -4, b"not covered"),
                           ((4, 4096, 13, 9), -1, b"tile_log2"), ((4, 4096, 13, 15), -1, b"tile_log2"),
                           ((4, 4096, 13, -1), -1, b"tile_log2"), ((4, 4096, 13, 0, -1), -1, b"slab"),
                           ((4, 4096, 13, 0, 14), -1, b"slab"), ((-1, 8, 4), -1, b"bad dims"), ((1, 0, 4), -1, b"bad dims"),
                           ((1, 8, 0), -1, b"bad dims"), ((65536, 8, 4), -1, b"bad dims"), ((65535, 1 << 20, 1024), -1, b"bad dims")):
        full = args + (0,) * (5 - len(args))
        assert entry(*args) == rc and text in l.sph3d_last_error(), args
        assert query(*full) == rc == S.plan(*full), args
    # dimensions before the shape limits, the shape limits before the test arguments
    assert entry(-1, (1 << 20) + 1, 13) == -1 and entry(4, (1 << 20) + 1, 13, 9) == -4 and entry(4, 8, 1025, 0, -1) == -4
    assert entry(0, 8, 4) == 0                                                         # no block: nothing to do
    assert entry(1, 8, 4) == -1 and b"null" in l.sph3d_last_error()
    assert l.sph3d_lovasz_softmax_large_plan(1, 8, 4, 0, 0, None) == -1
    with pytest.raises(_lib.Sph3dError):
        tf_loss.lovasz_softmax_large(torch.zeros(1, 8, 4), torch.zeros(1, 8, dtype=torch.long))


def test_limits_of_both_entries():
    l = _lib.lib()
    assert lovasz.MAX_N == 16384 and l.sph3d_lovasz_softmax_supported(16384, 13) == 1 and l.sph3d_lovasz_softmax_supported(16385, 13) == 0
    assert tf_loss.supported(16384, 2) and not tf_loss.supported(16385, 2)
    assert lovasz.MAX_N_LARGE == S.MAX_N == 1 << 20
    assert l.sph3d_lovasz_softmax_large_supported(lovasz.MAX_N_LARGE, 1024) == 1
    assert l.sph3d_lovasz_softmax_large_supported(lovasz.MAX_N_LARGE + 1, 13) == 0 and l.sph3d_lovasz_softmax_large_supported(8, 1025) == 0
    assert l.sph3d_lovasz_softmax_large_supported(1, 1) == 1 and l.sph3d_lovasz_softmax_large_supported(0, 1) == 0
    assert tf_loss.supported_large(16385, 2) and tf_loss.supported_large(1 << 20, 1024) and not tf_loss.supported_large((1 << 20) + 1, 2)


def test_summation_depth_of_the_large_entry():
    """the tree of include/sph3d.h, at the shapes of the GPU tests"""
    assert RL.tiles_of(1, 1024) == 1 and RL.tiles_of(1025, 1024) == 2 and RL.tiles_of(16385) == 20 and RL.tiles_of(1 << 20) == 1024
    assert RL.sum_depth_large(1, 1024) == 27 and RL.sum_depth_large(65536) == 27 and RL.sum_depth_large(65537) == 28
    assert RL.sum_depth_large(1 << 20) == 42


def test_batch_scope_is_the_statement_on_the_reshape():
    x, label, inner = R.lovasz_inputs(4, 257, 5)
    for probs in (None, R.softmax64(x)[0].astype(np.float32)):
        got = lovasz.lovasz_reference(x, label, inner, probs=probs, scope="batch")
        flat = None if probs is None else probs.reshape(1, -1, 5)
        want = lovasz.lovasz_reference(x.reshape(1, -1, 5), label.reshape(1, -1), inner.reshape(1, -1), probs=flat)
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), k
        assert got["loss"].shape == (1,) and got["order"].shape == (1, 5, 4 * 257) and got["n_valid"][0] == R.valid_rows(label, inner).sum()
    block = lovasz.lovasz_reference(x, label, inner)
    assert np.array_equal(lovasz.lovasz_reference(x, label, inner, scope="block")["loss"], block["loss"])
    assert abs(got["loss"][0] - block["loss"].sum()) > 1e-3                # (not the sum of the blocks' losses)
    with pytest.raises(ValueError):
        lovasz.lovasz_reference(x, label, inner, scope="image")


def _paper_lovasz_softmax_flat(p, label, valid, C):
    """Berman et al., lovasz_softmax(per_image=False, classes='present') in float64: all rows of the batch flattened, per present
    class errors |fg - p_c| sorted descending, dotted with the first differences of 1 - intersection / union, the mean over classes"""
    p, label = p.reshape(-1, C)[valid.reshape(-1)], label.reshape(-1)[valid.reshape(-1)]
    losses = []
    for c in range(C):
        fg = (label == c).astype(np.float64)
        if fg.sum() == 0:
            continue
        errors = np.abs(fg - p[:, c])
        perm = np.argsort(-errors, kind="stable")
        gt = fg[perm]
        gts = gt.sum()
        jaccard = 1.0 - (gts - np.cumsum(gt)) / (gts + np.cumsum(1.0 - gt))
        jaccard[1:] = jaccard[1:] - jaccard[:-1]
        losses.append(float(np.dot(errors[perm], jaccard)))
    return float(np.mean(losses)) if losses else 0.0


def test_batch_scope_is_the_papers_per_image_false():
    """inputs without exact ties of e: random logits of scale 1 (the planted copies of lovasz_inputs are not used)"""
    rng = np.random.RandomState(21)
    B, N, C = 3, 333, 6
    x = rng.randn(B, N, C)
    label = rng.randint(0, C - 1, (B, N))                      # the last class is absent
    label[rng.rand(B, N) < 0.05] = R.IGNORE
    inner = (rng.rand(B, N) < 0.8).astype(np.float32)
    ref = lovasz.lovasz_reference(x, label, inner, scope="batch")
    valid = R.valid_rows(label, inner)
    for c in range(C):
        e = np.where(label == c, 1.0 - ref["probs"][0, :, c].reshape(B, N), ref["probs"][0, :, c].reshape(B, N))[valid]
        assert len(np.unique(e)) == len(e)
    want = _paper_lovasz_softmax_flat(R.softmax64(x)[0], label, valid, C)
    assert abs(ref["loss"][0] - want) <= 1e-12 and not ref["present"][0, C - 1] and ref["present"][0, :C - 1].all()


def test_loss_on_cpu_tensors_with_batch_scope():
    x, label, inner = R.lovasz_inputs(4, 257, 5)
    pred, lab, inn = torch.from_numpy(x).double(), torch.from_numpy(label), torch.from_numpy(inner)
    flat = lovasz.lovasz_torch(pred.reshape(1, -1, 5), lab.reshape(1, -1), inn.reshape(1, -1))
    ref = lovasz.lovasz_reference(x, label, inner, scope="batch")
    assert flat.shape == (1,) and abs(float(flat) - ref["loss"][0]) <= 1e-12
    assert torch.equal(lovasz.lovasz_torch(pred, lab, inn, scope="batch"), flat)
    for large in (False, True):
        assert torch.equal(lovasz.loss(pred, lab, inn, scope="batch", large=large), flat.sum())
        assert torch.equal(lovasz.loss(pred, lab, inn, large=large), lovasz.lovasz_torch(pred, lab, inn).sum())
    assert torch.equal(lovasz.loss(pred, lab, scope="batch"), lovasz.lovasz_torch(pred.reshape(1, -1, 5), lab.reshape(1, -1)).sum())
    calls = []

    def xent(p, l, *rest):
        calls.append(len(rest))
        return p.sum() * 0.0 + 2.0
    got = lovasz.with_xent(xent, 0.5, scope="batch", large=True)(pred, lab, inn)
    assert abs(float(got) - (2.0 + 0.5 * ref["loss"][0])) <= 1e-12 and calls == [1]
    with pytest.raises(ValueError):
        lovasz.loss(pred, lab, inn, scope="image")
    with pytest.raises(ValueError):
        lovasz.with_xent(xent, scope="image")
