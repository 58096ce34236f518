"""Farthest-point sampling held to the oracle at every launch form (csrc/sample.hip; the forms: csrc/fps_plan.hpp).
Every case of tests/_fps_forms.py's list is pinned to its form by the plan query before anything is launched, run at least twice
through the C entry with a workspace of the test's own, and every run's samples must be the oracle's, index for index
(tf_sample_gpu.cu:7-73 restated in oracle/).  The planted clouds make that equality decide the tie rule: tests/test_fps_forms.py
shows on the CPU that either wrong rule gives other samples on each of them.  After a co-operative launch the error word, the
first int of the workspace, must be 0: the samples are then that kernel's own and not its repair pass's."""
import time

import numpy as np
import pytest
import torch

import _fps_forms as S
import oracle
from sph3d_gcn_amd import _lib

pytestmark = pytest.mark.gpu


def _plan(b, n, m):
    out = np.zeros(len(S.FIELDS), np.int64)
    assert _lib.lib().sph3d_farthest_point_sample_plan(b, n, m, out.ctypes.data) == 0
    return dict(zip(S.FIELDS, out.tolist()))


def _sample(dev, pts_t, m, p):
    """one call of the entry -> samples [b, m], the error word (None where the plan has no co-operative launch)"""
    l = _lib.lib()
    b, n, _ = pts_t.shape
    need = l.sph3d_farthest_point_sample_workspace(b, n, m)
    assert need == p["workspace_bytes"]
    # (the samples start at -1 and the workspace at all ones: whatever the kernels leave unwritten or uncleared shows)
    out = torch.full((b, m), -1, dtype=torch.int32, device=dev)
    ws = torch.full((max(need, 4),), 0xff, dtype=torch.uint8, device=dev)
    _lib.check(l.sph3d_farthest_point_sample(b, n, m, _lib.ptr(pts_t), _lib.ptr(out), _lib.ptr(ws) if need else None, need,
                                             _lib.stream_ptr()))
    torch.cuda.synchronize()
    err = int(ws[:4].view(torch.int32).item()) if p["kernel"] == S.COOP else None
    return out.cpu().numpy(), err


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c[0])
def test_fps_form_equals_the_oracle(dev, case):
    name, claim, b, n, m, kind, _, launches = case
    p = _plan(b, n, m)
    assert {f: p[f] for f in claim} == claim, p                 # the form, before anything is launched
    pts = S.clouds(case)
    with np.errstate(invalid="ignore", over="ignore"):
        want = oracle.farthest_point_sample(m, pts)
    pts_t = torch.from_numpy(pts).to(dev)
    t0 = time.perf_counter()
    runs = [_sample(dev, pts_t, m, p) for _ in range(launches)]
    dt = (time.perf_counter() - t0) / launches
    print("\nFPS form %s: %d x %d -> %d, %.1f ms per call" % (name, b, n, m, dt * 1e3))
    for got, err in runs:
        # a raised error word: the co-operative pass gave up and the repair pass wrote the samples.  A finding, not a retry
        assert err in (None, 0), "co-operative pass raised its error word"
        np.testing.assert_array_equal(got, want)
    for got, _ in runs[1:]:
        np.testing.assert_array_equal(got, runs[0][0])
    # what the case is there for, said of the expected samples themselves
    if m == 1:
        assert want.tolist() == [[0]] * b
    if "every-point" in name:
        assert all(sorted(row) == list(range(n)) for row in want.tolist())
    if name == "plain1-one-point":
        assert want.tolist() == [[0, 0, 0]] * b
    if "m-past-n" in name:
        assert sorted(want[0, :n].tolist()) == list(range(n)) and want[0, n:].tolist() == [0] * (m - n) and m - n >= 3
