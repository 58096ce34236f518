"""The pointwise products' launch choice, held on the host: the library's query sph3d_pointwise_gemm_plan (csrc/gemm.hip: gemm_plan,
which every entry point launches from) against tests/_gemm_forms.py, the restatement of the launchers as they stood before the
choice was gathered into that one function — field for field on a grid of ~340 000 plans and on every product shape of
tests/test_gpu_gemm_split.py and tests/test_gpu_gemm_xs.py, misaligned operands and streams without an exchange buffer included —
and the older shape queries against the plan.  No device is touched."""
import ctypes

import pytest

import _gemm_forms as G


@pytest.fixture(scope="module")
def query():
    from sph3d_gcn_amd import _lib
    fn = ctypes.CDLL(_lib.LIB_PATH).sph3d_pointwise_gemm_plan
    fn.restype = ctypes.c_int
    out = (ctypes.c_int * len(G.FIELDS))()

    def q(*case):
        assert fn(*case, out) == 0, case
        return tuple(out)
    return q


def test_plan_equals_the_old_launchers_on_the_grid(query):
    n, forms = 0, set()
    for case in G.grid():
        f = G.form(*case)
        assert query(*case) == tuple(f[k] for k in G.FIELDS), (case, f["tag"], dict(zip(G.FIELDS, query(*case))))
        forms.add(f["tag"])
        n += 1
    assert n == 4 * 22 * 22 * 22 * 8
    per_product = {p: sum(1 for t in forms if t.split()[0] == p and not t.endswith("none")) for p in G.NAMES}
    assert per_product["NN"] >= 15 and per_product["NT"] >= 11 and per_product["TN"] >= 18 and per_product["NNS"] >= 9, per_product
    # every form has its case, every case reaches the form it names
    assert {c[0] for c in G.FORM_CASES} == forms
    for c in G.FORM_CASES:
        assert G.form(*c[1:])["tag"] == c[0], c


def test_plan_equals_the_old_launchers_on_the_gpu_tests_product_shapes(query):
    """the shapes of tests/test_gpu_gemm_split.py and tests/test_gpu_gemm_xs.py (most are on the grid, a few ragged ones are not):
    forward and statistics (R, Ci -> Co), input gradient (R, Co -> Ci), weight gradient"""
    import ast
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    for name, var in (("test_gpu_gemm_split.py", "SHAPES"), ("test_gpu_gemm_xs.py", "XS_SHAPES")):
        tree = ast.parse(open(os.path.join(here, name)).read())
        shapes = [ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) and n.targets[0].id == var][0]
        assert len(shapes) >= 5
        for R, Ci, Co in shapes:
            for product, Cin, Cout in ((G.NN, Ci, Co), (G.NNS, Ci, Co), (G.NT, Co, Ci), (G.TN, Ci, Co)):
                for flags in ((a, m, x) for a in (0, 1) for m in (0, 1) for x in (0, 1)):
                    case = (product, R, Cin, Cout) + flags
                    assert query(*case) == tuple(G.form(*case)[k] for k in G.FIELDS), case


def test_shape_queries_read_the_plan(query):
    from sph3d_gcn_amd import _lib
    l = ctypes.CDLL(_lib.LIB_PATH)
    l.sph3d_pointwise_gemm_tn_workspace.restype = ctypes.c_size_t
    f = {k: i for i, k in enumerate(G.FIELDS)}
    for R in G.GRID_R:
        for Cin in G.GRID_C:
            for Cout in G.GRID_C:
                ws, nblk = l.sph3d_pointwise_gemm_tn_workspace(R, Cin, Cout), l.sph3d_pointwise_gemm_bnstats_blocks(R, Cin, Cout)
                assert ws == G.tn_workspace(R, Cin, Cout) and nblk == G.bnstats_blocks(R, Cin, Cout), (R, Cin, Cout)
                for aligned in (0, 1):
                    for mode in (0, 1):
                        # the workspace is the slab plan's (a stream without an exchange buffer), whichever plan takes the call
                        p = query(G.TN, R, Cin, Cout, aligned, mode, 0)
                        assert ws == (4 * p[f["nsplit"]] * Cin * Cout if p[f["reduce"]] else 0), (R, Cin, Cout, p)
                        for x in (0, 1):
                            assert query(G.NNS, R, Cin, Cout, aligned, mode, x)[f["stats_blocks"]] == nblk, (R, Cin, Cout)


def test_plan_without_an_exchange_buffer(query):
    """NN / NT / NNS keep tile and k-step and lose the exchange, TN takes its slab plan"""
    f = {k: i for i, k in enumerate(G.FIELDS)}
    seen = 0
    for c in G.FORM_CASES:
        tag, product, R, Cin, Cout, aligned, mode, _ = c
        with_x, without = query(product, R, Cin, Cout, aligned, mode, 1), query(product, R, Cin, Cout, aligned, mode, 0)
        if with_x[f["xs"]] == 1:
            assert without == with_x, c
            continue
        seen += 1
        assert without[f["xs"]] == 1
        if product == G.TN:
            assert without[f["bm"]] == 128 and without[f["reduce"]] == 1 and without[f["nsplit"]] > 1
        else:
            keep = [f[k] for k in ("pipe", "bm", "bn", "bk", "guard", "stats", "nsplit", "reduce", "stats_blocks")]
            assert [without[i] for i in keep] == [with_x[i] for i in keep] and without[f["kchunk"]] == 0
            assert without[f["grid"]] * with_x[f["xs"]] == with_x[f["grid"]]
    assert seen == 8


def test_query_validates_and_follows_the_process_mode(query):
    from sph3d_gcn_amd import _lib
    l = _lib.lib()
    out = (ctypes.c_int * len(G.FIELDS))()
    p = ctypes.cast(out, ctypes.c_void_p)
    for bad in ((4, 128, 64, 64, 1, 1, 1), (-1, 128, 64, 64, 1, 1, 1), (0, 0, 64, 64, 1, 1, 1), (0, 128, 0, 64, 1, 1, 1),
                (0, 128, 64, -3, 1, 1, 1), (0, 128, 64, 64, 2, 1, 1), (0, 128, 64, 64, 1, 2, 1), (0, 128, 64, 64, 1, -2, 1),
                (0, 128, 64, 64, 1, 1, 2)):
        assert l.sph3d_pointwise_gemm_plan(*bad, p) == -1, bad
    assert l.sph3d_pointwise_gemm_plan(0, 128, 64, 64, 1, 1, 1, None) == -1
    prev = l.sph3d_pointwise_gemm_mode(-1)
    try:
        for mode in (0, 1):
            l.sph3d_pointwise_gemm_mode(mode)
            assert l.sph3d_pointwise_gemm_plan(G.NN, 128, 32, 64, 1, -1, 1, p) == 0
            assert tuple(out) == query(G.NN, 128, 32, 64, 1, mode, 1)
    finally:
        l.sph3d_pointwise_gemm_mode(prev)
