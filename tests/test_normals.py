"""harness/normals.py, the numpy statement of the normal kernels, against plain Python integers and hand-made geometry.  No GPU."""
import numpy as np
import pytest

from sph3d_gcn_amd.harness import normals as nrm


def _python_moments(database, query, idx, cnt, radius):
    """one cloud, Python ints and floats only -> (moments as lists, skipped)"""
    q_scale = 262144.0 / float(np.float32(radius))
    out, skipped = [], 0
    K = idx.shape[1]
    for m in range(query.shape[0]):
        row = [0] * 10
        for k in range(min(max(int(cnt[m]), 0), K)):
            i = int(idx[m, k])
            if not 0 <= i < database.shape[0]:
                skipped += 1
                continue
            d = [float(np.float32(database[i, a]) - np.float32(query[m, a])) for a in range(3)]
            u = [x * q_scale for x in d]
            if not all(abs(x) <= 2097152.0 for x in u):           # (a NaN compares false)
                skipped += 1
                continue
            t = [round(x) for x in u]                             # (Python rounds halves to even)
            row[0] += 1
            for a in range(3):
                row[1 + a] += t[a]
            for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                row[4 + j] += t[a] * t[b]
        out.append(row)
    return out, skipped


def _hand_case():
    """radius 1: Q = 2^18, so an offset of 8 quantises to exactly 2^21 (the limit) and the next fp32 above 8 lies beyond it"""
    beyond = np.nextafter(np.float32(8.0), np.float32(9.0))
    database = np.array([[0, 0, 0], [0.25, -0.5, 0.125], [8.0, 0, 0], [beyond, 0, 0], [np.nan, 0, 0], [0, np.inf, 0],
                         [1e-6, 3e-6, -2e-6], [0.1, 0.2, 0.3], [-8.0, -8.0, 8.0], [0.5 ** 19, 1.5 * 0.5 ** 18, 2.5 * 0.5 ** 18]],
                        dtype=np.float32)
    query = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [np.nan, 0, 0], [0, 0, 0]], dtype=np.float32)
    idx = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 1, 0], [1, 2, 3, 4], [3, 3, 3, 3], [0, 1, 2, 3], [1, 12, -1, 7]], dtype=np.int32)
    cnt = np.array([4, 4, 9, 0, 1, 4, 4], dtype=np.int32)                   # (9 > K: the first K count)
    return database, query, idx, cnt


def test_moments_equal_a_python_integer_loop():
    database, query, idx, cnt = _hand_case()
    ref = nrm.graph_normals_reference(database[None], query[None], idx[None], cnt[None], 1.0, None, 3)
    want, skipped = _python_moments(database, query, idx, cnt, 1.0)
    assert ref.moments[0].tolist() == want
    assert ref.skipped == skipped
    assert ref.count[0].tolist() == [3, 2, 4, 0, 0, 0, 2]
    # the neighbour at the limit counts with t = 2^21, the one just beyond it does not
    assert ref.moments[0, 0].tolist()[0:5] == [3, 65536 + 2097152, -131072, 32768, 65536 ** 2 + 2097152 ** 2]
    # halves round to even: (0.5, 1.5, 2.5) -> (0, 2, 2)
    t, valid = nrm.quantise(database[9][None] - query[0][None], 1.0)
    assert valid.all() and t[0].tolist() == [0, 2, 2]
    # counts 0, 1 (skipped) and 2, a NaN query: zero rows
    assert ref.zero[0].tolist() == [False, True, False, True, True, True, True]
    assert not ref.normals[0][ref.zero[0]].any() and not ref.variation[0][ref.zero[0]].any()


def test_counts_below_min_count_and_bad_arguments():
    database, query, idx, cnt = _hand_case()
    for c, live in ((0, False), (1, False), (2, False), (3, True)):
        ref = nrm.graph_normals_reference(database[None], query[None, 0:1], np.array([[[1, 7, 6, 0]]], np.int32),
                                          np.array([[c]], np.int32), 1.0, None, 3)
        assert int(ref.count[0, 0]) == c and bool(ref.zero[0, 0]) == (not live)
    ref = nrm.graph_normals_reference(database[None], query[None, 0:1], np.array([[[1, 7, 6, 0]]], np.int32),
                                      np.array([[3]], np.int32), 1.0, None, 4)
    assert ref.zero.all()
    for radius, min_count in ((0.0, 3), (-1.0, 3), (np.inf, 3), (np.nan, 3), (1.0, 2)):
        with pytest.raises(ValueError):
            nrm.check_args(radius, min_count)


def _plane_cloud():
    rng = np.random.RandomState(5)
    xy = rng.randint(-64, 65, size=(200, 2)).astype(np.float32) / 128.0      # exactly representable, and so are the offsets
    return np.concatenate([xy, np.zeros((200, 1), np.float32)], axis=1)


def test_exact_plane():
    xyz = _plane_cloud()
    for toward, z in ((np.array([0.1, -0.2, 3.0], np.float32), 1.0), (np.array([0.1, -0.2, -3.0], np.float32), -1.0)):
        ref = nrm.ball_normals_reference(xyz, 0.3, toward, 3)
        live = ~ref.zero
        assert live.sum() > 150
        assert not ref.moments[:, [6, 8, 9]].any()                           # S2_xz, S2_yz, S2_zz
        assert (ref.normals[live] == np.array([0.0, 0.0, z], np.float32)).all()
        assert not ref.variation.any()
    ref = nrm.ball_normals_reference(xyz, 0.3, None, 3)
    assert (ref.normals[~ref.zero] == np.array([0.0, 0.0, 1.0], np.float32)).all()     # canonical: the largest component is positive


def test_three_collinear_points():
    xyz = np.array([[0.0, 0.0, 0.0], [0.125, 0.25, -0.125], [0.25, 0.5, -0.25]], dtype=np.float32)
    ref = nrm.ball_normals_reference(xyz, 1.0, None, 3)
    assert ref.count.tolist() == [3, 3, 3] and not ref.zero.any()
    line = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    n = ref.normals.astype(np.float64)
    assert (np.abs(np.sqrt((n * n).sum(axis=1)) - 1.0) <= 2.0 ** -23).all()
    assert (np.abs(n @ line) <= 2.0 ** -23).all()
    assert (ref.variation <= 2.0 ** -40).all()


def test_ball_form_is_the_graph_form_over_all_points_in_the_ball():
    import _normal_ref as nr
    xyz = nr.family("box", 300, 2)
    xyz[17] = [np.nan, 0.0, 0.0]
    xyz[18] = [0.0, np.inf, 0.0]
    ball = nrm.ball_normals_reference(xyz, 0.2, None, 3)
    idx, cnt = nr.plain_graph(xyz[None], xyz[None], 0.2, 300)
    graph = nrm.graph_normals_reference(xyz[None], xyz[None], idx, cnt, 0.2, None, 3)
    assert np.array_equal(ball.moments, graph.moments[0]) and graph.skipped == 0
    assert ball.count[17] == 0 and ball.count[18] == 0 and ball.zero[17] and ball.zero[18]
    assert np.array_equal(ball.normals, graph.normals[0]) and np.array_equal(ball.variation, graph.variation[0])
    some = np.array([5, 17, 250])
    assert np.array_equal(nrm.ball_moments_reference(xyz, 0.2, rows=some, chunk_elems=1000), ball.moments[some])
