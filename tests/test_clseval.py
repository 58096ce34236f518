"""harness/clseval.py's numpy statement against a literal restatement of modelnet40_cls/evaluate_modelnet.py:180-207, the merge of
the ranks' shares, the batch statement against objfeed's, and harness/objio.py's records.  No GPU."""
import os
import struct

import numpy as np
import pytest

from sph3d_gcn_amd.harness import blockio, clseval, feed, objfeed, objio

from _clseval_cases import KINDS, same_result, vote_logits


# ---------------------------------------------------------------------------------------------------------------
# the vote
# ---------------------------------------------------------------------------------------------------------------
def _literal(logits, batch_label, NUM_CLASSES):
    """evaluate_modelnet.py:180-207 for one batch, its names kept"""
    BATCH_SIZE = bsize = batch_label.shape[0]
    total_seen_class = [0 for _ in range(NUM_CLASSES)]
    total_correct_class = [0 for _ in range(NUM_CLASSES)]
    batch_pred_sum = np.zeros((BATCH_SIZE, NUM_CLASSES))  # score for classes
    with np.errstate(invalid="ignore"):
        for vote_idx in range(len(logits)):
            pred_val = logits[vote_idx]
            batch_pred_sum += pred_val
    pred_val = np.argmax(batch_pred_sum, 1)
    correct = np.sum(pred_val[0:bsize] == batch_label[0:bsize])
    for i in range(0, bsize):
        l = batch_label[i]
        total_seen_class[l] += 1
        total_correct_class[l] += (pred_val[i] == l)
    return batch_pred_sum, pred_val, int(correct), bsize, total_seen_class, total_correct_class


@pytest.mark.parametrize("V", [1, 2, 12])
@pytest.mark.parametrize("C", [1, 2, 40, 64])
def test_vote_reference_is_the_literal_loop(C, V):
    """float64 sums as bit patterns, predictions, totals and per-class counts, on ties, NaN, +-inf and -0.0 against +0.0"""
    for B in (1, 3, 32):
        for shift in range(KINDS):
            logits = vote_logits(B, C, V, 100 * C + V, shift)
            labels = np.random.RandomState(B + shift).randint(0, C, B).astype(np.int32)
            got = clseval.vote_reference(logits, labels, C)
            sums, pred, correct, seen, class_seen, class_correct = _literal(logits, labels, C)
            assert got.sums.dtype == np.float64 and np.array_equal(got.sums.view(np.int64), sums.view(np.int64))
            assert np.array_equal(got.pred, pred) and got.pred.dtype == np.int32
            assert (got.seen, got.correct, got.bad_label) == (seen, correct, 0)
            assert got.class_seen.tolist() == class_seen and got.class_correct.tolist() == [int(c) for c in class_correct]
            assert got.nonfinite == int((~np.isfinite(sums)).any(axis=1).sum())


def test_vote_reference_special_values():
    """the rules spelled out: the first maximum, a NaN is a maximum, np.zeros + -0.0 is +0.0, the sum is float64 not fp32"""
    z = np.float32(-0.0)
    got = clseval.vote_reference([np.array([[z, 0.0, z]], np.float32)], [1], 3)
    assert got.pred.tolist() == [0] and not np.signbit(got.sums).any() and got.correct == 0
    got = clseval.vote_reference([np.array([[1.0, np.nan, 7.0, np.nan]], np.float32)], [1], 4)
    assert got.pred.tolist() == [1] and got.nonfinite == 1 and got.correct == 1
    got = clseval.vote_reference([np.array([[np.inf, 3.0]], np.float32), np.array([[-np.inf, 3.0]], np.float32)], [0], 2)
    assert np.isnan(got.sums[0, 0]) and got.pred.tolist() == [0]
    # fp32 would lose the 1: (2^24 + 1) - 2^24 is 1 in float64 and 0 in fp32, and the arg-max differs
    votes = [np.array([[2.0 ** 24, 0.5]], np.float32), np.array([[1.0, 0.0]], np.float32), np.array([[-2.0 ** 24, 0.0]], np.float32)]
    got = clseval.vote_reference(votes, [0], 2)
    assert got.sums.tolist() == [[1.0, 0.5]] and got.pred.tolist() == [0]
    fp32 = votes[0] + votes[1] + votes[2]
    assert fp32.tolist() == [[0.0, 0.5]]
    # a label outside [0, C) counts in bad_label only
    got = clseval.vote_reference([np.zeros((3, 2), np.float32)], [0, 2, -1], 2)
    assert (got.seen, got.correct, got.bad_label) == (1, 1, 2) and got.class_seen.tolist() == [1, 0]
    with pytest.raises(ValueError):
        clseval.vote_reference([np.zeros((3, 3), np.float32)], [0, 1, 1], 2)


# ---------------------------------------------------------------------------------------------------------------
# the result and its merge
# ---------------------------------------------------------------------------------------------------------------
def _recorded(P, B, C, V, seed):
    nb = feed.batches_per_epoch(P, B)
    sizes = [min(P, (i + 1) * B) - i * B for i in range(nb)]
    logits = {i: vote_logits(sizes[i], C, V, seed + i, i) for i in range(nb)}
    return lambda i, v: logits[i][v]


@pytest.mark.parametrize("keep", [False, True])
def test_merge_of_the_shares_equals_one_rank(keep):
    P, B, C, V = 23, 3, 5, 3
    category = np.random.RandomState(1).randint(0, C + 1, P).astype(np.int32)          # (some labels are C: bad_label)
    fn = _recorded(P, B, C, V, 7)
    one = clseval.evaluate_reference(fn, category, B, C, V, keep_votes=keep)
    assert one.shapes.tolist() == list(range(P)) and (one.pred >= 0).all() and one.bad_label == int((category == C).sum())
    assert one.seen + one.bad_label == P and one.batches == list(range(8)) and one.nonfinite > 0
    assert one.accuracy == one.correct / float(one.seen)
    assert one.mean_class_acc == np.mean(one.class_correct / one.class_seen.astype(np.float64))     # every class occurs
    for world in (2, 3):
        shares = [clseval.evaluate_reference(fn, category, B, C, V, rank=r, world=world, keep_votes=keep) for r in range(world)]
        assert all((s.pred >= 0).sum() == len(s.shapes) < P for s in shares)
        same_result(clseval.ClsResult.merge(shares), one)
        same_result(clseval.ClsResult.merge(shares[::-1]), one)
    with pytest.raises(ValueError):
        clseval.ClsResult.merge([one, one])


def test_classes_never_seen_are_nan_and_leave_the_mean():
    category = np.array([0, 0, 2], np.int32)
    res = clseval.evaluate_reference(lambda i, v: np.array([[3, 1, 2], [1, 3, 2], [1, 2, 3]], np.float32), category, 4, 3, 1)
    assert res.pred.tolist() == [0, 1, 2] and np.isnan(res.class_acc[1]) and res.class_acc[[0, 2]].tolist() == [0.5, 1.0]
    assert res.mean_class_acc == 0.75 and res.accuracy == 2 / 3.0
    empty = clseval.evaluate_reference(None, category, 4, 3, 1, rank=1, world=2)
    assert empty.seen == 0 and np.isnan(empty.accuracy) and np.isnan(empty.mean_class_acc) and (empty.pred == -1).all()


# ---------------------------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------------------------
SIZES = [1, 255, 256, 257, 700]


def _rows(seed=0):
    rng = np.random.RandomState(seed)
    return (rng.rand(sum(SIZES), 3) * 2.0 - 1.0).astype(np.float32)


def test_assemble_reference_copies_and_swaps():
    rows, off = _rows(), np.concatenate(([0], np.cumsum(SIZES)))
    ids = np.array([4, 2, -1, 1, 5, 0])
    for N in (1, 255, 256, 257):
        got = clseval.assemble_reference(SIZES, rows, ids, N, 3, 9, 0, 1, 1)
        assert got.points.dtype == np.float64 and got.index.dtype == np.int32 and got.source.dtype == np.float32
        for b, i in enumerate(ids):
            if not 0 <= i < len(SIZES):
                assert (got.index[b] == -1).all() and not got.points[b].any()
                continue
            n = min(SIZES[i], N)
            xyz = rows[off[i]:off[i] + n]
            assert got.index[b].tolist() == list(range(n)) + [-1] * (N - n) and not got.points[b, n:].any()
            assert np.array_equal(got.points[b, :n].astype(np.float32).view(np.int32), xyz[:, [0, 2, 1]].view(np.int32))
            assert np.array_equal(got.points[b, :n], xyz[:, [0, 2, 1]].astype(np.float64))
        plain = clseval.assemble_reference(SIZES, rows, ids, N, 3, 9, 0, 1, 0)
        assert np.array_equal(plain.source, got.source[:, :, [0, 2, 1]]) and np.array_equal(plain.index, got.index)


def test_assemble_reference_draws_are_objfeeds():
    rows, off = _rows(1), np.concatenate(([0], np.cumsum(SIZES)))
    ids = np.array([3, 0, 4, 1, 2])
    for N in (255, 257):
        want = objfeed.assemble_reference(SIZES, ids, N, 11, 1 << 21, 0).index
        assert np.array_equal(clseval.assemble_reference(SIZES, rows, ids, N, 11, 1 << 21, 0, 0, 0).index, want)
        assert np.array_equal(want, feed.assemble_reference(SIZES, ids, N, 11, 1 << 21, False).index)
        for mask in (1, 2, 4, 8, 15):
            for order in (0, 1):
                got = clseval.assemble_reference(SIZES, rows, ids, N, 11, 1 << 21, mask, order, 1)
                ref = objfeed.assemble_reference(SIZES, ids, N, 11, 1 << 21, mask)
                assert np.array_equal(got.index, want) if order == 0 else (got.index[2] == np.arange(N)).all()
                for b, i in enumerate(ids):
                    took = got.index[b] >= 0
                    swapped = rows[off[i] + got.index[b, took]][:, [0, 2, 1]]
                    t = objfeed.transform(swapped, mask, ref.theta[b], ref.tilt[b], ref.scale[b], ref.shift[b])
                    assert np.array_equal(got.points[b, took], t) and not np.array_equal(t, swapped.astype(np.float64))
                    assert not got.points[b, ~took].any()
    for bad in (16, 31, -1, [0, 1, 2, 3, 32]):
        with pytest.raises(ValueError):
            clseval.assemble_reference(SIZES, rows, ids, 8, 1, 1, bad, 1, 0)
    assert clseval.EVAL_AUGMENT == 15 and clseval.vote_recipe(0) == 0 and clseval.vote_recipe(5) == 15
    assert objfeed.train_recipe(4, "modelnet").max() == clseval.MASKS


# ---------------------------------------------------------------------------------------------------------------
# the records
# ---------------------------------------------------------------------------------------------------------------
def _cloud(n, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(n, 3).astype(np.float32), rng.randn(n, 3).astype(np.float32)


def test_record_round_trips(tmp_path):
    xyz, normal = _cloud(50, 0)
    a, b, label = objio.parse_modelnet(objio.encode_modelnet(xyz, normal, 37))
    assert np.array_equal(a.view(np.int32), xyz.view(np.int32)) and np.array_equal(b.view(np.int32), normal.view(np.int32)) and label == 37
    seg, part = np.arange(50) % 7 + 20, np.arange(50) % 7
    a, s, p, c = objio.parse_shapenet(objio.encode_shapenet(xyz, seg, part, 11))
    assert np.array_equal(a, xyz) and s.dtype == np.int32 and np.array_equal(s, seg) and np.array_equal(p, part) and c == 11
    a, s, p, c = objio.parse_shapenet(objio.encode_shapenet(xyz, seg, None, 3))
    assert np.array_equal(a, xyz) and np.array_equal(s, seg) and p is None and c == 3
    assert b"part_label" not in objio.encode_shapenet(xyz, seg, None, 3)
    for bad in (lambda: objio.encode_modelnet(xyz, normal[:49], 1), lambda: objio.encode_shapenet(xyz, seg[:49], None, 1),
                lambda: objio.parse_modelnet(objio.encode_shapenet(xyz, seg, part, 1)),
                lambda: objio.parse_shapenet(objio.encode_modelnet(xyz, normal, 1))):
        with pytest.raises(ValueError):
            bad()

    # files -> pools (on the CPU device: the pool is plain tensors)
    clouds = [_cloud(n, n) for n in (5, 9, 4)]
    path = [str(tmp_path / "m0.tfrecord"), str(tmp_path / "m1.tfrecord")]
    blockio.write_records(path[0], [objio.encode_modelnet(x, nn, k + 30) for k, (x, nn) in enumerate(clouds[:2])])
    blockio.write_records(path[1], [objio.encode_modelnet(clouds[2][0], clouds[2][1], 2)])
    pool = objio.shape_pool_from_records(path, "modelnet", device="cpu")
    assert pool.sizes.tolist() == [5, 9, 4] and pool.category.tolist() == [30, 31, 2]
    rows = pool.rows.numpy()
    assert np.array_equal(rows[:, 0:3], np.concatenate([x for x, _ in clouds])) and not rows[:, 3:6].any() and (rows[:, 7] == 1).all()
    assert rows[:, 6].tolist() == [30] * 5 + [31] * 9 + [2] * 4
    spath = str(tmp_path / "s.tfrecord")
    blockio.write_records(spath, [objio.encode_shapenet(x, np.arange(len(x)) % 2 + 4, np.arange(len(x)) % 2, 2) for x, _ in clouds])
    per_cat = objio.shape_pool_from_records([spath], "shapenet", device="cpu")
    onehot = objio.shape_pool_from_records([spath], "shapenet_onehot", part_lo=[0, 2, 4], part_n=[2, 2, 2], device="cpu")
    assert per_cat.category.tolist() == onehot.category.tolist() == [2, 2, 2] and per_cat.part_lo is None
    assert per_cat.rows[:, 6].tolist() == [k % 2 for n in (5, 9, 4) for k in range(n)]
    assert onehot.rows[:, 6].tolist() == [k % 2 + 4 for n in (5, 9, 4) for k in range(n)] and onehot.part_lo.tolist() == [0, 2, 4]
    opath = str(tmp_path / "o.tfrecord")
    blockio.write_records(opath, [objio.encode_shapenet(clouds[0][0], np.zeros(5), None, 0)])
    with pytest.raises(ValueError):
        objio.shape_pool_from_records([opath], "shapenet", device="cpu")          # the one-hot writer's records have no part_label
    with pytest.raises(ValueError):
        objio.shape_pool_from_records([opath], "scannet", device="cpu")


def _varint(n):
    out = bytearray()
    while True:
        out.append((n & 0x7F) | (0x80 if n >> 7 else 0))
        n >>= 7
        if not n:
            return bytes(out)


def _ld(field, payload):
    return _varint((field << 3) | 2) + _varint(len(payload)) + payload


def _hand_example(xyz, normal, label, packed):
    """a tf.train.Example from the protobuf wire rules alone: Example{1: Features{1: map entry{1: key, 2: Feature{1: BytesList{1:
    bytes} | 3: Int64List{1: int64, packed into one length-delimited field or one varint field per value}}}}}; the entries in
    the order the reference's writer names them"""
    def entry(key, feature):
        return _ld(1, _ld(1, key.encode()) + _ld(2, feature))
    int64_list = _ld(1, _varint(label)) if packed else _varint((1 << 3) | 0) + _varint(label)
    feats = (entry("normal_raw", _ld(1, _ld(1, normal.tobytes()))) + entry("label", _ld(3, int64_list))
             + entry("xyz_raw", _ld(1, _ld(1, xyz.tobytes()))))
    return _ld(1, feats)


@pytest.mark.parametrize("packed", [True, False])
def test_a_hand_assembled_modelnet_example_parses(packed):
    xyz, normal = _cloud(300, 5)                       # (300 * 12 bytes: a two-byte length varint)
    record = _hand_example(xyz, normal, 39, packed)
    a, b, label = objio.parse_modelnet(record)
    assert np.array_equal(a.view(np.int32), xyz.view(np.int32)) and np.array_equal(b.view(np.int32), normal.view(np.int32)) and label == 39
    if packed:                                         # the project's encoder writes the packed form, keys sorted
        again = blockio.decode_example(objio.encode_modelnet(xyz, normal, 39))
        assert again["xyz_raw"] == xyz.tobytes() and again["label"].tolist() == [39] and sorted(again) == ["label", "normal_raw", "xyz_raw"]


def test_truncated_and_corrupt_files_are_refused(tmp_path):
    records = [objio.encode_modelnet(*_cloud(20, k), k) for k in range(3)]
    good = str(tmp_path / "good.tfrecord")
    blockio.write_records(good, records)
    assert [s[2] for s in objio.read_shapes([good], "modelnet")] == [0, 1, 2]
    data = open(good, "rb").read()
    one = 8 + 4 + len(records[0]) + 4
    # the file ends inside: the last payload, the last CRC, a length word, a length's CRC
    for k, cut in enumerate((len(data) - 10, len(data) - 2, one + 5, one + 10)):
        path = str(tmp_path / ("cut%d.tfrecord" % k))
        open(path, "wb").write(data[:cut])
        with pytest.raises(IOError):
            objio.read_shapes([path], "modelnet")
        with pytest.raises(IOError):
            objio.shape_pool_from_records([path], "modelnet", device="cpu")
    for k, at in enumerate((one + 12 + 30, 3, one - 1)):           # a payload byte, a length byte, a CRC byte
        bad = bytearray(data)
        bad[at] ^= 0x10
        path = str(tmp_path / ("crc%d.tfrecord" % k))
        open(path, "wb").write(bytes(bad))
        with pytest.raises(IOError):
            objio.read_shapes([path], "modelnet")
    assert struct.unpack("<Q", data[:8])[0] == len(records[0]) and os.path.getsize(good) == 3 * one
