"""The canonical order of a transposed graph's entries (include/sph3d.h: sph3d_graph_canonical_order) stated in numpy: no torch,
no library.

Inside every segment (cloud, source, bin) the entries are ascending by row m; entries of equal m are ascending by the factor's
bit pattern read as an unsigned 32-bit integer.  A packed entry word is  m | nn_count[m] << 24: its row is word & 0xffffff and
its factor float32(1) / float32(word >> 24), so a packed and an un-packed build of one graph list the same (m, factor) sequence.
Entries that tie on both fields are identical, so the canonical arrays are unique.  That is the row order of
tests/_tgraph_ref.py::transpose_reference, which sorts its (segment, m, factor bits) rows by all three.

Everything here is an integer or a float's bit pattern (factors travel as uint32 so that a NaN keeps its payload)."""
import numpy as np

KEY_MASK = 0xffffff


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def segment_positions(offsets, B, L):
    """-> (pos int64 [E], seg int64 [E]): the positions of the entry arrays that hold an entry, ascending per cloud, and the
    segment b * L + n * F + f each belongs to (where the offsets put it)"""
    off = np.asarray(offsets).astype(np.int64).reshape(B, L + 1)
    pos, seg = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for b in range(B):
        sizes = np.diff(off[b])
        assert (sizes >= 0).all()
        pos.append(np.arange(off[b, 0], off[b, L], dtype=np.int64))
        seg.append(np.repeat(np.arange(L, dtype=np.int64) + b * L, sizes))
    return np.concatenate(pos), np.concatenate(seg)


def entry_fields(key, scale_bits):
    """(row m, factor bits) of entries, both int64.  scale_bits None: packed words"""
    if scale_bits is None:
        w = np.ascontiguousarray(key).view(np.uint32)
        with np.errstate(divide="ignore"):
            f = fbits(np.float32(1) / (w >> np.uint32(24)).astype(np.float32))
        return (w & np.uint32(KEY_MASK)).astype(np.int64), f.astype(np.int64)
    return np.ascontiguousarray(key).view(np.uint32).astype(np.int64), np.asarray(scale_bits, np.uint32).astype(np.int64)


def _permute(offsets, key, scale_bits, B, L, order_of):
    pos, seg = segment_positions(offsets, B, L)
    key = np.ascontiguousarray(key).copy()
    sb = None if scale_bits is None else np.asarray(scale_bits, np.uint32).copy()
    o = order_of(seg, key[pos], None if sb is None else sb[pos])
    np.testing.assert_array_equal(seg[o], seg)          # entries stay inside their segment
    key[pos] = key[pos][o]
    if sb is not None:
        sb[pos] = sb[pos][o]
    return key, sb


def canonical_order(offsets, key, scale_bits, B, L):
    """the statement: -> (key, scale_bits) with every segment in canonical order; what lies outside the segments is kept"""
    def order_of(seg, k, s):
        m, f = entry_fields(k, s)
        return np.lexsort((f, m, seg))
    return _permute(offsets, key, scale_bits, B, L, order_of)


def shuffle_segments(offsets, key, scale_bits, B, L, rng):
    """the same entries, permuted at random inside every segment"""
    return _permute(offsets, key, scale_bits, B, L, lambda seg, k, s: np.lexsort((rng.rand(seg.size), seg)))


def arrays_from_reference(offsets, triples, cnt, B, M, K, L, packed, fill=0x7f7f7f7f):
    """the entry arrays in canonical order from transpose_reference's sorted rows (segment, m, factor bits):
    -> (key int32 [B*M*K], scale_bits uint32 [B*M*K] | None); words outside the segments hold `fill`"""
    pos, seg = segment_positions(offsets, B, L)
    triples = np.asarray(triples, np.int64).reshape(-1, 3)
    np.testing.assert_array_equal(triples[:, 0], seg)
    n = max(B * M * K, 16)
    key = np.full(n, fill, np.uint32)
    m = triples[:, 1].astype(np.uint32)
    if packed:
        c = np.asarray(cnt).astype(np.uint32)[seg // L, triples[:, 1]]
        key[pos] = m | (c << np.uint32(24))
        return key.view(np.int32), None
    key[pos] = m
    sb = np.full(n, fill, np.uint32)
    sb[pos] = triples[:, 2].astype(np.uint32)
    return key.view(np.int32), sb
