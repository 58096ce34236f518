"""The inputs tests/test_clseval.py and tests/test_gpu_clseval.py share: injected logits with the values an arg-max and a float64
sum can get wrong, and the comparison of two ClsResults."""
import numpy as np

KINDS = 7


def vote_logits(B, C, V, seed, shift=0):
    """-> logits [V, B, C] fp32.  Cloud b is of kind (b + shift) % KINDS:
      0  plain random values
      1  an exact tie: every class the same value in every vote, so the first class wins
      2  a NaN in one class of one vote (a NaN is a maximum; with a second NaN in a later class the first still wins)
      3  +inf in one class, -inf in another
      4  +inf and, in a later vote, -inf in the SAME class (the sum is a generated NaN from vote 1 on); with V = 1 just -inf
      5  every logit -0.0 but one class +0.0: all sums are +0.0 (np.zeros + -0.0), so the first class wins
      6  two classes tie for the maximum after cancelling differences across the votes"""
    rng = np.random.RandomState(seed)
    x = (rng.randn(V, B, C) * 4.0).astype(np.float32)
    for b in range(B):
        kind, c0, c1, v0 = (b + shift) % KINDS, rng.randint(C), rng.randint(C), rng.randint(V)
        if kind == 1:
            x[:, b, :] = np.float32(1.25)
        elif kind == 2:
            x[v0, b, c0] = np.nan
            if c1 > c0:
                x[V - 1, b, c1] = np.nan
        elif kind == 3:
            x[v0, b, c0] = np.inf
            if c1 != c0:
                x[v0, b, c1] = -np.inf
        elif kind == 4:
            x[0, b, c0] = np.inf if V > 1 else -np.inf
            if V > 1:
                x[V - 1, b, c0] = -np.inf
        elif kind == 5:
            x[:, b, :] = np.float32(-0.0)
            x[:, b, c0] = np.float32(0.0)
        elif kind == 6:
            x[:, b, :] = np.float32(-3.0)
            x[:, b, c0] = x[:, b, c1] = np.float32(2.0)
            if V > 1 and c0 != c1:                      # the same float64 total by two different routes
                x[0, b, c0], x[1, b, c0] = np.float32(0.5), np.float32(3.5)
    return x


def same_f64(a, b):
    """two float64 arrays as bit patterns.  A NaN must be a NaN in both, but its sign and payload are not compared: they are the
    processor's choice, not a value (inf - inf is the negative default NaN on x86 and the positive one on CDNA)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


def same_result(a, b):
    """every field of two ClsResults"""
    for name in ("pred", "label", "class_seen", "class_correct", "shapes"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for name in ("seen", "correct", "nonfinite", "bad_label", "batches"):
        assert getattr(a, name) == getattr(b, name), name
    assert np.array_equal(a.class_acc, b.class_acc, equal_nan=True)
    for name in ("accuracy", "mean_class_acc"):
        x, y = getattr(a, name), getattr(b, name)
        assert x == y or (np.isnan(x) and np.isnan(y)), name
    assert (a.votes is None) == (b.votes is None)
    if a.votes is not None:
        assert a.votes.shape == b.votes.shape and np.array_equal(a.votes.view(np.int32), b.votes.view(np.int32))
