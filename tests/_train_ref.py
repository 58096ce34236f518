"""The optimiser updates of csrc/train.hip (sph3d_train_update) stated in float64, the per-element bounds the kernel and the
fp32 torch branch of harness/optim.py are held to, and a literal transcription of the reference's metric loops.

With g = s grad (s = grad_scale), u = 2^-24, and the fp32 VALUES of b1, b2, eps, lr_t (momentum, lr) the kernel receives:
  rule 0   m' = m + (1 - b1)(g - m);   v' = v + (1 - b2)(g g - v);   p' = p - (lr_t m') / (sqrt(v') + eps)
  rule 1   a' = mom a + g;             p' = p - (g lr + (a' mom) lr)
The bounds are derived, not measured: every fp32 operation rounds once, by at most u times the magnitude of its result, and a
result is at most the sum of the magnitudes of its terms; gamma(k) = k u / (1 - k u) covers k roundings on one path with their
higher-order products.  Nothing is tuned.

m'   terms |m| and c1 (|g| + |m|), c1 = 1 - b1.  Roundings on the longest path, that of g: `s * grad` (1), `g - m` (1),
     `1.f - b1` (1), the product (1), the sum (1): 5.                             E_m = gamma(5) (|m| + c1 (|g| + |m|))
v'   terms |v| and c2 (g g + |v|).  g enters twice (2), `g * g` (1), `- v` (1), `1.f - b2` (1), the product (1), the sum (1): 7.
                                                                                  E_v = gamma(7) (|v| + c2 (g g + |v|))
sqrt correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt).  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) is at
     most |a - b| / sqrt(b) and at most sqrt(|a - b|):                            E_r = min(E_v / sqrt(v'), sqrt(E_v))
                                                                                  E_s = E_r + u (sqrt(v') + E_r)
den  = s + eps, one rounding:                                                     E_d = E_s + u (den + E_s)
num  = lr_t m', one rounding:                                                     E_n = lr_t E_m + u (|num| + lr_t E_m)
q    = num / den, correctly rounded; |x/y - X/Y| <= (|x - X| + |X/Y| |y - Y|) / |y|, |y| >= den - E_d:
                                                                                  E_q = (E_n + |q| E_d) / (den - E_d), + u (|q| + that)
p'   = p - q, one rounding:                                                       E_p = E_q + u (|p| + |q| + E_q)
rule 1:  a': `s * grad` (1), `mom * a` (1), the sum (1): 3.                       E_a = gamma(3) (|mom a| + |g|)
     upd = g lr + (a' mom) lr: per term the longest path has 3 roundings (g or the product a' mom, the product with lr, the
     sum), and a' carries E_a:                                                    E_w = gamma(3) (|g lr| + |a' mom lr|) + mom lr E_a (1 + gamma(3))
                                                                                  E_p = E_w + u (|p| + |upd| + E_w)
A gradient of exactly 0 on m = v = 0 (a = 0) makes every operation exact: p' = p - 0 / (0 + eps) = p; the bound still holds
u |p| from the last line, so the tests ask for equality there themselves.
E_p is close to u |p| wherever the update is far below an ulp of p, and the last subtraction alone may round by u |p'|: a kernel
that is right uses nearly all of the bound on such elements (measured: 0.99)."""
import numpy as np

U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(x):
    return float(np.float32(x))


def lr_t(lr, b1, b2, step):
    """what sph3d_train_update forms on the host: double arithmetic on the fp32 values, rounded once"""
    lr, b1, b2 = f32(lr), f32(b1), f32(b2)
    return f32(lr * (1.0 - b2 ** float(step)) ** 0.5 / (1.0 - b1 ** float(step)))


def tf_adam_ref(p, grad, m, v, lr, b1, b2, eps, step, grad_scale=1.0):
    """-> (p', m', v'), (E_p, E_m, E_v): float64 results from fp32 state arrays, and the per-element bounds"""
    p, grad, m, v = (np.asarray(x, np.float32).astype(np.float64) for x in (p, grad, m, v))
    b1, b2, eps, s, lt = f32(b1), f32(b2), f32(eps), f32(grad_scale), lr_t(lr, b1, b2, step)
    c1, c2 = 1.0 - b1, 1.0 - b2
    g = s * grad
    with np.errstate(invalid="ignore"):
        m1 = m + c1 * (g - m)
        v1 = v + c2 * (g * g - v)
        root = np.sqrt(v1)
        den = root + eps
        num = lt * m1
        q = num / den
        p1 = p - q
    e_m = gamma(5) * (np.abs(m) + c1 * (np.abs(g) + np.abs(m)))
    e_v = gamma(7) * (np.abs(v) + c2 * (g * g + np.abs(v)))
    with np.errstate(divide="ignore", invalid="ignore"):
        e_r = np.where(root > 0, np.minimum(e_v / root, np.sqrt(e_v)), np.sqrt(e_v))
    e_s = e_r + U * (root + e_r)
    e_d = e_s + U * (den + e_s)
    e_n = lt * e_m + U * (np.abs(num) + lt * e_m)
    ok = np.isfinite(g)                  # (elements with a non-finite gradient have no bound: NaN, the caller leaves them out)
    assert (den[ok] > 2 * e_d[ok]).all(), "the denominator's bound must stay far from the denominator"
    with np.errstate(invalid="ignore"):
        e_q = (e_n + np.abs(q) * e_d) / (den - e_d)
        e_q = e_q + U * (np.abs(q) + e_q)
        e_p = e_q + U * (np.abs(p) + np.abs(q) + e_q)
    return (p1, m1, v1), (e_p, e_m, e_v)


def torch_adam_ref(p, grad, m, v, lr, b1, b2, eps, step):
    """torch.optim.Adam's form in float64 (sph3d_adam_step): p' = p - lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps)"""
    p, grad, m, v = (np.asarray(x, np.float32).astype(np.float64) for x in (p, grad, m, v))
    b1, b2, eps, lr = f32(b1), f32(b2), f32(eps), f32(lr)
    m1 = m + (1.0 - b1) * (grad - m)
    v1 = b2 * v + (1.0 - b2) * grad * grad
    bc1, bc2 = 1.0 - b1 ** float(step), 1.0 - b2 ** float(step)
    return p - lr / bc1 * m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps), m1, v1


def nesterov_ref(p, grad, a, lr, mom, grad_scale=1.0):
    """-> (p', a'), (E_p, E_a)"""
    p, grad, a = (np.asarray(x, np.float32).astype(np.float64) for x in (p, grad, a))
    lr, mom, s = f32(lr), f32(mom), f32(grad_scale)
    g = s * grad
    a1 = mom * a + g
    upd = g * lr + (a1 * mom) * lr
    p1 = p - upd
    e_a = gamma(3) * (np.abs(mom * a) + np.abs(g))
    e_w = gamma(3) * (np.abs(g * lr) + np.abs(a1 * mom * lr)) + mom * lr * e_a * (1.0 + gamma(3))
    e_p = e_w + U * (np.abs(p) + np.abs(upd) + e_w)
    return (p1, a1), (e_p, e_a)


def why_inputs(rng, n):
    """the input distribution of the issue's comparison: gradients N(0,1) 10^U(-6,-1), p ~ N(0, 0.1)"""
    g = (rng.randn(n) * 10.0 ** rng.uniform(-6, -1, n)).astype(np.float32)
    p = (rng.randn(n) * 0.1).astype(np.float32)
    return p, g


def wide_inputs(rng, n):
    """gradients of magnitudes 10^U(-12, 12) with random signs (g g neither overflows nor goes denormal in fp32), some exactly 0"""
    g = (np.where(rng.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-12, 12, n)).astype(np.float32)
    g[rng.rand(n) < 0.1] = 0.0
    p = (rng.randn(n) * 0.1).astype(np.float32)
    return p, g


def worst(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0) and the elements outside"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return float(ratio.max()) if ratio.size else 0.0, int((err > bound).sum())


# ---------------------------------------------------------------------------------------------------------------
# train_s3dis.py:461-492, line by line (the loops over blocks and classes as they stand there)
# ---------------------------------------------------------------------------------------------------------------
def literal_eval_counts(pred_val, batch_label, batch_inner, num_classes):
    """-> total_correct, total_seen, total_seen_class, total_correct_class, total_union_class, class_acc, class_iou"""
    total_correct = 0
    total_seen = 0
    total_seen_class = [0 for _ in range(num_classes)]
    total_correct_class = [0 for _ in range(num_classes)]
    total_union_class = [0 for _ in range(num_classes)]
    bsize = pred_val.shape[0]
    pred_label = np.argmax(pred_val, 2)
    for b in range(bsize):
        inIdx = (batch_inner[b] == 1)
        correct = np.sum(pred_label[b, inIdx] == batch_label[b, inIdx])
        total_correct += correct
        total_seen += sum(batch_inner[b])
        for l in range(num_classes):
            total_seen_class[l] += np.sum(batch_label[b, inIdx] == l)
            total_correct_class[l] += (np.sum((pred_label[b, inIdx] == l) & (batch_label[b, inIdx] == l)))
            total_union_class[l] += (np.sum((pred_label[b, inIdx] == l) | (batch_label[b, inIdx] == l)))
    class_iou = [total_correct_class[l] / (float(total_union_class[l]) + np.finfo(float).eps) for l in range(num_classes)]
    class_acc = [total_correct_class[l] / (float(total_seen_class[l]) + np.finfo(float).eps) for l in range(num_classes)]
    return total_correct, total_seen, total_seen_class, total_correct_class, total_union_class, class_acc, class_iou


def metric_case(rng, B, N, C, with_inner=True):
    """logits with tied maxima, a NaN and an inf, labels -1 and C, and (with_inner, B > 1) one block whose inner is all zero"""
    logits = rng.randn(B, N, C).astype(np.float32)
    logits[rng.rand(B, N, C) < 0.3] = 1.5                 # ties, among them tied maxima
    label = rng.randint(0, C, (B, N)).astype(np.int32)
    flat_l, flat_x = label.reshape(-1), logits.reshape(B * N, C)
    R = B * N
    flat_x[rng.randint(R), rng.randint(C)] = np.nan
    flat_x[rng.randint(R), rng.randint(C)] = np.inf
    flat_x[rng.randint(R), rng.randint(C)] = -np.inf
    if R >= 4:
        flat_l[rng.randint(R)] = -1
        flat_l[rng.randint(R)] = C
    inner = None
    if with_inner:
        inner = (rng.rand(B, N) < 0.6).astype(np.int32)
        if B > 1:
            inner[B // 2] = 0
    return logits, label, inner
