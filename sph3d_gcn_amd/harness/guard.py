"""The guarded update stated in numpy: clip by the global norm, skip a step whose gradient is not finite, keep an exponential
moving average of the weights.  There is no reference counterpart (the reference's loop has none of the three); like knn, fuzzy and
lovasz this statement is the yardstick: csrc/train.hip (sph3d_train_update_guarded) is held to it bit for bit, and the CPU-tensor
branch of harness/optim.py calls it.

Per step: the flat gradient g (fp32 [n], the alignment padding included: it is zero), grad_scale s, the options clip_norm (None
or > 0), skip_nonfinite, ema_decay (None or in (0, 1)); the kernel receives the fp32 values of s, lr, the betas, eps, clip_norm and
ema_decay, and so does the statement.  A state of STATE_WORDS 8-byte words (include/sph3d.h has the same layout) is carried from
step to step.

 1. gg0_i = fl32(s g_i): the element sph3d_train_update forms.                                                     (scaled)
 2. bad = #{i : gg0_i is not finite}.
 3. S = the sum of (double)gg0_i^2 — each square is exact in float64 — in ONE fixed order: LANES = 2^18 lanes, lane l adds the
    elements i = l (mod LANES) in ascending i starting from +0.0, and the lane sums are reduced by the adjacent-pair tree
    a <- a[0::2] + a[1::2] until one value is left; norm = sqrt(S) in float64.  All terms are >= 0, so S is within
    (ceil(n / LANES) + 18) 2^-53 relative of the exact sum.  With a NaN among the squares S is a NaN whose payload is left
    open (IEEE 754 does not fix it); nothing reads S then.                                                         (sumsq)
 4. skip = skip_nonfinite and bad > 0: skipped += 1, bad is added to the nonfinite word, the flag becomes 0 and NOTHING else
    changes: parameters, slots, EMA and the running powers keep their bits.
 5. otherwise the update is applied: applied += 1; rule 0: b1pow *= (double)fl32(b1), b2pow *= (double)fl32(b2) (running powers
    in float64, as TensorFlow keeps its beta*_power variables: lr_t is a function of the APPLIED count, which only the device
    knows) and lr_t = fl32(lr sqrt(1 - b2pow) / (1 - b1pow)) formed in float64; rule 1: lr_t = fl32(lr).
    c = clip_norm / (norm + 1e-6) in float64; clipped = clip_norm is not None and bad == 0 and c < 1; c32 = fl32(c) when
    clip_norm is not None and bad == 0, else 1.  gg_i = fl32(c32 gg0_i) if clipped else gg0_i, then sph3d_train_update's rule 0
    or 1 on gg, operation for operation in fp32.  With an EMA and a = the updates applied before this one:
    d = min(ema_decay, (1 + a) / (10 + a)) (tf.train.ExponentialMovingAverage(decay, num_updates)), om = fl32(1 - d),
    e_i <- e_i - fl32(fl32(e_i - p'_i) om).  clipped_steps += clipped, last_norm = norm, max_norm_seen = norm where norm is
    greater (a NaN norm never replaces it); the flag becomes 1, or 3 when clipped.                                  (decide, apply)
 6. skip_nonfinite off and bad > 0: sph3d_train_update's behaviour — the NaN propagates — and bad is added to the nonfinite word.
"""
import collections
import math

import numpy as np

LANES = 1 << 18
STATE_WORDS = 16
S, BAD, APPLIED, SKIPPED, CLIPPED, B1POW, B2POW, LAST_NORM, MAX_NORM, LR_T, C32, OM, FLAG = range(13)
FIELDS = ("S", "bad", "applied", "skipped", "clipped_steps", "b1pow", "b2pow", "last_norm", "max_norm_seen", "lr_t", "c32", "om",
          "flag")
_DOUBLE = (S, B1POW, B2POW, LAST_NORM, MAX_NORM, LR_T, C32, OM)
RULE_TF_ADAM, RULE_NESTEROV = 0, 1

GuardStats = collections.namedtuple("GuardStats", "applied skipped clipped_steps last_norm max_norm_seen")


def f32(x):
    return float(np.float32(x))


def new_state():
    """-> int64 [STATE_WORDS]: every word 0 except b1pow = b2pow = 1.0 and flag = 1 (no step was skipped yet)"""
    w = np.zeros(STATE_WORDS, np.int64)
    w.view(np.float64)[[B1POW, B2POW]] = 1.0
    w[FLAG] = 1
    return w


def fields(words):
    """the state's words by name: the float64 words as floats, the others as ints"""
    words = np.ascontiguousarray(words, dtype=np.int64)
    f = words.view(np.float64)
    return {name: (float(f[k]) if k in _DOUBLE else int(words[k])) for k, name in enumerate(FIELDS)}


def stats(words):
    d = fields(words)
    return GuardStats(d["applied"], d["skipped"], d["clipped_steps"], d["last_norm"], d["max_norm_seen"])


def powers_after(beta1, beta2, applied):
    """b1pow, b2pow after `applied` updates from 1.0: iterated float64 products of the fp32 values"""
    b1, b2, p1, p2 = f32(beta1), f32(beta2), 1.0, 1.0
    for _ in range(int(applied)):
        p1 *= b1
        p2 *= b2
    return p1, p2


def lr_t_from_powers(lr, b1pow, b2pow):
    return f32(f32(lr) * math.sqrt(1.0 - b2pow) / (1.0 - b1pow))


def scaled(g, grad_scale):
    with np.errstate(all="ignore"):
        return np.float32(grad_scale) * np.asarray(g, dtype=np.float32).reshape(-1)


def sumsq(gg0):
    """S of the fp32 elements gg0, in the statement's order -> a Python float (float64)"""
    with np.errstate(all="ignore"):
        x = np.asarray(gg0, dtype=np.float32).reshape(-1).astype(np.float64)
        x = x * x
        n = x.size
        acc = np.zeros(LANES, np.float64)
        full = n // LANES
        for r in range(full):
            acc = acc + x[r * LANES:(r + 1) * LANES]
        rem = n - full * LANES
        if rem:
            acc[:rem] = acc[:rem] + x[full * LANES:]
        while acc.size > 1:
            acc = acc[0::2] + acc[1::2]
    return float(acc[0])


def measure(g, grad_scale):
    """-> gg0 (fp32 [n]), S, bad"""
    gg0 = scaled(g, grad_scale)
    return gg0, sumsq(gg0), int((~np.isfinite(gg0)).sum())


def decide(state, S_value, bad, rule, lr, beta1, beta2, clip_norm, skip_nonfinite, ema_decay, nonfinite=None):
    """steps 4 and 5 without the elements: updates `state` (int64 [STATE_WORDS]) in place from S and bad; nonfinite: an int64
    array whose word 0 grows by bad, or None -> True when the update is to be applied"""
    if rule not in (RULE_TF_ADAM, RULE_NESTEROV):
        raise ValueError("guard: rule 0 (Adam) or 1 (Nesterov momentum) required, got %r" % (rule,))
    f = state.view(np.float64)
    bad = int(bad)
    f[S] = S_value
    state[BAD] = bad
    if nonfinite is not None and bad:
        nonfinite[0] += bad
    if skip_nonfinite and bad:
        state[SKIPPED] += 1
        state[FLAG] = 0
        return False
    with np.errstate(all="ignore"):
        norm = float(np.sqrt(np.float64(S_value)))
    clipped, c32 = False, 1.0
    if clip_norm is not None and bad == 0:
        with np.errstate(all="ignore"):
            c = float(np.float64(f32(clip_norm)) / (np.float64(norm) + np.float64(1e-6)))
            c32 = f32(c)
        clipped = c < 1.0
    before = int(state[APPLIED])
    state[APPLIED] = before + 1
    lr_t = f32(lr)
    if rule == RULE_TF_ADAM:
        f[B1POW] = f[B1POW] * f32(beta1)
        f[B2POW] = f[B2POW] * f32(beta2)
        lr_t = lr_t_from_powers(lr, float(f[B1POW]), float(f[B2POW]))
    om = 0.0
    if ema_decay is not None:
        om = f32(1.0 - min(f32(ema_decay), (1.0 + before) / (10.0 + before)))
    if clipped:
        state[CLIPPED] += 1
    f[LAST_NORM] = norm
    if norm > f[MAX_NORM]:
        f[MAX_NORM] = norm
    f[LR_T], f[C32], f[OM] = lr_t, c32, om
    state[FLAG] = 3 if clipped else 1
    return True


def apply(state, p, gg0, slot0, slot1, ema, rule, beta1_or_momentum, beta2, eps):
    """the elements of step 5, in place on the fp32 arrays p, slot0, slot1 (rule 0), ema (or None), from the state's lr_t, c32,
    om and flag; nothing is written when the flag says skip"""
    flag = int(state[FLAG])
    if flag == 0:
        return
    f = state.view(np.float64)
    lr, c32, om = np.float32(f[LR_T]), np.float32(f[C32]), np.float32(f[OM])
    one, b1 = np.float32(1.0), np.float32(beta1_or_momentum)
    with np.errstate(all="ignore"):
        gg = c32 * gg0 if flag & 2 else gg0
        if rule == RULE_TF_ADAM:
            c1, c2, eps = one - b1, one - np.float32(beta2), np.float32(eps)
            slot0[:] = slot0 + c1 * (gg - slot0)
            slot1[:] = slot1 + c2 * (gg * gg - slot1)
            p[:] = p - (lr * slot0) / (np.sqrt(slot1) + eps)
        else:
            slot0[:] = b1 * slot0 + gg
            p[:] = p - (gg * lr + (slot0 * b1) * lr)
        if ema is not None:
            ema[:] = ema - (ema - p) * om


def step(state, p, g, slot0, slot1, ema, rule, lr, beta1_or_momentum, beta2, eps, grad_scale=1.0, clip_norm=None,
         skip_nonfinite=False, ema_decay=None, nonfinite=None):
    """one guarded step, in place on the fp32 arrays and the state -> True when the update was applied"""
    for a in (p, g, slot0, slot1, ema):
        if a is not None and (a.dtype != np.float32 or a.ndim != 1 or a.size != p.size):
            raise ValueError("guard.step: flat float32 arrays of one length required")
    if (ema is None) != (ema_decay is None):
        raise ValueError("guard.step: ema and ema_decay go together")
    gg0, s_value, bad = measure(g, grad_scale)
    applied = decide(state, s_value, bad, rule, lr, beta1_or_momentum, beta2, clip_norm, skip_nonfinite, ema_decay, nonfinite)
    apply(state, p, gg0, slot0, slot1, ema, rule, beta1_or_momentum, beta2, eps)
    return applied
