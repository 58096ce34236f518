"""Adam over ONE flat fp32 parameter buffer (harness plumbing: train_s3dis.py:224 uses tf.train.AdamOptimizer).

On the GPU the update is one streaming kernel (csrc/optim.hip: sph3d_adam_step, torch.optim.Adam's arithmetic to 2e-6);
on CPU tensors (oracle-backed tests) it wraps torch.optim.Adam.  The surface a training loop needs from an optimiser is
kept: a settable learning rate (``lr`` / ``param_groups[0]['lr']``: the reference decays it every step), ``state_dict`` /
``load_state_dict`` for checkpoint / resume, ``zero_grad``.
"""
import torch

from .. import _lib
from . import guard as _guard


class FlatAdam:
    """torch.optim.Adam's form (eps outside the bias correction), not the reference's: FlatTFAdam below is tf.train.AdamOptimizer's.
    It has no guarded form (Guard below belongs to the reference's rules): asking for one raises ValueError."""

    def __init__(self, flat_param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, guard=None):
        if guard is not None:
            raise ValueError("FlatAdam has no guarded update: use FlatTFAdam or FlatNesterov with a Guard")
        if flat_param.dtype != torch.float32 or not flat_param.is_contiguous():
            raise ValueError("FlatAdam needs one contiguous float32 parameter buffer")
        self.p = flat_param
        self.b1, self.b2, self.eps = float(betas[0]), float(betas[1]), float(eps)
        self.t = 0
        # one group, torch-style, so that `for g in opt.param_groups: g['lr'] = ...` works on both branches
        self._groups = [{"params": [flat_param], "lr": float(lr), "betas": (self.b1, self.b2), "eps": self.eps}]
        if flat_param.is_cuda:
            self.m = torch.zeros_like(flat_param.data)
            self.v = torch.zeros_like(flat_param.data)
            self._torch = None
        else:
            self._torch = torch.optim.Adam([flat_param], lr=lr, betas=betas, eps=eps)

    @property
    def param_groups(self):
        # the wrapped optimiser's list is looked up on every access: torch.optim.Optimizer.load_state_dict REPLACES it, an alias
        # taken at construction would go stale after a resume and a per-step learning-rate decay would be ignored
        return self._torch.param_groups if self._torch is not None else self._groups

    @property
    def lr(self):
        return float(self.param_groups[0]["lr"])

    @lr.setter
    def lr(self, value):
        self.param_groups[0]["lr"] = float(value)

    @property
    def guard(self):
        return None

    @guard.setter
    def guard(self, value):
        if value is not None:
            raise ValueError("FlatAdam has no guarded update: use FlatTFAdam or FlatNesterov with a Guard")

    def step(self):
        if self._torch is not None:
            return self._torch.step()
        g = self.p.grad
        if g is None:                      # nothing was back-propagated: torch.optim.Adam skips such parameters too
            return
        if g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.p.device or g.numel() != self.p.numel():
            raise ValueError("FlatAdam: the gradient must be a contiguous float32 buffer on the parameter's device")
        self.t += 1
        _lib.check(_lib.lib().sph3d_adam_step(self.p.numel(), _lib.ptr(self.p.data), _lib.ptr(g), _lib.ptr(self.m), _lib.ptr(self.v),
                                              self.lr, self.b1, self.b2, self.eps, self.t, _lib.stream_ptr()))

    def zero_grad(self, set_to_none=False):
        if self._torch is not None:
            return self._torch.zero_grad(set_to_none=set_to_none)
        if self.p.grad is not None:
            if set_to_none:
                self.p.grad = None
            else:
                self.p.grad.zero_()

    def state_dict(self):
        if self._torch is not None:
            return self._torch.state_dict()
        return {"step": self.t, "exp_avg": self.m.clone(), "exp_avg_sq": self.v.clone(), "lr": self.lr,
                "betas": (self.b1, self.b2), "eps": self.eps}

    def load_state_dict(self, state):
        if self._torch is not None:
            return self._torch.load_state_dict(state)
        self.t = int(state["step"])
        self.m.copy_(state["exp_avg"])
        self.v.copy_(state["exp_avg_sq"])
        self.lr = state.get("lr", self.lr)


# ---------------------------------------------------------------------------------------------------------------
# the reference's own optimisers (train_s3dis.py:223-226), TensorFlow 1's arithmetic: csrc/train.hip, sph3d_train_update
# ---------------------------------------------------------------------------------------------------------------
RULE_TF_ADAM, RULE_NESTEROV = 0, 1


def _f32(x):
    """the float the kernel receives for a Python number"""
    import numpy as np
    return float(np.float32(x))


def tf_adam_lr_t(lr, beta1, beta2, step):
    """lr sqrt(1 - b2^step) / (1 - b1^step) as sph3d_train_update forms it: from the fp32 values of lr, b1, b2, in double,
    rounded to fp32 once (-> a Python float holding that fp32 value)"""
    lr, b1, b2 = _f32(lr), _f32(beta1), _f32(beta2)
    return _f32(lr * (1.0 - b2 ** float(step)) ** 0.5 / (1.0 - b1 ** float(step)))


GuardStats = _guard.GuardStats


class Guard:
    """The options of the guarded update (harness/guard.py is its statement) and what it carries from step to step on the
    parameter's device: the state words, the workspace of the partial sums and, with ema_decay, the averaged copy of the weights
    (initialised to the parameters when the guard is bound to them, as TensorFlow initialises the shadow).  clip_norm: None or
    > 0, the global norm the scaled gradient is clipped to; skip_nonfinite: a step whose gradient holds a NaN or an infinity
    changes nothing and is counted; ema_decay: None or in (0, 1).  Give it to one FlatTFAdam / FlatNesterov as `opt.guard`."""

    def __init__(self, clip_norm=None, skip_nonfinite=False, ema_decay=None):
        if clip_norm is not None and not (float(clip_norm) > 0.0 and _f32(clip_norm) > 0.0):
            raise ValueError("Guard: clip_norm should be None or > 0, got %r" % (clip_norm,))
        if ema_decay is not None and not 0.0 < _f32(ema_decay) < 1.0:
            raise ValueError("Guard: ema_decay should be None or in (0, 1), got %r" % (ema_decay,))
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.p = self.state = self.ema = self.workspace = None

    def bind(self, flat_param):
        """allocates the state, the workspace and the EMA for `flat_param` (once: a second call with the same buffer is a no-op)"""
        if self.p is flat_param:
            return self
        if self.p is not None:
            raise ValueError("Guard: already bound to another parameter buffer")
        self.p = flat_param
        dev = flat_param.device
        self.state = torch.from_numpy(_guard.new_state()).to(dev)
        self.ema = flat_param.detach().clone() if self.ema_decay is not None else None
        if flat_param.is_cuda:
            self.workspace = torch.empty(_lib.lib().sph3d_train_guard_workspace(flat_param.numel()), dtype=torch.uint8, device=dev)
        return self

    def options(self):
        return {"clip_norm": self.clip_norm, "skip_nonfinite": self.skip_nonfinite, "ema_decay": self.ema_decay}

    def words(self):
        """the state's words on the host (int64 [16]): one read, it waits for the work issued so far"""
        return self.state.cpu().numpy().copy()

    def read(self):
        """-> GuardStats(applied, skipped, clipped_steps, last_norm, max_norm_seen) in one host read"""
        return _guard.stats(self.words())

    def restore(self, dst, src):
        """dst <- src (flat fp32 buffers of one length) if the last step was skipped, decided on the device: one launch"""
        if dst.dtype != torch.float32 or src.dtype != torch.float32 or dst.numel() != src.numel() or not dst.is_contiguous() \
                or not src.is_contiguous() or dst.device != self.state.device or src.device != self.state.device:
            raise ValueError("Guard.restore: two contiguous float32 buffers of one length on the guard's device")
        if dst.is_cuda:
            _lib.check(_lib.lib().sph3d_guard_restore(dst.numel(), _lib.ptr(dst), _lib.ptr(src), _lib.ptr(self.state), _lib.stream_ptr()))
        elif int(self.state[_guard.FLAG]) == 0:
            dst.copy_(src)

    def start_from(self, applied, beta1, beta2):
        """a fresh state that has `applied` updates behind it (a checkpoint without a guard): the powers by iterated products"""
        w = _guard.new_state()
        w[_guard.APPLIED] = int(applied)
        w.view("float64")[[_guard.B1POW, _guard.B2POW]] = _guard.powers_after(beta1, beta2, applied)
        self.state.copy_(torch.from_numpy(w))
        if self.ema is not None:
            self.ema.copy_(self.p.detach())


class _FlatRule:
    """What FlatTFAdam and FlatNesterov share: FlatAdam's surface (``lr``, ``param_groups``, ``step``, ``zero_grad``,
    ``state_dict`` / ``load_state_dict``) plus ``grad_scale`` (the gradient is multiplied by it inside the update: 1 / world
    size replaces all_reduce(average=True)'s own launch) and ``nonfinite``, an int64 [1] tensor on the parameter's device that
    counts the gradient elements that were not finite (never read here: the training loop reads it when it logs).  On the HIP
    device a step is one sph3d_train_update launch; on CPU tensors the same formulas, operation by operation, in torch fp32.
    ``guard``: None, or a Guard — a step is then sph3d_train_update_guarded (on CPU tensors harness/guard.py's statement), the
    learning rate's bias correction follows the count of APPLIED updates on the device, and ``state_dict`` carries the guard's
    state and the EMA ("step" is then the applied count: saving reads it from the device)."""
    rule = None
    slots = ()
    guard = None

    def __init__(self, flat_param, lr, group):
        name = type(self).__name__
        if flat_param.dtype != torch.float32 or not flat_param.is_contiguous():
            raise ValueError("%s needs one contiguous float32 parameter buffer" % name)
        self.p = flat_param
        self.t = 0
        self.grad_scale = 1.0
        self._groups = [dict({"params": [flat_param], "lr": float(lr)}, **group)]
        self.state = {s: torch.zeros_like(flat_param.data) for s in self.slots}
        self.nonfinite = torch.zeros(1, dtype=torch.int64, device=flat_param.device)

    @property
    def param_groups(self):
        return self._groups

    @property
    def lr(self):
        return float(self._groups[0]["lr"])

    @lr.setter
    def lr(self, value):
        self._groups[0]["lr"] = float(value)

    def _args(self):
        """-> (beta1 or momentum, beta2, eps) as the kernel takes them"""
        raise NotImplementedError

    def _cpu_step(self, p, g):
        raise NotImplementedError

    def step(self):
        g = self.p.grad
        if g is None:
            return
        if g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.p.device or g.numel() != self.p.numel():
            raise ValueError("%s: the gradient must be a contiguous float32 buffer on the parameter's device" % type(self).__name__)
        self.t += 1
        if self.guard is not None:
            return self._guarded_step(g)
        if self.p.is_cuda:
            a, b2, eps = self._args()
            s = [self.state[k] for k in self.slots]
            _lib.check(_lib.lib().sph3d_train_update(self.p.numel(), _lib.ptr(self.p.data), _lib.ptr(g), _lib.ptr(s[0]),
                                                     _lib.ptr(s[1]) if len(s) > 1 else None, self.rule, self.lr, a, b2, eps, self.t,
                                                     self.grad_scale, _lib.ptr(self.nonfinite), _lib.stream_ptr()))
            return
        with torch.no_grad():
            g = torch.tensor(self.grad_scale, dtype=torch.float32) * g
            self.nonfinite += int((~torch.isfinite(g)).sum())
            self._cpu_step(self.p.data, g)

    def _guarded_step(self, g):
        gd = self.guard.bind(self.p)
        a, b2, eps = self._args()
        s = [self.state[k] for k in self.slots]
        if self.p.is_cuda:
            _lib.check(_lib.lib().sph3d_train_update_guarded(
                self.p.numel(), _lib.ptr(self.p.data), _lib.ptr(g), _lib.ptr(s[0]), _lib.ptr(s[1]) if len(s) > 1 else None,
                _lib.ptr(gd.ema), self.rule, self.lr, a, b2, eps, self.grad_scale, gd.clip_norm if gd.clip_norm is not None else 0.0,
                1 if gd.skip_nonfinite else 0, gd.ema_decay if gd.ema_decay is not None else 0.0, _lib.ptr(gd.state),
                _lib.ptr(self.nonfinite), _lib.ptr(gd.workspace), gd.workspace.numel(), _lib.stream_ptr()))
            return
        with torch.no_grad():
            _guard.step(gd.state.numpy(), self.p.data.numpy(), g.detach().numpy(), s[0].numpy(), s[1].numpy() if len(s) > 1 else None,
                        gd.ema.numpy() if gd.ema is not None else None, self.rule, self.lr, a, b2, eps, self.grad_scale, gd.clip_norm,
                        gd.skip_nonfinite, gd.ema_decay, self.nonfinite.numpy())

    def zero_grad(self, set_to_none=False):
        if self.p.grad is not None:
            if set_to_none:
                self.p.grad = None
            else:
                self.p.grad.zero_()

    def state_dict(self):
        d = {k: v.clone() for k, v in self.state.items()}
        d.update({k: v for k, v in self._groups[0].items() if k != "params"})
        d["step"] = self.t
        d["grad_scale"] = self.grad_scale
        if self.guard is not None:
            gd = self.guard.bind(self.p)
            d["guard_state"] = gd.state.clone()
            d["step"] = int(gd.state[_guard.APPLIED])          # (the applied count: one host read)
            d["guard"] = gd.options()
            if gd.ema is not None:
                d["ema"] = gd.ema.clone()
        return d

    def load_state_dict(self, state):
        self.t = int(state["step"])
        for k in self.slots:
            self.state[k].copy_(state[k])
        self.lr = state.get("lr", self.lr)
        if self.guard is not None:
            gd = self.guard.bind(self.p)
            if "guard_state" in state:
                gd.state.copy_(state["guard_state"])
                if gd.ema is not None:
                    gd.ema.copy_(state["ema"] if "ema" in state else self.p.detach())
            else:                                               # a checkpoint written without a guard
                a, b2, _eps = self._args() if self.rule == RULE_TF_ADAM else (1.0, 1.0, 0.0)          # (only rule 0 has powers)
                gd.start_from(self.t, a, b2)


class FlatTFAdam(_FlatRule):
    """tf.train.AdamOptimizer(lr, beta1, beta2, epsilon): m += (1 - b1)(g - m); v += (1 - b2)(g g - v);
    p -= (lr_t m) / (sqrt(v) + eps) with lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) — eps INSIDE the bias correction, which is where
    it differs from FlatAdam (by sqrt(1 - b2^t) on eps: 0.03 at the first step; with the reference's eps = 1e-4 far outside
    rounding)."""
    rule = RULE_TF_ADAM
    slots = ("exp_avg", "exp_avg_sq")

    def __init__(self, flat_param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.b1, self.b2, self.eps = float(betas[0]), float(betas[1]), float(eps)
        super().__init__(flat_param, lr, {"betas": (self.b1, self.b2), "eps": self.eps})

    @property
    def m(self):
        return self.state["exp_avg"]

    @property
    def v(self):
        return self.state["exp_avg_sq"]

    def _args(self):
        return self.b1, self.b2, self.eps

    def _cpu_step(self, p, g):
        f = lambda x: torch.tensor(x, dtype=torch.float32)
        one, m, v = f(1.0), self.m, self.v
        m.copy_(m + (one - f(self.b1)) * (g - m))
        v.copy_(v + (one - f(self.b2)) * (g * g - v))
        # the root through float64: torch's fp32 sqrt on the CPU is not correctly rounded (0.6 % of the elements are one ulp off),
        # the kernel's is, and so is the float64 root rounded to fp32 (53 >= 2 * 24 + 2 bits)
        root = torch.sqrt(v.double()).float()
        p.copy_(p - (f(tf_adam_lr_t(self.lr, self.b1, self.b2, self.t)) * m) / (root + f(self.eps)))


class FlatNesterov(_FlatRule):
    """tf.train.MomentumOptimizer(lr, momentum, use_nesterov=True): accum = momentum accum + g; p -= g lr + (accum momentum) lr"""
    rule = RULE_NESTEROV
    slots = ("accum",)

    def __init__(self, flat_param, lr=1e-3, momentum=0.9):
        self.momentum = float(momentum)
        super().__init__(flat_param, lr, {"momentum": self.momentum})

    @property
    def accum(self):
        return self.state["accum"]

    def _args(self):
        return self.momentum, 0.0, 0.0

    def _cpu_step(self, p, g):
        f = lambda x: torch.tensor(x, dtype=torch.float32)
        a, mom, lr = self.accum, f(self.momentum), f(self.lr)
        a.copy_(mom * a + g)
        p.copy_(p - (g * lr + (a * mom) * lr))
