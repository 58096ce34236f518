"""Adam over ONE flat fp32 parameter buffer (harness plumbing: train_s3dis.py:224 uses tf.train.AdamOptimizer).

On the GPU the update is one streaming kernel (csrc/optim.hip: sph3d_adam_step, torch.optim.Adam's arithmetic to 2e-6);
on CPU tensors (oracle-backed tests) it wraps torch.optim.Adam.  The surface a training loop needs from an optimiser is
kept: a settable learning rate (``lr`` / ``param_groups[0]['lr']``: the reference decays it every step), ``state_dict`` /
``load_state_dict`` for checkpoint / resume, ``zero_grad``.
"""
import torch

from .. import _lib


class FlatAdam:
    """torch.optim.Adam's form (eps outside the bias correction), not the reference's: FlatTFAdam below is tf.train.AdamOptimizer's."""

    def __init__(self, flat_param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
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


class _FlatRule:
    """What FlatTFAdam and FlatNesterov share: FlatAdam's surface (``lr``, ``param_groups``, ``step``, ``zero_grad``,
    ``state_dict`` / ``load_state_dict``) plus ``grad_scale`` (the gradient is multiplied by it inside the update: 1 / world
    size replaces all_reduce(average=True)'s own launch) and ``nonfinite``, an int64 [1] tensor on the parameter's device that
    counts the gradient elements that were not finite (never read here: the training loop reads it when it logs).  On the HIP
    device a step is one sph3d_train_update launch; on CPU tensors the same formulas, operation by operation, in torch fp32."""
    rule = None
    slots = ()

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
        return d

    def load_state_dict(self, state):
        self.t = int(state["step"])
        for k in self.slots:
            self.state[k].copy_(state[k])
        self.lr = state.get("lr", self.lr)


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
        p.copy_(p - (f(tf_adam_lr_t(self.lr, self.b1, self.b2, self.t)) * m) / (torch.sqrt(v) + f(self.eps)))


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
