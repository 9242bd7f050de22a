"""Adam for the batched learner, with RMSpropAsync's surface (an extension:
the reference trains with RMSpropAsync only, tuned for one Hogwild process; the
lockstep learner takes one step per window on the gradient of all envs).

The arithmetic is Chainer 1.8.1's optimizers.Adam as NumPy evaluates it on
float32 arrays (restated in include/asyncrl_hip.h): for update number t,
  lr_t = alpha * sqrt(1 - beta2**t) / (1 - beta1**t)
  m += (1 - beta1) * (g - m); v += (1 - beta2) * (g * g - v)
  p -= lr_t * m / (sqrt(v) + eps)
on the gradient the GradientClipping / NonbiasWeightDecay hooks left.  It is
one fused HIP kernel over the flat parameter buffer, with every duty of the
RMSProp one (clip, decay, the FC weight planes, the window advance).  The net's
`ms` buffer holds v, `adam_m` holds m, and the update count of a net lives on
the device (DeviceNet.adam_t), so a graph-captured window replays with a fresh
bias correction.
"""
from __future__ import annotations

import math

import torch

from ._lib import check, lib, ptr, stream_handle
from .net import nets_aliasing
from .rmsprop_async import GradientClipping, NonbiasWeightDecay


class Adam:
    """chainer.optimizers.Adam(alpha, beta1, beta2, eps).  For graph-captured
    windows set `anneal_total_steps` and alpha is annealed on the device, as
    RMSpropAsync's lr."""

    def __init__(self, alpha: float = 0.001, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
        self.alpha = alpha
        self.beta1 = beta1
        self.beta2 = beta2
        self.eps = eps
        self.hooks = []
        self.target = None
        self.anneal_total_steps = 0   # 0 = use self.alpha as given
        self.n_total_envs = 0         # envs over all ranks (global_t per window)
        self._scratch = None
        self.t = 0                    # Chainer Optimizer.t / epoch (serialized into '.opt')
        self.epoch = 0

    def setup(self, model):
        """Chainer Optimizer.setup: bind the model and make Adam its net's
        optimizer (m zero-initialised; v lives in the net's `ms`)."""
        self.target = model
        model.net.set_adam(self.beta1, self.beta2)
        return self

    def add_hook(self, hook):
        """GradientClipping, NonbiasWeightDecay or both, clip first
        (RMSpropAsync.add_hook's rules: the fused update clips by the norm of
        the gradient before the decay)."""
        if not isinstance(hook, (GradientClipping, NonbiasWeightDecay)):
            raise TypeError(f"Adam.add_hook: unsupported hook {type(hook).__name__} "
                            "(GradientClipping, NonbiasWeightDecay)")
        if any(type(h) is type(hook) for h in self.hooks):
            raise ValueError(f"Adam.add_hook: a {hook.name} hook is already installed")
        if isinstance(hook, GradientClipping) and self.hooks:
            raise ValueError("Adam.add_hook: GradientClipping after NonbiasWeightDecay would clip the "
                             "decayed gradient; add the clip first")
        self.hooks.append(hook)

    @property
    def clip_threshold(self) -> float:
        for h in self.hooks:
            if isinstance(h, GradientClipping):
                return h.threshold
        return 0.0

    @property
    def weight_decay(self) -> float:
        for h in self.hooks:
            if isinstance(h, NonbiasWeightDecay):
                return h.rate
        return 0.0

    @property
    def lr(self) -> float:
        """Chainer's Adam.lr: the bias-corrected step size for self.t."""
        fix1 = 1.0 - self.beta1 ** self.t
        fix2 = 1.0 - self.beta2 ** self.t
        return self.alpha * math.sqrt(fix2) / fix1

    def update_args(self) -> dict:
        """The arguments of one update (net.optimize's, without the stream),
        counting it; lr0 is Adam's alpha and `alpha` (RMSProp's decay) is
        ignored by the Adam kernel.  The net the model holds now is (re)told
        its optimizer and weight decay here, as RMSpropAsync.update_args."""
        if self.anneal_total_steps > 0 and self.n_total_envs <= 0:
            raise ValueError("anneal_total_steps > 0 needs n_total_envs > 0 (envs over all ranks)")
        if self.target is not None:
            net = self.target.net
            if net.adam_betas != (float(self.beta1), float(self.beta2)):
                net.set_adam(self.beta1, self.beta2)
            net.set_weight_decay(self.weight_decay)
        self.t += 1
        return dict(lr0=self.alpha, total_steps=self.anneal_total_steps, n_total=self.n_total_envs, alpha=0.0,
                    eps=self.eps, clip=self.clip_threshold)

    def update(self, stream=None, advance_window=False):
        """Hooks, then one Adam update of the bound model's device buffers;
        advance_window: also end the lockstep window (arl_optimize_advance)."""
        self.target.net.optimize(stream=stream, advance=advance_window, **self.update_args())

    def update_arrays(self, param: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad: torch.Tensor, t: int | None = None,
                      nonbias: bool = False, stream=None):
        """One Adam update of explicit flat f32 device tensors (arl_adam) for
        update number t; None counts self.t up and uses it.  nonbias: an
        installed NonbiasWeightDecay hook applies to the array."""
        if t is None:
            self.t += 1
            t = self.t
        clip = self.clip_threshold
        if clip > 0 and self._scratch is None:
            self._scratch = torch.zeros(1024, dtype=torch.float64, device=param.device)
        rate = self.weight_decay if nonbias else 0.0
        check(lib.arl_adam(ptr(param), ptr(m), ptr(v), ptr(grad), param.numel(), self.alpha, self.beta1, self.beta2,
                           self.eps, int(t), clip, ptr(self._scratch) if clip > 0 else None, rate,
                           stream_handle(stream)), "arl_adam")
        for net in nets_aliasing(param):
            net.params_changed()
