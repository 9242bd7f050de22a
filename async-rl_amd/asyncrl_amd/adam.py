"""Adam for the batched learner, with RMSpropAsync's surface (an extension:
the reference trains with RMSpropAsync only, tuned for one Hogwild process; the
lockstep learner takes one step per window on the gradient of all envs).

The arithmetic is Chainer 1.8.1's optimizers.Adam as NumPy evaluates it on
float32 arrays (restated in include/asyncrl_hip.h): for update number t,
  lr_t = alpha * sqrt(1 - beta2**t) / (1 - beta1**t)
  m += (1 - beta1) * (g - m); v += (1 - beta2) * (g * g - v)
  p -= lr_t * m / (sqrt(v) + eps)
on the gradient the GradientClipping / NonbiasWeightDecay hooks left.  It is
one fused HIP kernel over the flat parameter buffer: the RMSProp kernel's body
with this rule (clip, decay, the FC weight planes, the window advance).  The net's
`ms` buffer holds v, `adam_m` holds m, and the update count of a net lives on
the device (DeviceNet.adam_t), so a graph-captured window replays with a fresh
bias correction.
"""
from __future__ import annotations

import math

import torch

from ._lib import check, lib, ptr, stream_handle
from .rmsprop_async import FusedOptimizer


class Adam(FusedOptimizer):
    """chainer.optimizers.Adam(alpha, beta1, beta2, eps).  For graph-captured
    windows set `anneal_total_steps` and alpha is annealed on the device, as
    RMSpropAsync's lr."""

    def __init__(self, alpha: float = 0.001, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
        super().__init__()
        self.alpha = alpha
        self.beta1 = beta1
        self.beta2 = beta2
        self.eps = eps

    def setup(self, model):
        """Chainer Optimizer.setup: bind the model and make Adam its net's
        optimizer (m zero-initialised; v lives in the net's `ms`)."""
        self.target = model
        model.net.set_adam(self.beta1, self.beta2)
        return self

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
        self._check_anneal()
        if self.target is not None:
            net = self.target.net
            if net.adam_betas != (float(self.beta1), float(self.beta2)):
                net.set_adam(self.beta1, self.beta2)
            net.set_weight_decay(self.weight_decay)
        self.t += 1
        return dict(lr0=self.alpha, total_steps=self.anneal_total_steps, n_total=self.n_total_envs, alpha=0.0,
                    eps=self.eps, clip=self.clip_threshold)

    def update_arrays(self, param: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad: torch.Tensor, t: int | None = None,
                      nonbias: bool = False, stream=None):
        """One Adam update of explicit flat f32 device tensors (arl_adam) for
        update number t; None counts self.t up and uses it.  nonbias: an
        installed NonbiasWeightDecay hook applies to the array."""
        if t is None:
            self.t += 1
            t = self.t
        rate = self.weight_decay if nonbias else 0.0
        check(lib.arl_adam(ptr(param), ptr(m), ptr(v), ptr(grad), param.numel(), self.alpha, self.beta1, self.beta2,
                           self.eps, int(t), self.clip_threshold, self._clip_scratch(param.device), rate,
                           stream_handle(stream)), "arl_adam")
        self._arrays_changed(param)
