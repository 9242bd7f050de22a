"""RMSpropAsync + GradientClipping + NonbiasWeightDecay, mirroring
rmsprop_async.py:7-38, the Chainer hook used at a3c_ale.py:224-226 and
nonbias_weight_decay.py (a3c_ale.py:227-228, --weight-decay).

The reference's update is `ms = alpha*ms + (1-alpha)*g*g; p -= lr*g/sqrt(ms+eps)`
(eps OUTSIDE the sqrt) per parameter array, CPU or a dormant CuPy
ElementwiseKernel.  Here it is one fused HIP kernel over the flat parameter
buffer (plus a norm pass when a GradientClipping hook is installed), bitwise
equal to update_one_cpu's f32 arithmetic.  A NonbiasWeightDecay hook is
folded into that kernel (g += rate * p after the clip, biases skipped).
"""
from __future__ import annotations

import torch

from ._lib import check, lib, ptr, stream_handle
from .net import nets_aliasing


class GradientClipping:
    """chainer.optimizer.GradientClipping(threshold) (a3c_ale.py:226)."""

    name = "GradientClipping"

    def __init__(self, threshold: float):
        self.threshold = float(threshold)


class NonbiasWeightDecay:
    """nonbias_weight_decay.NonbiasWeightDecay(rate) (a3c_ale.py:227-228):
    g += rate * p for every parameter that is not a bias, run after the
    clip.  The update kernel does it (arl_net_set_weight_decay)."""

    name = "NonbiasWeightDecay"

    def __init__(self, rate: float):
        self.rate = float(rate)


class FusedOptimizer:
    """What RMSpropAsync and Adam share: Chainer's Optimizer surface (hooks,
    target, t / epoch), the on-device anneal's settings and the two ways into
    the fused update kernel (update on the bound model, update_arrays on flat
    tensors)."""

    _add_hook_ref = ""   # where the reference orders the two hooks (add_hook's message)

    def __init__(self):
        self.hooks = []
        self.target = None
        self.anneal_total_steps = 0   # 0 = use the lr (Adam: alpha) as given
        self.n_total_envs = 0         # envs over all ranks (global_t per window)
        self._scratch = None
        self.t = 0                    # Chainer Optimizer.t / epoch (serialized into '.opt')
        self.epoch = 0

    def add_hook(self, hook):
        """GradientClipping, NonbiasWeightDecay or both in the reference's
        order (a3c_ale.py:226-228: clip, then decay).  Chainer runs hooks in
        insertion order; the fused update clips by the norm of the gradient
        before the decay, so a clip added after a decay is refused."""
        who = type(self).__name__
        if not isinstance(hook, (GradientClipping, NonbiasWeightDecay)):
            raise TypeError(f"{who}.add_hook: unsupported hook {type(hook).__name__} "
                            "(GradientClipping, NonbiasWeightDecay)")
        if any(type(h) is type(hook) for h in self.hooks):
            raise ValueError(f"{who}.add_hook: a {hook.name} hook is already installed")
        if isinstance(hook, GradientClipping) and self.hooks:
            raise ValueError(f"{who}.add_hook: GradientClipping after NonbiasWeightDecay would clip the "
                             f"decayed gradient; add the clip first{self._add_hook_ref}")
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

    def _check_anneal(self):
        """update_args' first step, before anything is counted or set."""
        if self.anneal_total_steps > 0 and self.n_total_envs <= 0:
            # global_t per window = (window start + t_max) * n_total_envs: with 0
            # envs it never moves and the anneal would silently keep lr fixed
            raise ValueError("anneal_total_steps > 0 needs n_total_envs > 0 (envs over all ranks)")

    def update(self, stream=None, advance_window=False):
        """The hooks, then one update of every parameter, on the bound model's
        device buffers (a3c.py:139).  advance_window: also end the lockstep
        window (arl_optimize_advance)."""
        self.target.net.optimize(stream=stream, advance=advance_window, **self.update_args())

    def _clip_scratch(self, device):
        """update_arrays: the norm partials' scratch (None without a clip)."""
        if self.clip_threshold <= 0:
            return None
        if self._scratch is None:
            self._scratch = torch.zeros(1024, dtype=torch.float64, device=device)
        return ptr(self._scratch)

    @staticmethod
    def _arrays_changed(param):
        """update_arrays wrote `param` behind torch's back: a net whose params it
        aliases rebuilds its derived FC planes before the next forward."""
        for net in nets_aliasing(param):
            net.params_changed()


class RMSpropAsync(FusedOptimizer):
    """rmsprop_async.py:7-21.  `lr` may be reassigned between updates (the
    reference anneals it every step, a3c_ale.py:111-112); for graph-captured
    windows set `anneal_total_steps` and the lr is annealed on the device."""

    _add_hook_ref = " (a3c_ale.py:226-228)"

    def __init__(self, lr: float = 0.01, alpha: float = 0.99, eps: float = 1e-8):
        super().__init__()
        self.lr = lr
        self.alpha = alpha
        self.eps = eps

    def setup(self, model):
        """Chainer Optimizer.setup: bind the model whose flat params/grads and
        `ms` state (rmsprop_async.py:19-21, zero-initialised) are updated.  A net
        that an Adam had set up goes back to the RMSProp kernel."""
        self.target = model
        model.net.set_adam(None)
        return self

    def update_args(self) -> dict:
        """The arguments of one update (net.optimize's, without the stream),
        counting it (Chainer's Optimizer.t).  The NonbiasWeightDecay rate
        (0 without the hook) goes to the bound model's net here, so every
        update path -- update, A3C.run_window, A3C.act -- launches with it."""
        self._check_anneal()
        if self.target is not None:
            self.target.net.set_weight_decay(self.weight_decay)
        self.t += 1
        return dict(lr0=self.lr, total_steps=self.anneal_total_steps, n_total=self.n_total_envs, alpha=self.alpha,
                    eps=self.eps, clip=self.clip_threshold)

    def update_arrays(self, param: torch.Tensor, ms: torch.Tensor, grad: torch.Tensor, stream=None,
                      nonbias: bool = False):
        """update_one on explicit flat f32 device tensors (the drop-in for
        RMSpropAsync.update_one_cpu / update_one_gpu on one array).  nonbias:
        the array is not a bias, so an installed NonbiasWeightDecay hook
        applies to it (arl_rmsprop_wd)."""
        clip, scratch = self.clip_threshold, self._clip_scratch(param.device)
        rate = self.weight_decay if nonbias else 0.0
        if rate > 0:
            check(lib.arl_rmsprop_wd(ptr(param), ptr(ms), ptr(grad), param.numel(), self.lr, self.alpha, self.eps,
                                     clip, scratch, rate, stream_handle(stream)), "arl_rmsprop_wd")
        else:
            check(lib.arl_rmsprop(ptr(param), ptr(ms), ptr(grad), param.numel(), self.lr, self.alpha, self.eps,
                                  clip, scratch, stream_handle(stream)), "arl_rmsprop")
        self._arrays_changed(param)
