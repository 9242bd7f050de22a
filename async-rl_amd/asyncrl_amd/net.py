"""Device-resident A3C model + lockstep actor-learner workspace.

Replaces the reference's process-shared parameters (async.py:11-65:
RawArray-backed params and RMSProp `ms`, Hogwild writes) with ONE flat fp32
parameter buffer, one flat gradient buffer and one flat `ms` buffer in HBM,
laid out in Chainer namedparams order (a3c_ale.py:35,52) so checkpoints map
1:1 (HDF5 paths "0/0/W", ...).  PyTorch only allocates the memory; all
compute is in libasyncrl_hip.so.
"""
from __future__ import annotations

import ctypes
import math
import weakref

import numpy as np
import torch

from ._lib import (ARCH_FF, ARCH_FF_NATURE, ARCH_LSTM, ARCH_RGB, ARCH_STACK, ARCH_STATES, CTL_ADAM_T, ENV_CATCH,
                   ENV_GROUP_ALIGN, EPISODE_LOG, EPISODE_STAT_FIELDS, FORM_AUTO, FORMS, FWD_KEEP_STATE, POOL_DONES,
                   POOL_FRAMES, POOL_REWARDS, PPO_AUX_DOUBLES, PPO_AUX_HEAD, PPO_LOG, PPO_STAT_FIELDS, PPO_STAT_NAMES,
                   RESIZE_SCALAR, STAGE_HOST, STAGE_NAMES, WINDOW_LOG, WINDOW_STAT_FIELDS, WINDOW_STAT_NAMES, check,
                   env_defaults, lib, ptr, stream_handle)


def param_shapes(arch: int, n_actions: int):
    """Chainer parameter shapes in link order (dqn_head.py:40-44,
    policy.py:49, v_function.py:25, Chainer L.LSTM upward/lateral; the
    Nature head dqn_head.py:16-20 with 512-wide policy / value heads; the
    RGB flag: NIPSDQNHead(n_input_channels=3), train_a3c_doom.py:28,46)."""
    c_in = 3 if arch & ARCH_RGB else 4
    arch &= ~(ARCH_RGB | ARCH_STACK | ARCH_STATES)
    if arch == ARCH_FF_NATURE:
        return [("0/0/W", (32, 4, 8, 8)), ("0/0/b", (32,)), ("0/1/W", (64, 32, 4, 4)), ("0/1/b", (64,)),
                ("0/2/W", (64, 64, 3, 3)), ("0/2/b", (64,)), ("0/3/W", (512, 3136)), ("0/3/b", (512,)),
                ("1/0/W", (n_actions, 512)), ("1/0/b", (n_actions,)), ("2/0/W", (1, 512)), ("2/0/b", (1,))]
    head = [("0/0/W", (16, c_in, 8, 8)), ("0/0/b", (16,)), ("0/1/W", (32, 16, 4, 4)), ("0/1/b", (32,)),
            ("0/2/W", (256, 2592)), ("0/2/b", (256,))]
    if arch == ARCH_FF:
        return head + [("1/0/W", (n_actions, 256)), ("1/0/b", (n_actions,)), ("2/0/W", (1, 256)),
                       ("2/0/b", (1,))]
    return head + [("1/upward/W", (1024, 256)), ("1/upward/b", (1024,)), ("1/lateral/W", (1024, 256)),
                   ("2/0/W", (n_actions, 256)), ("2/0/b", (n_actions,)), ("3/0/W", (1, 256)),
                   ("3/0/b", (1,))]


def init_like_torch(arch: int, n_actions: int, rng: np.random.Generator):
    """init_like_torch.py:5-22: U(+-1/sqrt(fan_in)) for every W and b
    (fan_in = in*kh*kw); host-side setup, not on the hot path."""
    shapes = dict(param_shapes(arch, n_actions))
    out = {}
    for name, shape in param_shapes(arch, n_actions):
        w = shapes[name.rsplit("/", 1)[0] + "/W"]
        stdv = 1.0 / np.sqrt(int(np.prod(w[1:])))
        out[name] = rng.uniform(-stdv, stdv, size=shape).astype(np.float32)
    return out



# every live DeviceNet, so a writer of a flat tensor can find the nets whose params it aliases
_NETS: "weakref.WeakSet[DeviceNet]" = weakref.WeakSet()


def nets_aliasing(t: torch.Tensor):
    """The live DeviceNets whose bound params overlap the memory of `t`."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        return []
    lo = t.data_ptr()
    hi = lo + t.numel() * t.element_size()
    out = []
    for n in list(_NETS):
        p = n._params
        b = p.data_ptr()
        if p.device == t.device and lo < b + p.numel() * p.element_size() and b < hi:
            out.append(n)
    return out


def check_pools(pool_len: int, *pools):
    """pool_len against each pool's leading dimension (the C ABI checks it
    again against the extents registered with arl_net_set_pool)."""
    if pool_len < 1:
        raise ValueError(f"pool_len must be >= 1, got {pool_len}")
    for p in pools:
        if p is not None and isinstance(p, torch.Tensor) and (p.dim() == 0 or p.shape[0] < pool_len):
            raise ValueError(f"pool_len {pool_len} exceeds a pool of shape {tuple(p.shape)}")


def episode_stats_dict(v) -> dict:
    """The 8 doubles of arl_episode_stats as a dict, plus what the host derives:
    mean and mean_length (nan without an episode), stdev (sample standard
    deviation; nan below two episodes)."""
    d = {k: float(x) for k, x in zip(EPISODE_STAT_FIELDS, v)}
    for k in ("episodes", "length_sum", "steps"):
        d[k] = int(d[k])
    n = d["episodes"]
    nan = float("nan")
    d["mean"] = d["return_sum"] / n if n else nan
    d["mean_length"] = d["length_sum"] / n if n else nan
    d["stdev"] = math.sqrt(max(d["return_sumsq"] - d["return_sum"] ** 2 / n, 0.0) / (n - 1)) if n > 1 else nan
    return d


def window_stats_dict(row) -> dict:
    """One record of the window log (WINDOW_STAT_NAMES order) as a dict, the
    counters as int, plus what the host derives: entropy, value_mean,
    return_mean, adv_mean (sum / samples; nan without a sample),
    explained_variance = 1 - Var(adv) / Var(R) from the sums (nan when Var(R)
    is 0), grad_norm, clipped (the update scaled the gradient) and total_loss."""
    if len(row) != WINDOW_STAT_FIELDS:
        raise ValueError(f"window_stats_dict: need {WINDOW_STAT_FIELDS} values")
    d = {k: float(x) for k, x in zip(WINDOW_STAT_NAMES, row)}
    for k in ("window", "step", "samples", "terminals"):
        d[k] = int(d[k])
    n = d["samples"]
    nan = float("nan")
    for out, src in (("entropy", "entropy_sum"), ("value_mean", "value_sum"), ("return_mean", "return_sum"),
                     ("adv_mean", "adv_sum")):
        d[out] = d[src] / n if n else nan
    ev = nan
    if n:
        var_r = d["return_sumsq"] / n - d["return_mean"] ** 2
        var_a = d["adv_sumsq"] / n - d["adv_mean"] ** 2
        if var_r > 0:
            ev = 1.0 - var_a / var_r
    d["explained_variance"] = ev
    d["grad_norm"] = math.sqrt(d["grad_sqnorm"])
    d["clipped"] = d["clip_scale"] < 1
    d["total_loss"] = d["pi_loss"] + d["v_loss"]
    return d


def ppo_epoch_stats_dict(row) -> dict:
    """One per-epoch record of the PPO options' log (PPO_STAT_NAMES order) as
    the dict A3C.ppo_epoch_stats returns: window, epoch, samples as int,
    ratio_max / ratio_min as stored, and from the sums clip_fraction,
    approx_kl = kl_sum / samples, vclip_fraction, adv_mean and adv_std (the
    population form; nan without a sample)."""
    if len(row) != PPO_STAT_FIELDS:
        raise ValueError(f"ppo_epoch_stats_dict: need {PPO_STAT_FIELDS} values")
    r = {k: float(x) for k, x in zip(PPO_STAT_NAMES, row)}
    n = int(r["samples"])
    nan = float("nan")
    mean = r["adv_sum"] / n if n else nan
    return {"window": int(r["window"]), "epoch": int(r["epoch"]), "samples": n,
            "clip_fraction": r["clipped"] / n if n else nan, "approx_kl": r["kl_sum"] / n if n else nan,
            "ratio_max": r["ratio_max"], "ratio_min": r["ratio_min"],
            "vclip_fraction": r["vclipped"] / n if n else nan, "adv_mean": mean,
            "adv_std": math.sqrt(max(r["adv_sumsq"] / n - mean * mean, 0.0)) if n else nan}


class DeviceNet:
    """One arl_net handle + the device memory it borrows."""

    def __init__(self, arch: int, n_actions: int, n_envs: int, t_max: int = 5, env_offset: int = 0,
                 seed: int = 0, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        self.arch, self.n_actions, self.n_envs, self.t_max = arch, n_actions, n_envs, t_max
        self.rgb = bool(arch & ARCH_RGB)
        self.stack = bool(arch & ARCH_STACK)
        self.states = bool(arch & ARCH_STATES)
        self.base_arch = arch & ~(ARCH_RGB | ARCH_STACK | ARCH_STATES)
        self.env_offset, self.seed = env_offset, seed
        h = ctypes.c_void_p()
        check(lib.arl_net_create(ctypes.byref(h), arch, n_actions, n_envs, t_max, env_offset, seed),
              "arl_net_create")
        self._h = h
        self.set_forms(**{k: v for k, v in env_defaults().items() if k in FORMS})
        P = lib.arl_net_param_floats(h)
        self.param_floats = P
        self._params = torch.zeros(P, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros(P, dtype=torch.float32, device=self.device)
        self.ms = torch.zeros(P, dtype=torch.float32, device=self.device)
        self.workspace = torch.zeros(lib.arl_net_workspace_bytes(h), dtype=torch.uint8, device=self.device)
        check(lib.arl_net_bind(h, ptr(self._params), ptr(self.grads), ptr(self.ms), ptr(self.workspace)),
              "arl_net_bind")
        self._pver = self._params._version   # (binding bumped the net's parameter generation)
        _NETS.add(self)
        self.layout = {}
        shapes = dict(param_shapes(arch, n_actions))
        name = ctypes.create_string_buffer(64)
        for i in range(lib.arl_net_param_count(h)):
            off, num = ctypes.c_int64(), ctypes.c_int64()
            check(lib.arl_net_param_info(h, i, ctypes.byref(off), ctypes.byref(num), name, 64))
            key = name.value.decode()
            assert int(np.prod(shapes[key])) == num.value, key
            self.layout[key] = (off.value, shapes[key])
        self.n_params = sum(int(np.prod(s)) for _, s in self.layout.values())

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.arl_net_destroy(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    # ------------------------------------------------------------ params
    @property
    def params(self) -> torch.Tensor:
        """The bound flat f32 parameters (Chainer namedparams order).  In-place
        writes through this tensor or a view of it are seen (torch's version
        counter) and rebuild the FC weight planes before the next forward."""
        return self._params

    @params.setter
    def params(self, value) -> None:
        """net.params = x copies x into the bound memory (the C library keeps
        its pointer) and bumps the parameter generation."""
        self._params.copy_(torch.as_tensor(value, dtype=torch.float32, device=self.device).reshape(-1))
        self.params_changed()

    def _sync_params(self) -> None:
        """Bump the parameter generation if torch's version counter of the
        params moved since the last bump (an in-place write from Python)."""
        if self._params._version != self._pver:
            self.params_changed()

    def prepare(self, stream=None) -> None:
        """Make derived device state current on `stream` (arl_net_prepare):
        before env-range chains fork from it and before a graph replay."""
        self._sync_params()
        check(lib.arl_net_prepare(self._h, stream_handle(stream)), "arl_net_prepare")

    def param_generation(self):
        """(param_gen, planes_gen) of the C net: the planes are current iff equal."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib.arl_net_param_generation(self._h, ctypes.byref(a), ctypes.byref(b)), "arl_net_param_generation")
        return a.value, b.value

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        off, shape = self.layout[name]
        return flat[off:off + int(np.prod(shape))].view(shape)

    def param(self, name: str) -> torch.Tensor:
        return self.view(self.params, name)

    def grad(self, name: str) -> torch.Tensor:
        return self.view(self.grads, name)

    def load_params(self, arrays: dict) -> None:
        for name, (off, shape) in self.layout.items():
            a = np.asarray(arrays[name], dtype=np.float32).reshape(shape)
            self.param(name).copy_(torch.from_numpy(a))
        self.params_changed()

    def params_changed(self) -> None:
        """Tell the net its params were written from outside (arl_net_params_changed):
        derived device state (the FC weight's split planes) is rebuilt before
        the next forward.  load_params / copy_params_from / the params setter /
        RMSpropAsync.update_arrays on these params call it; other in-place
        writes through the tensor are caught by its version counter."""
        check(lib.arl_net_params_changed(self._h), "arl_net_params_changed")
        self._pver = self._params._version

    def copy_params_from(self, other: "DeviceNet") -> None:
        """copy_param.copy_param (copy_param.py): this net's params <- other's."""
        self.params.copy_(other.params)
        self.params_changed()

    def state_dict(self, flat: torch.Tensor | None = None) -> dict:
        flat = self.params if flat is None else flat
        return {n: self.view(flat, n).detach().cpu().numpy().copy() for n in self.layout}

    # ------------------------------------------------------------ workspace
    def buffer(self, name: str, dtype=torch.uint8, shape=None) -> torch.Tensor:
        off, nb = ctypes.c_int64(), ctypes.c_int64()
        check(lib.arl_net_buffer(self._h, name.encode(), ctypes.byref(off), ctypes.byref(nb)), "arl_net_buffer")
        raw = self.workspace[off.value:off.value + nb.value]
        t = raw.view(dtype)
        return t.view(shape) if shape is not None else t

    # ------------------------------------------------------------ hot path
    def set_pools(self, frames=None, rewards=None, dones=None):
        """Register the input pools' extents with the net (arl_net_set_pool):
        the C ABI refuses an observation whose pools it does not know."""
        for kind, t in ((POOL_FRAMES, frames), (POOL_REWARDS, rewards), (POOL_DONES, dones)):
            if t is not None:
                check(lib.arl_net_set_pool(self._h, kind, ptr(t), t.numel() * t.element_size()), "arl_net_set_pool")

    def reset(self, stream=None):
        check(lib.arl_net_reset(self._h, stream_handle(stream)), "arl_net_reset")

    def observe(self, t: int, pair_pool: torch.Tensor, reward_pool=None, done_pool=None, pool_len: int = 1,
                force_reset: bool = False, resize_mode: int = RESIZE_SCALAR, stream=None, envs=None):
        """pair_pool: (pool_len, n, 2, 210, 160, 3) uint8 frame pairs; for an
        RGB net (arch | ARCH_RGB) the screens (pool_len, n, H, W, 3) instead.
        envs=(e0, ne): only envs [e0, e0 + ne) (arl_observe_envs)."""
        check_pools(pool_len, pair_pool, reward_pool, done_pool)
        self.set_pools(pair_pool, reward_pool, done_pool)
        if (self.stack or self.states) and envs is None:
            self.observe_stack(t, pair_pool, reward_pool, done_pool, pool_len, force_reset, stream)
            return
        if envs is not None:
            e0, ne = envs
            H, W = (pair_pool.shape[-3], pair_pool.shape[-2]) if self.rgb else (0, 0)
            check(lib.arl_observe_envs(self._h, t, e0, ne, ptr(pair_pool), H, W, ptr(reward_pool), ptr(done_pool),
                                       pool_len, int(force_reset), resize_mode, stream_handle(stream)),
                  "arl_observe_envs")
            return
        if self.rgb:
            H, W = pair_pool.shape[-3], pair_pool.shape[-2]
            check(lib.arl_observe_rgb(self._h, t, ptr(pair_pool), H, W, ptr(reward_pool), ptr(done_pool), pool_len,
                                      int(force_reset), resize_mode, stream_handle(stream)), "arl_observe_rgb")
            return
        check(lib.arl_observe(self._h, t, ptr(pair_pool), ptr(reward_pool), ptr(done_pool), pool_len,
                              int(force_reset), resize_mode, stream_handle(stream)), "arl_observe")

    def observe_stack(self, t: int, stack_pool=None, reward_pool=None, done_pool=None, pool_len: int = 1,
                      force_reset: bool = False, stream=None):
        """ARCH_STACK nets: stack_pool (pool_len, n, 4, 84, 84) uint8 whole
        frame stacks (arl_observe_stack); ARCH_STATES nets: (pool_len, n, 4,
        84, 84) f32 states, phi's output (arl_observe_states).  None ingests
        only the reward / done of step t (a terminal observation)."""
        check_pools(pool_len, stack_pool, reward_pool, done_pool)
        self.set_pools(stack_pool, reward_pool, done_pool)
        if self.states:
            if stack_pool is not None and stack_pool.dtype != torch.float32:
                raise ValueError("observe_stack: an ARCH_STATES net takes float32 states")
            check(lib.arl_observe_states(self._h, t, ptr(stack_pool), ptr(reward_pool), ptr(done_pool), pool_len,
                                         int(force_reset), stream_handle(stream)), "arl_observe_states")
            return
        check(lib.arl_observe_stack(self._h, t, ptr(stack_pool), ptr(reward_pool), ptr(done_pool), pool_len,
                                    int(force_reset), stream_handle(stream)), "arl_observe_stack")

    def truncate_window(self, t_len: int, stream=None):
        """Window steps [t_len, t_max) get no loss in the next learn (arl_truncate_window)."""
        check(lib.arl_truncate_window(self._h, t_len, stream_handle(stream)), "arl_truncate_window")

    def set_norm_fold(self, on: bool = True):
        """Fold the clip norm into learn()'s conv reduce (arl_net_set_norm_fold):
        only when the gradient is not all-reduced between learn and update."""
        check(lib.arl_net_set_norm_fold(self._h, int(on)), "arl_net_set_norm_fold")

    def set_forms(self, conv_epw=None, fc_big=None, lstm_xred=None, conv_bwd_ws=None):
        """Choose between the bit-identical kernel forms of this net's launches
        (arl_net_set_form): None leaves a form alone, "auto" restores the
        library's rule, anything else is the concrete value (conv_epw 1 / 2,
        the others 0 / 1).  Read when a launch is issued."""
        for name, v in (("conv_epw", conv_epw), ("fc_big", fc_big), ("lstm_xred", lstm_xred),
                        ("conv_bwd_ws", conv_bwd_ws)):
            if v is not None:
                check(lib.arl_net_set_form(self._h, FORMS[name], FORM_AUTO if v == "auto" else int(v)),
                      "arl_net_set_form")

    def form(self, name: str, launch_envs: int | None = None) -> int:
        """The concrete form a launch over launch_envs envs (default: all of
        the net's) would run now (arl_net_form): conv_epw 1 / 2, the others
        0 / 1."""
        v = ctypes.c_int()
        check(lib.arl_net_form(self._h, FORMS[name], self.n_envs if launch_envs is None else launch_envs,
                               ctypes.byref(v)), "arl_net_form")
        return v.value

    def set_returns_fusion(self, on: bool, gamma: float = 0.99, beta: float = 0.01, v_loss_coef: float = 0.5,
                           clip_reward: bool = True):
        """Run the learner's returns + heads backward inside the bootstrap
        step's policy launch (arl_net_set_returns_fusion; FF nets, one launch
        over all envs): the next act at t = t_max does them, and the window's
        LEARN_RETURNS part is skipped.  Bit-identical to the separate launch."""
        check(lib.arl_net_set_returns_fusion(self._h, int(on), gamma, beta, v_loss_coef, int(clip_reward)),
              "arl_net_set_returns_fusion")

    def set_loss(self, pi_loss_coef: float = 1.0, keep_loss_scale_same: bool = False):
        check(lib.arl_net_set_loss(self._h, pi_loss_coef, int(keep_loss_scale_same)), "arl_net_set_loss")

    def set_weight_decay(self, rate: float = 0.0):
        """NonbiasWeightDecay(rate) inside the update kernel (arl_net_set_weight_decay):
        after the clip, g += rate * p for every non-bias parameter; 0 = off.
        A captured window keeps the rate it was captured with."""
        check(lib.arl_net_set_weight_decay(self._h, float(rate)), "arl_net_set_weight_decay")

    def set_gae(self, lambda_: float = 1.0):
        """GAE(lambda) advantages in the policy term (arl_net_set_gae); the value
        target stays the n-step return.  1 = the n-step advantage: the kernels
        and arguments of a net that never called this.  A captured window keeps
        the lambda it was captured with."""
        check(lib.arl_net_set_gae(self._h, float(lambda_)), "arl_net_set_gae")

    # ------------------------------------------------------------ PPO epochs
    ppo_snap = None   # (4, t_max, n_envs) f32: logp_old, adv, ret, ratio; allocated by the first set_ppo
    ppo_clip = None   # clip_eps while PPO is on, else None
    ppo_carry = None  # LSTM: (2, n_envs, 256) f32, the rollout's (h_T, c_T) of the window; allocated by the first set_ppo

    def set_ppo(self, clip_eps: float | None = 0.2):
        """Run the window's update as clipped-surrogate epochs (arl_net_set_ppo):
        ppo_begin after the bootstrap forward, then per epoch [act(t, mode=0)
        for t < t_max, t ascending,] ppo_learn and optimize.  FF and LSTM nets
        with the NIPS head; an LSTM also registers its carry buffer
        (arl_net_set_ppo_state), so the next window starts from the rollout's
        recurrent state whatever the epoch count.  None switches it off.
        run_window (the one-call window) refuses while it is on."""
        lstm = self.base_arch == ARCH_LSTM
        if clip_eps is None:
            check(lib.arl_net_set_ppo(self._h, None, 0.0), "arl_net_set_ppo")
            if lstm and self.ppo_carry is not None:
                check(lib.arl_net_set_ppo_state(self._h, None), "arl_net_set_ppo_state")
            self.ppo_clip = None
            return
        if lstm:
            if self.ppo_carry is None:
                self.ppo_carry = torch.zeros((2, self.n_envs, 256), dtype=torch.float32, device=self.device)
            check(lib.arl_net_set_ppo_state(self._h, ptr(self.ppo_carry)), "arl_net_set_ppo_state")
        if self.ppo_snap is None:
            self.ppo_snap = torch.zeros((4, self.t_max, self.n_envs), dtype=torch.float32, device=self.device)
        check(lib.arl_net_set_ppo(self._h, ptr(self.ppo_snap), float(clip_eps)), "arl_net_set_ppo")
        self.ppo_clip = float(clip_eps)

    def ppo_begin(self, gamma=0.99, clip_reward=True, stream=None):
        """The window's snapshot (logp_old, adv, ret) from the workspace, after
        the bootstrap forward (arl_ppo_begin)."""
        check(lib.arl_ppo_begin(self._h, gamma, int(clip_reward), stream_handle(stream)), "arl_ppo_begin")

    def ppo_learn(self, beta=1e-2, v_loss_coef=0.5, stream=None):
        """One epoch's gradient from the slots' current contents (arl_ppo_learn)."""
        check(lib.arl_ppo_learn(self._h, beta, v_loss_coef, stream_handle(stream)), "arl_ppo_learn")

    def ppo_planes(self) -> dict:
        """Views of the snapshot's four (t_max, n_envs) planes."""
        if self.ppo_snap is None:
            raise RuntimeError("ppo_planes: PPO was never set (set_ppo)")
        return dict(zip(("logp_old", "adv", "ret", "ratio"), self.ppo_snap))

    ppo_v_old = None   # (t_max, n_envs) f32: the rollout's values, allocated by the first set_ppo_options(vclip=)
    ppo_aux = None     # PPO_AUX_DOUBLES f64: count, moments, epoch records; allocated by the first option set
    ppo_options = (False, None)   # (norm_adv, vclip) as last set

    def set_ppo_options(self, norm_adv: bool = False, vclip: float | None = None):
        """Options of the PPO epochs (arl_net_set_ppo_options): norm_adv
        normalises the snapshot's advantages over the window's live samples,
        vclip = eps clips the value loss around the rollout's values; either
        also switches the device-side per-epoch record on (ppo_epoch_log).
        The defaults switch all of it off: the launches of a net that never
        called this.  A captured window keeps what it was captured with."""
        if vclip is not None and not (0.0 < float(vclip) < float("inf")):   # (nan fails)
            raise ValueError("set_ppo_options: vclip must be finite and > 0 (None: off)")
        if not norm_adv and vclip is None:
            check(lib.arl_net_set_ppo_options(self._h, 0, 0.0, None, None), "arl_net_set_ppo_options")
            self.ppo_options = (False, None)
            return
        if vclip is not None and self.ppo_v_old is None:
            self.ppo_v_old = torch.zeros((self.t_max, self.n_envs), dtype=torch.float32, device=self.device)
        if self.ppo_aux is None:
            self.ppo_aux = torch.zeros(PPO_AUX_DOUBLES, dtype=torch.float64, device=self.device)
        check(lib.arl_net_set_ppo_options(self._h, int(bool(norm_adv)), 0.0 if vclip is None else float(vclip),
                                          ptr(self.ppo_v_old) if vclip is not None else None, ptr(self.ppo_aux)),
              "arl_net_set_ppo_options")
        self.ppo_options = (bool(norm_adv), None if vclip is None else float(vclip))

    def ppo_aux_raw(self, stream=None):
        """The aux block as the kernels left it: one copy to the host ->
        (count of epoch records ever written, (n_live, mean, std) of the last
        normalisation, the (PPO_LOG, PPO_STAT_FIELDS) f64 ring of records)."""
        if self.ppo_aux is None:
            raise RuntimeError("ppo_aux_raw: no PPO option was ever set (set_ppo_options)")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            a = self.ppo_aux.cpu()
        count = int(a[:1].view(torch.int64)[0])
        return count, a[1:4].tolist(), a[PPO_AUX_HEAD:].reshape(PPO_LOG, PPO_STAT_FIELDS).numpy()

    def ppo_epoch_log(self, last: int = 1, stream=None) -> list:
        """The newest `last` epoch records (at most PPO_LOG, and no more than
        were written), oldest first, each PPO_STAT_FIELDS floats
        (PPO_STAT_NAMES)."""
        count, _, ring = self.ppo_aux_raw(stream)
        k = max(0, min(int(last), count, PPO_LOG))
        return [ring[r % PPO_LOG].tolist() for r in range(count - k, count)]

    # ------------------------------------------------------------ Adam
    adam_m = None    # Adam's first moment (flat f32, the params' layout), allocated by the first set_adam
    adam_betas = None   # (beta1, beta2) while Adam is the net's optimizer, else None

    def set_adam(self, beta1: float | None = 0.9, beta2: float = 0.999):
        """Make Adam the optimizer of every update of this net (arl_net_set_adam):
        the first moment in `adam_m` (allocated once, zeroed), the second in
        `ms`, the update count on the device (adam_t).  beta1=None switches
        back to RMSpropAsync.  A captured window keeps the optimizer it was
        captured with."""
        if beta1 is None:
            check(lib.arl_net_set_adam(self._h, None, 0.0, 0.0), "arl_net_set_adam")
            self.adam_betas = None
            return
        if self.adam_m is None:
            self.adam_m = torch.zeros(self.param_floats, dtype=torch.float32, device=self.device)
        check(lib.arl_net_set_adam(self._h, ptr(self.adam_m), float(beta1), float(beta2)), "arl_net_set_adam")
        self.adam_betas = (float(beta1), float(beta2))

    def set_adam_t(self, t: int, stream=None):
        """Write the device-side count of Adam updates made (arl_net_set_adam_t;
        checkpoint resume).  Asynchronous on `stream`."""
        check(lib.arl_net_set_adam_t(self._h, int(t), stream_handle(stream)), "arl_net_set_adam_t")

    def adam_t(self) -> int:
        """The device-side count of Adam updates made (the host waits for it): a
        graph replay moves it, not the optimizer object's t."""
        return int(self.buffer("ctl", torch.int64)[CTL_ADAM_T].item())

    # ------------------------------------------------------------ episode statistics
    episode_stats_on = False

    def set_episode_stats(self, on: bool = True):
        """Accumulate episode returns / lengths on the device while observing
        (arl_net_set_episode_stats; a3c_ale.py:114-124 episode_r, total_r).
        Off by default; a captured window keeps the setting it was captured with."""
        check(lib.arl_net_set_episode_stats(self._h, int(on)), "arl_net_set_episode_stats")
        self.episode_stats_on = bool(on)

    def episode_stats_reset(self, stream=None):
        """Zero the whole episode-statistics block (arl_episode_stats_reset)."""
        check(lib.arl_episode_stats_reset(self._h, stream_handle(stream)), "arl_episode_stats_reset")

    def episode_stats_raw(self, clear: bool = False, stream=None) -> np.ndarray:
        """The 8 doubles of arl_episode_stats (EPISODE_STAT_FIELDS order): one
        reduce launch and one 64-byte copy to the host, which waits for it."""
        s = stream if stream is not None else torch.cuda.current_stream()
        out = getattr(self, "_ep_out", None)
        if out is None:
            out = self._ep_out = torch.zeros(8, dtype=torch.float64, device=self.device)
        with torch.cuda.stream(s):
            check(lib.arl_episode_stats(self._h, ptr(out), int(clear), stream_handle(s)), "arl_episode_stats")
            return out.cpu().numpy()

    def episode_stats(self, clear: bool = False, stream=None) -> dict:
        """Statistics of the episodes completed since the last reset (or the
        last clear=True read): the 8 reduced values plus mean, stdev (the
        sample standard deviation, as statistics.stdev) and mean_length."""
        return episode_stats_dict(self.episode_stats_raw(clear, stream))

    def episode_log(self) -> dict:
        """Device views of the per-env episode log: count (n,) episodes ever
        logged, and ret / len / step (EPISODE_LOG, n): entry k % EPISODE_LOG of
        env i is its k-th episode's return, length and global observation index."""
        n, L = self.n_envs, EPISODE_LOG
        return {"count": self.buffer("ep_log_count", torch.int64, (n,)),
                "ret": self.buffer("ep_log_ret", torch.float64, (L, n)),
                "len": self.buffer("ep_log_len", torch.int64, (L, n)),
                "step": self.buffer("ep_log_step", torch.int64, (L, n))}

    # ------------------------------------------------------------ window statistics
    window_stats_on = False

    def set_window_stats(self, on: bool = True):
        """Append one record of training statistics per update to the device-side
        window log (arl_net_set_window_stats; a3c.py:123-124,136-141,161-163:
        losses, gradient norm, entropy, value).  Off by default; a captured
        window keeps the setting it was captured with."""
        check(lib.arl_net_set_window_stats(self._h, int(on)), "arl_net_set_window_stats")
        self.window_stats_on = bool(on)

    def window_stats_reset(self, stream=None):
        """Zero the window log and its record count (arl_window_stats_reset)."""
        check(lib.arl_window_stats_reset(self._h, stream_handle(stream)), "arl_window_stats_reset")

    def window_stats_raw(self, last: int = 1, stream=None) -> np.ndarray:
        """The newest min(last, records written, WINDOW_LOG) records, oldest
        first, as (k, WINDOW_STAT_FIELDS) float64: one copy of the log and its
        count to the host, which waits for it."""
        if not self.window_stats_on:
            raise ValueError("window_stats: the feature is off (set_window_stats)")
        if last < 0:
            raise ValueError("window_stats: last must be >= 0")
        lo, nb = ctypes.c_int64(), ctypes.c_int64()
        check(lib.arl_net_buffer(self._h, b"win_log", ctypes.byref(lo), ctypes.byref(nb)), "arl_net_buffer")
        co = ctypes.c_int64()
        check(lib.arl_net_buffer(self._h, b"win_count", ctypes.byref(co), None), "arl_net_buffer")
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):   # win_count follows win_log in the workspace: one copy for both
            raw = self.workspace[lo.value:co.value + 8].cpu().numpy()
        log = raw[:nb.value].view(np.float64).reshape(WINDOW_LOG, WINDOW_STAT_FIELDS)
        count = int(raw[co.value - lo.value:].view(np.int64)[0])
        k = min(last, count, WINDOW_LOG)
        return log[[i % WINDOW_LOG for i in range(count - k, count)]].copy()

    def window_stats(self, last: int = 1, stream=None) -> list:
        """window_stats_raw as a list of dicts (window_stats_dict), oldest first."""
        return [window_stats_dict(r) for r in self.window_stats_raw(last, stream)]

    # ------------------------------------------------------------ device environment
    env = None        # the attached DeviceCatch / DeviceBreakout / DevicePong / DeviceTMaze / DeviceMaze (set_env), else None
    env_direct = False   # set_env(env, direct=True): the env renders straight into the frame ring, no pools

    def set_env(self, env=None, direct: bool = False):
        """Attach a device-resident env (envs.DeviceCatch, envs.DeviceBreakout,
        envs.DevicePong, envs.DeviceTMaze or envs.DeviceMaze, by its `kind`; arl_net_set_env) built
        for this net's n_envs, seed and env_offset, or detach with None.  While
        attached, run_window steps it after every act(t), t < t_max, and the
        pools handed to the window are written.  A captured window keeps the
        env it was captured with.

        direct=True (arl_net_set_env_direct): the env-step and the observation
        that follows it are one launch that writes the 84x84 plane into the
        frame ring and never the frame pair (env_reset_observe /
        env_step_observe); windows then take None for their pools.  The ring,
        the window buffers and every result are bit-identical to direct=False."""
        if env is None:
            check(lib.arl_net_set_env(self._h, ENV_CATCH, None), "arl_net_set_env")
            self.env, self.env_direct = None, False
            return
        if (env.n, env.seed, env.env_offset) != (self.n_envs, self.seed, self.env_offset):
            raise ValueError("set_env: the env must be built with the net's n_envs, seed and env_offset")
        check(lib.arl_net_set_env(self._h, env.kind, ptr(env.state)), "arl_net_set_env")
        check(lib.arl_net_set_env_direct(self._h, int(bool(direct))), "arl_net_set_env_direct")
        self.env, self.env_direct = env, bool(direct)

    def env_reset_observe(self, resize_mode: int = RESIZE_SCALAR, stream=None):
        """Direct env: env_reset + observe(0, force_reset=True) in one launch,
        without pools (arl_env_reset_observe)."""
        check(lib.arl_env_reset_observe(self._h, resize_mode, stream_handle(stream)), "arl_env_reset_observe")

    def env_step_observe(self, t: int, resize_mode: int = RESIZE_SCALAR, stream=None, envs=None):
        """Direct env: env_step(t) + observe(t + 1) in one launch, without pools
        (arl_env_step_observe); envs=(e0, ne): only that range."""
        e0, ne = envs if envs is not None else (0, self.n_envs)
        check(lib.arl_env_step_observe(self._h, t, e0, ne, resize_mode, stream_handle(stream)),
              "arl_env_step_observe")

    def env_reset(self, pair_pool, reward_pool, done_pool, pool_len: int, stream=None):
        """Episode 0 of every env into pool entry (step counter) % pool_len
        (arl_env_reset); the window that follows runs with first=True."""
        check_pools(pool_len, pair_pool, reward_pool, done_pool)
        self.set_pools(pair_pool, reward_pool, done_pool)
        check(lib.arl_env_reset(self._h, ptr(pair_pool), ptr(reward_pool), ptr(done_pool), pool_len,
                                stream_handle(stream)), "arl_env_reset")

    def env_step(self, t: int, pair_pool, reward_pool, done_pool, pool_len: int, stream=None, envs=None):
        """One env-step from row t of the actions buffer into the pool entry
        observe(t + 1) reads (arl_env_step); envs=(e0, ne): only that range."""
        check_pools(pool_len, pair_pool, reward_pool, done_pool)
        self.set_pools(pair_pool, reward_pool, done_pool)
        e0, ne = envs if envs is not None else (0, self.n_envs)
        check(lib.arl_env_step(self._h, t, e0, ne, ptr(pair_pool), ptr(reward_pool), ptr(done_pool), pool_len,
                               stream_handle(stream)), "arl_env_step")

    def reset_state(self, e0: int = 0, n: int | None = None, stream=None):
        """LSTM: the pi_and_v recurrent state of rows [e0, e0 + n) -> None (arl_reset_state)."""
        n = self.n_envs - e0 if n is None else n
        check(lib.arl_reset_state(self._h, e0, n, stream_handle(stream)), "arl_reset_state")

    def act(self, t: int, mode: int = 1, stream=None, envs=None):
        """mode: 0 forward only, 1 sampled action, 2 greedy (first argmax);
        envs=(e0, ne): only envs [e0, e0 + ne) (arl_act_envs)."""
        self._sync_params()
        if envs is not None:
            check(lib.arl_act_envs(self._h, t, envs[0], envs[1], mode, stream_handle(stream)), "arl_act_envs")
            return
        check(lib.arl_act_mode(self._h, t, mode, stream_handle(stream)), "arl_act_mode")

    def observe_act(self, t: int, pair_pool: torch.Tensor, reward_pool=None, done_pool=None, pool_len: int = 1,
                    force_reset: bool = False, resize_mode: int = RESIZE_SCALAR, mode: int = 1, stream=None,
                    envs=None):
        """observe(t, ...) then act(t, mode) of envs (all if None).  (phi fused into the
        conv launch was built bit-identical and measured slower: DESIGN.md.)"""
        self.observe(t, pair_pool, reward_pool, done_pool, pool_len, force_reset, resize_mode, stream, envs)
        self.act(t, mode, stream, envs)

    def default_env_groups(self) -> int:
        """Forward chains per window that measured fastest on one MI355X:
        2 from 1,024 envs up, else 1.  Since the 512-env launches run two envs a
        conv workgroup and 64-row FC tiles, one chain of 512 envs beats two of
        256 (C4 0.497 vs 0.509-0.518 ms), while 1,024 LSTM envs still gain
        from two chains of 512 (profiles/r03/r3l)."""
        return 2 if self.n_envs >= 1024 else 1

    def env_groups(self, groups: int):
        """Split the envs into <= `groups` contiguous ranges (e0, ne) with e0 a
        multiple of ENV_GROUP_ALIGN; [(0, n_envs)] when they do not split."""
        if groups <= 1 or self.arch == ARCH_FF_NATURE or self.states:
            return [(0, self.n_envs)]
        per = -(-self.n_envs // groups)
        per = -(-per // ENV_GROUP_ALIGN) * ENV_GROUP_ALIGN
        out, e0 = [], 0
        while e0 < self.n_envs:
            ne = min(per, self.n_envs - e0)
            out.append((e0, ne))
            e0 += ne
        return out

    STAGES = {"conv_fwd": 1, "fc_fwd": 2, "policy": 3, "fc_bwd": 4, "conv_bwd": 5, "returns": 6, "conv_reduce": 7,
              "grad_sqnorm": 8, "lstm_gates": 9, "lstm_bptt": 10, "lstm_wgrad": 11, "rmsprop": 13}

    def run_stage(self, stage: str, t: int = 0, stream=None):
        """One window stage alone on the current workspace (timing / profiling)."""
        check(lib.arl_run_stage(self._h, self.STAGES[stage], t, stream_handle(stream)), "arl_run_stage")

    def learn(self, gamma=0.99, beta=1e-2, v_loss_coef=0.5, clip_reward=True, stream=None):
        """Gradient of the window (arl_learn)."""
        check(lib.arl_learn(self._h, gamma, beta, v_loss_coef, int(clip_reward), stream_handle(stream)), "arl_learn")

    def learn_parts(self, parts, gamma=0.99, beta=1e-2, v_loss_coef=0.5, clip_reward=True, stream=None):
        """arl_learn_part for each part in order on one stream (NIPS heads)."""
        h = stream_handle(stream)
        for p in parts:
            check(lib.arl_learn_part(self._h, p, gamma, beta, v_loss_coef, int(clip_reward), h), "arl_learn_part")

    def optimize(self, lr0=7e-4, total_steps=0, n_total=0, alpha=0.99, eps=0.1, clip=40.0, stream=None,
                 advance=False):
        """Clip + RMSProp; advance=True also ends the window (arl_optimize_advance)."""
        self._sync_params()
        if advance:
            check(lib.arl_optimize_advance(self._h, lr0, int(total_steps), int(n_total), alpha, eps, clip,
                                           stream_handle(stream)), "arl_optimize_advance")
        else:
            check(lib.arl_optimize(self._h, lr0, int(total_steps), int(n_total), alpha, eps, clip,
                                   stream_handle(stream)), "arl_optimize")

    def run_window(self, pair_pool, reward_pool, done_pool, pool_len: int, first: bool, resize_mode: int,
                   gamma: float, beta: float, v_loss_coef: float, clip_reward: bool, lr0: float, total_steps: int,
                   n_total: int, alpha: float, eps: float, clip: float, stream=None):
        """A whole lockstep window in one call (arl_run_window): T x (observe,
        act), the bootstrap, learn, clip + RMSProp and the advance -- the
        launches of observe / act / learn / optimize(advance=True) in order."""
        if not self.env_direct:   # (a direct env reads no pools: None / 0 are fine)
            check_pools(pool_len, pair_pool, reward_pool, done_pool)
            self.set_pools(pair_pool, reward_pool, done_pool)
        self._sync_params()
        check(lib.arl_run_window(self._h, ptr(pair_pool), ptr(reward_pool), ptr(done_pool), pool_len, int(first),
                                 resize_mode, gamma, beta, v_loss_coef, int(clip_reward), lr0, int(total_steps),
                                 int(n_total), alpha, eps, clip, stream_handle(stream)), "arl_run_window")

    def advance(self, stream=None):
        check(lib.arl_advance(self._h, stream_handle(stream)), "arl_advance")

    def forward_states(self, states: torch.Tensor, mode: int = 0, stream=None, keep_same_state: bool = False):
        """pi_and_v on explicit f32 states into slot t_max (arl_forward_states);
        LSTM: advances the pi_and_v state unless keep_same_state."""
        n = states.shape[0]
        c = 3 if self.rgb else 4
        if states.dtype != torch.float32 or tuple(states.shape[1:]) != (c, 84, 84):
            raise ValueError(f"forward_states: need (n, {c}, 84, 84) float32 states")
        m = mode | (FWD_KEEP_STATE if keep_same_state else 0)
        self._sync_params()
        check(lib.arl_forward_states(self._h, ptr(states), n, m, stream_handle(stream)), "arl_forward_states")

    # ------------------------------------------------------------ window timeline (measurement)
    stamping = False

    def stamps_begin(self, cap: int):
        """From now on every stage launch records a timing event after its
        kernel(s) (arl_stamps_begin); read them with stamps_end()."""
        check(lib.arl_stamps_begin(self._h, int(cap)), "arl_stamps_begin")
        self.stamping = True

    def stamps_sparse(self, period: int):
        """Right after stamps_begin, for windows of `period` stamp calls: window w
        records only its calls t - 1 and t (t = w mod period; arl_stamps_sparse);
        stamps_end then gives ms = -1 for the intervals between unrelated calls."""
        check(lib.arl_stamps_sparse(self._h, int(period)), "arl_stamps_sparse")

    def stamp(self, stage: int = STAGE_HOST, stream=None):
        """A caller's stamp (e.g. after a collective); no-op unless stamping."""
        if self.stamping:
            check(lib.arl_stamp(self._h, int(stage), stream_handle(stream)), "arl_stamp")

    def stamps_end(self):
        """Stop the timeline; returns (ms, stages): ms[i] = time from stamp
        i - 1 to stamp i (ms[0] = 0), stages[i] = the stage name stamp i
        closes (arl_stamps_read; waits for the last stamp)."""
        self.stamping = False
        cnt = ctypes.c_int()
        check(lib.arl_stamps_end(self._h, ctypes.byref(cnt)), "arl_stamps_end")
        n = cnt.value
        ms = (ctypes.c_float * max(n, 1))()
        st = (ctypes.c_int * max(n, 1))()
        check(lib.arl_stamps_read(self._h, 0, n, ctypes.cast(ms, ctypes.c_void_p), ctypes.cast(st, ctypes.c_void_p)),
              "arl_stamps_read")
        return np.array(ms[:n], np.float64), [STAGE_NAMES.get(int(x), str(int(x))) for x in st[:n]]

    # ------------------------------------------------------------ outputs
    def step_outputs(self, t: int) -> dict:
        """Views of the policy / value outputs of window step t."""
        N, A, T1 = self.n_envs, self.n_actions, self.t_max + 1
        f32 = torch.float32
        return {
            "logits": self.buffer("logits", f32, (T1, N, A))[t],
            "probs": self.buffer("probs", f32, (T1, N, A))[t],
            "log_probs": self.buffer("logp", f32, (T1, N, A))[t],
            "v": self.buffer("v", f32, (T1, N))[t],
            "entropy": self.buffer("entropy", f32, (T1, N))[t],
            "actions": self.buffer("actions", torch.int32, (T1, N))[t],
            "action_log_probs": self.buffer("logp_a", f32, (T1, N))[t],
        }
