"""ctypes binding of libasyncrl_hip.so (C ABI in include/asyncrl_hip.h).

torch is imported first on purpose: torch ships its own libamdhip64.so
(SONAME libamdhip64.so.7), so the extension resolves to the SAME HIP runtime
instance and torch's streams / device pointers are valid in our calls.

There is no fallback: if the shared object is missing the import fails loudly
(build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C async-rl_amd/csrc`).
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL load, see module doc)

# ASYNCRL_HIP_LIB: alternative build of the same library (timing ablations only)
LIB_PATH = os.environ.get("ASYNCRL_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                             "libasyncrl_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"asyncrl_amd: native extension not built ({LIB_PATH} missing); "
        "run `make -C async-rl_amd/csrc` or __graft_entry__.build()")

lib = ctypes.CDLL(LIB_PATH)

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_i64 = ctypes.c_int64
c_u64 = ctypes.c_uint64
c_double = ctypes.c_double

# name -> (restype, argtypes); every symbol declared in include/asyncrl_hip.h
SIGNATURES = {
    "arl_abi_version": (c_int, []),
    "arl_last_error": (ctypes.c_char_p, []),
    "arl_current_screen": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "arl_max_luminance": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    "arl_phi_stack": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "arl_dqn_phi": (c_int, [c_void_p, c_void_p, c_i64, c_void_p]),
    "arl_rgb_phi": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_int, c_void_p]),
    "arl_net_create": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_u64]),
    "arl_net_destroy": (None, [c_void_p]),
    "arl_net_param_floats": (c_i64, [c_void_p]),
    "arl_net_param_count": (c_int, [c_void_p]),
    "arl_net_param_info": (c_int, [c_void_p, c_int, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64),
                                   ctypes.c_char_p, c_int]),
    "arl_net_workspace_bytes": (c_i64, [c_void_p]),
    "arl_net_buffer": (c_int, [c_void_p, ctypes.c_char_p, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "arl_net_bind": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "arl_net_reset": (c_int, [c_void_p, c_void_p]),
    "arl_net_params_changed": (c_int, [c_void_p]),
    "arl_net_prepare": (c_int, [c_void_p, c_void_p]),
    "arl_net_param_generation": (c_int, [c_void_p, ctypes.POINTER(c_u64), ctypes.POINTER(c_u64)]),
    "arl_net_set_pool": (c_int, [c_void_p, c_int, c_void_p, c_i64]),
    "arl_observe": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p]),
    "arl_observe_rgb": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_i64, c_int, c_int,
                                c_void_p]),
    "arl_observe_stack": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "arl_observe_states": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "arl_truncate_window": (c_int, [c_void_p, c_int, c_void_p]),
    "arl_net_set_loss": (c_int, [c_void_p, c_double, c_int]),
    "arl_net_set_weight_decay": (c_int, [c_void_p, c_double]),
    "arl_net_set_gae": (c_int, [c_void_p, c_double]),
    "arl_net_set_ppo": (c_int, [c_void_p, c_void_p, c_double]),
    "arl_net_set_ppo_state": (c_int, [c_void_p, c_void_p]),
    "arl_ppo_begin": (c_int, [c_void_p, c_double, c_int, c_void_p]),
    "arl_ppo_learn": (c_int, [c_void_p, c_double, c_double, c_void_p]),
    "arl_ppo_snapshot": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64, c_int, c_double,
                                 c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "arl_ppo_lossgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int, c_i64, c_int, c_double, c_double, c_double, c_double, c_int, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    "arl_net_set_ppo_options": (c_int, [c_void_p, c_int, c_double, c_void_p, c_void_p]),
    "arl_ppo_lossgrad_vclip": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_int, c_i64, c_int, c_double, c_double, c_double, c_double,
                                       c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "arl_ppo_normalize_adv": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_void_p, c_void_p]),
    "arl_ppo_epoch_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_int, c_i64, c_int, c_double, c_double, c_double, c_double, c_void_p,
                                    c_void_p]),
    "arl_net_set_adam": (c_int, [c_void_p, c_void_p, c_double, c_double]),
    "arl_net_set_adam_t": (c_int, [c_void_p, c_i64, c_void_p]),
    "arl_adam": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_double, c_double, c_double, c_double, c_i64,
                         c_double, c_void_p, c_double, c_void_p]),
    "arl_net_set_norm_fold": (c_int, [c_void_p, c_int]),
    "arl_net_set_form": (c_int, [c_void_p, c_int, c_int]),
    "arl_net_form": (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_int)]),
    "arl_net_set_returns_fusion": (c_int, [c_void_p, c_int, c_double, c_double, c_double, c_int]),
    "arl_reset_state": (c_int, [c_void_p, c_i64, c_i64, c_void_p]),
    "arl_act": (c_int, [c_void_p, c_int, c_void_p]),
    "arl_act_mode": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "arl_observe_envs": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_i64,
                                 c_int, c_int, c_void_p]),
    "arl_act_envs": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "arl_run_stage": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "arl_stamps_begin": (c_int, [c_void_p, c_int]),
    "arl_stamps_sparse": (c_int, [c_void_p, c_int]),
    "arl_stamp": (c_int, [c_void_p, c_int, c_void_p]),
    "arl_stamps_end": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "arl_stamps_read": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "arl_learn": (c_int, [c_void_p, c_double, c_double, c_double, c_int, c_void_p]),
    "arl_run_window": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_double, c_double,
                               c_double, c_int, c_double, c_i64, c_i64, c_double, c_double, c_double, c_void_p]),
    "arl_learn_part": (c_int, [c_void_p, c_int, c_double, c_double, c_double, c_int, c_void_p]),
    "arl_optimize": (c_int, [c_void_p, c_double, c_i64, c_i64, c_double, c_double, c_double, c_void_p]),
    "arl_advance": (c_int, [c_void_p, c_void_p]),
    "arl_optimize_advance": (c_int, [c_void_p, c_double, c_i64, c_i64, c_double, c_double, c_double, c_void_p]),
    "arl_forward_states": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "arl_rmsprop": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_double, c_double, c_double, c_double,
                            c_void_p, c_void_p]),
    "arl_rmsprop_wd": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_double, c_double, c_double, c_double,
                               c_void_p, c_double, c_void_p]),
    "arl_policy": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_u64, c_void_p,
                           c_i64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p]),
    "arl_returns_lossgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64,
                                     c_int, c_double, c_double, c_double, c_double, c_int, c_int, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    "arl_returns_lossgrad_gae": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64,
                                         c_int, c_double, c_double, c_double, c_double, c_double, c_int, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "arl_stream_copy": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p]),
    "arl_net_set_episode_stats": (c_int, [c_void_p, c_int]),
    "arl_episode_stats_reset": (c_int, [c_void_p, c_void_p]),
    "arl_episode_stats": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "arl_net_set_window_stats": (c_int, [c_void_p, c_int]),
    "arl_window_stats_reset": (c_int, [c_void_p, c_void_p]),
    "arl_catch_state_bytes": (c_i64, [c_i64]),
    "arl_catch_reset": (c_int, [c_void_p, c_i64, c_int, c_u64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "arl_catch_step": (c_int, [c_void_p, c_int, c_void_p, c_i64, c_int, c_u64, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "arl_breakout_state_bytes": (c_i64, [c_i64]),
    "arl_breakout_reset": (c_int, [c_void_p, c_i64, c_int, c_u64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "arl_breakout_step": (c_int, [c_void_p, c_int, c_void_p, c_i64, c_int, c_u64, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "arl_pong_state_bytes": (c_i64, [c_i64]),
    "arl_pong_reset": (c_int, [c_void_p, c_i64, c_int, c_u64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "arl_pong_step": (c_int, [c_void_p, c_int, c_void_p, c_i64, c_int, c_u64, c_int, c_void_p, c_void_p, c_void_p,
                              c_void_p]),
    "arl_tmaze_state_bytes": (c_i64, [c_i64]),
    "arl_tmaze_reset": (c_int, [c_void_p, c_i64, c_int, c_u64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "arl_tmaze_step": (c_int, [c_void_p, c_int, c_void_p, c_i64, c_int, c_u64, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "arl_maze_state_bytes": (c_i64, [c_i64]),
    "arl_maze_reset": (c_int, [c_void_p, c_i64, c_int, c_u64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "arl_maze_step": (c_int, [c_void_p, c_int, c_void_p, c_i64, c_int, c_u64, c_int, c_int, c_int, c_void_p, c_void_p,
                              c_void_p, c_void_p]),
    "arl_net_set_env": (c_int, [c_void_p, c_int, c_void_p]),
    "arl_env_reset": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    "arl_env_step": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    "arl_net_set_env_direct": (c_int, [c_void_p, c_int]),
    "arl_env_reset_observe": (c_int, [c_void_p, c_int, c_void_p]),
    "arl_env_step_observe": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "arl_env_step_screen": (c_int, [c_int, c_void_p, c_int, c_void_p, c_i64, c_int, c_u64, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args

if lib.arl_abi_version() != 4:
    raise ImportError(f"asyncrl_amd: {LIB_PATH} has ABI {lib.arl_abi_version()}, expected 4 (rebuild it)")

ARCH_FF = 0
ARCH_LSTM = 1
ARCH_FF_NATURE = 2   # A3CFF with NatureDQNHead (dqn_head.py:6-28)
ARCH_RGB = 16        # flag for FF / LSTM: the ViZDoom models (train_a3c_doom.py:25-63), RGB screens
ARCH_STACK = 32      # flag for FF / LSTM: observations are whole 4-screen stacks (ALE.state, ale.py:91-94)
ARCH_STATES = 64     # flag for FF / LSTM: observations are f32 (4, 84, 84) states, phi's output (a3c.py:34,73)
FWD_KEEP_STATE = 16  # arl_forward_states mode bit: LSTM keep_same_state (a3c_ale.py:57-60)
ABI_VERSION = 4
ACT_CONV_ONLY = 4      # arl_act_envs mode bits (env-group staggering)
ACT_AFTER_CONV = 8
ENV_GROUP_ALIGN = 32   # arl_observe_envs / arl_act_envs: e0 % ENV_GROUP_ALIGN == 0
LEARN_RETURNS, LEARN_TRUNK, LEARN_CONV = range(3)
POOL_FRAMES, POOL_REWARDS, POOL_DONES = range(3)   # arl_net_set_pool kinds
ENV_CATCH = 1          # ARL_ENV_CATCH: arl_net_set_env kind, the device-resident Catch
CATCH_STATE_INTS = 8   # int32 per env and half of its state: [bx, by, vx, px, episode, steps_in_episode, 0, 0]
ENV_BREAKOUT = 2       # ARL_ENV_BREAKOUT: the device-resident Breakout
ENV_GAME_OVER_ONLY = 0x100   # ARL_ENV_GAME_OVER_ONLY, or'ed into the Breakout kind: a life loss is not a terminal
BREAKOUT_STATE_INTS = 16     # [bx, by, vx, vy, px, lives, serves, steps_in_episode, game, game_steps, score,
                             #  bricks_left, b0, b1, b2, b3]
ENV_PONG = 4                 # ARL_ENV_PONG: the device-resident Pong; its kind carries the points of a game
PONG_STATE_INTS = 12         # [bx, by, vx, vy, py, oy, serves, steps_in_episode, game, game_steps, score_agent,
                             #  score_opp]
PONG_POINTS_MAX = 21
ENV_TMAZE = 8                # ARL_ENV_TMAZE: the device-resident T-maze; its kind carries the corridor's length
TMAZE_STATE_INTS = 8         # [pos, cue, length, steps_in_episode, episode, hits, misses, lapses]
TMAZE_LENGTH_MAX = 8
ENV_MAZE = 32                # ARL_ENV_MAZE: the device-resident maze; its kind carries rooms, view and levels
MAZE_STATE_INTS = 8          # [pos | goal << 8, bits, steps_in_episode, episode, wins, timeouts, level, cfg]
MAZE_ROOMS_MIN, MAZE_ROOMS_MAX, MAZE_VIEW_MAX, MAZE_LEVELS_MAX = 2, 4, 2, 1023


def env_pong_points(points: int) -> int:
    """ARL_ENV_PONG_POINTS(points): or'ed into ENV_PONG; 1..21, and 0 means 21."""
    return points << 16


def env_tmaze_length(length: int) -> int:
    """ARL_ENV_TMAZE_LENGTH(length): or'ed into ENV_TMAZE; 1..8, and 0 means 4."""
    return length << 16


def env_maze_fields(rooms: int, view: int, levels: int) -> int:
    """ARL_ENV_MAZE_ROOMS(rooms) | ARL_ENV_MAZE_VIEW(view) | ARL_ENV_MAZE_LEVELS(levels): or'ed into ENV_MAZE;
    rooms 2..4 (0 means 3), view 0..2, levels 0..1023."""
    return rooms << 16 | view << 19 | levels << 21


CTL_ADAM_T = 3         # ARL_CTL_ADAM_T: the control block's count of Adam updates made (buffer "ctl", int64[16])
EPISODE_LOG = 8        # ARL_EPISODE_LOG: episodes per env the device-side episode log keeps
# the 8 doubles of arl_episode_stats, in order
EPISODE_STAT_FIELDS = ("episodes", "return_sum", "return_sumsq", "return_min", "return_max", "length_sum", "steps",
                       "reward_sum")
WINDOW_LOG = 64           # ARL_WINDOW_LOG: records the device-side window log keeps
WINDOW_STAT_FIELDS = 17   # ARL_WINDOW_STAT_FIELDS: doubles per record, named in order:
WINDOW_STAT_NAMES = ("window", "step", "samples", "terminals", "reward_sum", "pi_loss", "v_loss", "entropy_sum",
                     "value_sum", "value_sumsq", "return_sum", "return_sumsq", "adv_sum", "adv_sumsq", "grad_sqnorm",
                     "clip_scale", "lr")
PPO_LOG = 16              # ARL_PPO_LOG: epoch records the aux block of arl_net_set_ppo_options keeps
PPO_STAT_FIELDS = 10      # ARL_PPO_STAT_FIELDS: doubles per epoch record, named in order:
PPO_STAT_NAMES = ("window", "epoch", "samples", "clipped", "kl_sum", "ratio_max", "ratio_min", "vclipped", "adv_sum",
                  "adv_sumsq")
PPO_AUX_HEAD = 8          # doubles before the records: the int64 count, n_live, mean, std, 4 reserved
PPO_AUX_DOUBLES = PPO_AUX_HEAD + PPO_LOG * PPO_STAT_FIELDS   # ARL_PPO_AUX_DOUBLES
# window timeline stages (arl_stamps_*): arl_run_stage's 1..11, then the stamp-only ones
STAGE_NAMES = {1: "conv_fwd", 2: "fc_fwd", 3: "policy", 4: "fc_bwd", 5: "conv_bwd", 6: "returns", 7: "conv_reduce",
               8: "grad_sqnorm", 9: "lstm_gates", 10: "lstm_bptt", 11: "lstm_wgrad", 12: "phi", 13: "rmsprop",
               14: "lstm_cell", 15: "host", 16: "other"}
STAGE_HOST = 15
FORM_AUTO = -1         # ARL_FORM_AUTO: arl_net_set_form's value for "the library's rule"
# DeviceNet.set_forms / form names -> ARL_FORM_* ids
FORMS = {"conv_epw": 0, "fc_big": 1, "lstm_xred": 2, "conv_bwd_ws": 3}
RESIZE_SCALAR = 0
RESIZE_SIMD = 1
RESIZE_CROP = 2      # flag, combine with SCALAR / SIMD: ale.py crop_or_scale='crop'


class ArlError(RuntimeError):
    pass


def env_defaults() -> dict:
    """Defaults of DeviceNet's kernel forms and A3C's window options from the
    process environment, read when a DeviceNet or an A3C is constructed (not at
    import); explicit constructor arguments and DeviceNet.set_forms win.

    A benchmarking convenience of this Python mirror only: bench.py models and
    labels its stages from the first four names and scripts/env_ab.sh drives it
    by them, so the package follows the same names.  The C library never reads
    the environment: there the forms are arl_net_set_form's per-net state.
    Forms: a concrete value, or None (auto) when unset or not one of the
    form's two values; window options: on unless set to "0"."""
    env = os.environ.get

    def form(name, values):
        v = env(name, "")[:1]
        return int(v) if v in values else None

    return {"conv_epw": form("ARL_CONV_EPW", ("1", "2")), "fc_big": form("ARL_FC_BIG", ("0", "1")),
            "lstm_xred": form("ARL_LSTM_XRED", ("0", "1")), "conv_bwd_ws": form("ARL_CB_WS", ("0", "1")),
            "window_c": env("ARL_WINDOW_C", "1") != "0", "fuse_returns": env("ARL_FUSE_RETURNS", "1") != "0",
            "overlap_allreduce": env("ARL_OVERLAP_ALLREDUCE", "1") != "0"}


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib.arl_last_error().decode(errors="replace")
        raise ArlError(f"{what or 'asyncrl_hip'} failed (code {rc}): {msg}")


def ptr(t) -> int | None:
    """Device pointer of a torch tensor (None passes NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ArlError("asyncrl_amd: tensors must live on the GPU (HIP device)")
    if not t.is_contiguous():
        raise ArlError("asyncrl_amd: tensors must be contiguous")
    return t.data_ptr()


def stream_handle(stream=None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream
