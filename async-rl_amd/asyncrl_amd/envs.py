"""Env-side adapter: emulator frames -> the hot path's frame-pair input
(SURVEY §8(f) item 4).

The reference wraps ALE in `ale.ALE` (ale.py:11-161): frame skip 4 with the
screen before the 4th act kept for the max-of-two, a life loss treated as
terminal, up to 30 no-op starts, the game reset on game over, and it runs the
whole phi pre-stage (max, luminance, resize, stack) on the CPU.  Here the
phi pre-stage is the GPU kernel, so the adapter stops at the raw frame pair:

  ALEFramePairs  one emulator, the reference's stepping semantics verbatim
                 (same ALE calls in the same order, so the same frames,
                 rewards, terminals and no-op counts), returning
                 (frame 4, frame 3) pairs instead of processed screens;
  VecALE         N of them stepped by host worker threads (the emulator
                 releases the GIL in act()) into pinned host buffers, copied
                 to the device asynchronously, in the (n, 2, 210, 160, 3)
                 uint8 / reward / terminal layout A3C.act takes;
  DeviceCatch    no emulator at all: a small game whose transition and render
                 are one HIP kernel (csrc/catch.hip), so the loop env -> phi ->
                 forward -> sample -> env closes on the device;
  DeviceBreakout the same for Breakout (csrc/breakout.hip): bricks, lives,
                 rewards of 1, 4 and 7, episodes of different lengths;
  DevicePong     and for Pong (csrc/pong.hip): an opponent, rewards of both
                 signs inside a game, games of hundreds of steps, a
                 background that is not black;
  DeviceTMaze    and for a cue-recall T-maze (csrc/tmaze.hip): the cue is on
                 an episode's first screen alone and is asked for `length`
                 steps later -- the one env here the FF model cannot solve;
  DeviceMaze     and for a grid maze (csrc/maze.hip) whose layout, start and
                 goal are drawn per episode from a numbered set of levels:
                 train on `levels` tasks, score on all of them.

Batched convention: a step whose action ends the episode returns
done = 1, the reward of that step, and the FIRST pair of the next episode
(the env re-initialises at once -- the reference's train loop does the same
one act() call later, a3c_ale.py:117-124).  Host-side code, not a kernel.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ._lib import (BREAKOUT_STATE_INTS, CATCH_STATE_INTS, ENV_BREAKOUT, ENV_CATCH, ENV_GAME_OVER_ONLY, ENV_MAZE,
                   ENV_PONG, ENV_TMAZE, MAZE_LEVELS_MAX, MAZE_ROOMS_MAX, MAZE_ROOMS_MIN, MAZE_STATE_INTS,
                   MAZE_VIEW_MAX, PONG_POINTS_MAX, PONG_STATE_INTS, TMAZE_LENGTH_MAX, TMAZE_STATE_INTS, check,
                   env_maze_fields, env_pong_points, env_tmaze_length, lib, ptr, stream_handle)

SCREEN = (210, 160, 3)


class ALEFramePairs:
    """ale.ALE (ale.py:11-161) up to the raw frame pair.

    `ale` is an ale_python_interface.ALEInterface (ROM already loaded) or
    anything with its methods (act, getScreenRGB, lives, game_over,
    reset_game, getMinimalActionSet).  `nullop_rng` draws the no-op count
    with .randint(0, max_start_nullops + 1) -- numpy's global RNG by
    default, exactly like the reference."""

    def __init__(self, ale, frame_skip: int = 4, treat_life_lost_as_terminal: bool = True,
                 max_start_nullops: int = 30, nullop_rng=None):
        if frame_skip != 4:
            raise ValueError("the reference's receive_action is written for frame_skip = 4 (ale.py:118)")
        self.ale = ale
        self.treat_life_lost_as_terminal = treat_life_lost_as_terminal
        self.max_start_nullops = max_start_nullops
        self.rng = nullop_rng if nullop_rng is not None else np.random
        self.legal_actions = ale.getMinimalActionSet()
        self.pair = np.zeros((2,) + SCREEN, np.uint8)   # (current, previous raw screen)
        self.initialize()

    @classmethod
    def from_rom(cls, rom_filename: str, seed: int, **kw):
        """ale.py:21-49 setup (repeat_action_probability 0, no colour
        averaging, seeded) on a real ALE; needs ale_python_interface."""
        try:
            from ale_python_interface import ALEInterface
        except ImportError as e:
            raise ImportError("ale_python_interface is not installed; pass an emulator object instead") from e
        if not 0 <= seed < 2 ** 16:
            raise ValueError("ALE's random seed must be represented by unsigned int")
        ale = ALEInterface()
        ale.setInt(b"random_seed", seed)
        ale.setFloat(b"repeat_action_probability", 0.0)
        ale.setBool(b"color_averaging", False)
        ale.loadROM(str.encode(rom_filename))
        return cls(ale, **kw)

    @property
    def number_of_actions(self) -> int:
        return len(self.legal_actions)

    @property
    def is_terminal(self) -> bool:                       # ale.py:98-103
        if self.treat_life_lost_as_terminal:
            return self.lives_lost or self.ale.game_over()
        return self.ale.game_over()

    def initialize(self) -> np.ndarray:
        """ale.py:141-161: reset on game over, no-op starts; the first
        observation pairs the screen with itself (max of equal frames)."""
        if self.ale.game_over():
            self.ale.reset_game()
        if self.max_start_nullops > 0:
            for _ in range(self.rng.randint(0, self.max_start_nullops + 1)):
                self.ale.act(0)
        self.reward = 0
        scr = self.ale.getScreenRGB()
        self.pair[0] = scr
        self.pair[1] = scr
        self.lives_lost = False
        self.lives = self.ale.lives()
        return self.pair

    def receive_action(self, action: int):
        """ale.py:111-139: 4 frames, the raw screen before the 4th act kept;
        stops early on a terminal.  Returns the summed reward; on a
        non-terminal step self.pair = (screen after act 4, screen before)."""
        assert not self.is_terminal
        rewards = []
        last = None
        for i in range(4):
            if i == 3:
                last = self.ale.getScreenRGB()
            rewards.append(self.ale.act(self.legal_actions[action]))
            self.lives_lost = self.lives > self.ale.lives()
            self.lives = self.ale.lives()
            if self.is_terminal:
                break
        if not self.is_terminal:
            self.pair[0] = self.ale.getScreenRGB()
            self.pair[1] = last
        self.reward = sum(rewards)
        return self.reward

    def step(self, action: int):
        """One batched-convention step: (pair, reward, done)."""
        r = self.receive_action(action)
        done = self.is_terminal
        if done:
            self.initialize()
        return self.pair, r, done


class VecALE:
    """N emulators -> device tensors for A3C.act.

        env = VecALE([make_ale(i) for i in range(N)], device="cuda")
        pairs, r, d = env.reset()                  # (N,2,210,160,3) u8, (N,) f32, (N,) u8
        a = agent.act(pairs, r, d)
        pairs, r, d = env.step(a)

    Each env draws its no-op counts from its own RandomState(seed + i) (the
    global RNG would make the counts depend on thread timing)."""

    def __init__(self, ales, device=None, seed: int = 0, workers: int = 8, **kw):
        self.n = len(ales)
        self.envs = [ALEFramePairs(a, nullop_rng=np.random.RandomState(seed + i), **kw) for i, a in enumerate(ales)]
        self.device = torch.device(device if device is not None else "cuda")
        pin = self.device.type == "cuda"
        self.h_pairs = torch.empty((self.n, 2) + SCREEN, dtype=torch.uint8, pin_memory=pin)
        self.h_rewards = torch.zeros(self.n, dtype=torch.float32, pin_memory=pin)
        self.h_dones = torch.zeros(self.n, dtype=torch.uint8, pin_memory=pin)
        self.d_pairs = torch.empty((self.n, 2) + SCREEN, dtype=torch.uint8, device=self.device)
        self.d_rewards = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.d_dones = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(workers, self.n)))
        self._copied = None        # event after the last host -> device copy
        self._chunks = [list(range(i, self.n, max(1, min(workers, self.n)))) for i in range(max(1, min(workers, self.n)))]

    @property
    def number_of_actions(self) -> int:
        return self.envs[0].number_of_actions

    def _upload(self, stream=None):
        with torch.cuda.stream(stream) if stream is not None and self.device.type == "cuda" else _null():
            self.d_pairs.copy_(self.h_pairs, non_blocking=True)
            self.d_rewards.copy_(self.h_rewards, non_blocking=True)
            self.d_dones.copy_(self.h_dones, non_blocking=True)
            if self.device.type == "cuda":
                self._copied = torch.cuda.Event()
                self._copied.record()
        return self.d_pairs, self.d_rewards, self.d_dones

    def _host_free(self):
        """The pinned buffers may be rewritten once the previous copy landed."""
        if self._copied is not None:
            self._copied.synchronize()

    def reset(self, stream=None):
        self._host_free()
        hp = self.h_pairs.numpy()
        for i, e in enumerate(self.envs):
            hp[i] = e.pair
        self.h_rewards.zero_()
        self.h_dones.zero_()
        return self._upload(stream)

    def step(self, actions, stream=None):
        acts = actions.cpu().numpy() if torch.is_tensor(actions) else np.asarray(actions)
        self._host_free()
        hp, hr, hd = self.h_pairs.numpy(), self.h_rewards.numpy(), self.h_dones.numpy()

        def run(idx):
            for i in idx:
                pair, r, d = self.envs[i].step(int(acts[i]))
                hp[i] = pair
                hr[i] = r
                hd[i] = d

        list(self.pool.map(run, self._chunks))
        return self._upload(stream)

    def close(self):
        self.pool.shutdown(wait=True)


class _DeviceEnv:
    """What the device envs share: the double-buffered state, the pools and
    the granular reset() / step().  A subclass gives `kind`, `STATE_INTS`,
    `_state_bytes` and the library's two calls, `_reset` and `_step`."""

    envs = ()        # no host emulators behind it (evaluation.run_episodes walks this)
    number_of_actions = 4

    def __init__(self, n_envs: int, device=None, seed: int = 0, env_offset: int = 0):
        if n_envs < 1:
            raise ValueError(f"{type(self).__name__}: n_envs must be >= 1")
        self.n, self.seed, self.env_offset = n_envs, seed, env_offset
        self.device = torch.device(device if device is not None else "cuda")
        self.state = torch.zeros(self._state_bytes(n_envs) // 4, dtype=torch.int32,
                                 device=self.device).view(2, n_envs, self.STATE_INTS)
        self.parity = 0          # the state half the granular calls read next
        self._out = None

    def make_pools(self, pool_len: int):
        """(pairs, rewards, dones) pools of pool_len >= 2 entries, zeroed."""
        if pool_len < 2:
            raise ValueError(f"{type(self).__name__}: pool_len must be >= 2")
        return (torch.zeros((pool_len, self.n, 2) + SCREEN, dtype=torch.uint8, device=self.device),
                torch.zeros((pool_len, self.n), dtype=torch.float32, device=self.device),
                torch.zeros((pool_len, self.n), dtype=torch.uint8, device=self.device))

    def _buffers(self):
        if self._out is None:
            self._out = (torch.empty((self.n, 2) + SCREEN, dtype=torch.uint8, device=self.device),
                         torch.empty(self.n, dtype=torch.float32, device=self.device),
                         torch.empty(self.n, dtype=torch.uint8, device=self.device))
        return self._out

    def reset(self, stream=None):
        """The first episode of every env -> (pairs, r = 0, d = 0)."""
        pairs, r, d = self._buffers()
        self.parity = 0
        self._reset(ptr(self.state), self.n, self.env_offset, self.seed, self.parity, ptr(pairs), ptr(r), ptr(d),
                    stream_handle(stream))
        return pairs, r, d

    def step(self, actions, stream=None):
        """One env-step of every env; actions: (n,) integers.  The returned
        tensors are rewritten by the next call."""
        a = torch.as_tensor(actions, device=self.device).to(torch.int32).contiguous()
        if a.shape != (self.n,):
            raise ValueError(f"{type(self).__name__}.step: need {self.n} actions")
        pairs, r, d = self._buffers()
        self._step(ptr(self.state), self.parity, ptr(a), self.n, self.env_offset, self.seed, ptr(pairs), ptr(r),
                   ptr(d), stream_handle(stream))
        self.parity ^= 1
        return pairs, r, d

    def step_screen(self, actions, resize_mode: int = 0, stream=None):
        """step() followed by phi's current_screen on the pair, as the one
        launch of the direct-to-ring path (arl_env_step_screen): -> (screens
        (n, 84, 84) uint8, r, d), bit-identical to the two calls; the frame
        pair is never written.  The tensors are rewritten by the next call."""
        a = torch.as_tensor(actions, device=self.device).to(torch.int32).contiguous()
        if a.shape != (self.n,):
            raise ValueError(f"{type(self).__name__}.step_screen: need {self.n} actions")
        if self._screen_out is None:
            self._screen_out = (torch.empty((self.n, 84, 84), dtype=torch.uint8, device=self.device),
                                torch.empty(self.n, dtype=torch.float32, device=self.device),
                                torch.empty(self.n, dtype=torch.uint8, device=self.device))
        screens, r, d = self._screen_out
        check(lib.arl_env_step_screen(self.kind, ptr(self.state), self.parity, ptr(a), self.n, self.env_offset,
                                      self.seed, resize_mode, ptr(screens), ptr(r), ptr(d), stream_handle(stream)),
              "arl_env_step_screen")
        self.parity ^= 1
        return screens, r, d

    _screen_out = None

    def close(self):
        pass


class DeviceCatch(_DeviceEnv):
    """Catch on the device (include/asyncrl_hip.h, "device environment"): the
    env of the closed actor-learner loop.  It owns the double-buffered env state
    (2, n, 8) int32; one kernel launch per env-step moves every env and renders
    its 210x160x3 frame pair.  Two ways to run it:

    * attached to a net -- net.set_env(env), net.env_reset(*pools, pool_len),
      then A3C.run_window(*pools, pool_len, first=True) and on: the window steps
      the env from the actions it sampled, with no host work per step
      (make_pools builds the pools; seed and env_offset must be the net's);
    * granular, VecALE's surface -- reset() / step(actions) -> (pairs, r, d)
      device tensors (n, 2, 210, 160, 3) uint8 / (n,) f32 / (n,) uint8, so
      A3C.act_batch and evaluation.run_episodes take it unchanged.

    Actions: 2 = right, 3 = left, anything else a no-op (n_actions >= 4).  Every
    episode lasts 14 env-steps and returns +1 (caught) or -1."""

    kind = ENV_CATCH   # what DeviceNet.set_env hands arl_net_set_env
    STATE_INTS = CATCH_STATE_INTS
    _state_bytes = staticmethod(lib.arl_catch_state_bytes)

    def _reset(self, *args):
        check(lib.arl_catch_reset(*args), "arl_catch_reset")

    def _step(self, *args):
        check(lib.arl_catch_step(*args), "arl_catch_step")


class DeviceBreakout(_DeviceEnv):
    """Breakout on the device (include/asyncrl_hip.h, "device environment"; the
    rules are there): DeviceCatch's surface over a game with 120 bricks that
    persist across lives, brick rewards of 1, 4 and 7 (raw, unclipped), five
    lives and episodes of different lengths.  The state is (2, n, 16) int32.

    life_loss_terminal=True (training, ale.py:98-99): done = life lost or game
    over.  False (evaluation, a3c_ale.py:75-76; what evaluation.run_episodes
    wants): done = game over only.  The two differ in nothing else."""

    STATE_INTS = BREAKOUT_STATE_INTS
    _state_bytes = staticmethod(lib.arl_breakout_state_bytes)

    def __init__(self, n_envs: int, device=None, seed: int = 0, env_offset: int = 0, life_loss_terminal: bool = True):
        super().__init__(n_envs, device, seed, env_offset)
        self.life_loss_terminal = bool(life_loss_terminal)
        self.flags = 0 if self.life_loss_terminal else ENV_GAME_OVER_ONLY
        self.kind = ENV_BREAKOUT | self.flags

    def _reset(self, *args):
        check(lib.arl_breakout_reset(*args), "arl_breakout_reset")

    def _step(self, state, parity, actions, n, env_offset, seed, *out):   # the flags go before the outputs
        check(lib.arl_breakout_step(state, parity, actions, n, env_offset, seed, self.flags, *out), "arl_breakout_step")


class DevicePong(_DeviceEnv):
    """Pong on the device (include/asyncrl_hip.h, "device environment"; the
    rules are there): DeviceCatch's surface over a game against a paddle that
    follows the ball, played to `points` (1..21).  Every point is a reward of
    +1 or -1 that does not end the episode; done = game over (a side reached
    `points`, or 5,000 env-steps).  Actions: 2 and 4 = up, 3 and 5 = down,
    anything else a no-op (n_actions >= 4; 6 is ALE Pong's minimal set).  The
    state is (2, n, 12) int32.  points=1 gives episodes of about 11 env-steps
    under a random policy, points=21 of about 230."""

    STATE_INTS = PONG_STATE_INTS
    _state_bytes = staticmethod(lib.arl_pong_state_bytes)

    def __init__(self, n_envs: int, device=None, seed: int = 0, env_offset: int = 0, points: int = 21):
        if not 1 <= points <= PONG_POINTS_MAX:
            raise ValueError(f"DevicePong: points must be in 1..{PONG_POINTS_MAX}")
        super().__init__(n_envs, device, seed, env_offset)
        self.points = int(points)
        self.kind = ENV_PONG | env_pong_points(self.points)

    def _reset(self, *args):
        check(lib.arl_pong_reset(*args), "arl_pong_reset")

    def _step(self, state, parity, actions, n, env_offset, seed, *out):   # the points go before the outputs
        check(lib.arl_pong_step(state, parity, actions, n, env_offset, seed, self.points, *out), "arl_pong_step")


class DeviceTMaze(_DeviceEnv):
    """A cue-recall T-maze on the device (include/asyncrl_hip.h, "device
    environment"; the rules are there): DeviceCatch's surface over a partially
    observed task.  An episode's first screen shows a cue ("up" or "down");
    the agent is then carried down a corridor of `length` (1..8) env-steps,
    its actions ignored, and at the junction has to name the cue: 2 = up, 3 =
    down, anything else no choice (n_actions >= 4).  Reward +1 for the cue's
    arm, -1 for the other, 0 for no choice; each ends the episode, so every
    episode lasts length + 1 env-steps and the optimum is +1.  From length 4
    on the cue has left the 4-observation stack at the junction: the FF
    model's expected return is exactly 0 whatever it learns, and the LSTM has
    to carry the cue in its state.  The default length 4 makes an episode one
    t_max = 5 window.  The state is (2, n, 8) int32."""

    STATE_INTS = TMAZE_STATE_INTS
    _state_bytes = staticmethod(lib.arl_tmaze_state_bytes)

    def __init__(self, n_envs: int, device=None, seed: int = 0, env_offset: int = 0, length: int = 4):
        if not 1 <= length <= TMAZE_LENGTH_MAX:
            raise ValueError(f"DeviceTMaze: length must be in 1..{TMAZE_LENGTH_MAX}")
        super().__init__(n_envs, device, seed, env_offset)
        self.length = int(length)
        self.kind = ENV_TMAZE | env_tmaze_length(self.length)

    def _reset(self, state, n, env_offset, seed, *rest):   # the length goes before the parity
        check(lib.arl_tmaze_reset(state, n, env_offset, seed, self.length, *rest), "arl_tmaze_reset")

    def _step(self, state, parity, actions, n, env_offset, seed, *out):   # the length goes before the outputs
        check(lib.arl_tmaze_step(state, parity, actions, n, env_offset, seed, self.length, *out), "arl_tmaze_step")


class DeviceMaze(_DeviceEnv):
    """A grid maze with procedurally generated levels on the device
    (include/asyncrl_hip.h, "device environment"; the rules are there):
    DeviceCatch's surface over a family of tasks.  The maze is (2 rooms + 1)^2
    tiles, a binary-tree maze over rooms x rooms rooms (rooms in 2..4); its
    carving, the start room and the goal room are a function of (seed,
    level).  Every episode draws a level: from 0..levels-1 with levels in
    1..1023, from all 2^32 with levels = 0 -- train on `levels` tasks, score
    on all of them, and the difference is a generalisation gap.  Actions
    a & 3: 0 up, 1 down, 2 right, 3 left (n_actions >= 4); a move into a wall
    is a bump.  Reward 1 on reaching the goal, which ends the episode; an
    episode also ends, with reward 0, after 8 rooms env-steps.  Every level
    can be solved in 8 rooms - 10, so the optimum is 1.  With view = V in
    1..2 only the tiles within V of the agent are drawn, the goal's included:
    an exploration task under partial observability.  The state is (2, n, 8)
    int32; `wins` and `timeouts` are columns 4 and 5."""

    STATE_INTS = MAZE_STATE_INTS
    _state_bytes = staticmethod(lib.arl_maze_state_bytes)

    def __init__(self, n_envs: int, device=None, seed: int = 0, env_offset: int = 0, rooms: int = 3, view: int = 0,
                 levels: int = 0):
        if not MAZE_ROOMS_MIN <= rooms <= MAZE_ROOMS_MAX:
            raise ValueError(f"DeviceMaze: rooms must be in {MAZE_ROOMS_MIN}..{MAZE_ROOMS_MAX}")
        if not 0 <= view <= MAZE_VIEW_MAX:
            raise ValueError(f"DeviceMaze: view must be in 0..{MAZE_VIEW_MAX}")
        if not 0 <= levels <= MAZE_LEVELS_MAX:
            raise ValueError(f"DeviceMaze: levels must be in 0..{MAZE_LEVELS_MAX}")
        super().__init__(n_envs, device, seed, env_offset)
        self.rooms, self.view, self.levels = int(rooms), int(view), int(levels)
        self.kind = ENV_MAZE | env_maze_fields(self.rooms, self.view, self.levels)

    def _reset(self, state, n, env_offset, seed, *rest):   # the fields go before the parity
        check(lib.arl_maze_reset(state, n, env_offset, seed, self.rooms, self.view, self.levels, *rest),
              "arl_maze_reset")

    def _step(self, state, parity, actions, n, env_offset, seed, *out):   # the fields go before the outputs
        check(lib.arl_maze_step(state, parity, actions, n, env_offset, seed, self.rooms, self.view, self.levels, *out),
              "arl_maze_step")


class _null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False
