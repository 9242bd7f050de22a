"""Test-side NumPy restatement of the device-resident T-maze (include/asyncrl_hip.h, "device
environment"): the integer state, the full-frame painter, the cue through the oracle's Philox, and
counters of every event class so that a test can prove its script reached what it claims.  Nothing
here imports the package under test.  The game is exact in integer arithmetic, so the kernel has to
agree bit for bit.

The step is a scalar Python loop per env on purpose: it is the header's text line by line."""
import numpy as np

from oracle import philox4x32

H, W = 210, 160
FLOOR_RGB, AGENT_RGB, CUE_RGB = (84, 84, 84), (92, 186, 92), ((200, 72, 72), (66, 72, 200))
FLOOR_ROWS, ARM_ROWS, AGENT_ROWS, CUE_ROWS = (96, 112), (48, 160), (100, 108), ((72, 88), (120, 136))
CELL, AGENT, AGENT_X0, CUE = 16, 8, 4, 16
LENGTH_MAX, LENGTH_DEFAULT = 8, 4
UP, DOWN = 2, 3
STATE_INTS = 8
POS, CUE_BIT, LENGTH, STEPS, EPISODE, HITS, MISSES, LAPSES = range(8)


def render(ax, length, cue=None):
    """One screen (210, 160, 3) uint8: the agent over the floor over the background; cue None (not
    drawn), 0 ("up") or 1 ("down")."""
    s = np.zeros((H, W, 3), np.uint8)
    s[FLOOR_ROWS[0]:FLOOR_ROWS[1], 0:CELL * length + CELL] = FLOOR_RGB
    s[ARM_ROWS[0]:ARM_ROWS[1], CELL * length:CELL * length + CELL] = FLOOR_RGB
    if cue is not None:
        s[CUE_ROWS[cue][0]:CUE_ROWS[cue][1], 0:CUE] = CUE_RGB[cue]
    s[AGENT_ROWS[0]:AGENT_ROWS[1], ax:ax + AGENT] = AGENT_RGB
    return s


def cue_of(seed, env_id, episode):
    """w0 & 1 of philox4x32_10(counter = (env_id, episode, 0, 5), key = (seed lo, seed hi))."""
    w = philox4x32((np.array([env_id], np.uint64), np.array([episode], np.uint64), np.zeros(1, np.uint64),
                    np.full(1, 5, np.uint64)), (seed & 0xffffffff, seed >> 32))
    return int(w[0][0]) & 1


class TMazeRef:
    """n envs; state (n, 8) int32 [pos, cue, length, steps_in_episode, episode, hits, misses, lapses]."""

    def __init__(self, n, seed=0, env_offset=0, length=LENGTH_DEFAULT):
        assert 1 <= length <= LENGTH_MAX
        self.n, self.seed, self.env_offset, self.length = n, seed, env_offset, length
        self.state = np.zeros((n, STATE_INTS), np.int32)
        # event counters, summed over envs
        self.corridor_steps = 0
        self.junctions = {"hit": 0, "miss": 0, "lapse": 0}
        self.choices = {}                        # (cue, action) at a junction -> count
        self.draws = []                          # (env id, episode) of every Philox draw

    def _start(self, e, s):
        self.draws.append((e + self.env_offset, s[EPISODE]))
        s[POS] = s[STEPS] = 0
        s[CUE_BIT] = cue_of(self.seed, e + self.env_offset, s[EPISODE])

    @staticmethod
    def _screen(s):
        """The screen between env-steps, as render's arguments: the cue on an episode's first screen alone."""
        return (AGENT_X0 + CELL * s[POS], s[LENGTH], s[CUE_BIT] if s[POS] == 0 else None)

    def reset(self):
        """-> pairs (n, 2, 210, 160, 3) uint8, rewards (n,) f32 = 0, dones (n,) uint8 = 0."""
        pairs = np.zeros((self.n, 2, H, W, 3), np.uint8)
        for e in range(self.n):
            s = [0] * STATE_INTS
            s[LENGTH] = self.length
            self._start(e, s)
            self.state[e] = s
            pairs[e, 0] = pairs[e, 1] = render(*self._screen(s))
        return pairs, np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)

    def step_env(self, e, act):
        """One env-step of env e -> (cur screen args, prev screen args, reward, done)."""
        s = [int(x) for x in self.state[e]]
        s[LENGTH] = self.length
        if s[POS] < s[LENGTH]:                   # the corridor: four frames of 4 px, the action ignored
            s[POS] += 1
            s[STEPS] += 1
            self.corridor_steps += 1
            cur = (AGENT_X0 + CELL * s[POS], s[LENGTH], None)
            prev = (cur[0] - 4, s[LENGTH], None)
            reward, done = 0, 0
        else:                                    # the junction
            choice = 0 if act == UP else 1 if act == DOWN else None
            reward = 0 if choice is None else 1 if choice == s[CUE_BIT] else -1
            done = 1
            self.junctions["lapse" if choice is None else "hit" if reward > 0 else "miss"] += 1
            self.choices[(s[CUE_BIT], act)] = self.choices.get((s[CUE_BIT], act), 0) + 1
            s[HITS] += reward > 0
            s[MISSES] += reward < 0
            s[LAPSES] += choice is None
            s[EPISODE] += 1
            self._start(e, s)
            cur = prev = self._screen(s)
        self.state[e] = s
        return cur, prev, reward, done

    def step(self, actions, render_pairs=True):
        a = np.asarray(actions).astype(np.int64)
        rewards, dones = np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)
        pairs = np.zeros((self.n, 2, H, W, 3), np.uint8) if render_pairs else None
        for e in range(self.n):
            cur, prev, r, d = self.step_env(e, int(a[e]))
            rewards[e], dones[e] = r, d
            if render_pairs:
                pairs[e, 0] = render(*cur)
                pairs[e, 1] = pairs[e, 0] if prev == cur else render(*prev)
        return pairs, rewards, dones


def cycle_actions(n, t):
    """(n,) int32: the actions 0..5 in turn, offset by the env, so that over six junctions every env
    takes every action value."""
    return ((np.arange(n) + t) % 6).astype(np.int32)


def episode_pairs(length, cue, action=UP):
    """The L + 1 pairs (2, 210, 160, 3) an episode with the given cue shows, observation 0 (the cue's screen)
    to observation L (the junction's), from a one-env restatement whose draw is overridden."""
    ref = TMazeRef(1, length=length)
    ref.reset()
    ref.state[0, CUE_BIT] = cue
    out = [np.stack([render(*ref._screen([int(x) for x in ref.state[0]]))] * 2)]
    for _ in range(length):
        pairs, r, d = ref.step([action])
        assert r[0] == 0 and d[0] == 0
        out.append(pairs[0])
    assert ref.state[0, POS] == length
    return out
