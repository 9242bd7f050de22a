"""Test-side NumPy restatement of the device-resident Catch (include/asyncrl_hip.h, "device
environment"): integer state, the render, and the episode starts through the oracle's Philox.
Nothing here imports the package under test.  The dynamics are exact in integer arithmetic, so
the kernel has to agree bit for bit."""
import numpy as np

from oracle import philox4x32

H, W = 210, 160
PADDLE_W, PADDLE_H, PADDLE_Y, PADDLE_RGB = 16, 4, 190, (200, 72, 72)
BALL, BALL_RGB = 8, (236, 236, 236)
BY0, PX0 = 18, 72
EPISODE_STEPS = 14
# mean return of a uniform random policy over 4 actions, 20,000 episodes (test_catch.py
# test_random_policy_mean_is_the_recorded_constant recomputes it): what "has not learned" scores
RANDOM_MEAN = -0.7014
OPTIMUM = 1.0
LEARNED = 0.15      # the learning test's pass mark: the midpoint of RANDOM_MEAN and OPTIMUM, rounded up


def render(bx, by, px):
    """One screen (210, 160, 3) uint8."""
    s = np.zeros((H, W, 3), np.uint8)
    s[PADDLE_Y:PADDLE_Y + PADDLE_H, px:px + PADDLE_W] = PADDLE_RGB
    lo, hi = max(by, 0), min(by + BALL, H)
    if hi > lo:
        s[lo:hi, bx:bx + BALL] = BALL_RGB          # the ball covers the paddle
    return s


class CatchRef:
    """n envs; state (n, 8) int32 [bx, by, vx, px, episode, steps_in_episode, 0, 0]."""

    def __init__(self, n, seed=0, env_offset=0):
        self.n, self.seed, self.env_offset = n, seed, env_offset
        self.state = np.zeros((n, 8), np.int32)
        self.bounced = np.zeros((n, 2), bool)      # env e ever reflected off the left / right wall
        self.catches = 0

    def _start(self, envs, episodes):
        """Episode `episodes[i]` of env `envs[i]` begins: the state rows of an episode start."""
        m = len(envs)
        ctr = (np.asarray(envs, np.uint64) + np.uint64(self.env_offset), np.asarray(episodes, np.uint64),
               np.zeros(m, np.uint64), np.full(m, 2, np.uint64))
        w0, w1, _, _ = philox4x32(ctr, (self.seed & 0xffffffff, self.seed >> 32))
        rows = np.zeros((m, 8), np.int32)
        rows[:, 0] = (w0 % np.uint64(153)).astype(np.int32)
        rows[:, 1] = BY0
        rows[:, 2] = (w1 % np.uint64(5)).astype(np.int32) - 2
        rows[:, 3] = PX0
        rows[:, 4] = episodes
        self.state[envs] = rows

    def _pairs(self, cur, prev):
        """(n, 2, 210, 160, 3): screen `cur` then screen `prev` of every env ((n, 3) bx, by, px each)."""
        return np.stack([np.stack([render(*(int(x) for x in cur[e])), render(*(int(x) for x in prev[e]))])
                         for e in range(self.n)])

    def reset(self):
        """-> pairs (n, 2, 210, 160, 3) uint8, rewards (n,) f32 = 0, dones (n,) uint8 = 0."""
        self._start(np.arange(self.n), np.zeros(self.n, np.int64))
        first = self.state[:, [0, 1, 3]]
        return self._pairs(first, first), np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)

    def step(self, actions, render_pairs=True):
        a = np.asarray(actions).astype(np.int64)
        bx, by, vx, px, episode, steps = (self.state[:, i].astype(np.int64) for i in range(6))
        live = np.ones(self.n, bool)                       # the skip loop has not broken yet
        rewards = np.zeros(self.n, np.float32)
        cur = np.stack([bx, by, px], 1)
        prev = cur.copy()
        for _ in range(4):
            prev = np.where(live[:, None], cur, prev)
            px = np.where(live & (a == 2), np.minimum(px + 3, 144), np.where(live & (a == 3), np.maximum(px - 3, 0), px))
            nb = bx + vx
            lo, hi = live & (nb < 0), live & (nb > 152)
            self.bounced[:, 0] |= lo
            self.bounced[:, 1] |= hi
            bx = np.where(live, np.where(lo, -nb, np.where(hi, 304 - nb, nb)), bx)
            vx = np.where(lo | hi, -vx, vx)
            by = np.where(live, by + 3, by)
            end = live & (by + 8 >= 190)                    # the episode ends in this frame
            caught = (bx + 8 > px) & (bx < px + 16)
            rewards[end] = np.where(caught[end], 1.0, -1.0)
            self.catches += int((end & caught).sum())
            live &= ~end
            cur = np.where(live[:, None], np.stack([bx, by, px], 1), cur)
        dones = (~live).astype(np.uint8)
        self.state[:, 0], self.state[:, 1], self.state[:, 2], self.state[:, 3] = bx, by, vx, px
        self.state[:, 5] = steps + 1
        if (~live).any():                                   # the next episode starts at once
            ended = np.flatnonzero(~live)
            self._start(ended, episode[ended] + 1)
            first = self.state[ended][:, [0, 1, 3]]
            cur[ended] = first
            prev[ended] = first
        return (self._pairs(cur, prev) if render_pairs else None), rewards, dones


def tracking_action(state):
    """The policy that tracks the ball: (n,) actions from (n, 8) states -- of no-op, right and left
    the one whose paddle centre after this env-step is nearest the ball's centre after it (the
    first of equals).  The paddle moves 12 a step and the ball at most 8, so once under the ball it
    stays within 6 (+ 5 in the 3-frame terminal step) of it: inside the 12 a catch needs."""
    bx, vx, px = (state[:, i].astype(np.int64) for i in (0, 2, 3))
    for _ in range(4):
        bx = bx + vx
        lo, hi = bx < 0, bx > 152
        bx = np.where(lo, -bx, np.where(hi, 304 - bx, bx))
        vx = np.where(lo | hi, -vx, vx)
    target = bx + BALL // 2
    best, best_err = np.zeros(len(bx), np.int32), None
    for a, dx in ((0, 0), (2, 12), (3, -12)):
        err = np.abs(target - (np.clip(px + dx, 0, 144) + PADDLE_W // 2))
        if best_err is None:
            best_err = err
        else:
            better = err < best_err
            best, best_err = np.where(better, a, best).astype(np.int32), np.where(better, err, best_err)
    return best
