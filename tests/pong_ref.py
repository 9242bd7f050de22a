"""Test-side NumPy restatement of the device-resident Pong (include/asyncrl_hip.h, "device
environment"): the integer state, the full-frame painter, the serves through the oracle's Philox,
a paddle-follows-the-ball policy, and counters of every event class so that a test can prove its
script reached what it claims.  Nothing here imports the package under test.  The dynamics are
exact in integer arithmetic, so the kernel has to agree bit for bit.

The step is a scalar Python loop per env on purpose: it is the header's text line by line."""
import numpy as np

from oracle import philox4x32

H, W = 210, 160
BG_RGB, WALL_RGB, OPP_RGB, AGENT_RGB, BALL_RGB = (144, 72, 17), (236, 236, 236), (213, 130, 74), (92, 186, 92), \
    (236, 236, 236)
WALL_ROWS = ((24, 34), (194, 204))
OPP_X, AGENT_X, PADDLE_W, PADDLE_H, Y_MIN, PADDLE_MAX, BALL_Y_MAX = 16, 140, 4, 16, 34, 178, 190
BALL, SERVE_X, PADDLE_Y0, STEP_CAP = 4, 78, 106, 5000
STATE_INTS = 12
BX, BY, VX, VY, PY, OY, SERVES, STEPS, GAME, GAME_STEPS, SCORE_AGENT, SCORE_OPP = range(12)
UP, DOWN = (2, 4), (3, 5)
# mean return of a uniform random policy over 4 actions (what the FF learner of scripts/train_catch.py has) at
# points = 1, the first 16 games of each of 250 envs, and its standard error (test_pong.py
# test_random_policy_return_is_the_recorded_constant recomputes both): what "has not learned" scores, and what
# DESIGN.md "Device environment" holds the measured lr0 = 0 curve against.  Over all 6 actions the same count
# gives -0.3565.
RANDOM_MEAN_POINTS1, RANDOM_SE_POINTS1 = -0.3575, 0.0148


def make_state(bx, by, vx, vy, py=PADDLE_Y0, oy=PADDLE_Y0, serves=1, steps=0, game=0, game_steps=0, score_agent=0,
               score_opp=0):
    """A crafted state row (12,) int32."""
    return np.array([bx, by, vx, vy, py, oy, serves, steps, game, game_steps, score_agent, score_opp], np.int32)


def render(bx, by, py, oy):
    """One screen (210, 160, 3) uint8: the ball over a paddle, a paddle over the background."""
    s = np.empty((H, W, 3), np.uint8)
    s[:] = BG_RGB
    for y0, y1 in WALL_ROWS:
        s[y0:y1] = WALL_RGB
    s[oy:oy + PADDLE_H, OPP_X:OPP_X + PADDLE_W] = OPP_RGB
    s[py:py + PADDLE_H, AGENT_X:AGENT_X + PADDLE_W] = AGENT_RGB
    s[by:by + BALL, max(bx, 0):max(bx + BALL, 0)] = BALL_RGB
    return s


def hit_vy(by, y):
    return 2 * (min(max(by + 2 - y, 0), 15) >> 2) - 3


class PongRef:
    """n envs; state (n, 12) int32 [bx, by, vx, vy, py, oy, serves, steps_in_episode, game,
    game_steps, score_agent, score_opp]."""

    def __init__(self, n, seed=0, env_offset=0, points=21):
        assert 1 <= points <= 21
        self.n, self.seed, self.env_offset, self.points = n, seed, env_offset, points
        self.state = np.zeros((n, STATE_INTS), np.int32)
        # event counters, summed over envs
        self.wall = [0, 0]                       # bounces off the top / bottom wall
        self.agent_hits, self.opp_hits = [0] * 4, [0] * 4     # by hit bin
        self.agent_points, self.opp_points = [0] * 4, [0] * 4  # by the frame of the skip the point fell in
        self.game_overs = {"agent": 0, "opp": 0, "cap": 0}
        self.draws = []                          # (env id, serves) of every Philox draw

    def _serve(self, e, s, toward):
        self.draws.append((e + self.env_offset, s[SERVES]))
        w0, w1, w2, _ = philox4x32((np.array([e + self.env_offset], np.uint64), np.array([s[SERVES]], np.uint64),
                                    np.zeros(1, np.uint64), np.full(1, 4, np.uint64)),
                                   (self.seed & 0xffffffff, self.seed >> 32))
        s[BX], s[BY], s[VY] = SERVE_X, Y_MIN + int(w0[0]) % 157, 2 * (int(w1[0]) % 4) - 3
        s[VX] = toward if toward else (3 if int(w2[0]) & 1 else -3)
        s[SERVES] += 1

    def _new_game(self, e, s):
        s[PY] = s[OY] = PADDLE_Y0
        s[SCORE_AGENT] = s[SCORE_OPP] = s[GAME_STEPS] = 0
        self._serve(e, s, 0)

    def reset(self):
        """-> pairs (n, 2, 210, 160, 3) uint8, rewards (n,) f32 = 0, dones (n,) uint8 = 0."""
        pairs = np.zeros((self.n, 2, H, W, 3), np.uint8)
        for e in range(self.n):
            s = [0] * STATE_INTS
            self._new_game(e, s)
            self.state[e] = s
            pairs[e, 0] = pairs[e, 1] = render(s[BX], s[BY], s[PY], s[OY])
        return pairs, np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)

    def step_env(self, e, act):
        """One env-step of env e -> (cur screen args, prev screen args, reward, done)."""
        s = [int(x) for x in self.state[e]]
        cur = prev = (s[BX], s[BY], s[PY], s[OY])
        reward = 0
        for f in range(4):
            prev = cur
            if act in UP:
                s[PY] = max(s[PY] - 4, Y_MIN)
            elif act in DOWN:
                s[PY] = min(s[PY] + 4, PADDLE_MAX)
            c = s[BY] + 2 - (s[OY] + 8)
            if c > 2:
                s[OY] = min(s[OY] + 2, PADDLE_MAX)
            elif c < -2:
                s[OY] = max(s[OY] - 2, Y_MIN)
            s[BY] += s[VY]
            if s[BY] < Y_MIN:
                s[BY], s[VY] = 68 - s[BY], -s[VY]
                self.wall[0] += 1
            elif s[BY] > BALL_Y_MAX:
                s[BY], s[VY] = 380 - s[BY], -s[VY]
                self.wall[1] += 1
            s[BX] += s[VX]
            if s[VX] > 0 and 136 <= s[BX] < 139:
                if s[BY] + 4 > s[PY] and s[BY] < s[PY] + 16:
                    s[BX], s[VX], s[VY] = 272 - s[BX], -3, hit_vy(s[BY], s[PY])
                    self.agent_hits[(s[VY] + 3) // 2] += 1
            elif s[VX] < 0 and 16 < s[BX] <= 19:
                if s[BY] + 4 > s[OY] and s[BY] < s[OY] + 16:
                    s[BX], s[VX], s[VY] = 40 - s[BX], 3, hit_vy(s[BY], s[OY])
                    self.opp_hits[(s[VY] + 3) // 2] += 1
            if s[BX] < 0:
                reward = 1
                self.agent_points[f] += 1
            elif s[BX] > 156:
                reward = -1
                self.opp_points[f] += 1
            if reward:
                break
            cur = (s[BX], s[BY], s[PY], s[OY])
        s[GAME_STEPS] += 1
        s[STEPS] += 1
        s[SCORE_AGENT] += reward > 0
        s[SCORE_OPP] += reward < 0
        done = s[SCORE_AGENT] >= self.points or s[SCORE_OPP] >= self.points or s[GAME_STEPS] >= STEP_CAP
        if done:
            self.game_overs["agent" if s[SCORE_AGENT] >= self.points else
                            "opp" if s[SCORE_OPP] >= self.points else "cap"] += 1
            s[GAME] += 1
            s[STEPS] = 0
            self._new_game(e, s)
            cur = prev = (s[BX], s[BY], s[PY], s[OY])
        elif reward:
            self._serve(e, s, -3 if reward > 0 else 3)
            cur = prev = (s[BX], s[BY], s[PY], s[OY])
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


def follow_action(state):
    """The paddle follows the ball: (n,) actions from (n, 12) states -- up (2) if the ball's centre is
    above the paddle's, down (3) if below, else a no-op."""
    c = state[:, BY].astype(np.int64) + 2 - (state[:, PY].astype(np.int64) + 8)
    return np.where(c < -3, 2, np.where(c > 3, 3, 0)).astype(np.int32)


def crafted_states():
    """name -> (state row, action or "follow").  The agent's face is crossed when bx goes from 133..135
    to 136..138, the opponent's when it goes from 20..22 to 17..19."""
    st = {
        "top_wall": (make_state(80, 35, 3, -3), 0),                  # by 35 -> 32 -> 36, vy -> +3
        "bottom_wall": (make_state(80, 189, -3, 3), 0),              # by 189 -> 192 -> 188
        "agent_clamp_top": (make_state(80, 100, 3, 1, py=36), 2),    # 36 -> 34 in frame 0
        "agent_clamp_bottom": (make_state(80, 100, 3, 1, py=176), 3),
        "opp_clamp_top": (make_state(80, 34, 3, -1, oy=35), 0),
        "opp_clamp_bottom": (make_state(80, 190, 3, 1, oy=177), 0),
        # the dead zone: c = by + 2 - (oy + 8) in frame 0, the ball then moving toward the paddle's centre
        "dead_zone_p2": (make_state(80, 110, 3, -1, oy=102), 0),     # c = 2, 1, 0, -1: oy stays
        "dead_zone_m2": (make_state(80, 106, 3, 1, oy=102), 0),      # c = -2, -1, 0, 1
        "dead_zone_p3": (make_state(80, 111, 3, -1, oy=102), 0),     # c = 3: oy += 2, then c = 0, -1, -2
        "dead_zone_m3": (make_state(80, 105, 3, 1, oy=102), 0),
        "step_cap": (make_state(80, 100, 3, 1, game_steps=STEP_CAP - 2, steps=STEP_CAP - 2), "follow"),
        "alias_up": (make_state(80, 100, 3, 1, py=100), 4),
        "alias_down": (make_state(80, 100, 3, 1, py=100), 5),
        "noop_1": (make_state(80, 100, 3, 1, py=100), 1),
        "noop_6": (make_state(80, 100, 3, 1, py=100), 6),
    }
    # The face of a paddle whose top edge is 100 in the crossing frame (frame 0), the ball then at by = 100 + off
    # (vy = 1 before it).  The agent's paddle stands (a no-op); the opponent's makes its move of the frame first,
    # 2 toward the ball, so it starts 2 further away.
    def agent(off):
        return make_state(133, 99 + off, 3, 1, py=100, oy=40)

    def opp(off):
        return make_state(22, 99 + off, -3, 1, py=40, oy=102 if off < 6 else 98)
    # the four hit bins: by + 2 - y = -1 (clamped to 0), 5, 10, 17 (clamped to 15)
    for k, off in enumerate((-3, 3, 8, 15)):
        st["agent_bin%d" % k] = (agent(off), 0)
        st["opp_bin%d" % k] = (opp(off), 0)
    # a miss one row outside each edge of a paddle: by + 4 == y and by == y + 16 (bins 0 and 3 are the last rows
    # that touch)
    for name, off in (("above", -4), ("below", 16)):
        st["agent_miss_%s" % name] = (agent(off), 0)
        st["opp_miss_%s" % name] = (opp(off), 0)
    # a point in frame f of the skip, for each side: the ball f + 1 frames from the edge, the paddles away
    for f in range(4):
        st["agent_point_f%d" % f] = (make_state(3 * f + 2, 60, -3, 1, oy=150, score_agent=1, score_opp=2), 0)
        st["opp_point_f%d" % f] = (make_state(155 - 3 * f, 60, 3, 1, py=150, score_agent=2, score_opp=1), 0)
    return st


def script_actions(state, policies, rng):
    """(n,) int32 actions of one step: policies[e] is an action, "follow" or "random" (0..5)."""
    follow = follow_action(state)
    return np.array([follow[e] if p == "follow" else rng.integers(0, 6) if p == "random" else p
                     for e, p in enumerate(policies)], np.int32)


def script_policies(n):
    """The granular test's script: env 0 always up, env 1 always down, 4 following envs, the rest random
    in 0..5.  -> policies."""
    return [2 if e == 0 else 3 if e == 1 else "follow" if e < 6 else "random" for e in range(n)]


def returns_of(rewards, dones, per):
    """The returns of the first `per` games of every env from (steps, n) rewards and dones, env-major."""
    n = rewards.shape[1]
    out = []
    for e in range(n):
        ends = np.flatnonzero(dones[:, e])[:per]
        assert len(ends) == per
        cs = np.concatenate(([0.0], np.cumsum(rewards[:, e].astype(np.float64))))
        starts = np.concatenate(([0], ends[:-1] + 1))
        out.append(cs[ends + 1] - cs[starts])
    return np.concatenate(out)
