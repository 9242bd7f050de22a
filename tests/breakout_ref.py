"""Test-side NumPy restatement of the device-resident Breakout (include/asyncrl_hip.h, "device
environment"): the integer state, the render, both done modes, the serves through the oracle's
Philox, a tracking policy, and counters of every event class so that a test can prove its script
reached what it claims.  Nothing here imports the package under test.  The dynamics are exact in
integer arithmetic, so the kernel has to agree bit for bit.

The step is a scalar Python loop per env on purpose: it is the header's text line by line."""
import numpy as np

from oracle import philox4x32

H, W = 210, 160
ROWS, COLS, BRICK_W, BRICK_H, BRICK_Y0 = 6, 20, 8, 6, 57
ROW_RGB = ((200, 72, 72), (198, 108, 58), (180, 122, 48), (162, 162, 42), (72, 160, 72), (66, 72, 200))
ROW_VALUE = (7, 7, 4, 4, 1, 1)
PADDLE_W, PADDLE_H, PADDLE_Y, PADDLE_RGB = 16, 4, 190, (200, 72, 72)
BALL, BALL_RGB = 4, (236, 236, 236)
VX = (-2, -1, 1, 2)
LIVES, PX0, SERVE_Y, STEP_CAP = 5, 72, 100, 1000
ALL_BRICKS = (1 << (ROWS * COLS)) - 1
STATE_INTS = 16
BX, BY, VXI, VY, PX, LIVES_I, SERVES, STEPS, GAME, GAME_STEPS, SCORE, LEFT, B0 = range(13)
# mean raw return per life of a uniform random policy over 4 actions, the first 20 lives of each of
# 250 envs (test_breakout.py test_random_policy_mean_is_the_recorded_constant recomputes it): what
# "has not learned" scores
RANDOM_MEAN_PER_LIFE = 0.1442
# The learning test's constants, measured on the MI355X (DESIGN.md "Device environment", Breakout): the
# untrained net with lr0 = 0 scores 0.1480 per life (1,011,974 lives); of seeds 0, 1 and 2 the lowest mean
# over the last tenth of 17,802 windows is 182.4; the pass mark is the midpoint of the two; the three seeds
# first crossed it after 8,901, 6,501 and 6,701 windows, and the test runs twice the largest of those.
LR0_MEAN_PER_LIFE = 0.1480
LEARNED = 91.3
LEARN_WINDOWS = 17802


def brick_bit(r, c):
    return 1 << (COLS * r + c)


def words_of(bricks):
    """The four uint32 words of a 120-bit brick set, as int32 state values."""
    return [int(np.array((bricks >> (32 * w)) & 0xffffffff, np.uint32).astype(np.int32)) for w in range(4)]


def bricks_of(row):
    """The 120-bit brick set of a state row."""
    return sum((int(row[B0 + w]) & 0xffffffff) << (32 * w) for w in range(4))


def make_state(bx, by, vx, vy, px=PX0, lives=LIVES, serves=1, steps=0, game=0, game_steps=0, score=0,
               bricks=ALL_BRICKS):
    """A crafted state row (16,) int32; bricks_left is the population count of `bricks`."""
    return np.array([bx, by, vx, vy, px, lives, serves, steps, game, game_steps, score, bin(bricks).count("1")]
                    + words_of(bricks), np.int32)


def render(bx, by, px, bricks):
    """One screen (210, 160, 3) uint8."""
    s = np.zeros((H, W, 3), np.uint8)
    present = np.array([[(bricks >> (COLS * r + c)) & 1 for c in range(COLS)] for r in range(ROWS)], np.uint8)
    mask = np.repeat(np.repeat(present, BRICK_H, 0), BRICK_W, 1)                     # (36, 160): brick (r, c)'s pixels
    colours = np.repeat(np.array(ROW_RGB, np.uint8), BRICK_H, 0)                     # (36, 3): the row's colour
    s[BRICK_Y0:BRICK_Y0 + ROWS * BRICK_H] = mask[:, :, None] * colours[:, None]
    s[PADDLE_Y:PADDLE_Y + PADDLE_H, px:px + PADDLE_W] = PADDLE_RGB
    s[by:by + BALL, bx:bx + BALL] = BALL_RGB          # a ball pixel covers anything under it
    return s


class BreakoutRef:
    """n envs; state (n, 16) int32 [bx, by, vx, vy, px, lives, serves, steps_in_episode, game,
    game_steps, score, bricks_left, b0, b1, b2, b3]."""

    def __init__(self, n, seed=0, env_offset=0, life_loss_terminal=True):
        self.n, self.seed, self.env_offset, self.life_loss_terminal = n, seed, env_offset, life_loss_terminal
        self.state = np.zeros((n, STATE_INTS), np.int32)
        # event counters, summed over envs
        self.wall = [0, 0]                 # bounces off the left / right wall
        self.ceiling = 0
        self.row_hits = [0] * ROWS
        self.paddle_hits = [0] * 4         # by segment
        self.life_losses = 0
        self.game_overs = {"lives": 0, "cleared": 0, "cap": 0}
        self.max_reward = 0

    def _serve(self, e, s):
        w0, w1, _, _ = philox4x32((np.array([e + self.env_offset], np.uint64), np.array([s[SERVES]], np.uint64),
                                   np.zeros(1, np.uint64), np.full(1, 3, np.uint64)),
                                  (self.seed & 0xffffffff, self.seed >> 32))
        s[BX], s[VXI] = int(w0[0]) % 157, VX[int(w1[0]) % 4]
        s[BY], s[VY] = SERVE_Y, 4
        s[SERVES] += 1

    def _new_game(self, e, s):
        s[LIVES_I], s[PX], s[GAME_STEPS], s[SCORE], s[LEFT] = LIVES, PX0, 0, 0, ROWS * COLS
        self._serve(e, s)
        return ALL_BRICKS

    def _store(self, e, s, bricks):
        self.state[e, :B0] = s[:B0]
        self.state[e, B0:] = words_of(bricks)

    def reset(self):
        """-> pairs (n, 2, 210, 160, 3) uint8, rewards (n,) f32 = 0, dones (n,) uint8 = 0."""
        pairs = np.zeros((self.n, 2, H, W, 3), np.uint8)
        for e in range(self.n):
            s = [0] * B0
            bricks = self._new_game(e, s)
            self._store(e, s, bricks)
            pairs[e, 0] = pairs[e, 1] = render(s[BX], s[BY], s[PX], bricks)
        return pairs, np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)

    def step_env(self, e, act):
        """One env-step of env e -> (cur screen args, prev screen args, reward, life lost, game over, done)."""
        s = [int(x) for x in self.state[e, :B0]]
        bricks = bricks_of(self.state[e])
        cur = prev = (s[BX], s[BY], s[PX], bricks)
        reward, lost = 0, False
        for _ in range(4):
            prev = cur
            if act == 2:
                s[PX] = min(s[PX] + 3, 144)
            elif act == 3:
                s[PX] = max(s[PX] - 3, 0)
            s[BX] += s[VXI]
            if s[BX] < 0:
                s[BX], s[VXI] = -s[BX], -s[VXI]
                self.wall[0] += 1
            elif s[BX] > 156:
                s[BX], s[VXI] = 312 - s[BX], -s[VXI]
                self.wall[1] += 1
            s[BY] += s[VY]
            if s[BY] < 32:
                s[BY], s[VY] = 64 - s[BY], -s[VY]
                self.ceiling += 1
            cx, cy = s[BX] + 2, s[BY] if s[VY] < 0 else s[BY] + 3
            if 57 <= cy < 93:
                r, c = (cy - 57) // 6, cx >> 3
                if bricks & brick_bit(r, c):
                    bricks &= ~brick_bit(r, c)
                    reward += ROW_VALUE[r]
                    s[VY] = -s[VY]
                    s[LEFT] -= 1
                    self.row_hits[r] += 1
            if s[VY] > 0 and s[BY] + 4 >= 190:
                if s[BX] + 4 > s[PX] and s[BX] < s[PX] + 16:
                    seg = min(max(s[BX] + 2 - s[PX], 0), 15) >> 2
                    s[BY], s[VY], s[VXI] = 372 - s[BY], -s[VY], VX[seg]
                    self.paddle_hits[seg] += 1
                else:
                    s[LIVES_I] -= 1
                    lost = True
                    self.life_losses += 1
            if lost or s[LEFT] == 0:
                break
            cur = (s[BX], s[BY], s[PX], bricks)
        s[GAME_STEPS] += 1
        s[SCORE] += reward
        s[STEPS] += 1
        self.max_reward = max(self.max_reward, reward)
        over = s[LIVES_I] == 0 or s[LEFT] == 0 or s[GAME_STEPS] >= STEP_CAP
        if over:
            self.game_overs["lives" if s[LIVES_I] == 0 else "cleared" if s[LEFT] == 0 else "cap"] += 1
            s[GAME] += 1
            bricks = self._new_game(e, s)
            cur = prev = (s[BX], s[BY], s[PX], bricks)
        elif lost:
            self._serve(e, s)
            cur = prev = (s[BX], s[BY], s[PX], bricks)
        done = over or (lost and self.life_loss_terminal)
        if done:
            s[STEPS] = 0
        self._store(e, s, bricks)
        return cur, prev, reward, lost, over, done

    def step(self, actions, render_pairs=True):
        a = np.asarray(actions).astype(np.int64)
        rewards, dones = np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)
        pairs = np.zeros((self.n, 2, H, W, 3), np.uint8) if render_pairs else None
        self.lost = np.zeros(self.n, bool)          # of this step: a life was lost / the game ended
        self.over = np.zeros(self.n, bool)
        for e in range(self.n):
            cur, prev, r, self.lost[e], self.over[e], d = self.step_env(e, int(a[e]))
            rewards[e], dones[e] = r, d
            if render_pairs:
                pairs[e, 0] = render(*cur)
                pairs[e, 1] = pairs[e, 0] if prev == cur else render(*prev)
        return pairs, rewards, dones


def tracking_action(state):
    """The naive tracking policy: (n,) actions from (n, 16) states -- of no-op, right and left the
    one whose paddle centre after this env-step is nearest the ball's centre after it (walls
    included; the first of equals)."""
    bx, vx, px = (state[:, i].astype(np.int64) for i in (BX, VXI, PX))
    for _ in range(4):
        bx = bx + vx
        lo, hi = bx < 0, bx > 156
        bx = np.where(lo, -bx, np.where(hi, 312 - bx, bx))
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


def column(c, rows):
    """The bricks of column c in the given rows."""
    return sum(brick_bit(r, c) for r in rows)


def crafted_states():
    """name -> (state row, policy) of the states natural play reaches only after hundreds of
    steps; policy is an action or "track".  The ball at (82, y) moving (+1, -4) tests column 10
    one frame later, at cx = 85."""
    def below_row(r):          # column 10 cleared below brick row r, the ball one frame under that row
        return make_state(82, 64 + 6 * r, 1, -4, bricks=ALL_BRICKS & ~column(10, range(r + 1, ROWS)))
    hole = ALL_BRICKS & ~sum(column(c, range(ROWS)) for c in (9, 10, 11))
    return {
        "hole_to_ceiling": (make_state(82, 120, 1, -4, bricks=hole), "track"),
        "last_brick": (make_state(82, 72, 1, -4, bricks=brick_bit(1, 10), score=425), 0),        # a row-1 brick: 7
        "step_cap": (make_state(40, 100, 2, 4, game_steps=998, score=3, bricks=ALL_BRICKS & ~column(4, (5,))), "track"),
        "last_life": (make_state(150, 176, 1, 4, px=0, lives=1, serves=5), 3),
        "row0": (below_row(0), "track"),                                                         # a 7-point brick
        "row2": (below_row(2), "track"),
        "row3": (below_row(3), "track"),
        "segment0": (make_state(69, 182, 1, 4), 0),            # bx + 2 - px = 0 at the paddle's row
        "segment3": (make_state(85, 182, 1, 4), 0),            # bx + 2 - px = 16, clamped to 15
        "left_wall": (make_state(3, 110, -2, -4), "track"),
        "right_wall": (make_state(154, 110, 2, -4), "track"),
    }


def seven_point_state():
    """The ball one frame under brick (0, 10) with columns 10 and 11 cleared below it: the step
    that follows scores exactly 7 whatever the action, and the ball falls back through the gap."""
    return make_state(82, 64, 1, -4, bricks=ALL_BRICKS & ~column(10, range(1, ROWS)) & ~column(11, range(1, ROWS)))


def script_actions(state, policies, rng):
    """(n,) int32 actions of one step: policies[e] is an action, "track" or "random" (0..5)."""
    track = tracking_action(state)
    return np.array([track[e] if p == "track" else rng.integers(0, 6) if p == "random" else p
                     for e, p in enumerate(policies)], np.int32)


def script_policies(n):
    """The granular test's script: env 0 always left, env 1 always right, then the crafted states,
    then 8 tracking envs, the rest random in 0..5.  -> (policies, {env: crafted state row})."""
    crafted = list(crafted_states().values())
    policies, rows = [], {}
    for e in range(n):
        if e < 2:
            policies.append(3 if e == 0 else 2)
        elif e - 2 < len(crafted):
            rows[e], p = crafted[e - 2]
            policies.append(p)
        else:
            policies.append("track" if e - 2 - len(crafted) < 8 else "random")
    return policies, rows


def assert_every_event_class(ref):
    """The counters of a script that claims to reach everything."""
    assert ref.wall[0] > 0 and ref.wall[1] > 0 and ref.ceiling > 0, (ref.wall, ref.ceiling)
    assert all(h > 0 for h in ref.row_hits), ref.row_hits
    assert all(h > 0 for h in ref.paddle_hits), ref.paddle_hits
    assert ref.life_losses > 0 and all(v > 0 for v in ref.game_overs.values()), (ref.life_losses, ref.game_overs)
    assert ref.max_reward >= 7
