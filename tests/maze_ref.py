"""Test-side NumPy restatement of the device-resident maze (include/asyncrl_hip.h, "device
environment"), in the header's order: the geometry, the carving of a level's binary-tree maze, the
level of an episode and the task of a level through the oracle's Philox, the step, the painter with
the view's fog, counters of every event class so that a test can prove its script reached what it
claims, and a scripted policy whose coverage does not depend on luck.  Nothing here imports the
package under test.  The game is exact in integer arithmetic, so the kernel has to agree bit for
bit.

The step is a scalar Python loop per env on purpose: it is the header's text line by line."""
import functools
from collections import deque

import numpy as np

from oracle import philox4x32

H, W = 210, 160
OPEN_RGB, WALL_RGB, GOAL_RGB, AGENT_RGB = (40, 40, 40), (96, 96, 96), (236, 236, 120), (92, 186, 92)
TILE, MAZE_Y0, AGENT, AGENT_OFF, FRAME_PX = 16, 32, 8, 4, 4
ROOMS, VIEWS, LEVELS_MAX, ROOMS_DEFAULT = (2, 3, 4), (0, 1, 2), 1023, 3
STREAM = 6
UP, DOWN, RIGHT, LEFT = range(4)
DELTA = ((-1, 0), (1, 0), (0, 1), (0, -1))               # (dy, dx) of a & 3
STATE_INTS = 8
POSGOAL, BITS, STEPS, EPISODE, WINS, TIMEOUTS, LEVEL, CFG = range(8)


def cap(R):
    return 8 * R


def cfg_of(R, V, levels):
    return R | V << 3 | levels << 5


def mulhi(a, b):
    return (int(a) * int(b)) >> 32


def _philox(c0, c1, c2, seed):
    w = philox4x32((np.array([c0], np.uint64), np.array([c1], np.uint64), np.array([c2], np.uint64),
                    np.full(1, STREAM, np.uint64)), (seed & 0xffffffff, seed >> 32))
    return [int(x[0]) for x in w]


@functools.lru_cache(maxsize=None)
def open_tiles(bits, R):
    """The open tiles (ty, tx) of the binary-tree maze `bits` carves over R x R rooms."""
    out = set()
    for i in range(R):
        for j in range(R):
            out.add((2 * i + 1, 2 * j + 1))
            if i == 0 and j == R - 1:
                continue
            if i == 0:
                north = False
            elif j == R - 1:
                north = True
            else:
                north = bool(bits >> ((i - 1) * (R - 1) + j) & 1)
            out.add((2 * i, 2 * j + 1) if north else (2 * i + 1, 2 * j + 2))
    return frozenset(out)


def room_tile(idx, R):
    """Room index i R + j -> (ty, tx)."""
    return 2 * (idx // R) + 1, 2 * (idx % R) + 1


@functools.lru_cache(maxsize=None)
def task_of(seed, level, R):
    """Level -> (bits, start tile, goal tile)."""
    w0, w1, w2, _ = _philox(level, 0, 1, seed)
    bits = w0 & ((1 << (R - 1) ** 2) - 1)
    s = mulhi(w1, R * R)
    g = s + 1 + mulhi(w2, R * R - 1)
    if g >= R * R:
        g -= R * R
    return bits, room_tile(s, R), room_tile(g, R)


def level_of(seed, env_id, episode, levels):
    w0 = _philox(env_id, episode, 0, seed)[0]
    return mulhi(w0, levels) if levels else w0


def shortest_path(bits, R, start, goal):
    """The actions of one BFS shortest path from start to goal (neighbours tried in the order up, down, right,
    left)."""
    tiles = open_tiles(bits, R)
    prev = {start: None}
    q = deque([start])
    while q:
        cur = q.popleft()
        if cur == goal:
            break
        for a, (dy, dx) in enumerate(DELTA):
            nxt = (cur[0] + dy, cur[1] + dx)
            if nxt in tiles and nxt not in prev:
                prev[nxt] = (cur, a)
                q.append(nxt)
    path = []
    cur = goal
    while prev[cur] is not None:
        cur, a = prev[cur]
        path.append(a)
    return path[::-1]


def distances(bits, R, start):
    """BFS distance from start to every open tile."""
    tiles = open_tiles(bits, R)
    dist = {start: 0}
    q = deque([start])
    while q:
        cur = q.popleft()
        for dy, dx in DELTA:
            nxt = (cur[0] + dy, cur[1] + dx)
            if nxt in tiles and nxt not in dist:
                dist[nxt] = dist[cur] + 1
                q.append(nxt)
    return dist


@functools.lru_cache(maxsize=4096)
def _render(R, V, bits, goal, at, ax, ay):
    s = np.zeros((H, W, 3), np.uint8)
    G = 2 * R + 1
    tiles = open_tiles(bits, R)
    for ty in range(G):
        for tx in range(G):
            if V and max(abs(ty - at[0]), abs(tx - at[1])) > V:
                continue                                  # fog: black
            rgb = GOAL_RGB if (ty, tx) == goal else OPEN_RGB if (ty, tx) in tiles else WALL_RGB
            s[MAZE_Y0 + TILE * ty:MAZE_Y0 + TILE * (ty + 1), TILE * tx:TILE * (tx + 1)] = rgb
    s[ay:ay + AGENT, ax:ax + AGENT] = AGENT_RGB
    s.setflags(write=False)
    return s


def render(R, V, bits, goal, at, ax=None, ay=None):
    """One screen (210, 160, 3) uint8 (read-only, cached): the maze `bits` over R x R rooms with the goal tile,
    the view V centred on the agent's tile `at`, and the agent's 8 x 8 at (ax, ay) -- at rest on its tile by
    default."""
    if ax is None:
        ax, ay = TILE * at[1] + AGENT_OFF, MAZE_Y0 + TILE * at[0] + AGENT_OFF
    return _render(R, V, bits, tuple(goal), tuple(at), ax, ay)


def pack(tile):
    return tile[0] << 4 | tile[1]


def unpack(p):
    return p >> 4, p & 15


class MazeRef:
    """n envs; state (n, 8) int32 [pos | goal << 8, bits, steps_in_episode, episode, wins, timeouts, level, cfg]."""

    def __init__(self, n, seed=0, env_offset=0, rooms=ROOMS_DEFAULT, view=0, levels=0):
        assert rooms in ROOMS and view in VIEWS and 0 <= levels <= LEVELS_MAX
        self.n, self.seed, self.env_offset = n, seed, env_offset
        self.rooms, self.view, self.levels = rooms, view, levels
        self.state = np.zeros((n, STATE_INTS), np.int32)
        # event counters, summed over envs
        self.moves = [0, 0, 0, 0]                # by direction
        self.bumps = self.wins = self.timeouts = 0
        self.draws = []                          # (env id, episode, level) of every episode start
        self.plan = {}                           # env -> the actions left of its BFS path (the scripted policy)

    # the state row as Python ints; level is stored as its 32-bit pattern
    def _get(self, e):
        return [int(x) for x in self.state[e]]

    def _put(self, e, s):
        self.state[e] = np.array(s, np.int64).astype(np.uint32).view(np.int32)

    def _start(self, e, s):
        level = level_of(self.seed, e + self.env_offset, s[EPISODE], self.levels)
        bits, start, goal = task_of(self.seed, level, self.rooms)
        self.draws.append((e + self.env_offset, s[EPISODE], level))
        s[POSGOAL] = pack(start) | pack(goal) << 8
        s[BITS], s[STEPS], s[LEVEL] = bits, 0, level
        self.plan.pop(e, None)

    def _screen(self, s):
        """render's arguments for the screen between env-steps."""
        at = unpack(s[POSGOAL] & 0xff)
        return (self.rooms, self.view, s[BITS], unpack(s[POSGOAL] >> 8), at, TILE * at[1] + AGENT_OFF,
                MAZE_Y0 + TILE * at[0] + AGENT_OFF)

    def reset(self):
        """-> pairs (n, 2, 210, 160, 3) uint8, rewards (n,) f32 = 0, dones (n,) uint8 = 0."""
        pairs = np.zeros((self.n, 2, H, W, 3), np.uint8)
        self.plan = {}
        for e in range(self.n):
            s = [0] * STATE_INTS
            s[CFG] = cfg_of(self.rooms, self.view, self.levels)
            self._start(e, s)
            self._put(e, s)
            pairs[e, 0] = pairs[e, 1] = render(*self._screen(s))
        return pairs, np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)

    def step_env(self, e, act):
        """One env-step of env e -> (cur screen args, prev screen args, reward, done)."""
        s = self._get(e)
        s[CFG] = cfg_of(self.rooms, self.view, self.levels)
        R = self.rooms
        pos, goal = unpack(s[POSGOAL] & 0xff), unpack(s[POSGOAL] >> 8)
        d = act & 3
        dy, dx = DELTA[d]
        s[STEPS] += 1
        target = (pos[0] + dy, pos[1] + dx)
        moved = target in open_tiles(s[BITS] & 0xffffffff, R)
        if moved:
            pos = target
            self.moves[d] += 1
        else:
            self.bumps += 1
        s[POSGOAL] = pack(pos) | pack(goal) << 8
        reward = done = 0
        if pos == goal:
            reward = done = 1
            s[WINS] += 1
            self.wins += 1
        elif s[STEPS] == cap(R):
            done = 1
            s[TIMEOUTS] += 1
            self.timeouts += 1
        if done:
            s[EPISODE] += 1
            self._start(e, s)
            cur = prev = self._screen(s)         # the next episode's first screen, twice
        else:
            cur = self._screen(s)
            prev = cur[:5] + (cur[5] - (FRAME_PX * dx if moved else 0), cur[6] - (FRAME_PX * dy if moved else 0))
        self._put(e, s)
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
                pairs[e, 1] = render(*prev)
        return pairs, rewards, dones

    def scripted_actions(self, t):
        """(n,) int32, the scripted policy at env-step t: env e with e % 3 == 0 follows a BFS shortest path (it
        wins within 8R - 10 steps), e % 3 == 1 plays (t + e) & 3, e % 3 == 2 repeats the action (e // 3) & 3 (it
        bumps, and times out at the cap unless the goal lies on its one line)."""
        out = np.zeros(self.n, np.int32)
        for e in range(self.n):
            if e % 3 == 0:
                if e not in self.plan:
                    s = self._get(e)
                    self.plan[e] = shortest_path(s[BITS] & 0xffffffff, self.rooms, unpack(s[POSGOAL] & 0xff),
                                                 unpack(s[POSGOAL] >> 8))
                out[e] = self.plan[e].pop(0)
            elif e % 3 == 1:
                out[e] = (t + e) & 3
            else:
                out[e] = (e // 3) & 3
        return out


def coverage(n, rooms, view, levels, steps, seed=0, env_offset=0):
    """The counters of `steps` env-steps of the scripted policy from a reset, no rendering."""
    ref = MazeRef(n, seed=seed, env_offset=env_offset, rooms=rooms, view=view, levels=levels)
    ref.reset()
    for t in range(steps):
        ref.step(ref.scripted_actions(t), render_pairs=False)
    return ref


# What test_gpu_maze.py drives with the scripted policy, as (n, rooms, view, levels, steps, seed, env_offset):
# test_maze.py proves on the restatement alone that each reaches every event class.
GRANULAR_SEED, SCREEN_SEED = (9 << 32) | 12345, (4 << 32) | 321
GRANULAR_CASES = tuple((n, R, V, L, 2 * cap(R) + 2, GRANULAR_SEED, 7 if (n, R) == (33, 3) else 0)
                       for n in (1, 33, 75) for R, V, L in ((2, 0, 0), (3, 1, 5), (4, 2, 0), (4, 0, 1)))
SCREEN_CASES = tuple((33, R, V, 0, cap(R) + 4, SCREEN_SEED, 6) for R in (2, 4) for V in (0, 2))
SCRIPTED_GPU_CASES = GRANULAR_CASES + SCREEN_CASES


def random_success_exact(R):
    """The success rate of the uniform random policy over 4 actions on a uniformly drawn task (layout, start,
    goal != start), within the cap of 8R steps: exact, by the Markov chain's hitting probabilities."""
    G = 2 * R + 1
    total, tasks = 0.0, 0
    rooms = [room_tile(k, R) for k in range(R * R)]
    for bits in range(1 << (R - 1) ** 2):
        tiles = sorted(open_tiles(bits, R))
        idx = {t: k for k, t in enumerate(tiles)}
        P = np.zeros((len(tiles), len(tiles)))
        for t, k in idx.items():
            for dy, dx in DELTA:
                nxt = (t[0] + dy, t[1] + dx)
                P[k, idx.get(nxt, k)] += 0.25             # a bump stays
        assert all(0 <= t[0] < G and 0 <= t[1] < G for t in tiles)
        for goal in rooms:
            g = idx[goal]
            Q = P.copy()
            Q[g] = 0.0
            Q[g, g] = 1.0                                 # absorbing
            h = np.zeros(len(tiles))
            h[g] = 1.0
            for _ in range(cap(R)):
                h = Q @ h
            for start in rooms:
                if start != goal:
                    total += h[idx[start]]
                    tasks += 1
    return total / tasks, tasks
