"""CPU: the NumPy restatement of the device-resident maze (maze_ref.py) does what the header says
-- the facts the rules rest on, by enumeration of every task of every R (task counts, 2 R^2 - 1 open
tiles and a spanning tree, the longest shortest path 8R - 10 under the cap of 8R), the uniform-random
success rate (exactly, and from 20,000 episodes through the oracle's Philox), the step and the
painter with the view's fog --, the agent, the goal and every carved bit survive the luminance and
the resize of the oracle's phi in all four modes, a goal in the fog leaves no trace, the maze entry
points of the C ABI validate their arguments on the host, before any launch (fake, never-dereferenced
device pointers; no GPU here), and the scripted policy of the GPU tests reaches every event class in
every case they run.  (The render's chunk function is compiled for the device alone, as the other
games' are, so the painter is compared on the GPU: test_gpu_maze.py.)"""
import itertools
import os
import re

import numpy as np
import pytest

import maze_ref as M
from conftest import ROOT
from test_catch import make_net

OK, EINVAL, ESTATE = 0, 1, 3
ENV_CATCH, ENV_BREAKOUT, ENV_PONG, ENV_TMAZE, ENV_MAZE, GAME_OVER_ONLY = 1, 2, 4, 8, 32, 0x100
PAIR = 2 * 210 * 160 * 3


def kind_of(rooms=0, view=0, levels=0):
    return ENV_MAZE | rooms << 16 | view << 19 | levels << 21


# ---------------------------------------------------------------- the facts the rules rest on
# the issue's table: tasks, the longest shortest path, the cap, and its own 20,000-episode estimate of the
# uniform-random success rate (NumPy's generator in place of Philox)
FACTS = {2: (24, 6, 16, 0.364), 3: (1152, 14, 24, 0.207), 4: (122880, 22, 32, 0.142)}


@pytest.mark.parametrize("R", M.ROOMS)
def test_every_task_is_solvable_within_the_cap(R):
    """Every layout x start x goal of R by enumeration: 2 R^2 - 1 open tiles, all of them reachable from every
    room (a spanning tree), inside the border; the task count; the longest shortest path is exactly 8R - 10,
    below the cap 8R; the BFS path the scripted policy follows has that length and walks open tiles only."""
    tasks, longest, cap, _ = FACTS[R]
    assert longest == 8 * R - 10 and cap == M.cap(R) == 8 * R
    G = 2 * R + 1
    n_tasks = worst = 0
    for bits in range(1 << (R - 1) ** 2):
        tiles = M.open_tiles(bits, R)
        assert len(tiles) == 2 * R * R - 1
        assert all(1 <= ty <= G - 2 and 1 <= tx <= G - 2 for ty, tx in tiles)
        for s in range(R * R):
            dist = M.distances(bits, R, M.room_tile(s, R))
            assert set(dist) == tiles
            for g in range(R * R):
                if g != s:
                    n_tasks += 1
                    worst = max(worst, dist[M.room_tile(g, R)])
        s, g = M.room_tile(0, R), M.room_tile(R * R - 1, R)
        path = M.shortest_path(bits, R, s, g)
        assert len(path) == M.distances(bits, R, s)[g]
        cur = s
        for a in path:
            cur = (cur[0] + M.DELTA[a][0], cur[1] + M.DELTA[a][1])
            assert cur in tiles
        assert cur == g
    assert n_tasks == tasks and worst == longest


RANDOM_EPISODES = 20000


def random_success(R, episodes, seed=11):
    """Uniform-random play of `episodes` episodes of levels = 0 on one env of the restatement's rules: the level
    of every episode and its task through the oracle's Philox (one batched call each), the actions from NumPy."""
    from oracle import philox4x32
    key = (seed & 0xffffffff, seed >> 32)
    ep = np.arange(episodes, dtype=np.uint64)
    zero = np.zeros(episodes, np.uint64)
    level = philox4x32((zero, ep, zero, np.full(episodes, M.STREAM, np.uint64)), key)[0]
    w0, w1, w2, _ = philox4x32((level, zero, zero + np.uint64(1), np.full(episodes, M.STREAM, np.uint64)), key)
    assert int(level[5]) == M.level_of(seed, 0, 5, 0)
    rng = np.random.default_rng(seed)
    acts = rng.integers(0, 4, size=(episodes, M.cap(R)))
    wins = 0
    for k in range(episodes):
        bits = int(w0[k]) & ((1 << (R - 1) ** 2) - 1)
        s = M.mulhi(w1[k], R * R)
        g = s + 1 + M.mulhi(w2[k], R * R - 1)
        g -= R * R if g >= R * R else 0
        if k < 50:
            assert (bits, M.room_tile(s, R), M.room_tile(g, R)) == M.task_of(seed, int(level[k]), R)
        tiles, pos, goal = M.open_tiles(bits, R), M.room_tile(s, R), M.room_tile(g, R)
        for a in acts[k]:
            nxt = (pos[0] + M.DELTA[a][0], pos[1] + M.DELTA[a][1])
            if nxt in tiles:
                pos = nxt
                if pos == goal:
                    wins += 1
                    break
    return wins / episodes


@pytest.mark.parametrize("R", M.ROOMS)
def test_uniform_random_success_rate(R):
    """The rate a learner has to beat.  Exactly, from the Markov chain of uniform play over every task: 0.3680
    (R = 2), 0.2112 (R = 3), 0.1440 (R = 4) -- the values to quote.  20,000 episodes of the restatement's rules
    with Philox-drawn levels lie within 5 standard errors of it, and so does the estimate the rules were chosen
    with (two independent 20,000-episode estimates: sqrt 2 standard errors)."""
    p, tasks = M.random_success_exact(R)
    got = random_success(R, RANDOM_EPISODES)
    se = (p * (1 - p) / RANDOM_EPISODES) ** 0.5
    print("R = %d: uniform-random success exact %.4f, %d episodes %.4f (se %.4f)" % (R, p, RANDOM_EPISODES, got, se))
    assert tasks == FACTS[R][0]
    assert round(p, 4) == {2: 0.3680, 3: 0.2112, 4: 0.1440}[R]
    assert abs(got - p) <= 5 * se
    assert abs(FACTS[R][3] - p) <= 5 * se + 0.0005        # (the table's figure is rounded to three places)


# ---------------------------------------------------------------- the restatement's own invariants
def test_levels_and_tasks_come_from_philox():
    """level = mulhi(w0, levels) (or w0 itself) of the oracle's Philox at counter (env_offset + e, episode, 0,
    6); bits, start and goal from counter (level, 0, 1, 6); key = the seed's two halves; goal != start; with
    levels = L only L tasks occur, all of them in range, and levels = 0 leaves that set."""
    from oracle import philox4x32
    seed, off, n = (7 << 32) | 99, 3, 16

    def words(c0, c1, c2):
        w = philox4x32((np.array([c0], np.uint64), np.array([c1], np.uint64), np.array([c2], np.uint64),
                        np.full(1, 6, np.uint64)), (99, 7))
        return [int(x[0]) for x in w]

    for levels in (0, 1, 5, 1023):
        ref = M.MazeRef(n, seed=seed, env_offset=off, rooms=3, levels=levels)
        ref.reset()
        for ep in range(3):
            for e in range(n):
                w0 = words(off + e, ep, 0)[0]
                level = (w0 * levels) >> 32 if levels else w0
                t = words(level, 0, 1)
                s = (t[1] * 9) >> 32
                g = (s + 1 + ((t[2] * 8) >> 32)) % 9
                assert g != s
                row = ref.state[e]
                assert int(row[M.LEVEL]) & 0xffffffff == level and int(row[M.BITS]) == t[0] & 15
                assert int(row[M.POSGOAL]) == M.pack(M.room_tile(s, 3)) | M.pack(M.room_tile(g, 3)) << 8
                assert int(row[M.EPISODE]) == ep and int(row[M.STEPS]) == 0
            ref.state[:, M.STEPS] = M.cap(3) - 1          # the next step ends every env's episode, won or not
            _, r, d = ref.step(np.zeros(n, np.int32), render_pairs=False)
            assert d.all()
            assert (ref.state[:, M.EPISODE] == ep + 1).all()
        seen = {lv for _, _, lv in ref.draws}
        if levels:
            assert seen <= set(range(levels)) and (levels > 1 or seen == {0})
        else:
            assert max(seen) > 1 << 24
        assert int(ref.state[0, M.CFG]) == M.cfg_of(3, 0, levels)


@pytest.mark.parametrize("R,V", [(2, 0), (3, 1), (4, 2)])
def test_step_and_painter(R, V):
    """One env, every action from every open tile of one level: a move shows the agent on the target tile in
    pair[0] and 4 px short of it in pair[1], a bump shows the unmoved agent twice, the goal pays 1 and shows the
    next episode's first screen twice, the cap ends an episode with 0; the screen is the tiles' colours with
    the 8 x 8 agent at (4, 4) in its tile, black outside the maze and outside the view."""
    ref = M.MazeRef(1, seed=3, rooms=R, view=V)
    ref.reset()
    G = 2 * R + 1
    row0 = ref.state[0].copy()
    bits, goal = int(row0[M.BITS]), M.unpack(int(row0[M.POSGOAL]) >> 8)
    tiles = M.open_tiles(bits, R)
    for pos in sorted(tiles - {goal}):
        for a in range(6):
            ref.state[0] = row0
            ref.state[0, M.POSGOAL] = M.pack(pos) | M.pack(goal) << 8
            ref.state[0, M.STEPS] = 3
            pairs, r, d = ref.step([a])
            dy, dx = M.DELTA[a & 3]
            tgt = (pos[0] + dy, pos[1] + dx)
            if tgt == goal:
                assert r[0] == 1 and d[0] == 1 and ref.state[0, M.WINS] == 1 and ref.state[0, M.EPISODE] == 1
                assert ref.state[0, M.STEPS] == 0 and (pairs[0, 0] == pairs[0, 1]).all()
                assert (pairs[0, 0] == M.render(*ref._screen(ref._get(0)))).all()
                continue
            assert r[0] == 0 and d[0] == 0 and ref.state[0, M.STEPS] == 4
            now = tgt if tgt in tiles else pos
            assert M.unpack(int(ref.state[0, M.POSGOAL]) & 0xff) == now
            ax, ay = 16 * now[1] + 4, 32 + 16 * now[0] + 4
            assert (pairs[0, 0] == M.render(R, V, bits, goal, now, ax, ay)).all()
            short = (ax - 4 * dx, ay - 4 * dy) if tgt in tiles else (ax, ay)
            assert (pairs[0, 1] == M.render(R, V, bits, goal, now, *short)).all()
            assert (pairs[0, 0] != pairs[0, 1]).any() == (tgt in tiles)
            s = pairs[0, 0]
            assert not s[:32].any() and not s[32 + 16 * G:].any() and not s[:, 16 * G:].any()
            assert (s[ay:ay + 8, ax:ax + 8] == M.AGENT_RGB).all()
            assert int((s == np.array(M.AGENT_RGB, np.uint8)).all(-1).sum()) == 64
            for ty in range(G):
                for tx in range(G):
                    want = ((0, 0, 0) if V and max(abs(ty - now[0]), abs(tx - now[1])) > V else
                            M.GOAL_RGB if (ty, tx) == goal else M.OPEN_RGB if (ty, tx) in tiles else M.WALL_RGB)
                    assert tuple(s[32 + 16 * ty, 16 * tx]) == want and tuple(s[47 + 16 * ty, 16 * tx + 15]) == want
    # the cap: a bump on step 8R ends the episode with reward 0
    ref.state[0] = row0
    ref.state[0, M.STEPS] = M.cap(R) - 1
    pos = M.unpack(int(row0[M.POSGOAL]) & 0xff)
    bump = next(a for a in range(4) if (pos[0] + M.DELTA[a][0], pos[1] + M.DELTA[a][1]) not in tiles)
    pairs, r, d = ref.step([bump])
    assert r[0] == 0 and d[0] == 1 and ref.state[0, M.TIMEOUTS] == 1 and ref.state[0, M.STEPS] == 0
    assert (pairs[0, 0] == pairs[0, 1]).all() and ref.bumps > 0 and ref.timeouts == 1


# ---------------------------------------------------------------- what the models can see
def plane(mode, *args):
    import oracle as O
    s = M.render(*args)
    return O.current_screen(s, s, mode)


@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("R", M.ROOMS)
def test_agent_goal_and_every_carved_bit_show_on_the_plane(R, mode):
    """View 0, all four resize modes of the oracle's phi: two screens that differ in the agent's tile, in the
    goal's tile or in one carved bit give different 84 x 84 planes; the five luminances are distinct."""
    import oracle as O
    lum = {k: int(O.luminance_u8(np.array(v, np.uint8).reshape(1, 1, 3))[0, 0])
           for k, v in (("open", M.OPEN_RGB), ("wall", M.WALL_RGB), ("goal", M.GOAL_RGB), ("agent", M.AGENT_RGB),
                        ("background", (0, 0, 0)))}
    print("luminance:", lum)
    assert len(set(lum.values())) == 5 and lum["background"] == 0
    nbits = (R - 1) ** 2
    bits = 0b101010101 & ((1 << nbits) - 1)
    rooms = [M.room_tile(k, R) for k in range(R * R)]
    tiles = sorted(M.open_tiles(bits, R))
    goal = rooms[-1]
    planes = [plane(mode, R, 0, bits, goal, at) for at in tiles if at != goal]
    for a, b in itertools.combinations(planes, 2):
        assert (a != b).any()                             # the agent's tile
    planes = [plane(mode, R, 0, bits, g, rooms[0]) for g in rooms[1:]]
    for a, b in itertools.combinations(planes, 2):
        assert (a != b).any()                             # the goal's tile
    base = plane(mode, R, 0, bits, goal, rooms[0])
    for k in range(nbits):
        assert (plane(mode, R, 0, bits ^ 1 << k, goal, rooms[0]) != base).any()   # one carved bit


@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("V", [1, 2])
def test_a_goal_in_the_fog_leaves_the_plane_unchanged(V, mode):
    """View V >= 1: two screens that differ only in a goal outside the window are the same screen, so the same
    plane; a goal inside the window shows."""
    R, bits = 4, 0b110100101
    at = (1, 2)                                           # the passage east of room 0: rooms at distance 1
    assert at in M.open_tiles(bits, R)
    far = [g for g in (M.room_tile(k, R) for k in range(R * R)) if max(abs(g[0] - at[0]), abs(g[1] - at[1])) > V]
    near = [g for g in (M.room_tile(k, R) for k in range(R * R)) if g not in far]
    assert len(far) >= 2 and near
    base = plane(mode, R, V, bits, far[0], at)
    for g in far[1:]:
        assert (M.render(R, V, bits, g, at) == M.render(R, V, bits, far[0], at)).all()
        assert (plane(mode, R, V, bits, g, at) == base).all()
    for g in near:
        assert (plane(mode, R, V, bits, g, at) != base).any()
    assert (plane(mode, R, 0, bits, far[0], at) != base).any()   # the fog itself shows


# ---------------------------------------------------------------- the C ABI, no device
def test_header_and_table_carry_the_maze_symbols():
    import asyncrl_amd
    from asyncrl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "asyncrl_hip.h")).read()
    assert re.search(r"#define ARL_ENV_MAZE 32\b", txt)
    assert re.search(r"#define ARL_ENV_MAZE_ROOMS\(r\) \(\(r\) << 16\)", txt)
    assert re.search(r"#define ARL_ENV_MAZE_VIEW\(v\) \(\(v\) << 19\)", txt)
    assert re.search(r"#define ARL_ENV_MAZE_LEVELS\(l\) \(\(l\) << 21\)", txt)
    for s in ("arl_maze_state_bytes", "arl_maze_reset", "arl_maze_step"):
        assert re.search(r"\b%s\s*\(" % s, txt) and hasattr(_lib.lib, s) and s in _lib.SIGNATURES, s
    assert _lib.ENV_MAZE == ENV_MAZE and _lib.MAZE_STATE_INTS == 8 == M.STATE_INTS
    assert (_lib.MAZE_ROOMS_MIN, _lib.MAZE_ROOMS_MAX, _lib.MAZE_VIEW_MAX, _lib.MAZE_LEVELS_MAX) == (2, 4, 2, 1023)
    assert _lib.env_maze_fields(4, 2, 1023) == kind_of(4, 2, 1023) - ENV_MAZE
    lib = _lib.lib
    assert lib.arl_abi_version() == 4
    for n in (0, 1, 35):
        assert lib.arl_maze_state_bytes(n) == 2 * n * 32
    assert lib.arl_maze_state_bytes(-1) == -1
    with pytest.raises(ValueError):
        asyncrl_amd.DeviceMaze(0, device="cpu")
    for bad in (dict(rooms=1), dict(rooms=5), dict(rooms=0), dict(view=3), dict(view=-1), dict(levels=1024),
                dict(levels=-1)):
        with pytest.raises(ValueError):
            asyncrl_amd.DeviceMaze(3, device="cpu", **bad)
    env = asyncrl_amd.DeviceMaze(3, device="cpu", seed=1, env_offset=2, rooms=4, view=1, levels=16)
    assert env.kind == kind_of(4, 1, 16) and tuple(env.state.shape) == (2, 3, 8) and env.envs == ()
    assert asyncrl_amd.DeviceMaze(3, device="cpu").kind == kind_of(3, 0, 0)
    assert tuple(env.make_pools(2)[0].shape) == (2, 3, 2, 210, 160, 3)
    with pytest.raises(ValueError):
        env.step_screen([0, 0])                               # 3 envs


BAD_FIELDS = ((1, 0, 0), (0, 0, 0), (5, 0, 0), (7, 0, 0), (-1, 0, 0), (3, 3, 0), (3, -1, 0), (3, 0, 1024),
              (3, 0, -1), (GAME_OVER_ONLY, 0, 0), (3, 0, 1 << 16))


def test_granular_calls_validate():
    from asyncrl_amd._lib import lib
    f = 1 << 40
    st, pr, rw, dn, ac = f, f + (1 << 30), f + (2 << 30), f + (3 << 30), f + (4 << 30)
    for R, V, L in itertools.product((2, 3, 4), (0, 1, 2), (0, 1, 1023)):
        assert lib.arl_maze_reset(st, 0, 0, 0, R, V, L, 0, pr, rw, dn, None) == OK      # nothing to do
        assert lib.arl_maze_step(st, 0, ac, 0, 0, 0, R, V, L, pr, rw, dn, None) == OK
    for R, V, L in BAD_FIELDS:
        for n in (0, 4):
            assert lib.arl_maze_reset(st, n, 0, 0, R, V, L, 0, pr, rw, dn, None) == EINVAL
            assert b"rooms" in lib.arl_last_error() and b"view" in lib.arl_last_error()
            assert lib.arl_maze_step(st, 0, ac, n, 0, 0, R, V, L, pr, rw, dn, None) == EINVAL
            assert b"levels" in lib.arl_last_error()
    g = (3, 1, 5)
    assert lib.arl_maze_reset(st, 4, 0, 0, *g, 2, pr, rw, dn, None) == EINVAL      # parity
    assert lib.arl_maze_step(st, -1, ac, 4, 0, 0, *g, pr, rw, dn, None) == EINVAL
    assert lib.arl_maze_reset(None, 4, 0, 0, *g, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_maze_reset(st, 4, 0, 0, *g, 0, None, rw, dn, None) == EINVAL
    assert lib.arl_maze_reset(st, 4, 0, 0, *g, 0, pr, None, dn, None) == EINVAL
    assert lib.arl_maze_reset(st, 4, 0, 0, *g, 0, pr, rw, None, None) == EINVAL
    assert lib.arl_maze_reset(st + 4, 4, 0, 0, *g, 0, pr, rw, dn, None) == EINVAL  # misaligned state
    assert lib.arl_maze_reset(st, 4, 0, 0, *g, 0, pr + 4, rw, dn, None) == EINVAL  # misaligned frames
    assert lib.arl_maze_step(st, 0, ac, 4, 0, 0, *g, pr, rw + 2, dn, None) == EINVAL
    assert lib.arl_maze_step(st, 0, None, 4, 0, 0, *g, pr, rw, dn, None) == EINVAL   # no actions
    assert lib.arl_maze_step(st, 0, ac + 2, 4, 0, 0, *g, pr, rw, dn, None) == EINVAL
    assert lib.arl_maze_step(st, 0, ac, 65536, 0, 0, *g, pr, rw, dn, None) == EINVAL
    assert lib.arl_maze_reset(st, 65536, 0, 0, *g, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_maze_step(st, 0, ac, -1, 0, 0, *g, pr, rw, dn, None) == EINVAL
    assert lib.arl_maze_step(st, 0, ac, 0, 0, 0, *g, pr, rw, dn, None) == OK        # n = 0


# every combination of valid fields (rooms 0 means 3), and each invalid field alone
MAZE_KINDS = tuple(kind_of(r, v, l) for r in (0, 2, 3, 4) for v in (0, 1, 2) for l in (0, 1, 16, 1023))
SOME_KINDS = (kind_of(), kind_of(2, 0, 0), kind_of(3, 1, 5), kind_of(4, 2, 1023))
BAD_KINDS = (kind_of(1), kind_of(5), kind_of(6), kind_of(7), kind_of(3, 3), kind_of(0, 3, 7),
             ENV_MAZE | GAME_OVER_ONLY, kind_of(3, 1, 5) | GAME_OVER_ONLY, ENV_MAZE | 0x200, ENV_MAZE | 0x8000,
             ENV_MAZE | 1 << 31, -ENV_MAZE, ENV_MAZE | ENV_CATCH, ENV_MAZE | ENV_BREAKOUT,
             ENV_MAZE | ENV_PONG, ENV_MAZE | ENV_TMAZE, ENV_MAZE | 16, ENV_MAZE | 64, ENV_CATCH | 1 << 19,
             ENV_BREAKOUT | 1 << 21, ENV_TMAZE | 2 << 19, ENV_PONG | 1 << 21, 1 << 21, 0, 3, 16, 33, 64)
OTHER_KINDS = (ENV_CATCH, ENV_BREAKOUT, ENV_BREAKOUT | GAME_OVER_ONLY, ENV_PONG, ENV_PONG | (1 << 16),
               ENV_PONG | (21 << 16), ENV_TMAZE, ENV_TMAZE | (8 << 16))


def as_int(kind):
    """A kind as the C int it is passed as."""
    return (kind + (1 << 31)) % (1 << 32) - (1 << 31)


@pytest.mark.parametrize("bind", [False, True])
def test_set_env_validation(bind):
    """Kind 32 with every combination of valid fields attaches to FF, LSTM and Nature nets with A in {4, 6}, on
    an unbound and on a (fake-)bound handle; frames-flag nets are ARL_ESTATE; A = 3, a misaligned state, and
    each invalid field alone (rooms 1, 5..7, view 3, 0x100, any other bit) are ARL_EINVAL with "kind" in the
    text; the other four kinds attach as before."""
    from asyncrl_amd._lib import lib
    state = (1 << 40) + (5 << 30)
    for arch in (16, 17, 32, 33, 64):                       # RGB / STACK / STATES nets take no frame pairs
        h = make_net(arch, 4, bind=bind)
        try:
            for kind in MAZE_KINDS:
                assert lib.arl_net_set_env(h, kind, state) == ESTATE, arch
                assert lib.arl_net_set_env(h, kind, None) == OK       # detaching nothing is fine
        finally:
            lib.arl_net_destroy(h)
    h = make_net(0, 3, bind=bind)
    try:
        for kind in SOME_KINDS:
            assert lib.arl_net_set_env(h, kind, state) == EINVAL      # n_actions = 3
            assert b"n_actions" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)
    for arch in (0, 1, 2):
        for A in (4, 6):
            h = make_net(arch, A, bind=bind)
            try:
                for kind in MAZE_KINDS:
                    assert lib.arl_net_set_env(h, kind, state + 4) == EINVAL     # misaligned
                    assert lib.arl_net_set_env(h, kind, state) == OK
                for bad in BAD_KINDS:
                    assert lib.arl_net_set_env(h, as_int(bad), state) == EINVAL, bad
                    assert b"kind" in lib.arl_last_error()
                    assert lib.arl_net_set_env(h, as_int(bad), None) == EINVAL, bad
                if not bind:
                    assert lib.arl_env_step(h, 0, 0, 4, state, state, state, 2, None) == ESTATE   # not bound
                assert lib.arl_net_set_env(h, ENV_MAZE, None) == OK
                for kind in OTHER_KINDS:                                                          # as before
                    assert lib.arl_net_set_env(h, kind, state) == OK
                    assert lib.arl_net_set_env(h, kind, None) == OK
            finally:
                lib.arl_net_destroy(h)
    assert lib.arl_net_set_env(None, ENV_MAZE, state) == EINVAL


@pytest.mark.parametrize("kind", SOME_KINDS)
def test_env_calls_fail_before_any_launch(kind):
    """arl_env_reset / arl_env_step / arl_run_window with a maze attached: pool_len = 1, unregistered or too
    short pools, a missing pool and t = t_max are ARL_EINVAL; no env attached is ARL_ESTATE."""
    from asyncrl_amd._lib import POOL_DONES, POOL_FRAMES, POOL_REWARDS, lib
    N, T = 4, 5
    h = make_net(0, 4, N, T)
    try:
        fake = 1 << 40
        pairs, rew, done, state = fake + (1 << 30), fake + (2 << 30), fake + (3 << 30), fake + (5 << 30)

        def step(t=0, L=2, p=pairs, r=rew, d=done, e0=0, ne=N):
            return lib.arl_env_step(h, t, e0, ne, p, r, d, L, None)

        def window(L=2):
            return lib.arl_run_window(h, pairs, rew, done, L, 1, 0, 0.99, 0.01, 0.5, 1, 7e-4, 0, 0, 0.99, 0.1, 40.0,
                                      None)

        assert step() == ESTATE and b"no env" in lib.arl_last_error()
        assert lib.arl_env_reset(h, pairs, rew, done, 2, None) == ESTATE
        assert lib.arl_net_set_env(h, kind, state) == OK
        assert step() == EINVAL and b"not registered" in lib.arl_last_error()
        assert lib.arl_env_reset(h, pairs, rew, done, 2, None) == EINVAL
        assert window() == EINVAL
        assert lib.arl_net_set_pool(h, POOL_FRAMES, pairs, 3 * N * PAIR) == 0
        assert step() == EINVAL and b"reward" in lib.arl_last_error()
        assert lib.arl_net_set_pool(h, POOL_REWARDS, rew, 3 * N * 4) == 0
        assert lib.arl_net_set_pool(h, POOL_DONES, done, 3 * N) == 0
        for bad in (1, 0, -3):
            assert step(L=bad) == EINVAL and b"pool_len" in lib.arl_last_error()
            assert lib.arl_env_reset(h, pairs, rew, done, bad, None) == EINVAL
        assert window(1) == EINVAL and b"pool_len" in lib.arl_last_error()
        assert step(L=4) == EINVAL and b"exceeds" in lib.arl_last_error()
        assert lib.arl_env_reset(h, pairs, rew, done, 4, None) == EINVAL
        assert window(4) == EINVAL and b"exceeds" in lib.arl_last_error()
        assert step(r=None) == EINVAL and step(d=None) == EINVAL and step(p=None) == EINVAL
        assert step(p=pairs + 8) == EINVAL                                       # misaligned frames
        assert step(t=T) == EINVAL and b"t_max" in lib.arl_last_error()
        assert step(t=-1) == EINVAL
        assert step(e0=1, ne=3) == EINVAL and step(e0=0, ne=N + 1) == EINVAL and step(ne=0) == EINVAL
        assert lib.arl_net_set_env(h, kind, None) == OK
        assert step() == ESTATE
    finally:
        lib.arl_net_destroy(h)


@pytest.mark.parametrize("bind", [False, True])
def test_set_env_direct_validation(bind):
    """arl_net_set_env_direct with the new kind: needs the env attached, refuses frames-flag nets, goes off
    with the env; a bound net with direct mode off refuses arl_env_step_observe."""
    from asyncrl_amd._lib import lib
    state = (1 << 40) + (5 << 30)
    for arch in (16, 32, 64):
        h = make_net(arch, 4, bind=bind)
        try:
            assert lib.arl_net_set_env(h, ENV_MAZE, state) == ESTATE
            assert lib.arl_net_set_env_direct(h, 1) == ESTATE and b"frame pairs" in lib.arl_last_error()
        finally:
            lib.arl_net_destroy(h)
    for arch in (0, 1, 2):
        h = make_net(arch, 4, bind=bind)
        try:
            assert lib.arl_net_set_env_direct(h, 1) == ESTATE and b"no env" in lib.arl_last_error()
            for kind in SOME_KINDS:
                assert lib.arl_net_set_env(h, kind, state) == OK
                assert lib.arl_net_set_env_direct(h, 1) == OK
                assert lib.arl_net_set_env_direct(h, 0) == OK
                assert lib.arl_net_set_env_direct(h, 1) == OK
                assert lib.arl_net_set_env(h, kind, None) == OK            # detach: direct goes with the env
                assert lib.arl_net_set_env(h, kind, state) == OK
                if bind:
                    assert lib.arl_env_step_observe(h, 0, 0, 4, 0, None) == ESTATE
                    assert b"direct mode is off" in lib.arl_last_error()
                    assert lib.arl_net_set_env_direct(h, 1) == OK
                    for t in (5, -1):
                        assert lib.arl_env_step_observe(h, t, 0, 4, 0, None) == EINVAL
                        assert b"t_max" in lib.arl_last_error()
                    for mode in (-1, 4):
                        assert lib.arl_env_step_observe(h, 0, 0, 4, mode, None) == EINVAL
                        assert lib.arl_env_reset_observe(h, mode, None) == EINVAL
                        assert b"resize_mode" in lib.arl_last_error()
                    assert lib.arl_env_step_observe(h, 0, 1, 3, 0, None) == EINVAL
                else:
                    assert lib.arl_net_set_env_direct(h, 1) == OK
                    assert lib.arl_env_step_observe(h, 0, 0, 4, 0, None) == ESTATE
                    assert lib.arl_env_reset_observe(h, 0, None) == ESTATE
                assert lib.arl_net_set_env(h, kind, None) == OK
        finally:
            lib.arl_net_destroy(h)


def test_step_screen_validates():
    from asyncrl_amd._lib import lib
    f = 1 << 40
    st, sc, rw, dn, ac = f, f + (1 << 30), f + (2 << 30), f + (3 << 30), f + (4 << 30)

    def call(kind=ENV_MAZE, state=st, parity=0, actions=ac, n=4, mode=0, screen=sc, r=rw, d=dn):
        return lib.arl_env_step_screen(as_int(kind), state, parity, actions, n, 0, 0, mode, screen, r, d, None)

    for kind in MAZE_KINDS + OTHER_KINDS:
        for mode in range(4):
            assert call(kind=kind, n=0, mode=mode) == OK                  # nothing to do
    for bad in BAD_KINDS:
        assert call(kind=bad) == EINVAL and b"kind" in lib.arl_last_error(), bad
        assert call(kind=bad, n=0) == EINVAL
    for kind in SOME_KINDS:
        for mode in (-1, 4, 7):
            assert call(kind=kind, mode=mode) == EINVAL and b"resize_mode" in lib.arl_last_error()
        for parity in (-1, 2):
            assert call(kind=kind, parity=parity) == EINVAL and b"parity" in lib.arl_last_error()
        assert call(kind=kind, n=-1) == EINVAL and call(kind=kind, n=65536) == EINVAL
        for kw in ({"state": None}, {"actions": None}, {"screen": None}, {"r": None}, {"d": None}):
            assert call(kind=kind, **kw) == EINVAL and b"null" in lib.arl_last_error(), kw
        for kw in ({"state": st + 4}, {"actions": ac + 2}, {"screen": sc + 2}, {"r": rw + 2}):
            assert call(kind=kind, **kw) == EINVAL and b"aligned" in lib.arl_last_error(), kw


# ---------------------------------------------------------------- the scripted policy covers what the GPU tests claim
@pytest.mark.parametrize("n,rooms,view,levels,steps,seed,off", M.SCRIPTED_GPU_CASES)
def test_scripted_policy_reaches_every_event_class(n, rooms, view, levels, steps, seed, off):
    """For each (n, rooms, view, levels) that test_gpu_maze.py drives with the scripted policy, within that
    test's step count, the restatement alone shows wins, timeouts, bumps and a move in each of the four
    directions.  A single env follows its BFS path alone (e % 3 == 0), so at n = 1 only the wins and the moves
    of its paths are there: that case checks the one-env launch, not the event classes."""
    ref = M.coverage(n, rooms, view, levels, steps, seed=seed, env_offset=off)
    print(n, rooms, view, levels, "moves", ref.moves, "bumps", ref.bumps, "wins", ref.wins, "timeouts", ref.timeouts)
    assert ref.wins > 0 and sum(ref.moves) > 0
    assert ref.wins == int(ref.state[:, M.WINS].sum()) and ref.timeouts == int(ref.state[:, M.TIMEOUTS].sum())
    if n >= 3:
        assert ref.timeouts > 0 and ref.bumps > 0 and min(ref.moves) > 0
        assert ref.wins >= (n + 2) // 3                       # every BFS env wins within 8R - 10 < steps
