"""CPU: the NumPy restatement of the device-resident Pong (pong_ref.py) does what the header says
from crafted states -- wall bounces, the four hit bins and the misses at both paddles, the clamps,
the opponent's dead zone, the aliased actions, a point in every frame of the skip for each side,
the serve that follows, game over at `points` and at the step cap, the serves counter driving the
draws -- the random-policy return is the recorded constant, and the Pong entry points of the C ABI
validate their arguments on the host, before any launch (fake, never-dereferenced device
pointers; no GPU here).  (The render's chunk function is compiled for the device alone, as the
other games' are, so the painter is compared on the GPU: test_gpu_pong.py.)"""
import os
import re

import numpy as np
import pytest

import pong_ref as P
from conftest import ROOT
from test_catch import make_net

OK, EINVAL, ESTATE = 0, 1, 3
ENV_CATCH, ENV_BREAKOUT, ENV_PONG, GAME_OVER_ONLY = 1, 2, 4, 0x100
PAIR = 2 * 210 * 160 * 3


def pts(p):
    return p << 16


def step_from(row, act, points=3, seed=11, env_offset=5):
    """One env of the restatement from a crafted row, one step -> (ref, pairs, reward, done, new row)."""
    ref = P.PongRef(1, seed=seed, env_offset=env_offset, points=points)
    ref.state[0] = row
    pairs, r, d = ref.step([act])
    return ref, pairs[0], float(r[0]), int(d[0]), [int(x) for x in ref.state[0]]


def crafted(name, **kw):
    row, act = P.crafted_states()[name]
    assert act != "follow"
    return step_from(row, act, **kw)


# ---------------------------------------------------------------- crafted states
def test_wall_bounces():
    ref, _, r, d, s = crafted("top_wall")                  # by 35 -> 32 -> 68 - 32 = 36, then +3 a frame
    assert (s[P.BY], s[P.VY], ref.wall) == (36 + 9, 3, [1, 0]) and r == 0 and d == 0
    ref, _, r, d, s = crafted("bottom_wall")               # by 189 -> 192 -> 380 - 192 = 188, then -3 a frame
    assert (s[P.BY], s[P.VY], ref.wall) == (188 - 9, -3, [0, 1])
    assert s[P.BX] == 80 - 12 and s[P.GAME_STEPS] == 1 and s[P.STEPS] == 1 and s[P.SERVES] == 1


@pytest.mark.parametrize("k,vy", [(0, -3), (1, -1), (2, 1), (3, 3)])
def test_hit_bins_on_both_paddles(k, vy):
    """The ball crosses the face in frame 0: reflected about it, vx toward the other side, vy from the bin;
    three more frames with the new velocity."""
    by0 = 100 + (-3, 3, 8, 15)[k]
    ref, _, r, d, s = crafted("agent_bin%d" % k)
    assert s[P.BX:P.VY + 1] == [272 - 136 - 9, by0 + 3 * vy, -3, vy] and ref.agent_hits[k] == 1 and r == 0
    assert sum(ref.agent_hits) == 1 and sum(ref.opp_hits) == 0 and s[P.PY] == 100
    ref, _, r, d, s = crafted("opp_bin%d" % k)
    assert s[P.BX:P.VY + 1] == [40 - 19 + 9, by0 + 3 * vy, 3, vy] and ref.opp_hits[k] == 1 and r == 0
    assert sum(ref.opp_hits) == 1 and sum(ref.agent_hits) == 0
    assert [P.hit_vy(100 + o, 100) for o in (-2, 1, 2, 5, 6, 9, 10, 13, 40)] == [-3, -3, -1, -1, 1, 1, 3, 3, 3]


@pytest.mark.parametrize("side", ["agent", "opp"])
@pytest.mark.parametrize("edge,by0", [("above", 96), ("below", 116)])
def test_miss_one_row_outside_a_paddle(side, edge, by0):
    """by + 4 == y and by == y + 16 do not touch: the ball goes on with its velocity (no point yet: the
    edge of the screen is 18 columns on)."""
    ref, pairs, r, d, s = crafted("%s_miss_%s" % (side, edge))
    vx = 3 if side == "agent" else -3
    assert s[P.BX:P.VY + 1] == [(136 if side == "agent" else 19) + 3 * vx, by0 + 3, vx, 1]
    assert sum(ref.agent_hits) + sum(ref.opp_hits) == 0 and r == 0 and d == 0
    # the opponent made its moves: toward the ball it missed (100 in frame 0, then 3 more), or from 40 down
    assert s[P.OY] == (40 + 8 if side == "agent" else 94 if edge == "above" else 106)
    assert not (pairs[0] == pairs[1]).all()


def test_paddle_clamps():
    assert crafted("agent_clamp_top")[4][P.PY] == 34 and crafted("agent_clamp_bottom")[4][P.PY] == 178
    assert crafted("opp_clamp_top")[4][P.OY] == 34 and crafted("opp_clamp_bottom")[4][P.OY] == 178


def test_opponent_dead_zone():
    """c = +-2 holds still, +-3 moves (once: the move and the ball's own bring c back inside)."""
    got = {k: crafted("dead_zone_" + k)[4][P.OY] for k in ("p2", "m2", "p3", "m3")}
    assert got == {"p2": 102, "m2": 102, "p3": 104, "m3": 100}


def test_action_aliases_and_noops():
    row = P.crafted_states()["alias_up"][0]
    out = {a: step_from(row, a)[4] for a in range(8)}
    assert out[4] == out[2] and out[5] == out[3]
    assert out[0] == out[1] == out[6] == out[7]
    assert (out[2][P.PY], out[3][P.PY], out[0][P.PY]) == (100 - 16, 100 + 16, 100)
    for name, py in (("alias_up", 84), ("alias_down", 116), ("noop_1", 100), ("noop_6", 100)):
        assert crafted(name)[4][P.PY] == py


@pytest.mark.parametrize("f", range(4))
def test_point_in_every_frame_of_the_skip(f):
    """A point in frame f, scores (1, 2) / (2, 1) of 3: reward, the scorer's count, a serve toward the side
    that conceded with the paddles where frame f left them, both frames of the pair the served screen."""
    ref, pairs, r, d, s = crafted("agent_point_f%d" % f)
    assert r == 1.0 and d == 0 and ref.agent_points == [int(i == f) for i in range(4)]
    assert (s[P.SCORE_AGENT], s[P.SCORE_OPP], s[P.VX], s[P.BX], s[P.SERVES]) == (2, 2, -3, 78, 2)
    assert s[P.OY] == 150 - 2 * (f + 1) and s[P.PY] == 106 and s[P.GAME_STEPS] == 1 and s[P.STEPS] == 1
    assert (pairs[0] == pairs[1]).all() and (pairs[0] == P.render(s[P.BX], s[P.BY], s[P.PY], s[P.OY])).all()
    assert ref.draws == [(5, 1)]
    ref, pairs, r, d, s = crafted("opp_point_f%d" % f)
    assert r == -1.0 and d == 0 and ref.opp_points == [int(i == f) for i in range(4)]
    assert (s[P.SCORE_AGENT], s[P.SCORE_OPP], s[P.VX], s[P.BX], s[P.SERVES]) == (2, 2, 3, 78, 2)
    assert (pairs[0] == pairs[1]).all() and (pairs[0] == P.render(s[P.BX], s[P.BY], s[P.PY], s[P.OY])).all()
    assert 34 <= s[P.BY] <= 190 and s[P.VY] in (-3, -1, 1, 3)


@pytest.mark.parametrize("points", [1, 3, 21])
def test_game_over_exactly_at_points(points):
    """Scores (points - 1, points - 1): one point short is no game over at points + 1; the point is one at
    `points`, for either side -- a new game: paddles at 106, counts 0, game + 1, vx from the draw."""
    for name, who in (("agent_point_f1", "agent"), ("opp_point_f2", "opp")):
        row = P.crafted_states()[name][0].copy()
        row[P.SCORE_AGENT] = row[P.SCORE_OPP] = points - 1
        row[P.GAME], row[P.GAME_STEPS], row[P.STEPS], row[P.SERVES] = 4, 77, 77, 9
        ref, pairs, r, d, s = step_from(row, 0, points=points)
        assert d == 1 and r == (1.0 if who == "agent" else -1.0) and ref.game_overs[who] == 1
        assert s[P.PY:] == [106, 106, 10, 0, 5, 0, 0, 0] and abs(s[P.VX]) == 3 and s[P.BX] == 78
        assert (pairs[0] == pairs[1]).all() and ref.draws == [(5, 9)]
        if points < 21:
            ref, _, r, d, s = step_from(row, 0, points=points + 1)
            assert d == 0 and sum(ref.game_overs.values()) == 0
            assert s[P.GAME] == 4 and s[P.GAME_STEPS] == 78 and s[P.STEPS] == 78
            assert s[P.SCORE_AGENT] + s[P.SCORE_OPP] == 2 * points - 1


def test_step_cap():
    """game_steps 4998 -> 4999 (no game over) -> 5000: game over without a point, reward 0, the new game's
    first screen twice."""
    row, _ = P.crafted_states()["step_cap"]
    ref = P.PongRef(1, seed=3, points=21)
    ref.state[0] = row
    _, r, d = ref.step(P.follow_action(ref.state))
    assert d[0] == 0 and ref.state[0, P.GAME_STEPS] == P.STEP_CAP - 1
    pairs, r, d = ref.step(P.follow_action(ref.state))
    s = ref.state[0]
    assert d[0] == 1 and r[0] == 0 and ref.game_overs == {"agent": 0, "opp": 0, "cap": 1}
    assert (s[P.GAME], s[P.GAME_STEPS], s[P.STEPS], s[P.SERVES]) == (1, 0, 0, 2)
    assert (pairs[0, 0] == pairs[0, 1]).all() and (pairs[0, 0] == P.render(s[P.BX], s[P.BY], 106, 106)).all()


def test_serves_counter_drives_the_draws():
    """The draw of a serve is a function of (env_offset + e, serves, seed) alone; a new game takes vx from
    its third word, a point's serve does not."""
    from oracle import philox4x32
    seed, off = (7 << 32) | 99, 3
    ref = P.PongRef(4, seed=seed, env_offset=off, points=21)
    ref.reset()
    for e in range(4):
        w = [int(x[0]) for x in philox4x32((np.array([off + e], np.uint64), np.zeros(1, np.uint64),
                                            np.zeros(1, np.uint64), np.full(1, 4, np.uint64)), (99, 7))]
        assert list(ref.state[e, :4]) == [78, 34 + w[0] % 157, 3 if w[2] & 1 else -3, 2 * (w[1] % 4) - 3]
        assert list(ref.state[e, 4:]) == [106, 106, 1, 0, 0, 0, 0, 0]
    seen = {tuple(ref.state[e, :4]) for e in range(4)}
    row = P.crafted_states()["agent_point_f0"][0]
    outs = []
    for serves in (1, 2, 1):
        r = row.copy()
        r[P.SERVES] = serves
        outs.append(step_from(r, 0, seed=seed)[4])
    assert outs[0] == outs[2] and outs[0][P.SERVES] == 2 and outs[1][P.SERVES] == 3
    assert outs[0][:4] != outs[1][:4] or len(seen) > 1
    a, b = step_from(row, 0, seed=seed)[4], step_from(row, 0, seed=seed + 1)[4]
    assert a[P.VX] == b[P.VX] == -3 and a[P.SERVES:] == b[P.SERVES:]


def test_painter():
    s = P.render(78, 100, 50, 150)
    assert tuple(s[0, 0]) == P.BG_RGB and tuple(s[209, 159]) == P.BG_RGB and tuple(s[23, 7]) == P.BG_RGB
    for y in (24, 33, 194, 203):
        assert tuple(s[y, 0]) == P.WALL_RGB and tuple(s[y, 159]) == P.WALL_RGB
    assert tuple(s[34, 0]) == P.BG_RGB and tuple(s[193, 0]) == P.BG_RGB and tuple(s[204, 0]) == P.BG_RGB
    assert tuple(s[150, 16]) == P.OPP_RGB and tuple(s[165, 19]) == P.OPP_RGB
    assert tuple(s[149, 16]) == P.BG_RGB and tuple(s[166, 19]) == P.BG_RGB and tuple(s[150, 20]) == P.BG_RGB
    assert tuple(s[50, 140]) == P.AGENT_RGB and tuple(s[65, 143]) == P.AGENT_RGB and tuple(s[50, 144]) == P.BG_RGB
    assert tuple(s[100, 78]) == P.BALL_RGB and tuple(s[103, 81]) == P.BALL_RGB and tuple(s[104, 81]) == P.BG_RGB
    s = P.render(138, 60, 50, 150)                       # the ball over the agent's paddle
    assert tuple(s[60, 140]) == P.BALL_RGB and tuple(s[60, 142]) == P.AGENT_RGB and tuple(s[64, 140]) == P.AGENT_RGB
    assert int((s != np.array(P.BG_RGB, np.uint8)).any(-1).sum()) == 20 * 160 + 2 * 64 + 16 - 8


# ---------------------------------------------------------------- the random policy
def random_games(n, per, points, seed=5):
    """The first `per` games of each of n envs under a uniform random policy over 4 actions (a fixed count
    per env: taking the first games to finish would favour short ones)."""
    env = P.PongRef(n, seed=seed, points=points)
    env.reset()
    rng = np.random.default_rng(2024)
    rew, don, count = [], [], np.zeros(n, int)
    while count.min() < per:
        _, r, d = env.step(rng.integers(0, 4, n), render_pairs=False)
        rew.append(r)
        don.append(d)
        count += d
    rew, don = np.array(rew), np.array(don)
    rets = P.returns_of(rew, don, per)
    lens = np.concatenate([np.diff(np.concatenate(([-1], np.flatnonzero(don[:, e])[:per]))) for e in range(n)])
    return env, rets, lens


def test_random_policy_return_is_the_recorded_constant():
    """4,000 games to 1 point (250 envs x 16) of a uniform random policy: the mean return is the constant
    the measured lr0 = 0 curve is held against (DESIGN.md "Device environment"), with a standard error below
    0.05."""
    env, rets, lens = random_games(250, 16, 1)
    se = rets.std(ddof=1) / np.sqrt(len(rets))
    print("random policy, points = 1: mean %.4f +- %.4f, games of %d..%d steps (mean %.2f)"
          % (rets.mean(), se, lens.min(), lens.max(), lens.mean()))
    assert len(rets) == 4000 and se <= 0.05
    assert set(np.unique(rets)) == {-1.0, 1.0}
    assert abs(rets.mean() - P.RANDOM_MEAN_POINTS1) < 5e-5 and abs(se - P.RANDOM_SE_POINTS1) < 5e-5
    assert -0.6 < P.RANDOM_MEAN_POINTS1 < -0.1                   # the opponent follows the ball, the agent does not
    assert 5 < lens.mean() < 30 and env.game_overs["cap"] == 0
    assert sum(env.agent_hits) > 0 and sum(env.opp_hits) > 0 and min(env.wall) > 0


def test_games_to_three_points_carry_both_signs():
    """points = 3, a following agent against the opponent: returns of both signs inside games, rewards that do
    not end them, and games much longer than a window."""
    env = P.PongRef(8, seed=1, points=3)
    env.reset()
    inner = {1.0: 0, -1.0: 0}
    steps = 0
    while sum(env.game_overs.values()) < 8 and steps < 4000:
        _, r, d = env.step(P.follow_action(env.state), render_pairs=False)
        steps += 1
        for x in r[(r != 0) & (d == 0)]:
            inner[float(x)] += 1
    assert inner[1.0] > 0 and inner[-1.0] > 0 and steps > 8 * 5
    assert all(min(h) >= 0 for h in (env.agent_hits, env.opp_hits)) and sum(env.agent_hits) > 0


# ---------------------------------------------------------------- the C ABI, no device
def test_header_and_table_carry_the_pong_symbols():
    import asyncrl_amd
    from asyncrl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "asyncrl_hip.h")).read()
    assert re.search(r"#define ARL_ENV_PONG 4\b", txt)
    assert re.search(r"#define ARL_ENV_PONG_POINTS\(p\) \(\(p\) << 16\)", txt)
    for s in ("arl_pong_state_bytes", "arl_pong_reset", "arl_pong_step"):
        assert re.search(r"\b%s\s*\(" % s, txt) and hasattr(_lib.lib, s) and s in _lib.SIGNATURES, s
    assert _lib.ENV_PONG == ENV_PONG and _lib.PONG_STATE_INTS == 12 == P.STATE_INTS
    assert _lib.env_pong_points(21) == pts(21)
    lib = _lib.lib
    assert lib.arl_abi_version() == 4
    for n in (0, 1, 35):
        assert lib.arl_pong_state_bytes(n) == 2 * n * 48
    assert lib.arl_pong_state_bytes(-1) == -1
    with pytest.raises(ValueError):
        asyncrl_amd.DevicePong(0, device="cpu")
    for bad in (0, 22, -1):
        with pytest.raises(ValueError):
            asyncrl_amd.DevicePong(3, device="cpu", points=bad)
    env = asyncrl_amd.DevicePong(3, device="cpu", seed=1, env_offset=2, points=5)
    assert env.kind == ENV_PONG | pts(5) and tuple(env.state.shape) == (2, 3, 12) and env.envs == ()
    assert asyncrl_amd.DevicePong(3, device="cpu").kind == ENV_PONG | pts(21)
    assert tuple(env.make_pools(2)[0].shape) == (2, 3, 2, 210, 160, 3)


def test_granular_calls_validate():
    from asyncrl_amd._lib import lib
    f = 1 << 40
    st, pr, rw, dn, ac = f, f + (1 << 30), f + (2 << 30), f + (3 << 30), f + (4 << 30)
    assert lib.arl_pong_reset(st, 0, 0, 0, 0, pr, rw, dn, None) == OK          # nothing to do
    for p in (1, 3, 21):
        assert lib.arl_pong_step(st, 0, ac, 0, 0, 0, p, pr, rw, dn, None) == OK
    for p in (0, 22, -1, GAME_OVER_ONLY, 1 << 16):
        assert lib.arl_pong_step(st, 0, ac, 0, 0, 0, p, pr, rw, dn, None) == EINVAL
        assert b"points" in lib.arl_last_error()
    assert lib.arl_pong_reset(st, 4, 0, 0, 2, pr, rw, dn, None) == EINVAL      # parity
    assert lib.arl_pong_step(st, -1, ac, 4, 0, 0, 1, pr, rw, dn, None) == EINVAL
    assert lib.arl_pong_reset(None, 4, 0, 0, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_pong_reset(st, 4, 0, 0, 0, None, rw, dn, None) == EINVAL
    assert lib.arl_pong_reset(st, 4, 0, 0, 0, pr, None, dn, None) == EINVAL
    assert lib.arl_pong_reset(st, 4, 0, 0, 0, pr, rw, None, None) == EINVAL
    assert lib.arl_pong_reset(st + 4, 4, 0, 0, 0, pr, rw, dn, None) == EINVAL  # misaligned state
    assert lib.arl_pong_reset(st, 4, 0, 0, 0, pr + 4, rw, dn, None) == EINVAL  # misaligned frames
    assert lib.arl_pong_step(st, 0, ac, 4, 0, 0, 1, pr, rw + 2, dn, None) == EINVAL
    assert lib.arl_pong_step(st, 0, None, 4, 0, 0, 1, pr, rw, dn, None) == EINVAL   # no actions
    assert lib.arl_pong_step(st, 0, ac + 2, 4, 0, 0, 1, pr, rw, dn, None) == EINVAL
    assert lib.arl_pong_step(st, 0, ac, 65536, 0, 0, 1, pr, rw, dn, None) == EINVAL
    assert lib.arl_pong_reset(st, 65536, 0, 0, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_pong_step(st, 0, ac, -1, 0, 0, 1, pr, rw, dn, None) == EINVAL


PONG_KINDS = (ENV_PONG, ENV_PONG | pts(1), ENV_PONG | pts(21))
BAD_KINDS = (ENV_PONG | GAME_OVER_ONLY, ENV_PONG | pts(22), ENV_PONG | pts(1) | GAME_OVER_ONLY, ENV_PONG | 0x200,
             ENV_PONG | 0x8000, ENV_PONG | pts(32), ENV_PONG | pts(1 << 8), ENV_PONG | (1 << 31) - (1 << 30),
             -ENV_PONG, ENV_CATCH | pts(1), ENV_BREAKOUT | pts(1), pts(1), 0, 3, 5, 7)


@pytest.mark.parametrize("bind", [False, True])
def test_set_env_validation(bind):
    """Kind 4 with p in {0, 1, 21} attaches to FF, LSTM and Nature nets with A in {4, 6}, on an unbound and
    on a (fake-)bound handle; frames-flag nets are ARL_ESTATE; A = 3, a misaligned state, 4 | 0x100, p = 22
    and every other bit are ARL_EINVAL with "kind" in the text; Catch and Breakout attach as before."""
    from asyncrl_amd._lib import lib
    state = (1 << 40) + (5 << 30)
    for arch in (16, 17, 32, 33, 64):                       # RGB / STACK / STATES nets take no frame pairs
        h = make_net(arch, 4, bind=bind)
        try:
            for kind in PONG_KINDS:
                assert lib.arl_net_set_env(h, kind, state) == ESTATE, arch
                assert lib.arl_net_set_env(h, kind, None) == OK       # detaching nothing is fine
        finally:
            lib.arl_net_destroy(h)
    h = make_net(0, 3, bind=bind)
    try:
        for kind in PONG_KINDS:
            assert lib.arl_net_set_env(h, kind, state) == EINVAL      # n_actions = 3
            assert b"n_actions" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)
    for arch in (0, 1, 2):
        for A in (4, 6):
            h = make_net(arch, A, bind=bind)
            try:
                for kind in PONG_KINDS:
                    assert lib.arl_net_set_env(h, kind, state + 4) == EINVAL     # misaligned
                    assert lib.arl_net_set_env(h, kind, state) == OK
                for bad in BAD_KINDS:
                    assert lib.arl_net_set_env(h, bad, state) == EINVAL, bad
                    assert b"kind" in lib.arl_last_error()
                    assert lib.arl_net_set_env(h, bad, None) == EINVAL, bad
                if not bind:
                    assert lib.arl_env_step(h, 0, 0, 4, state, state, state, 2, None) == ESTATE   # not bound
                assert lib.arl_net_set_env(h, ENV_PONG, None) == OK
                for kind in (ENV_CATCH, ENV_BREAKOUT, ENV_BREAKOUT | GAME_OVER_ONLY):        # as before
                    assert lib.arl_net_set_env(h, kind, state) == OK
                    assert lib.arl_net_set_env(h, kind, None) == OK
            finally:
                lib.arl_net_destroy(h)
    assert lib.arl_net_set_env(None, ENV_PONG, state) == EINVAL


@pytest.mark.parametrize("kind", PONG_KINDS)
def test_env_calls_fail_before_any_launch(kind):
    """arl_env_reset / arl_env_step / arl_run_window with a Pong attached: pool_len = 1, unregistered or too
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
