"""CPU: the NumPy restatement of the device-resident T-maze (tmaze_ref.py) does what the header says
-- episodes of L + 1 env-steps for every L, the three outcomes and their counters for all six action
values at the junction, the cue as a function of (seed, env id, episode) through the oracle's Philox,
the painter --, the FF model is blind at the junction exactly from L = 4 on (the 4-plane stack of the
oracle's phi is byte-identical for the two cues; for L <= 3 it differs), the cues, the floor and the
agent survive the luminance and the resize, and the T-maze entry points of the C ABI validate their
arguments on the host, before any launch (fake, never-dereferenced device pointers; no GPU here).
(The render's chunk function is compiled for the device alone, as the other games' are, so the
painter is compared on the GPU: test_gpu_tmaze.py.)"""
import os
import re

import numpy as np
import pytest

import tmaze_ref as M
from conftest import ROOT
from test_catch import make_net

OK, EINVAL, ESTATE = 0, 1, 3
ENV_CATCH, ENV_BREAKOUT, ENV_PONG, ENV_TMAZE, GAME_OVER_ONLY = 1, 2, 4, 8, 0x100
PAIR = 2 * 210 * 160 * 3
LENGTHS = range(1, 9)


def ln(length):
    return length << 16


# ---------------------------------------------------------------- the restatement's own invariants
@pytest.mark.parametrize("length", LENGTHS)
def test_every_episode_lasts_length_plus_one_steps(length):
    """3 envs, 4 episodes each, actions 0..5 in turn: done exactly at env-steps L, 2L + 1, ...; reward 0 and
    the agent at ax = 4 + 16 pos on every corridor step, its pair the screens after frames 4 and 3, no cue on
    either; the step after a terminal shows the next episode's first screen twice, with its cue."""
    n = 3
    ref = M.TMazeRef(n, seed=7, env_offset=2, length=length)
    pairs, r, d = ref.reset()
    assert not r.any() and not d.any()
    for e in range(n):
        assert (pairs[e, 0] == pairs[e, 1]).all()
        assert (pairs[e, 0] == M.render(4, length, int(ref.state[e, M.CUE_BIT]))).all()
    for t in range(4 * (length + 1)):
        phase = t % (length + 1)
        pairs, r, d = ref.step(M.cycle_actions(n, t))
        if phase < length:
            assert not r.any() and not d.any()
            assert list(ref.state[:, M.POS]) == [phase + 1] * n and list(ref.state[:, M.STEPS]) == [phase + 1] * n
            for e in range(n):
                assert (pairs[e, 0] == M.render(4 + 16 * (phase + 1), length)).all()
                assert (pairs[e, 1] == M.render(16 * (phase + 1), length)).all()
        else:
            assert d.all() and list(ref.state[:, M.POS]) == [0] * n and list(ref.state[:, M.STEPS]) == [0] * n
            assert list(ref.state[:, M.EPISODE]) == [t // (length + 1) + 1] * n
            for e in range(n):
                assert (pairs[e, 0] == pairs[e, 1]).all()
                assert (pairs[e, 0] == M.render(4, length, int(ref.state[e, M.CUE_BIT]))).all()
    assert ref.corridor_steps == 4 * length * n and sum(ref.junctions.values()) == 4 * n
    assert (ref.state[:, M.LENGTH] == length).all()
    assert (ref.state[:, M.HITS] + ref.state[:, M.MISSES] + ref.state[:, M.LAPSES] == 4).all()


@pytest.mark.parametrize("cue", [0, 1])
@pytest.mark.parametrize("act", range(6))
def test_junction_rewards_and_counters(cue, act):
    """Every action value at the junction, for each cue: +1 for the cue's arm, -1 for the other, 0 for no
    choice, done in all three, exactly one of the three counters advancing; in the corridor the same action
    changes nothing."""
    ref = M.TMazeRef(1, seed=3, length=2)
    ref.reset()
    ref.state[0, M.CUE_BIT] = cue
    for _ in range(2):
        _, r, d = ref.step([act])
        assert r[0] == 0 and d[0] == 0 and list(ref.state[0, M.HITS:]) == [0, 0, 0]
    _, r, d = ref.step([act])
    want = 0.0 if act not in (2, 3) else 1.0 if act - 2 == cue else -1.0
    assert d[0] == 1 and r[0] == want and r.dtype == np.float32
    assert list(ref.state[0, M.HITS:]) == [int(want > 0), int(want < 0), int(want == 0)]
    assert ref.state[0, M.EPISODE] == 1 and ref.choices == {(cue, act): 1}
    assert ref.junctions == {"hit": int(want > 0), "miss": int(want < 0), "lapse": int(want == 0)}


def test_cue_is_a_function_of_seed_env_and_episode():
    """cue = w0 & 1 of the oracle's Philox at counter (env_offset + e, episode, 0, 5), key = the seed's two
    halves: the reset draws episode 0, every terminal the next; both cues occur; the draw does not depend on
    what was played."""
    from oracle import philox4x32
    seed, off, n = (7 << 32) | 99, 3, 16

    def want(e, ep):
        w = philox4x32((np.array([off + e], np.uint64), np.array([ep], np.uint64), np.zeros(1, np.uint64),
                        np.full(1, 5, np.uint64)), (99, 7))
        return int(w[0][0]) & 1

    ref = M.TMazeRef(n, seed=seed, env_offset=off, length=1)
    ref.reset()
    seen = []
    for ep in range(6):
        assert [int(c) for c in ref.state[:, M.CUE_BIT]] == [want(e, ep) for e in range(n)]
        seen += [int(c) for c in ref.state[:, M.CUE_BIT]]
        ref.step(M.cycle_actions(n, ep))
        ref.step(M.cycle_actions(n, ep))
    assert ref.draws == [(off + e, ep) for ep in range(7) for e in range(n)]
    assert 0.25 < np.mean(seen) < 0.75                        # 96 fair bits
    other = M.TMazeRef(n, seed=seed, env_offset=off, length=8)
    other.reset()
    assert (other.state[:, M.CUE_BIT] == [want(e, 0) for e in range(n)]).all()
    assert M.cue_of(seed, off + 2, 5) == want(2, 5)
    shifted = M.TMazeRef(n, seed=seed + 1, env_offset=off, length=1)
    shifted.reset()
    cues = [[M.cue_of(s, e, ep) for e in range(8) for ep in range(8)] for s in (seed, seed + 1)]
    assert cues[0] != cues[1]


def test_painter():
    for length in LENGTHS:
        s = M.render(4 + 16 * length, length)
        xl = 16 * length
        assert tuple(s[96, 0]) == M.FLOOR_RGB and tuple(s[111, xl + 15]) == M.FLOOR_RGB
        assert tuple(s[95, 0]) == (0, 0, 0) and tuple(s[112, xl - 1]) == (0, 0, 0)
        assert tuple(s[48, xl]) == M.FLOOR_RGB and tuple(s[159, xl + 15]) == M.FLOOR_RGB
        assert tuple(s[47, xl]) == (0, 0, 0) and tuple(s[160, xl]) == (0, 0, 0)
        assert tuple(s[48, xl - 1]) == (0, 0, 0) and tuple(s[48, xl + 16]) == (0, 0, 0)
        assert tuple(s[100, xl + 4]) == M.AGENT_RGB and tuple(s[107, xl + 11]) == M.AGENT_RGB
        assert tuple(s[99, xl + 4]) == M.FLOOR_RGB and tuple(s[100, xl + 12]) == M.FLOOR_RGB
        grey = 16 * (xl + 16) + (112 - 16) * 16 - 64
        assert int((s == np.array(M.FLOOR_RGB, np.uint8)).all(-1).sum()) == grey
        assert int((s != 0).any(-1).sum()) == grey + 64
    up, down = M.render(4, 4, 0), M.render(4, 4, 1)
    assert tuple(up[72, 0]) == M.CUE_RGB[0] and tuple(up[87, 15]) == M.CUE_RGB[0]
    assert tuple(up[71, 0]) == (0, 0, 0) and tuple(up[88, 0]) == (0, 0, 0) and tuple(up[72, 16]) == (0, 0, 0)
    assert tuple(down[120, 0]) == M.CUE_RGB[1] and tuple(down[135, 15]) == M.CUE_RGB[1]
    assert tuple(down[119, 0]) == (0, 0, 0) and tuple(down[136, 15]) == (0, 0, 0)
    assert int((up != M.render(4, 4)).any(-1).sum()) == 256 == int((down != M.render(4, 4)).any(-1).sum())
    assert int((up != down).any(-1).sum()) == 512


# ---------------------------------------------------------------- what the models can see
def junction_stack(length, cue, mode=0):
    """The 4-plane stack (4, 84, 84) uint8 of the oracle's phi at the junction observation of an episode that
    started on a reset flag: observation 0 resets the stack (three zero planes), every later one pushes."""
    import oracle as O
    stack = None
    for j, pair in enumerate(M.episode_pairs(length, cue)):
        stack = O.stack_push(stack, O.current_screen(pair[0], pair[1], mode), reset=(j == 0))
    return stack


@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("length", LENGTHS)
def test_ff_blindness_from_length_four_on(length, mode):
    """The condition the FF learning check of test_gpu_tmaze.py rests on, for all four resize modes: for
    L >= 4 the stack the FF model acts on at the junction is byte-identical for cue 0 and cue 1, so its action
    there cannot depend on the cue and its expected return is exactly 0; for L <= 3 the cue's plane is still
    in the stack and the two differ."""
    a, b = junction_stack(length, 0, mode), junction_stack(length, 1, mode)
    assert a.shape == b.shape == (4, 84, 84) and a.dtype == np.uint8
    if length >= 4:
        assert a.tobytes() == b.tobytes()
        assert a[0].any()                                     # four real planes: the reset's zeros have left too
    else:
        assert a.tobytes() != b.tobytes()
        assert (a[3 - length] != b[3 - length]).any()         # in the cue's plane,
        assert (a[4 - length:] == b[4 - length:]).all()       # and in no later one


@pytest.mark.parametrize("mode", range(4))
def test_luminance_keeps_cues_floor_and_agent_apart_from_the_background(mode):
    """On the 84 x 84 plane of the oracle's phi the two cues, the floor and the agent are each brighter than
    the background by a wide margin, and the two cues differ from each other in place and in level."""
    import oracle as O
    lum = {k: int(O.luminance_u8(np.array(v, np.uint8).reshape(1, 1, 3))[0, 0])
           for k, v in (("up", M.CUE_RGB[0]), ("down", M.CUE_RGB[1]), ("floor", M.FLOOR_RGB), ("agent", M.AGENT_RGB))}
    print("luminance:", lum)
    assert min(lum.values()) >= 60 and len(set(lum.values())) == 4
    bare = M.render(4, 4)
    planes = {k: O.current_screen(s, s, mode) for k, s in (("bare", bare), ("up", M.render(4, 4, 0)),
                                                            ("down", M.render(4, 4, 1)))}
    empty = O.current_screen(np.zeros_like(bare), np.zeros_like(bare), mode)
    assert not empty.any()
    for k in ("up", "down"):
        diff = planes[k].astype(int) - planes["bare"].astype(int)
        assert (diff >= 0).all() and int((diff >= lum[k] - 2).sum()) >= 25, (k, int(diff.max()))
    only_up = (planes["up"] != planes["bare"]).any(1)
    only_down = (planes["down"] != planes["bare"]).any(1)
    assert not (only_up & only_down).any() and np.flatnonzero(only_up).max() < np.flatnonzero(only_down).min()
    p = planes["bare"]
    assert int((p == lum["floor"]).sum()) >= 100 and int((p == lum["agent"]).sum()) >= 4
    assert int((p == 0).sum()) >= 84 * 84 // 2
    moved = O.current_screen(M.render(20, 4), M.render(20, 4), mode)
    assert (moved != p).any()                                 # the agent's position shows


# ---------------------------------------------------------------- the C ABI, no device
def test_header_and_table_carry_the_tmaze_symbols():
    import asyncrl_amd
    from asyncrl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "asyncrl_hip.h")).read()
    assert re.search(r"#define ARL_ENV_TMAZE 8\b", txt)
    assert re.search(r"#define ARL_ENV_TMAZE_LENGTH\(l\) \(\(l\) << 16\)", txt)
    for s in ("arl_tmaze_state_bytes", "arl_tmaze_reset", "arl_tmaze_step"):
        assert re.search(r"\b%s\s*\(" % s, txt) and hasattr(_lib.lib, s) and s in _lib.SIGNATURES, s
    assert _lib.ENV_TMAZE == ENV_TMAZE and _lib.TMAZE_STATE_INTS == 8 == M.STATE_INTS
    assert _lib.TMAZE_LENGTH_MAX == 8 == M.LENGTH_MAX and _lib.env_tmaze_length(8) == ln(8)
    lib = _lib.lib
    assert lib.arl_abi_version() == 4
    for n in (0, 1, 35):
        assert lib.arl_tmaze_state_bytes(n) == 2 * n * 32
    assert lib.arl_tmaze_state_bytes(-1) == -1
    with pytest.raises(ValueError):
        asyncrl_amd.DeviceTMaze(0, device="cpu")
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            asyncrl_amd.DeviceTMaze(3, device="cpu", length=bad)
    env = asyncrl_amd.DeviceTMaze(3, device="cpu", seed=1, env_offset=2, length=6)
    assert env.kind == ENV_TMAZE | ln(6) and tuple(env.state.shape) == (2, 3, 8) and env.envs == ()
    assert asyncrl_amd.DeviceTMaze(3, device="cpu").kind == ENV_TMAZE | ln(4)
    assert tuple(env.make_pools(2)[0].shape) == (2, 3, 2, 210, 160, 3)
    with pytest.raises(ValueError):
        env.step_screen([0, 0])                               # 3 envs


def test_granular_calls_validate():
    from asyncrl_amd._lib import lib
    f = 1 << 40
    st, pr, rw, dn, ac = f, f + (1 << 30), f + (2 << 30), f + (3 << 30), f + (4 << 30)
    for length in (1, 4, 8):
        assert lib.arl_tmaze_reset(st, 0, 0, 0, length, 0, pr, rw, dn, None) == OK      # nothing to do
        assert lib.arl_tmaze_step(st, 0, ac, 0, 0, 0, length, pr, rw, dn, None) == OK
    for length in (0, 9, -1, GAME_OVER_ONLY, 1 << 16):
        assert lib.arl_tmaze_reset(st, 0, 0, 0, length, 0, pr, rw, dn, None) == EINVAL
        assert b"length" in lib.arl_last_error()
        assert lib.arl_tmaze_step(st, 0, ac, 0, 0, 0, length, pr, rw, dn, None) == EINVAL
        assert b"length" in lib.arl_last_error()
        assert lib.arl_tmaze_reset(st, 4, 0, 0, length, 0, pr, rw, dn, None) == EINVAL
        assert lib.arl_tmaze_step(st, 0, ac, 4, 0, 0, length, pr, rw, dn, None) == EINVAL
    assert lib.arl_tmaze_reset(st, 4, 0, 0, 4, 2, pr, rw, dn, None) == EINVAL      # parity
    assert lib.arl_tmaze_step(st, -1, ac, 4, 0, 0, 4, pr, rw, dn, None) == EINVAL
    assert lib.arl_tmaze_reset(None, 4, 0, 0, 4, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_tmaze_reset(st, 4, 0, 0, 4, 0, None, rw, dn, None) == EINVAL
    assert lib.arl_tmaze_reset(st, 4, 0, 0, 4, 0, pr, None, dn, None) == EINVAL
    assert lib.arl_tmaze_reset(st, 4, 0, 0, 4, 0, pr, rw, None, None) == EINVAL
    assert lib.arl_tmaze_reset(st + 4, 4, 0, 0, 4, 0, pr, rw, dn, None) == EINVAL  # misaligned state
    assert lib.arl_tmaze_reset(st, 4, 0, 0, 4, 0, pr + 4, rw, dn, None) == EINVAL  # misaligned frames
    assert lib.arl_tmaze_step(st, 0, ac, 4, 0, 0, 4, pr, rw + 2, dn, None) == EINVAL
    assert lib.arl_tmaze_step(st, 0, None, 4, 0, 0, 4, pr, rw, dn, None) == EINVAL   # no actions
    assert lib.arl_tmaze_step(st, 0, ac + 2, 4, 0, 0, 4, pr, rw, dn, None) == EINVAL
    assert lib.arl_tmaze_step(st, 0, ac, 65536, 0, 0, 4, pr, rw, dn, None) == EINVAL
    assert lib.arl_tmaze_reset(st, 65536, 0, 0, 4, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_tmaze_step(st, 0, ac, -1, 0, 0, 4, pr, rw, dn, None) == EINVAL
    assert lib.arl_tmaze_step(st, 0, ac, 0, 0, 0, 4, pr, rw, dn, None) == OK        # n = 0


TMAZE_KINDS = (ENV_TMAZE, ENV_TMAZE | ln(1), ENV_TMAZE | ln(4), ENV_TMAZE | ln(8))
BAD_KINDS = (ENV_TMAZE | GAME_OVER_ONLY, ENV_TMAZE | ln(9), ENV_TMAZE | 0x200, ENV_TMAZE | ln(4) | GAME_OVER_ONLY,
             ENV_TMAZE | 0x8000, ENV_TMAZE | ln(16), ENV_TMAZE | ln(1 << 8), ENV_TMAZE | (1 << 31) - (1 << 30),
             -ENV_TMAZE, ENV_TMAZE | ENV_CATCH, ENV_TMAZE | ENV_BREAKOUT, ENV_TMAZE | ENV_PONG, ENV_CATCH | ln(1),
             ENV_BREAKOUT | ln(1), ln(1), 0, 3, 5, 7, 16)
OTHER_KINDS = (ENV_CATCH, ENV_BREAKOUT, ENV_BREAKOUT | GAME_OVER_ONLY, ENV_PONG, ENV_PONG | (1 << 16),
               ENV_PONG | (21 << 16))


@pytest.mark.parametrize("bind", [False, True])
def test_set_env_validation(bind):
    """Kind 8 with l in {0, 1, 4, 8} attaches to FF, LSTM and Nature nets with A in {4, 6}, on an unbound
    and on a (fake-)bound handle; frames-flag nets are ARL_ESTATE; A = 3, a misaligned state, 8 | 0x100,
    l = 9, 8 | 0x200 and every other bit are ARL_EINVAL with "kind" in the text; the other three kinds attach
    as before."""
    from asyncrl_amd._lib import lib
    state = (1 << 40) + (5 << 30)
    for arch in (16, 17, 32, 33, 64):                       # RGB / STACK / STATES nets take no frame pairs
        h = make_net(arch, 4, bind=bind)
        try:
            for kind in TMAZE_KINDS:
                assert lib.arl_net_set_env(h, kind, state) == ESTATE, arch
                assert lib.arl_net_set_env(h, kind, None) == OK       # detaching nothing is fine
        finally:
            lib.arl_net_destroy(h)
    h = make_net(0, 3, bind=bind)
    try:
        for kind in TMAZE_KINDS:
            assert lib.arl_net_set_env(h, kind, state) == EINVAL      # n_actions = 3
            assert b"n_actions" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)
    for arch in (0, 1, 2):
        for A in (4, 6):
            h = make_net(arch, A, bind=bind)
            try:
                for kind in TMAZE_KINDS:
                    assert lib.arl_net_set_env(h, kind, state + 4) == EINVAL     # misaligned
                    assert lib.arl_net_set_env(h, kind, state) == OK
                for bad in BAD_KINDS:
                    assert lib.arl_net_set_env(h, bad, state) == EINVAL, bad
                    assert b"kind" in lib.arl_last_error()
                    assert lib.arl_net_set_env(h, bad, None) == EINVAL, bad
                if not bind:
                    assert lib.arl_env_step(h, 0, 0, 4, state, state, state, 2, None) == ESTATE   # not bound
                assert lib.arl_net_set_env(h, ENV_TMAZE, None) == OK
                for kind in OTHER_KINDS:                                                          # as before
                    assert lib.arl_net_set_env(h, kind, state) == OK
                    assert lib.arl_net_set_env(h, kind, None) == OK
            finally:
                lib.arl_net_destroy(h)
    assert lib.arl_net_set_env(None, ENV_TMAZE, state) == EINVAL


@pytest.mark.parametrize("kind", TMAZE_KINDS)
def test_env_calls_fail_before_any_launch(kind):
    """arl_env_reset / arl_env_step / arl_run_window with a T-maze attached: pool_len = 1, unregistered or too
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
            assert lib.arl_net_set_env(h, ENV_TMAZE, state) == ESTATE
            assert lib.arl_net_set_env_direct(h, 1) == ESTATE and b"frame pairs" in lib.arl_last_error()
        finally:
            lib.arl_net_destroy(h)
    for arch in (0, 1, 2):
        h = make_net(arch, 4, bind=bind)
        try:
            assert lib.arl_net_set_env_direct(h, 1) == ESTATE and b"no env" in lib.arl_last_error()
            for kind in TMAZE_KINDS:
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

    def call(kind=ENV_TMAZE, state=st, parity=0, actions=ac, n=4, mode=0, screen=sc, r=rw, d=dn):
        return lib.arl_env_step_screen(kind, state, parity, actions, n, 0, 0, mode, screen, r, d, None)

    for kind in TMAZE_KINDS + OTHER_KINDS:
        for mode in range(4):
            assert call(kind=kind, n=0, mode=mode) == OK                  # nothing to do
    for bad in BAD_KINDS:
        assert call(kind=bad) == EINVAL and b"kind" in lib.arl_last_error(), bad
        assert call(kind=bad, n=0) == EINVAL
    for kind in TMAZE_KINDS:
        for mode in (-1, 4, 7):
            assert call(kind=kind, mode=mode) == EINVAL and b"resize_mode" in lib.arl_last_error()
        for parity in (-1, 2):
            assert call(kind=kind, parity=parity) == EINVAL and b"parity" in lib.arl_last_error()
        assert call(kind=kind, n=-1) == EINVAL and call(kind=kind, n=65536) == EINVAL
        for kw in ({"state": None}, {"actions": None}, {"screen": None}, {"r": None}, {"d": None}):
            assert call(kind=kind, **kw) == EINVAL and b"null" in lib.arl_last_error(), kw
        for kw in ({"state": st + 4}, {"actions": ac + 2}, {"screen": sc + 2}, {"r": rw + 2}):
            assert call(kind=kind, **kw) == EINVAL and b"aligned" in lib.arl_last_error(), kw
