"""CPU: the NumPy restatement of the device-resident Breakout (breakout_ref.py) keeps the game's
invariants, the random-policy mean per life is the recorded constant, the two done modes differ
in nothing but the done byte and the per-episode step counter, and the Breakout entry points of
the C ABI validate their arguments on the host, before any launch (fake, never-dereferenced
device pointers; no GPU here)."""
import os
import re

import numpy as np
import pytest

import breakout_ref as B
from conftest import ROOT
from test_catch import make_net

OK, EINVAL, ESTATE = 0, 1, 3
ENV_CATCH, ENV_BREAKOUT, GAME_OVER_ONLY = 1, 2, 0x100
PAIR = 2 * 210 * 160 * 3


def random_lives(n, per, seed=5, life_loss_terminal=True):
    """The first `per` life-episodes of each of n envs under a uniform random policy over 4
    actions (a fixed count per env: taking the first lives to finish would favour short ones)."""
    env = B.BreakoutRef(n, seed=seed, life_loss_terminal=life_loss_terminal)
    env.reset()
    rng = np.random.default_rng(2024)
    rets, lens = [[] for _ in range(n)], [[] for _ in range(n)]
    acc, ln = np.zeros(n), np.zeros(n, int)
    while min(len(x) for x in rets) < per:
        _, r, d = env.step(rng.integers(0, 4, n), render_pairs=False)
        acc += r
        ln += 1
        for e in np.flatnonzero(d):
            rets[e].append(acc[e])
            lens[e].append(ln[e])
            acc[e] = ln[e] = 0
    return env, np.array([x[:per] for x in rets]).ravel(), np.array([x[:per] for x in lens]).ravel()


def test_random_policy_mean_is_the_recorded_constant():
    """5,000 lives (250 envs x 20) of a uniform random policy: the mean raw return per life is
    the constant "has not learned" is measured against; most lives score nothing and a life lasts
    at least the 6 env-steps the served ball needs to fall from row 100 to the paddle."""
    env, rets, lens = random_lives(250, 20)
    print("random policy: mean %.4f stdev %.4f, %.1f %% zero, lives of %d..%d steps (mean %.2f)"
          % (rets.mean(), rets.std(ddof=1), 100 * (rets == 0).mean(), lens.min(), lens.max(), lens.mean()))
    assert len(rets) == 5000
    assert abs(rets.mean() - B.RANDOM_MEAN_PER_LIFE) < 5e-5
    assert 0.10 < B.RANDOM_MEAN_PER_LIFE < 0.20 and (rets == 0).mean() > 0.8
    assert lens.min() == 6 and lens.max() > 2 * 6           # (and some lives see the paddle return the ball)
    assert B.SERVE_Y + 4 * (4 * 5 + 1) + 4 < 190 <= B.SERVE_Y + 4 * (4 * 5 + 2) + 4    # the 6th step's 2nd frame
    assert env.game_overs["lives"] > 0 and env.life_losses >= 5000


def test_brick_bit_layout_and_render():
    """Bit i = 20 r + c lives in word i >> 5, bit i & 31; brick (r, c) covers columns 8c..8c+7
    and rows 57+6r..62+6r in its row's colour; the ball covers anything under it."""
    assert B.words_of(B.ALL_BRICKS) == [-1, -1, -1, 0x00ffffff]
    for r, c in ((0, 0), (1, 11), (1, 12), (3, 3), (4, 15), (4, 16), (5, 19)):
        i = 20 * r + c
        words = np.array(B.words_of(B.brick_bit(r, c)), np.int32).view(np.uint32)
        assert [int(w) for w in words] == [(1 << (i & 31)) if w == i >> 5 else 0 for w in range(4)], (r, c)
        row = B.make_state(0, 100, 1, 4, bricks=B.brick_bit(r, c))
        assert B.bricks_of(row) == B.brick_bit(r, c) and row[B.LEFT] == 1
        s = B.render(0, 100, 0, B.brick_bit(r, c))
        ys, xs = np.nonzero(s[:150].any(-1) & ~(s[:150] == B.BALL_RGB).all(-1))
        assert (ys.min(), ys.max(), xs.min(), xs.max()) == (57 + 6 * r, 62 + 6 * r, 8 * c, 8 * c + 7)
        assert tuple(s[57 + 6 * r, 8 * c]) == B.ROW_RGB[r]
    s = B.render(10, 60, 72, B.ALL_BRICKS)
    assert tuple(s[60, 10]) == B.BALL_RGB and tuple(s[63, 13]) == B.BALL_RGB and tuple(s[64, 13]) == B.ROW_RGB[1]
    assert tuple(s[56, 0]) == (0, 0, 0) and tuple(s[93, 0]) == (0, 0, 0) and tuple(s[92, 159]) == B.ROW_RGB[5]
    assert tuple(s[190, 72]) == B.PADDLE_RGB and tuple(s[193, 87]) == B.PADDLE_RGB and tuple(s[194, 72]) == (0, 0, 0)
    s = B.render(70, 188, 72, 0)                       # the ball over the paddle
    assert tuple(s[190, 72]) == B.BALL_RGB and tuple(s[190, 74]) == B.PADDLE_RGB
    assert B.ROW_VALUE == (7, 7, 4, 4, 1, 1)


def test_the_two_done_modes_agree_in_everything_but_done():
    """The same actions through life_loss_terminal True and False: pairs, rewards and every state
    word but steps_in_episode are equal; the dones of the False arm are exactly the game overs."""
    n, steps = 6, 60
    rng = np.random.default_rng(3)
    a, b = B.BreakoutRef(n, seed=9), B.BreakoutRef(n, seed=9, life_loss_terminal=False)
    out_a, out_b = a.reset(), b.reset()
    keep = [i for i in range(B.STATE_INTS) if i != B.STEPS]
    lost_only = 0
    for t in range(steps):
        assert (out_a[0] == out_b[0]).all() and (out_a[1] == out_b[1]).all()
        assert (a.state[:, keep] == b.state[:, keep]).all()
        acts = rng.integers(0, 6, n)
        out_a, out_b = a.step(acts, render_pairs=t % 7 == 0), b.step(acts, render_pairs=t % 7 == 0)
        if t % 7:
            out_a, out_b = (np.zeros(1),) + out_a[1:], (np.zeros(1),) + out_b[1:]
        assert (out_a[2] == (a.lost | a.over)).all() and (out_b[2] == b.over).all() and (a.over == b.over).all()
        lost_only += int((a.lost & ~a.over).sum())
    assert lost_only > 0 and a.game_overs["lives"] > 0           # both kinds of terminal occurred
    assert (a.state[:, B.STEPS] != b.state[:, B.STEPS]).any()


def test_header_and_table_carry_the_breakout_symbols():
    from asyncrl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "asyncrl_hip.h")).read()
    assert re.search(r"#define ARL_ENV_BREAKOUT 2\b", txt) and re.search(r"#define ARL_ENV_GAME_OVER_ONLY 0x100\b", txt)
    for s in ("arl_breakout_state_bytes", "arl_breakout_reset", "arl_breakout_step"):
        assert re.search(r"\b%s\s*\(" % s, txt) and hasattr(_lib.lib, s) and s in _lib.SIGNATURES, s
    assert _lib.ENV_BREAKOUT == ENV_BREAKOUT and _lib.BREAKOUT_STATE_INTS == 16 == B.STATE_INTS
    assert _lib.ENV_GAME_OVER_ONLY == GAME_OVER_ONLY
    lib = _lib.lib
    assert lib.arl_abi_version() == 4
    for n in (0, 1, 35):
        assert lib.arl_breakout_state_bytes(n) == 2 * n * 64
    assert lib.arl_breakout_state_bytes(-1) == -1


def test_granular_calls_validate():
    from asyncrl_amd._lib import lib
    f = 1 << 40
    st, pr, rw, dn, ac = f, f + (1 << 30), f + (2 << 30), f + (3 << 30), f + (4 << 30)
    assert lib.arl_breakout_reset(st, 0, 0, 0, 0, pr, rw, dn, None) == OK          # nothing to do
    assert lib.arl_breakout_step(st, 0, ac, 0, 0, 0, 0, pr, rw, dn, None) == OK
    assert lib.arl_breakout_step(st, 0, ac, 0, 0, 0, GAME_OVER_ONLY, pr, rw, dn, None) == OK
    assert lib.arl_breakout_step(st, 0, ac, 0, 0, 0, 1, pr, rw, dn, None) == EINVAL and b"flags" in lib.arl_last_error()
    assert lib.arl_breakout_reset(st, 4, 0, 0, 2, pr, rw, dn, None) == EINVAL      # parity
    assert lib.arl_breakout_step(st, -1, ac, 4, 0, 0, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_breakout_reset(None, 4, 0, 0, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_breakout_reset(st + 4, 4, 0, 0, 0, pr, rw, dn, None) == EINVAL  # misaligned state
    assert lib.arl_breakout_reset(st, 4, 0, 0, 0, pr + 4, rw, dn, None) == EINVAL  # misaligned frames
    assert lib.arl_breakout_step(st, 0, None, 4, 0, 0, 0, pr, rw, dn, None) == EINVAL   # no actions
    assert lib.arl_breakout_step(st, 0, ac, 65536, 0, 0, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_breakout_step(st, 0, ac, -1, 0, 0, 0, pr, rw, dn, None) == EINVAL


@pytest.mark.parametrize("bind", [False, True])
def test_set_env_validation(bind):
    """Kind 2 and 2 | 0x100 attach to FF, LSTM and Nature nets with A >= 4, on an unbound and on a
    (fake-)bound handle; frames-flag nets are ARL_ESTATE; A = 3, a misaligned state, kind 7 and
    Catch | 0x100 are ARL_EINVAL."""
    from asyncrl_amd._lib import lib
    state = (1 << 40) + (5 << 30)
    kinds = (ENV_BREAKOUT, ENV_BREAKOUT | GAME_OVER_ONLY)
    for arch in (16, 17, 32, 33, 64):                       # RGB / STACK / STATES nets take no frame pairs
        h = make_net(arch, 4, bind=bind)
        try:
            for kind in kinds:
                assert lib.arl_net_set_env(h, kind, state) == ESTATE, arch
                assert lib.arl_net_set_env(h, kind, None) == OK       # detaching nothing is fine
        finally:
            lib.arl_net_destroy(h)
    h = make_net(0, 3, bind=bind)
    try:
        for kind in kinds:
            assert lib.arl_net_set_env(h, kind, state) == EINVAL      # n_actions = 3
            assert b"n_actions" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)
    for arch, A in ((0, 4), (1, 6), (2, 4)):
        h = make_net(arch, A, bind=bind)
        try:
            for kind in kinds:
                assert lib.arl_net_set_env(h, kind, state + 4) == EINVAL     # misaligned
                assert lib.arl_net_set_env(h, kind, state) == OK
            for bad in (7, ENV_CATCH | GAME_OVER_ONLY, ENV_BREAKOUT | 0x200, 0, 3, 7 | GAME_OVER_ONLY):
                assert lib.arl_net_set_env(h, bad, state) == EINVAL, bad
                assert lib.arl_net_set_env(h, bad, None) == EINVAL, bad
            assert b"kind" in lib.arl_last_error()
            if not bind:
                assert lib.arl_env_step(h, 0, 0, 4, state, state, state, 2, None) == ESTATE   # not bound
            assert lib.arl_net_set_env(h, ENV_BREAKOUT, None) == OK
            assert lib.arl_net_set_env(h, ENV_CATCH, state) == OK                             # Catch as before
            assert lib.arl_net_set_env(h, ENV_CATCH, None) == OK
        finally:
            lib.arl_net_destroy(h)
    assert lib.arl_net_set_env(None, ENV_BREAKOUT, state) == EINVAL


@pytest.mark.parametrize("kind", [ENV_CATCH, ENV_BREAKOUT, ENV_BREAKOUT | GAME_OVER_ONLY])
def test_env_calls_fail_before_any_launch(kind):
    """arl_env_reset / arl_env_step / arl_run_window with an env of either game attached: pool_len = 1,
    unregistered or too short pools, a missing pool and t = t_max are ARL_EINVAL; no env attached is
    ARL_ESTATE."""
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
        # unregistered pools
        assert step() == EINVAL and b"not registered" in lib.arl_last_error()
        assert lib.arl_env_reset(h, pairs, rew, done, 2, None) == EINVAL
        assert window() == EINVAL
        assert lib.arl_net_set_pool(h, POOL_FRAMES, pairs, 3 * N * PAIR) == 0
        assert step() == EINVAL and b"reward" in lib.arl_last_error()
        assert lib.arl_net_set_pool(h, POOL_REWARDS, rew, 3 * N * 4) == 0
        assert lib.arl_net_set_pool(h, POOL_DONES, done, 3 * N) == 0
        # pool_len = 1 (and below): the env writes the entry after the one just read
        for bad in (1, 0, -3):
            assert step(L=bad) == EINVAL and b"pool_len" in lib.arl_last_error()
            assert lib.arl_env_reset(h, pairs, rew, done, bad, None) == EINVAL
        assert window(1) == EINVAL and b"pool_len" in lib.arl_last_error()
        # pools too short for pool_len
        assert step(L=4) == EINVAL and b"exceeds" in lib.arl_last_error()
        assert lib.arl_env_reset(h, pairs, rew, done, 4, None) == EINVAL
        assert window(4) == EINVAL and b"exceeds" in lib.arl_last_error()
        assert lib.arl_net_set_pool(h, POOL_DONES, done, 2 * N) == 0            # only the done pool too short
        assert step(L=3) == EINVAL and b"done" in lib.arl_last_error()
        assert lib.arl_net_set_pool(h, POOL_DONES, done, 3 * N) == 0
        # the env writes all three pools
        assert step(r=None) == EINVAL and step(d=None) == EINVAL and step(p=None) == EINVAL
        assert step(p=pairs + 8) == EINVAL                                       # misaligned frames
        # t in [0, t_max); the env range rules of arl_observe_envs
        assert step(t=T) == EINVAL and b"t_max" in lib.arl_last_error()
        assert step(t=-1) == EINVAL
        assert step(e0=1, ne=3) == EINVAL and step(e0=0, ne=N + 1) == EINVAL and step(ne=0) == EINVAL
        # detached again: the env calls are refused, the window is an ordinary one
        assert lib.arl_net_set_env(h, kind, None) == OK
        assert step() == ESTATE
    finally:
        lib.arl_net_destroy(h)


def test_device_breakout_is_exported():
    import asyncrl_amd
    from asyncrl_amd import _lib
    assert asyncrl_amd.DeviceBreakout.number_of_actions == 4 and asyncrl_amd.DeviceBreakout.envs == ()
    assert asyncrl_amd.DeviceCatch.kind == _lib.ENV_CATCH
    with pytest.raises(ValueError):
        asyncrl_amd.DeviceBreakout(0, device="cpu")
    env = asyncrl_amd.DeviceBreakout(3, device="cpu", seed=1, env_offset=2, life_loss_terminal=False)
    assert env.kind == ENV_BREAKOUT | GAME_OVER_ONLY and tuple(env.state.shape) == (2, 3, 16)
    assert asyncrl_amd.DeviceBreakout(3, device="cpu").kind == ENV_BREAKOUT
    pools = env.make_pools(2)
    assert tuple(pools[0].shape) == (2, 3, 2, 210, 160, 3)
