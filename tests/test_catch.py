"""CPU: the NumPy restatement of the device-resident Catch (catch_ref.py) keeps the game's
invariants, the random-policy mean the learning test measures against is the recorded constant,
and the env entry points of the C ABI validate their arguments on the host, before any launch
(fake, never-dereferenced device pointers; no GPU here)."""
import ctypes

import numpy as np
import pytest

import catch_ref as C

OK, EINVAL, ESTATE = 0, 1, 3
ENV_CATCH = 1


def play(n, steps, policy, seed=11, env_offset=0):
    """Episode returns (in completion order) of n envs over `steps` env-steps, without the render."""
    env = C.CatchRef(n, seed=seed, env_offset=env_offset)
    env.reset()
    rets, lens = [], []
    for _ in range(steps):
        before = env.state[:, 5].copy()
        _, r, d = env.step(policy(env), render_pairs=False)
        assert (r[d == 0] == 0).all() and (np.abs(r[d == 1]) == 1).all()
        rets.extend(r[d == 1].tolist())
        lens.extend((before[d == 1] + 1).tolist())
    return env, np.array(rets), np.array(lens)


def test_episodes_last_14_steps_and_tracking_always_catches():
    env, rets, lens = play(64, 5 * C.EPISODE_STEPS, lambda e: C.tracking_action(e.state))
    assert len(rets) == 64 * 5 and (lens == C.EPISODE_STEPS).all()
    assert (rets == 1.0).all()
    assert (env.state[:, 4] == 5).all() and (env.state[:, 5] == 0).all()      # 5 episodes done, a fresh one each
    assert env.bounced[:, 0].any() and env.bounced[:, 1].any()
    # the terminal falls in frame 3 of the 14th step: by = 18 + 3 * (4 * 13 + 3) = 183 >= 182
    assert C.BY0 + 3 * (4 * 13 + 2) + 8 < 190 <= C.BY0 + 3 * (4 * 13 + 3) + 8


def test_rendered_frames_hold_three_colours_and_two_sprites():
    env = C.CatchRef(5, seed=3)
    rng = np.random.default_rng(0)
    frames = [env.reset()[0]]
    for _ in range(2 * C.EPISODE_STEPS + 2):
        frames.append(env.step(rng.integers(0, 6, 5))[0])
    def rgb(c):
        return (c[0] << 16) | (c[1] << 8) | c[2]

    for pairs in frames:
        p = pairs.astype(np.uint32)
        per_screen = ((p[..., 0] << 16) | (p[..., 1] << 8) | p[..., 2]).reshape(-1, 210 * 160)
        assert set(np.unique(per_screen).tolist()) == {0, rgb(C.PADDLE_RGB), rgb(C.BALL_RGB)}
        assert ((per_screen == rgb(C.PADDLE_RGB)).sum(-1) == C.PADDLE_W * C.PADDLE_H).all()   # 64 pixels
        assert ((per_screen == rgb(C.BALL_RGB)).sum(-1) == C.BALL * C.BALL).all()             # 64 pixels
    # a non-terminal pair shows two different screens, (frame 4, frame 3): the ball 3 rows apart
    p = frames[1][0]
    rows = [np.flatnonzero((p[i] == C.BALL_RGB).all(-1).any(-1))[0] for i in (0, 1)]
    assert rows[0] - rows[1] == 3 and rows[0] == C.BY0 + 12
    # the overlap rule: a pixel inside both sprites takes the ball's colour
    s = C.render(70, 186, 72)
    assert tuple(s[191, 72]) == C.BALL_RGB and tuple(s[191, 80]) == C.PADDLE_RGB and tuple(s[194, 72]) == (0, 0, 0)


def test_random_policy_mean_is_the_recorded_constant():
    """20,000 episodes (1,000 envs x 20) of a uniform random policy over 4 actions: the mean
    return is the constant the learning test's pass mark is built from."""
    rng = np.random.default_rng(2024)
    _, rets, _ = play(1000, 20 * C.EPISODE_STEPS, lambda e: rng.integers(0, 4, e.n), seed=5)
    assert len(rets) == 20000
    print("random policy: mean %.4f stdev %.4f" % (rets.mean(), rets.std(ddof=1)))
    assert abs(rets.mean() - C.RANDOM_MEAN) < 5e-5
    assert -0.75 < C.RANDOM_MEAN < -0.65
    assert C.LEARNED == 0.15 and 0 <= C.LEARNED - (C.RANDOM_MEAN + C.OPTIMUM) / 2 < 0.001


def make_net(arch=0, A=4, N=4, T=5, bind=True):
    """(test_breakout.py takes it from here; its test_env_calls_fail_before_any_launch covers both games)"""
    from asyncrl_amd._lib import lib
    h = ctypes.c_void_p()
    assert lib.arl_net_create(ctypes.byref(h), arch, A, N, T, 0, 0) == 0
    if bind:
        fake = 1 << 40
        assert lib.arl_net_bind(h, fake, fake, fake, fake) == 0
    return h


def test_set_env_validation():
    from asyncrl_amd._lib import lib
    state = (1 << 40) + (5 << 30)
    for arch in (16, 17, 32, 33, 64):                       # RGB / STACK / STATES nets take no frame pairs
        h = make_net(arch, 4, bind=False)
        try:
            assert lib.arl_net_set_env(h, ENV_CATCH, state) == ESTATE, arch
            assert lib.arl_net_set_env(h, ENV_CATCH, None) == OK      # detaching nothing is fine
        finally:
            lib.arl_net_destroy(h)
    h = make_net(0, 3, bind=False)
    try:
        assert lib.arl_net_set_env(h, ENV_CATCH, state) == EINVAL     # n_actions = 3
        assert b"n_actions" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)
    for arch in (0, 1, 2):
        h = make_net(arch, 4, bind=False)                             # host state: an unbound handle takes it
        try:
            assert lib.arl_net_set_env(h, ENV_CATCH, state + 4) == EINVAL    # misaligned
            assert lib.arl_net_set_env(h, 7, state) == EINVAL                # unknown kind
            assert lib.arl_net_set_env(h, ENV_CATCH, state) == OK
            assert lib.arl_env_step(h, 0, 0, 4, state, state, state, 2, None) == ESTATE   # not bound
            assert lib.arl_net_set_env(h, ENV_CATCH, None) == OK
        finally:
            lib.arl_net_destroy(h)
    assert lib.arl_net_set_env(None, ENV_CATCH, state) == EINVAL


def test_granular_calls_validate_and_symbols_are_exported():
    from asyncrl_amd import _lib
    lib = _lib.lib
    for s in ("arl_catch_state_bytes", "arl_catch_reset", "arl_catch_step", "arl_net_set_env", "arl_env_reset",
              "arl_env_step"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.arl_catch_state_bytes(35) == 2 * 35 * 8 * 4 and lib.arl_catch_state_bytes(0) == 0
    assert lib.arl_catch_state_bytes(-1) == -1
    assert _lib.ENV_CATCH == ENV_CATCH and _lib.CATCH_STATE_INTS == 8
    f = 1 << 40
    st, pr, rw, dn, ac = f, f + (1 << 30), f + (2 << 30), f + (3 << 30), f + (4 << 30)
    assert lib.arl_catch_reset(st, 0, 0, 0, 0, pr, rw, dn, None) == OK           # nothing to do
    assert lib.arl_catch_step(st, 0, ac, 0, 0, 0, pr, rw, dn, None) == OK
    assert lib.arl_catch_reset(st, 4, 0, 0, 2, pr, rw, dn, None) == EINVAL       # parity
    assert lib.arl_catch_step(st, -1, ac, 4, 0, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_catch_reset(None, 4, 0, 0, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_catch_reset(st + 4, 4, 0, 0, 0, pr, rw, dn, None) == EINVAL   # misaligned state
    assert lib.arl_catch_reset(st, 4, 0, 0, 0, pr + 4, rw, dn, None) == EINVAL   # misaligned frames
    assert lib.arl_catch_step(st, 0, None, 4, 0, 0, pr, rw, dn, None) == EINVAL  # no actions
    assert lib.arl_catch_step(st, 0, ac, 65536, 0, 0, pr, rw, dn, None) == EINVAL
    assert lib.arl_catch_step(st, 0, ac, -1, 0, 0, pr, rw, dn, None) == EINVAL


def test_device_catch_is_exported():
    import asyncrl_amd
    assert asyncrl_amd.DeviceCatch.number_of_actions == 4
    with pytest.raises(ValueError):
        asyncrl_amd.DeviceCatch(0, device="cpu")
