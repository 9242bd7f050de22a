"""CPU: the direct-to-ring device env's entry points (include/asyncrl_hip.h, "direct-to-ring device env") are
declared, exported and in the ctypes table, and validate their arguments on the host before any launch (fake,
never-dereferenced device pointers; no GPU here).  The window counts test_gpu_env_direct.py runs are checked here
against the NumPy restatements of the three games: under uniformly random actions terminals occur well inside
them.  (The kernel itself is compared on the GPU: test_gpu_env_direct.py.)"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_catch import make_net

OK, EINVAL, ESTATE = 0, 1, 3
ENV_CATCH, ENV_BREAKOUT, ENV_PONG, GAME_OVER_ONLY = 1, 2, 4, 0x100
KINDS = (ENV_CATCH, ENV_BREAKOUT, ENV_BREAKOUT | GAME_OVER_ONLY, ENV_PONG | (1 << 16), ENV_PONG | (21 << 16))
NEW = ("arl_net_set_env_direct", "arl_env_reset_observe", "arl_env_step_observe", "arl_env_step_screen")

# what test_gpu_env_direct.py runs (imported there): FF closed loop N = 35, t_max = 2
CLOSED_N, CLOSED_T, CLOSED_WINDOWS = 35, 2, 16


def test_symbols_declared_and_exported():
    from asyncrl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "asyncrl_hip.h")).read()
    for s in NEW:
        assert re.search(r"\bint %s\s*\(" % s, txt), s
        assert hasattr(_lib.lib, s) and s in _lib.SIGNATURES, s
    assert re.search(r"#define ARL_ABI_VERSION 4\b", txt)
    assert _lib.lib.arl_abi_version() == 4 == _lib.ABI_VERSION
    from asyncrl_amd import DeviceNet, envs
    for m in ("env_reset_observe", "env_step_observe"):
        assert callable(getattr(DeviceNet, m))
    assert callable(envs._DeviceEnv.step_screen) and DeviceNet.env_direct is False


@pytest.mark.parametrize("bind", [False, True])
def test_set_env_direct_validation(bind):
    """Needs an attached env; refuses what arl_net_set_env refuses (frames-flag nets: ARL_ESTATE); host state only,
    so it works on an unbound handle; detaching the env turns it off."""
    from asyncrl_amd._lib import lib
    state = (1 << 40) + (5 << 30)
    assert lib.arl_net_set_env_direct(None, 1) == EINVAL
    for arch in (16, 17, 32, 33, 64):
        h = make_net(arch, 4, bind=bind)
        try:
            for on in (0, 1):
                assert lib.arl_net_set_env_direct(h, on) == ESTATE, arch
                assert b"frame pairs" in lib.arl_last_error()
        finally:
            lib.arl_net_destroy(h)
    for arch in (0, 1, 2):
        h = make_net(arch, 4, bind=bind)
        try:
            assert lib.arl_net_set_env_direct(h, 1) == ESTATE and b"no env" in lib.arl_last_error()
            assert lib.arl_net_set_env_direct(h, 0) == OK
            for kind in KINDS:
                assert lib.arl_net_set_env(h, kind, state) == OK
                assert lib.arl_net_set_env_direct(h, 1) == OK
                assert lib.arl_net_set_env_direct(h, 0) == OK
                assert lib.arl_net_set_env_direct(h, 1) == OK
                assert lib.arl_net_set_env(h, kind, None) == OK            # detach: direct goes with the env
                assert lib.arl_net_set_env(h, kind, state) == OK
                if bind:
                    assert lib.arl_env_step_observe(h, 0, 0, 4, 0, None) == ESTATE
                    assert b"direct mode is off" in lib.arl_last_error()
                assert lib.arl_net_set_env(h, kind, None) == OK
        finally:
            lib.arl_net_destroy(h)


@pytest.mark.parametrize("kind", KINDS)
def test_direct_calls_fail_before_any_launch(kind):
    """Unbound net, no env attached, direct mode off: ARL_ESTATE; t outside [0, t_max), a range that is not
    arl_env_step's, a resize mode outside the four: ARL_EINVAL -- each with every other argument valid."""
    from asyncrl_amd._lib import lib
    N, T = 4, 5
    state = (1 << 40) + (5 << 30)
    h = make_net(0, 4, N, T, bind=False)
    try:
        assert lib.arl_net_set_env(h, kind, state) == OK and lib.arl_net_set_env_direct(h, 1) == OK
        assert lib.arl_env_step_observe(h, 0, 0, N, 0, None) == ESTATE and b"not bound" in lib.arl_last_error()
        assert lib.arl_env_reset_observe(h, 0, None) == ESTATE and b"not bound" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)
    assert lib.arl_env_step_observe(None, 0, 0, N, 0, None) == EINVAL
    assert lib.arl_env_reset_observe(None, 0, None) == EINVAL
    h = make_net(0, 4, N, T)
    try:
        def step(t=0, e0=0, ne=N, mode=0):
            return lib.arl_env_step_observe(h, t, e0, ne, mode, None)

        def window(mode=0):   # null pools, pool_len 0
            return lib.arl_run_window(h, None, None, None, 0, 1, mode, 0.99, 0.01, 0.5, 1, 7e-4, 0, 0, 0.99, 0.1, 40.0,
                                      None)

        assert step() == ESTATE and b"no env" in lib.arl_last_error()
        assert lib.arl_env_reset_observe(h, 0, None) == ESTATE and b"no env" in lib.arl_last_error()
        assert lib.arl_net_set_env(h, kind, state) == OK
        assert step() == ESTATE and b"direct mode is off" in lib.arl_last_error()
        assert lib.arl_env_reset_observe(h, 0, None) == ESTATE and b"direct mode is off" in lib.arl_last_error()
        assert window() == EINVAL                      # direct off: the window wants its pools, as before
        assert lib.arl_net_set_env_direct(h, 1) == OK
        for t in (T, T + 1, -1):
            assert step(t=t) == EINVAL and b"t_max" in lib.arl_last_error()
        for e0, ne in ((1, 3), (0, N + 1), (0, 0), (-32, 4), (32, 1), (0, -1)):
            assert step(e0=e0, ne=ne) == EINVAL and b"env range" in lib.arl_last_error(), (e0, ne)
        for mode in (-1, 4, 8, 256):
            assert step(mode=mode) == EINVAL and b"resize_mode" in lib.arl_last_error()
            assert lib.arl_env_reset_observe(h, mode, None) == EINVAL and b"resize_mode" in lib.arl_last_error()
            assert window(mode) == EINVAL and b"resize_mode" in lib.arl_last_error()
        assert lib.arl_net_set_env_direct(h, 0) == OK
        assert step() == ESTATE
        assert lib.arl_net_set_env_direct(h, 1) == OK and lib.arl_net_set_env(h, kind, None) == OK
        assert step() == ESTATE and b"no env" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)
    h = make_net(2, 4, 64, T)                           # the Nature head runs all envs in one launch
    try:
        assert lib.arl_net_set_env(h, kind, state) == OK and lib.arl_net_set_env_direct(h, 1) == OK
        assert lib.arl_env_step_observe(h, 0, 32, 32, 0, None) == EINVAL and b"Nature" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)


def test_step_screen_validates():
    from asyncrl_amd._lib import lib
    f = 1 << 40
    st, sc, rw, dn, ac = f, f + (1 << 30), f + (2 << 30), f + (3 << 30), f + (4 << 30)

    def call(kind=ENV_CATCH, state=st, parity=0, actions=ac, n=4, mode=0, screen=sc, r=rw, d=dn):
        return lib.arl_env_step_screen(kind, state, parity, actions, n, 0, 0, mode, screen, r, d, None)

    for kind in KINDS + (ENV_PONG,):
        for mode in range(4):
            assert call(kind=kind, n=0, mode=mode) == OK                  # nothing to do
    for bad in (0, 3, 5, ENV_CATCH | GAME_OVER_ONLY, ENV_PONG | GAME_OVER_ONLY, ENV_PONG | (22 << 16), -1):
        assert call(kind=bad) == EINVAL and b"kind" in lib.arl_last_error(), bad
        assert call(kind=bad, n=0) == EINVAL
    for mode in (-1, 4, 7):
        assert call(mode=mode) == EINVAL and b"resize_mode" in lib.arl_last_error()
    for parity in (-1, 2):
        assert call(parity=parity) == EINVAL and b"parity" in lib.arl_last_error()
    assert call(n=-1) == EINVAL and call(n=65536) == EINVAL
    for kw in ({"state": None}, {"actions": None}, {"screen": None}, {"r": None}, {"d": None}):
        assert call(**kw) == EINVAL and b"null" in lib.arl_last_error(), kw
    for kw in ({"state": st + 4}, {"actions": ac + 2}, {"screen": sc + 2}, {"r": rw + 2}):
        assert call(**kw) == EINVAL and b"aligned" in lib.arl_last_error(), kw


def test_python_surface_without_a_device():
    """A device env builds on the CPU (no launch); step_screen checks the action count before any call."""
    import asyncrl_amd
    env = asyncrl_amd.DeviceCatch(3, device="cpu")
    assert env._screen_out is None
    with pytest.raises(ValueError):
        env.step_screen([0, 0])                         # 3 envs


def _terminals(ref, steps, n_actions=4, seed=2024):
    """Done events of all envs over `steps` env-steps under uniformly random actions."""
    ref.reset()
    rng = np.random.default_rng(seed)
    count = 0
    for _ in range(steps):
        _, _, d = ref.step(rng.integers(0, n_actions, ref.n), render_pairs=False)
        count += int(np.asarray(d).astype(bool).sum())
    return count


def test_window_count_of_the_gpu_test_reaches_terminals():
    """test_gpu_env_direct.py asserts dones.any() over CLOSED_WINDOWS windows of t_max CLOSED_T.  Under uniformly
    random actions the 35 envs of every game produce at least 17 terminals (one for every second env) within HALF
    of those env-steps, for several action seeds: one terminal anywhere in the whole run is certain with a wide
    margin.  (Catch: every episode lasts 14 env-steps whatever the policy, so all 35 envs end one.)  The ring of
    t_max + 4 slots wraps more than five times."""
    import breakout_ref
    import catch_ref
    import pong_ref
    steps = CLOSED_WINDOWS * CLOSED_T
    assert steps >= 2 * 14 and steps >= 5 * (CLOSED_T + 4)
    for seed in (1, 2, 3):
        games = {"catch": catch_ref.CatchRef(CLOSED_N, seed=5), "breakout": breakout_ref.BreakoutRef(CLOSED_N, seed=5),
                 "pong": pong_ref.PongRef(CLOSED_N, seed=5, points=1)}
        for name, ref in games.items():
            got = _terminals(ref, steps // 2, seed=seed)
            print(name, seed, got, "terminals in", steps // 2, "env-steps of", CLOSED_N, "envs")
            assert got >= CLOSED_N // 2, (name, seed, got)
