"""GPU: the direct-to-ring device env (csrc/env_direct.hpp; include/asyncrl_hip.h "direct-to-ring device env")
against the pairs path of the same library, bit for bit.

1. Stage: arl_env_step_screen == arl_<game>_step followed by arl_current_screen on the pair it wrote, for the three
   games and the four resize modes, with the state halves, the reward and the done.
2. Closed loop: two agents with the same seeds, one over pools (set_env(env)), one without (set_env(env,
   direct=True)); after every window the frame ring, nvalid, the reset flags, rewards, dones, the actions, the env
   state, the parameters and the optimizer state are equal.
3. The same through env groups on two streams, the one-C-call window and a replayed graph.
4. LSTM, the Nature head and PPO epochs, with the episode log and the window records.

Every comparison is exact: both paths run the same arithmetic on the same bytes."""
import numpy as np
import pytest
import torch

from test_env_direct import CLOSED_N, CLOSED_T, CLOSED_WINDOWS

pytestmark = pytest.mark.gpu

GAMES = ("catch", "breakout", "pong")
BALL_H = {"catch": 8, "breakout": 4, "pong": 4}      # the ball: state[..., 1] = its top row in all three games


def make_game(game, n, gpu, seed=5, env_offset=0):
    from asyncrl_amd import DeviceBreakout, DeviceCatch, DevicePong
    if game == "pong":
        return DevicePong(n, device=gpu, seed=seed, env_offset=env_offset, points=1)
    return (DeviceBreakout if game == "breakout" else DeviceCatch)(n, device=gpu, seed=seed, env_offset=env_offset)


# ---------------------------------------------------------------- 1. stage
def boundary_tap_rows(mode):
    """Source rows the bilinear taps of the first and last output row of a 12-row band touch (phi_ops.hpp
    resize_coeff: f = f32((d + 0.5) * scale - 0.5), rows floor(f) and floor(f) + 1; crop: row d + 18 of 210 -> 110)."""
    rows = set()
    for b in range(1, 7):
        for dy in (12 * b - 1, 12 * b):
            d, scale = (dy + 18, 1.0 / (110 / 210)) if mode & 2 else (dy, 1.0 / (84 / 210))
            s = int(np.floor(np.float32((d + 0.5) * scale - 0.5)))
            rows |= {min(s, 209), min(s + 1, 209)}
    return rows


@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("game", GAMES)
def test_step_screen_equals_step_then_current_screen(gpu, game, mode):
    """N = 3 envs, 40 steps of fixed pseudo-random actions from the reset on (step 0 is the first step after a
    reset): screens, rewards, dones and both state halves, byte for byte.  The run has terminals, and steps where the
    ball lies on a tap row at a band boundary."""
    from asyncrl_amd import current_screen
    n, steps, seed, off = 3, 40, (4 << 32) | 321, 6
    a, b = make_game(game, n, gpu, seed, off), make_game(game, n, gpu, seed, off)
    a.reset()
    b.reset()
    actions = np.random.default_rng(7).integers(0, 6, (steps, n))
    taps, on_boundary, terminals = boundary_tap_rows(mode), 0, 0
    for t in range(steps):
        act = torch.from_numpy(actions[t]).to(gpu)
        pairs, r, d = a.step(act)
        want = current_screen(pairs[:, 0].contiguous(), pairs[:, 1].contiguous(), mode)
        screens, r2, d2 = b.step_screen(act, mode)
        torch.cuda.synchronize()
        assert torch.equal(screens, want), (t, int((screens != want).sum()))
        assert torch.equal(r.view(torch.int32), r2.view(torch.int32)) and torch.equal(d, d2), t
        assert a.parity == b.parity and torch.equal(a.state, b.state), t
        by = a.state[a.parity, :, 1].cpu().numpy()
        on_boundary += sum(any(y in taps for y in range(int(y0), int(y0) + BALL_H[game])) for y0 in by)
        terminals += int(d.sum())
    assert int(screens.max()) > 0 and on_boundary >= 1 and terminals >= 1, (on_boundary, terminals)


# ---------------------------------------------------------------- 2 - 4. the closed loop
def build(game, kind, n, T, gpu, direct, seed=5, P=3, ppo=1, window_stats=False, window_c=None):
    """An agent at the reference's hyperparameters with `game` attached: over pools of P entries, reset -- or direct,
    with no pools at all.  The window that follows runs with first=True."""
    from asyncrl_amd import A3C, A3CFF, A3CFFNature, A3CLSTM, GradientClipping, RMSpropAsync
    cls = {"ff": A3CFF, "lstm": A3CLSTM, "nature": A3CFFNature}[kind]
    model = cls(4, n_envs=n, t_max=T, seed=seed, init_seed=1, device=gpu, frames="pairs")
    opt = RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99).setup(model)
    opt.add_hook(GradientClipping(40))
    agent = A3C(model, opt, T, 0.99, ppo_epochs=ppo, window_c=window_c)
    net = model.net
    net.set_episode_stats(True)
    if window_stats:
        net.set_window_stats(True)
    env = make_game(game, n, gpu, seed)
    if direct:
        net.set_env(env, direct=True)
        return agent, net, env, (None, None, None, 0)
    pools = env.make_pools(P)
    net.set_env(env)
    net.env_reset(*pools, P)
    return agent, net, env, pools + (P,)


def snapshot(net, env, kind):
    T, n = net.t_max, net.n_envs
    out = {"frames": net.buffer("frames"), "nvalid": net.buffer("nvalid"), "reset": net.buffer("reset"),
           "rewards": net.buffer("rewards", torch.int32), "dones": net.buffer("dones"),
           "actions": net.buffer("actions", torch.int32, (T + 1, n))[:T], "ctl": net.buffer("ctl", torch.int64),
           "env_state": env.state, "params": net.params.view(torch.int32), "ms": net.ms.view(torch.int32)}
    if kind == "lstm":
        out["hbuf"], out["cbuf"] = net.buffer("hbuf", torch.int32), net.buffer("cbuf", torch.int32)
    return out


def assert_same(pairs_side, direct_side, kind, where):
    torch.cuda.synchronize()
    a, b = snapshot(*pairs_side, kind), snapshot(*direct_side, kind)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, where, int((a[k] != b[k]).sum()))


def lockstep(game, kind, n, T, windows, gpu, **run_kw):
    """`windows` windows of a pairs agent and a direct agent side by side, compared after each; returns both
    (agent, net, env) and the dones of the whole run."""
    build_kw = {k: run_kw.pop(k) for k in ("ppo", "window_stats", "window_c") if k in run_kw}
    pa, pnet, penv, ppools = build(game, kind, n, T, gpu, False, **build_kw)
    da, dnet, denv, dpools = build(game, kind, n, T, gpu, True, **build_kw)
    assert dpools[:3] == (None, None, None) and dnet.env_direct and not pnet.env_direct
    init = pnet.params.clone()
    dones = []
    for w in range(windows):
        pa.run_window(*ppools, first=(w == 0), **run_kw)
        da.run_window(*dpools, first=(w == 0), **run_kw)
        assert_same((pnet, penv), (dnet, denv), kind, w)
        dones.append(dnet.buffer("dones").clone())
    assert not torch.equal(pnet.params, init)
    return (pa, pnet, penv), (da, dnet, denv), torch.stack(dones)


@pytest.mark.parametrize("path", ["chain", "one_call", "groups"])
@pytest.mark.parametrize("game", GAMES)
def test_closed_loop_bitwise(gpu, game, path):
    """FF, N = 35, t_max = 2, 16 windows (the ring of 6 slots wraps five times; test_env_direct.py checks the
    terminals): the single chain from Python, the one-C-call window (arl_run_window with null pools), and two env
    groups on two streams (ranges (0, 32) and (32, 3))."""
    kw = dict(env_groups=2) if path == "groups" else {}
    kw["window_c"] = path == "one_call"
    (_, pnet, _), (_, dnet, _), dones = lockstep(game, "ff", CLOSED_N, CLOSED_T, CLOSED_WINDOWS, gpu, **kw)
    if path == "groups":
        assert dnet.env_groups(2) == [(0, 32), (32, 3)]
    assert bool(dones.any())
    assert np.array_equal(pnet.episode_stats_raw(), dnet.episode_stats_raw()) and dnet.episode_stats()["episodes"] >= 1


@pytest.mark.parametrize("game", GAMES)
def test_closed_loop_graph_replay(gpu, game):
    """Window 0 eagerly with first=True, then ONE captured direct window replayed, against the eager pairs run
    window by window: the captured launch reads the step counter on the device, so its slots advance."""
    n, T, windows = CLOSED_N, CLOSED_T, CLOSED_WINDOWS
    pa, pnet, penv, ppools = build(game, "ff", n, T, gpu, False)
    da, dnet, denv, dpools = build(game, "ff", n, T, gpu, True)
    pa.run_window(*ppools, first=True)
    da.run_window(*dpools, first=True)
    assert_same((pnet, penv), (dnet, denv), "ff", 0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        da.run_window(*dpools, first=False, stream=s)
    torch.cuda.synchronize()
    dones = []
    for w in range(1, windows):
        pa.run_window(*ppools)
        g.replay()
        assert_same((pnet, penv), (dnet, denv), "ff", w)
        dones.append(dnet.buffer("dones").clone())
    assert bool(torch.stack(dones).any())
    assert np.array_equal(pnet.episode_stats_raw(), dnet.episode_stats_raw())


@pytest.mark.parametrize("kind,game,T,windows,kw", [
    ("lstm", "pong", 3, 10, {}),
    ("nature", "breakout", 2, 12, {}),
    ("ff", "catch", 2, 16, dict(ppo=2, window_stats=True)),
])
def test_other_models_bitwise(gpu, kind, game, T, windows, kw):
    """LSTM (N = 35, t_max = 3: the recurrent rows and the reset flags), the Nature head, and PPO epochs on the FF
    model with the window statistics on: the direct run equals the pairs run after every window, and the episode
    log, the episode statistics and the window records at the end."""
    (pa, pnet, _), (da, dnet, _), dones = lockstep(game, kind, CLOSED_N, T, windows, gpu, **kw)
    assert bool(dones.any())
    assert np.array_equal(pnet.episode_stats_raw(), dnet.episode_stats_raw())
    pl, dl = pnet.episode_log(), dnet.episode_log()
    assert set(pl) == set(dl) and int(dl["count"].sum()) >= 1
    for k in pl:
        assert torch.equal(pl[k], dl[k]), k
    if kw.get("window_stats"):
        a, b = pnet.window_stats_raw(64), dnet.window_stats_raw(64)   # one record per update: every epoch
        assert a.shape[0] >= windows and a.tobytes() == b.tobytes()
        assert torch.equal(pnet.ppo_snap.view(torch.int32), dnet.ppo_snap.view(torch.int32))
