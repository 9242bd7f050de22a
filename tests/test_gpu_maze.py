"""GPU: the device-resident maze (csrc/maze.hip; include/asyncrl_hip.h "device environment") against
the NumPy restatement maze_ref.py, bit for bit -- the granular reset and step under the scripted
policy (BFS winners, cyclers, bumpers: test_maze.py proves the coverage on the restatement alone), the
one-launch step + screen against the two calls it replaces, the closed actor-learner loop through
arl_run_window against the same windows driven through host pools from the restatement, direct mode
against the pairs path eagerly and as a replayed graph (FF, LSTM, Nature, and PPO epochs), and the
batched evaluation.

Every comparison is exact: the game is integer arithmetic, and the learner's own buffers are compared
between two runs of the same kernels."""
import numpy as np
import pytest
import torch

import device_env_loop as loop
import maze_ref as M
from device_env_loop import dev, run_windows
from episode_replay import same_bits

pytestmark = pytest.mark.gpu


def compare(env, ref, want, got, where):
    for w, g, what in zip(want, got, ("pairs", "rewards", "dones")):
        assert same_bits(g.cpu().numpy(), w), (what, where)
    assert same_bits(env.state[env.parity].cpu().numpy(), ref.state), where


# ---------------------------------------------------------------- 1. granular parity
@pytest.mark.parametrize("n,rooms,view,levels,steps,seed,off", M.GRANULAR_CASES)
def test_granular_matches_the_restatement(gpu, n, rooms, view, levels, steps, seed, off):
    """reset + 2 * 8R + 2 steps of the scripted policy, a seed above 2^32 (and a non-zero env_offset once):
    pairs, rewards, dones and both state halves after every call.  One workgroup row (n = 1), and 33 and 75
    envs; every rooms, every view, all levels, five levels and one.  A second reset starts over in half 0."""
    from asyncrl_amd import DeviceMaze
    assert seed > 1 << 32 and steps == 2 * 8 * rooms + 2
    kw = dict(seed=seed, env_offset=off, rooms=rooms, view=view, levels=levels)
    ref = M.MazeRef(n, **kw)
    env = DeviceMaze(n, device=gpu, **kw)
    want, got = ref.reset(), env.reset()
    compare(env, ref, want, got, "reset")
    for t in range(steps):
        before = ref.state.copy()
        actions = ref.scripted_actions(t)
        want, got = ref.step(actions), env.step(dev(actions, gpu))
        compare(env, ref, want, got, t)
        assert same_bits(env.state[env.parity ^ 1].cpu().numpy(), before), t    # the half read is left alone
    assert ref.wins > 0
    if n >= 33:
        assert ref.timeouts > 0 and ref.bumps > 0 and min(ref.moves) > 0, (ref.moves, ref.bumps, ref.timeouts)
    if levels:
        assert {lv for _, _, lv in ref.draws} <= set(range(levels))
    got = env.reset()
    fresh = M.MazeRef(n, **kw)
    assert same_bits(got[0].cpu().numpy(), fresh.reset()[0])
    assert same_bits(env.state[0].cpu().numpy(), fresh.state)


# ---------------------------------------------------------------- 2. the one-launch step + screen
@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("n,rooms,view,levels,steps,seed,off", M.SCREEN_CASES)
def test_step_screen_equals_step_then_current_screen(gpu, n, rooms, view, levels, steps, seed, off, mode):
    """n = 33, 8R + 4 steps of the scripted policy from the reset on: arl_env_step_screen's screens, rewards,
    dones and both state halves equal arl_maze_step followed by arl_current_screen of the pair it wrote, byte
    for byte, in all four resize modes -- moves in all four directions, bumps, wins and timeouts included, with
    the whole maze shown and under the fog of view 2."""
    from asyncrl_amd import DeviceMaze, current_screen
    kw = dict(seed=seed, env_offset=off, rooms=rooms, view=view, levels=levels)
    a, b = DeviceMaze(n, device=gpu, **kw), DeviceMaze(n, device=gpu, **kw)
    ref = M.MazeRef(n, **kw)                                  # drives the scripted policy
    a.reset()
    b.reset()
    ref.reset()
    for t in range(steps):
        actions = ref.scripted_actions(t)
        _, wr, wd = ref.step(actions, render_pairs=False)
        act = dev(actions, gpu)
        pairs, r, d = a.step(act)
        want = current_screen(pairs[:, 0].contiguous(), pairs[:, 1].contiguous(), mode)
        screens, r2, d2 = b.step_screen(act, mode)
        torch.cuda.synchronize()
        assert torch.equal(screens, want), (t, int((screens != want).sum()))
        assert torch.equal(r.view(torch.int32), r2.view(torch.int32)) and torch.equal(d, d2), t
        assert same_bits(r2.cpu().numpy(), wr) and same_bits(d2.cpu().numpy(), wd), t
        assert a.parity == b.parity and torch.equal(a.state, b.state), t
    assert same_bits(b.state[b.parity].cpu().numpy(), ref.state)
    assert ref.wins > 0 and ref.timeouts > 0 and ref.bumps > 0 and min(ref.moves) > 0
    assert int(screens.max()) > 0


# ---------------------------------------------------------------- 3. the closed loop
ROOMS_LOOP = 2


def make_agent(*args, **kw):
    from asyncrl_amd import DeviceMaze
    return loop.make_agent(DeviceMaze, *args, rooms=ROOMS_LOOP, **kw)


def window_state(net, kind):
    T, n = net.t_max, net.n_envs
    out = {"frames": net.buffer("frames"), "nvalid": net.buffer("nvalid"), "reset": net.buffer("reset"),
           "rewards": net.buffer("rewards", torch.int32), "dones": net.buffer("dones"),
           "actions": net.buffer("actions", torch.int32, (T + 1, n))[:T], "ctl": net.buffer("ctl", torch.int64),
           "params": net.params.view(torch.int32), "ms": net.ms.view(torch.int32)}
    if kind == "lstm":
        out["hbuf"], out["cbuf"] = net.buffer("hbuf", torch.int32), net.buffer("cbuf", torch.int32)
    return out


# an episode of rooms 2 lasts at most 16 env-steps: 7 windows of t_max 5 are 35, at least two terminals an env
LOOP_WINDOWS = 7


@pytest.mark.parametrize("kind,A,n,kw,view,levels", [("ff", 4, 64, dict(env_groups=2), 0, 0),
                                                     ("lstm", 6, 33, {}, 1, 3)])
def test_closed_loop_equals_host_driven_windows(gpu, kind, A, n, kw, view, levels):
    """7 windows of t_max 5 through A3C.run_window (arl_run_window) with the maze attached, at rooms 2 (at least
    two terminals an env), replayed through the restatement driven by the sampled actions (rewards and dones
    rows, the state half, the pool entries, the episode statistics), and against a second net WITHOUT an env
    whose pools the host fills from the restatement's pairs, rewards and dones: the ring, the window buffers,
    the sampled actions and the parameters agree bit for bit after every window.  FF with A = 4 at 64 envs (and
    once more as two env groups on two streams), LSTM with A = 6 (actions 4 and 5 are up and down again) at 33
    envs under view 1 with three levels."""
    T, windows = 5, LOOP_WINDOWS
    Pl = T + 2
    game_kw = dict(view=view, levels=levels)
    agent, net, game, pools = make_agent(kind, A, n, T, Pl, gpu, **game_kw)
    host, hnet, _, hpools = make_agent(kind, A, n, T, Pl, gpu, env=False, **game_kw)
    cap = M.cap(ROOMS_LOOP)
    check = loop.LoopCheck(M.MazeRef(n, seed=5, rooms=ROOMS_LOOP, **game_kw), lambda k: n * (k // cap), keep=T + 3)
    init = net.params.clone()
    for w in range(windows):
        agent.run_window(*pools, Pl, first=(w == 0))
        check.window(net)                                     # steps the restatement through the sampled actions
        for k in range(w * T, (w + 1) * T + 1):               # the observations this window read
            for pool, want in zip(hpools, check.obs[k]):
                pool[k % Pl] = dev(want, gpu)
        host.run_window(*hpools, Pl, first=(w == 0))
        torch.cuda.synchronize()
        a, b = window_state(net, kind), window_state(hnet, kind)
        for key in a:
            assert torch.equal(a[key], b[key]), (key, w, int((a[key] != b[key]).sum()))
    check.end(net, game, pools, Pl)
    assert not torch.equal(net.params, init)
    assert same_bits(net.episode_stats_raw(), hnet.episode_stats_raw())
    don = np.concatenate(check.slots)
    assert int(don.sum(0).min()) >= 2                         # at least two terminals an env
    rew = np.concatenate(check.rewards)
    assert set(np.unique(rew)) <= {0.0, 1.0} and (rew[don == 0] == 0).all()
    ref = check.ref
    assert ref.wins + ref.timeouts == int(don.sum()) and ref.wins == int(rew.sum())
    assert ref.timeouts > 0 and ref.bumps > 0 and min(ref.moves) > 0
    if kw:                                                    # the same windows as env-group chains from Python
        chains, cnet, cgame, cpools = make_agent(kind, A, n, T, Pl, gpu, **game_kw)
        chains.window_c = False
        run_windows(chains, cpools, Pl, windows, **kw)
        torch.cuda.synchronize()
        assert cnet.env_groups(2) == [(0, 32), (32, 32)]
        assert torch.equal(cnet.params.view(torch.int32), net.params.view(torch.int32))
        assert torch.equal(cgame.state, game.state)


# ---------------------------------------------------------------- 4. direct mode
def build(kind, A, n, T, gpu, direct, game_kw, seed=5, P=3, ppo_epochs=1):
    """An agent at the reference's hyperparameters with a maze attached, episode statistics on: over pools of P
    entries, reset -- or direct, with no pools at all.  The window that follows runs with first=True."""
    from asyncrl_amd import A3C, A3CFF, A3CFFNature, A3CLSTM, DeviceMaze, GradientClipping, RMSpropAsync
    cls = {"ff": A3CFF, "lstm": A3CLSTM, "nature": A3CFFNature}[kind]
    model = cls(A, n_envs=n, t_max=T, seed=seed, init_seed=1, device=gpu, frames="pairs")
    opt = RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99).setup(model)
    opt.add_hook(GradientClipping(40))
    agent = A3C(model, opt, T, 0.99, ppo_epochs=ppo_epochs) if ppo_epochs > 1 else A3C(model, opt, T, 0.99)
    net = model.net
    net.set_episode_stats(True)
    env = DeviceMaze(n, device=gpu, seed=seed, **game_kw)
    if direct:
        net.set_env(env, direct=True)
        return agent, net, env, (None, None, None, 0)
    pools = env.make_pools(P)
    net.set_env(env)
    net.env_reset(*pools, P)
    return agent, net, env, pools + (P,)


def assert_same(pairs_side, direct_side, kind, where):
    torch.cuda.synchronize()
    (pnet, penv), (dnet, denv) = pairs_side, direct_side
    a, b = window_state(pnet, kind), window_state(dnet, kind)
    a["env_state"], b["env_state"] = penv.state, denv.state
    for k in a:
        assert torch.equal(a[k], b[k]), (k, where, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("kind,A,n,game_kw,K", [("ff", 4, 35, dict(rooms=2), 1),
                                                ("lstm", 6, 33, dict(rooms=3, view=1, levels=5), 1),
                                                ("nature", 4, 33, dict(rooms=4, view=2), 1),
                                                ("ff", 4, 33, dict(rooms=2, view=2, levels=1), 2)])
def test_direct_mode_equals_the_pairs_path(gpu, kind, A, n, game_kw, K, graph):
    """7 windows of t_max 5 with the env direct-to-ring (no pools) beside the pairs path, compared after every
    window: the frame ring, nvalid and the reset flags, the rewards, dones and actions rows, the control block,
    both env state halves, the parameters and the RMSProp state after the update (and the LSTM's rows), then the
    episode statistics.  FF, LSTM and Nature nets, and the FF net with K = 2 PPO epochs; eagerly, and with
    window 0 eager and ONE captured direct window replayed."""
    T, windows = 5, 7
    pa, pnet, penv, ppools = build(kind, A, n, T, gpu, False, game_kw, ppo_epochs=K)
    da, dnet, denv, dpools = build(kind, A, n, T, gpu, True, game_kw, ppo_epochs=K)
    assert dpools[:3] == (None, None, None) and dnet.env_direct and not pnet.env_direct
    init = pnet.params.clone()
    pa.run_window(*ppools, first=True)
    da.run_window(*dpools, first=True)
    assert_same((pnet, penv), (dnet, denv), kind, 0)
    g = None
    if graph:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            da.run_window(*dpools, first=False, stream=s)
        torch.cuda.synchronize()
    for w in range(1, windows):
        pa.run_window(*ppools)
        if graph:
            g.replay()
        else:
            da.run_window(*dpools)
        assert_same((pnet, penv), (dnet, denv), kind, w)
    assert not torch.equal(pnet.params, init)
    assert np.array_equal(pnet.episode_stats_raw(), dnet.episode_stats_raw())
    st = denv.state[(windows * T) & 1].cpu().numpy()
    assert dnet.episode_stats()["episodes"] == int(st[:, M.WINS].sum() + st[:, M.TIMEOUTS].sum())
    if game_kw["rooms"] == 2:
        assert int(st[:, M.EPISODE].min()) >= 2               # 35 env-steps, episodes of at most 16
    assert (st[:, M.CFG] == M.cfg_of(game_kw["rooms"], game_kw.get("view", 0), game_kw.get("levels", 0))).all()


# ---------------------------------------------------------------- 5. evaluation
@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("scores", ["host", "device"])
def test_run_episodes_takes_a_maze(gpu, scores, deterministic):
    """evaluation.run_episodes over DeviceMaze(rooms=2, levels=7), unchanged: 16 runs over 8 envs, greedy and
    sampled; the traced actions replayed serially through the restatement give the same dones and the same
    scores, each one episode's 1 or 0."""
    from asyncrl_amd import A3CLSTM, DeviceMaze, run_episodes
    n, n_runs, seed, off = 8, 16, 21, 3
    kw = dict(seed=seed, env_offset=off, rooms=2, view=0, levels=7)
    model = A3CLSTM(4, n_envs=n, t_max=5, seed=2, init_seed=1, device=gpu, frames="pairs")
    env = DeviceMaze(n, device=gpu, **kw)
    got, trace = run_episodes(model, env, n_runs, deterministic=deterministic, max_steps=100, scores=scores)
    ref = M.MazeRef(n, **kw)
    ref.reset()
    want, acc, eps = np.zeros(n_runs), np.zeros(n), [0] * n
    for a, d in zip(trace["actions"], trace["dones"]):
        _, r, rd = ref.step(a, render_pairs=False)
        assert same_bits(rd, d.astype(np.uint8))
        acc += r
        for e in np.flatnonzero(rd):
            if eps[e] * n + e < n_runs:
                want[eps[e] * n + e] = acc[e]
            eps[e] += 1
            acc[e] = 0
    print("evaluation scores:", got.tolist())
    assert same_bits(got, want)
    assert ref.wins + ref.timeouts >= n_runs and set(got.tolist()) <= {0.0, 1.0}
    assert len(trace["actions"]) >= 3
    if not deterministic:
        assert ref.bumps > 0 and sum(ref.moves) > 0


# ---------------------------------------------------------------- 6. learning
# By the rule of DESIGN.md "Device environment", from three seeds of 4,000 windows at rooms 2, view 0, levels 0
# (DESIGN.md "Maze, the fifth device environment", curves under profiles/maze/): the lr0 = 0 arm averages 0.3654
# over 391,450 episodes and the lowest seed's last-tenth level is 0.9972, so the mark is their midpoint; all three
# seeds first reported at or above it at 201 windows (reports of 50), and twice that is 402.
LEARN_WINDOWS = 402
LEARN_MARK = 0.681
RANDOM_SUCCESS = 0.3680        # test_maze.py test_uniform_random_success_rate: exact, and re-measured there


def test_the_learner_learns_the_maze(gpu):
    """scripts/train_catch.py's train() at --env maze --rooms 2 --view 0 --levels 0, FF, 256 envs, t_max 5, the
    reference's hyperparameters (RMSpropAsync lr 7e-4, alpha 0.99, eps 0.1, clip 40, beta 0.01), seed 0: the
    episodes of the last tenth of LEARN_WINDOWS windows succeed at a rate of at least LEARN_MARK (measured: 0.6973
    over 4,510 episodes; the run ends on the plateau near 0.70 that all seeds hold before they solve the task, at
    0.997 from 2,000 windows on).  The same run
    with lr0 = 0 stays within 5 standard errors, sqrt(p (1 - p) / episodes), of the uniform-random success rate
    p of the restatement (measured: 0.3618 over 3,126 episodes)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import train_catch
    # (window 0 runs eagerly before the first report: reports of 41 windows leave the last one 32, the last tenth)
    kw = dict(env="maze", rooms=2, view=0, levels=0, envs=256, windows=LEARN_WINDOWS, report=LEARN_WINDOWS // 10 + 1,
              seed=0, arch="ff", device=str(gpu), log=lambda *a: None)
    last = train_catch.train(lr=7e-4, **kw)[-1]
    frozen = train_catch.train(lr=0.0, **kw)[-1]
    print("maze, rooms 2: FF %.4f over %d episodes; at lr0 = 0 %.4f over %d"
          % (last["mean_return"], last["episodes"], frozen["mean_return"], frozen["episodes"]))
    assert last["windows"] == LEARN_WINDOWS == frozen["windows"]
    assert last["mean_return"] >= LEARN_MARK, last
    p = RANDOM_SUCCESS
    assert abs(frozen["mean_return"] - p) <= 5.0 * (p * (1 - p) / frozen["episodes"]) ** 0.5, frozen
