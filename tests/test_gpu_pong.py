"""GPU: the device-resident Pong (csrc/pong.hip; include/asyncrl_hip.h "device environment")
against the NumPy restatement pong_ref.py, bit for bit -- the granular step from the crafted states
of test_pong.py and over a random rollout of whole games, the closed actor-learner loop through
arl_run_window with rewards of both signs that do not end an episode, the Python chains, an LSTM
net with all six actions, a replayed graph, PPO epochs over the attached env, the batched evaluation
and the detached net.

Every comparison is exact: the game is integer arithmetic, and the learner's own buffers are compared
between two runs of the same kernels."""
import numpy as np
import pytest
import torch

import device_env_loop as loop
import pong_ref as P
from device_env_loop import dev, run_windows
from episode_replay import same_bits

pytestmark = pytest.mark.gpu


def compare(env, ref, want, got, where):
    for w, g, what in zip(want, got, ("pairs", "rewards", "dones")):
        assert same_bits(g.cpu().numpy(), w), (what, where)
    assert same_bits(env.state[env.parity].cpu().numpy(), ref.state), where


# ---------------------------------------------------------------- 1. granular parity
@pytest.mark.parametrize("n", [1, 35])
def test_granular_step_from_crafted_states(gpu, n):
    """Every crafted state of pong_ref.crafted_states (what test_pong.py asserts on the restatement), n at
    a time, two steps each (the step cap needs two), points = 3, env_offset 7, a seed above 2^32: pairs,
    rewards, dones and the state half after every step."""
    from asyncrl_amd import DevicePong
    seed, off = (9 << 32) | 12345, 7
    rng = np.random.default_rng(0)
    crafted = list(P.crafted_states().items())
    seen = P.PongRef(1)
    for i in range(0, len(crafted), n):
        batch = crafted[i:i + n]
        ref = P.PongRef(n, seed=seed, env_offset=off, points=3)
        env = DevicePong(n, device=gpu, seed=seed, env_offset=off, points=3)
        want, got = ref.reset(), env.reset()
        compare(env, ref, want, got, (i, "reset"))
        policies = [p for _, (_, p) in batch] + [0] * (n - len(batch))
        for e, (_, (row, _)) in enumerate(batch):
            env.state[env.parity, e] = dev(row, gpu)
            ref.state[e] = row
        for t in range(2):
            actions = P.script_actions(ref.state, policies, rng)
            want, got = ref.step(actions), env.step(dev(actions, gpu))
            compare(env, ref, want, got, (i, t))
        for k in ("wall", "agent_hits", "opp_hits", "agent_points", "opp_points"):
            setattr(seen, k, [a + b for a, b in zip(getattr(seen, k), getattr(ref, k))])
        seen.game_overs = {k: v + ref.game_overs[k] for k, v in seen.game_overs.items()}
    # the crafted states reached what they claim, on the restatement
    assert min(seen.wall) > 0 and min(seen.agent_hits) > 0 and min(seen.opp_hits) > 0, vars(seen)
    assert min(seen.agent_points) > 0 and min(seen.opp_points) > 0 and seen.game_overs["cap"] == 1


@pytest.mark.parametrize("n", [1, 35])
def test_granular_rollout_matches_the_restatement(gpu, n):
    """90 steps at points = 1 of pong_ref.script_policies (env 0 always up, env 1 always down -- both
    clamps --, 4 following envs, the rest random in 0..5): every env but the followers finishes several
    games.  Then a second reset starts over in half 0."""
    from asyncrl_amd import DevicePong
    seed, off, steps = (3 << 32) | 777, 2, 90
    rng = np.random.default_rng(n)
    ref = P.PongRef(n, seed=seed, env_offset=off, points=1)
    env = DevicePong(n, device=gpu, seed=seed, env_offset=off, points=1)
    want, got = ref.reset(), env.reset()
    policies = P.script_policies(n)
    games, py_seen = np.zeros(n, int), set()
    for t in range(steps + 1):
        compare(env, ref, want, got, t)
        if t == steps:
            break
        actions = P.script_actions(ref.state, policies, rng)
        want, got = ref.step(actions), env.step(dev(actions, gpu))
        games += want[2]
        py_seen.update(int(x) for x in ref.state[:2, P.PY])
    # (a following env can rally through all 90 steps; every other env finishes several games)
    assert min(g for g, p in zip(games, policies) if p != "follow") >= 3 and 34 in py_seen, (games, py_seen)
    if n > 1:
        assert 178 in py_seen and ref.game_overs["agent"] > 0 and ref.game_overs["opp"] > 0
        assert min(ref.wall) > 0 and sum(ref.agent_hits) > 0 and min(ref.opp_hits) > 0
    got = env.reset()
    fresh = P.PongRef(n, seed=seed, env_offset=off, points=1)
    assert same_bits(got[0].cpu().numpy(), fresh.reset()[0])
    assert same_bits(env.state[0].cpu().numpy(), fresh.state)


# ---------------------------------------------------------------- 2 - 4. the closed loop
def make_agent(*args, points=1, **kw):
    from asyncrl_amd import DevicePong
    return loop.make_agent(DevicePong, *args, points=points, **kw)


def LoopCheck(n, points=1, seed=5, keep=8):
    return loop.LoopCheck(P.PongRef(n, seed=seed, points=points), lambda k: 1, keep=keep)


def test_closed_loop_window_one_call(gpu):
    """FF, A = 4, 33 envs, t_max 5, pool_len 7 (not a multiple of t_max + 1), points = 3, 16 windows through
    A3C.run_window (arl_run_window).  What neither other env can show: rewards of +1 and of -1 that do not
    end the episode reach the learner's reward rows, and whole games end after them."""
    n, T, Pl = 33, 5, 7
    agent, net, game, pools = make_agent("ff", 4, n, T, Pl, gpu, points=3)
    check = LoopCheck(n, points=3)
    run_windows(agent, pools, Pl, 16, check)
    check.end(net, game, pools, Pl)
    rew, don = np.concatenate(check.rewards), np.concatenate(check.slots)
    inner = rew[don == 0]
    assert (inner == 1.0).any() and (inner == -1.0).any(), np.unique(rew, return_counts=True)
    assert set(np.unique(rew)) == {-1.0, 0.0, 1.0} and don.sum() >= 1
    assert (rew[don != 0] != 0).all()                               # no game ran into the cap here


@pytest.mark.parametrize("kind,A,n,Pl,kw", [("ff", 4, 64, 7, dict(env_groups=2)), ("lstm", 6, 33, 7, {})])
def test_closed_loop_python_chains(gpu, kind, A, n, Pl, kw):
    """The Python chains (_chain_steps): two env groups on two streams at 64 envs, and an LSTM net
    (A = 6: actions 4 and 5 are sampled and move the paddle) on the single chain; the parameters after 6
    windows equal the one-call path's bit for bit."""
    T = 5
    one, one_net, _, one_pools = make_agent(kind, A, n, T, Pl, gpu)
    check = LoopCheck(n)
    run_windows(one, one_pools, Pl, 6, check if kind == "lstm" else None)
    if kind == "lstm":
        check.end(one_net, one_net.env, one_pools, Pl)
    agent, net, game, pools = make_agent(kind, A, n, T, Pl, gpu)
    agent.window_c = False                                    # (the single chain from Python)
    init = net.params.clone()
    check = LoopCheck(n)
    run_windows(agent, pools, Pl, 6, check, **kw)
    check.end(net, game, pools, Pl)
    torch.cuda.synchronize()
    assert torch.equal(net.params.view(torch.int32), one_net.params.view(torch.int32))
    assert torch.equal(game.state, one_net.env.state)
    assert not torch.equal(net.params, init)                  # (and the six updates moved them)
    if A == 6:
        acts = net.buffer("actions", torch.int32, (T + 1, n))[:T].cpu().numpy()
        assert acts.max() >= 4


def test_closed_loop_graph_replay(gpu):
    """Window 0 eagerly with first=True, one window captured on a single stream and replayed 5
    times == 6 eager windows: parameters, env state (with `serves` advancing), episode statistics."""
    n, T, Pl = 33, 5, 2
    eager, enet, egame, epools = make_agent("ff", 4, n, T, Pl, gpu)
    run_windows(eager, epools, Pl, 6)
    agent, net, game, pools = make_agent("ff", 4, n, T, Pl, gpu)
    agent.run_window(*pools, Pl, first=True)
    torch.cuda.synchronize()
    serves_before = game.state[T & 1, :, P.SERVES].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        agent.run_window(*pools, Pl, first=False, stream=s)
    torch.cuda.synchronize()
    # (a capture launches nothing: the 5 replays are windows 1..5)
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(net.params.view(torch.int32), enet.params.view(torch.int32))
    assert torch.equal(game.state, egame.state)
    assert same_bits(net.episode_stats_raw(), enet.episode_stats_raw())
    assert net.episode_stats()["episodes"] >= n
    serves_after = game.state[(6 * T) & 1, :, P.SERVES]
    assert int((serves_after > serves_before).sum()) >= n // 2   # 25 replayed steps: most envs served again
    for a, b in zip(pools, epools):
        assert torch.equal(a, b)


def test_closed_loop_with_ppo_epochs(gpu):
    """A3C(ppo_epochs=2, gae_lambda=0.95) on Adam takes the env as it is: 4 windows at points = 2 (a point
    that does not end the game reaches the GAE recurrence).  The env steps t_max times a window, not t_max
    times an epoch -- the replay of the sampled actions through the restatement ends in the same state,
    pools and episode statistics -- and every epoch is an update."""
    from asyncrl_amd import A3C, A3CFF, Adam, DevicePong, GradientClipping
    n, T, Pl, K, seed = 32, 5, 7, 2, 5
    model = A3CFF(4, n_envs=n, t_max=T, seed=seed, init_seed=6, frames="pairs", device=gpu)
    opt = Adam(alpha=1e-3).setup(model)
    opt.add_hook(GradientClipping(40))
    agent = A3C(model, opt, T, 0.99, gae_lambda=0.95, ppo_epochs=K)
    net = model.net
    net.set_episode_stats(True)
    game = DevicePong(n, device=gpu, seed=seed, points=2)
    pools = game.make_pools(Pl)
    net.set_env(game)
    net.env_reset(*pools, Pl)
    init = net.params.clone()
    check = LoopCheck(n, points=2, seed=seed)
    run_windows(agent, pools, Pl, 4, check)
    check.end(net, game, pools, Pl)
    assert net.adam_t() == 4 * K and not torch.equal(net.params, init)
    st = agent.ppo_stats()
    assert 0.0 <= st["clip_fraction"] <= 1.0 and np.isfinite(st["approx_kl"])
    rew, don = np.concatenate(check.rewards), np.concatenate(check.slots)
    assert (rew[don == 0] != 0).any()


# ---------------------------------------------------------------- 5. evaluation
@pytest.mark.parametrize("scores", ["host", "device"])
def test_run_episodes_takes_a_pong(gpu, scores):
    """evaluation.run_episodes over DevicePong(points=3), unchanged: 12 greedy runs over 8 envs; the
    traced actions replayed through the restatement give the same scores, each a game's point difference."""
    from asyncrl_amd import A3CFF, DevicePong, run_episodes
    n, n_runs, seed, off = 8, 12, 21, 3
    model = A3CFF(4, n_envs=n, t_max=5, seed=2, init_seed=1, device=gpu, frames="pairs")
    env = DevicePong(n, device=gpu, seed=seed, env_offset=off, points=3)
    got, trace = run_episodes(model, env, n_runs, deterministic=True, max_steps=2 * P.STEP_CAP + 10, scores=scores)
    ref = P.PongRef(n, seed=seed, env_offset=off, points=3)
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
    assert sum(ref.game_overs.values()) >= n_runs and set(got.tolist()) <= {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}


# ---------------------------------------------------------------- 6. detached
def test_detached_net_leaves_the_env_alone(gpu):
    """After set_env(None) a window over the same pools writes neither the pools nor the env
    state, and its parameters equal those of a net that never had an env."""
    n, T, Pl = 33, 5, 3
    agent, net, game, pools = make_agent("ff", 4, n, T, Pl, gpu)
    net.set_env(None)
    torch.cuda.synchronize()
    before = [p.clone() for p in pools] + [game.state.clone()]
    assert int(before[0][0].max()) == 236 and int(before[0][0].min()) == 17    # the reset rendered entry 0
    plain, pnet, _, _ = make_agent("ff", 4, n, T, Pl, gpu, env=False)
    ppools = [p.clone() for p in pools]
    run_windows(agent, pools, Pl, 2)
    run_windows(plain, ppools, Pl, 2)
    torch.cuda.synchronize()
    for a, b in zip(list(pools) + [game.state], before):
        assert torch.equal(a, b)
    assert torch.equal(net.params.view(torch.int32), pnet.params.view(torch.int32))
    with pytest.raises(Exception):
        net.env_step(0, *pools, Pl)                                # ARL_ESTATE: no env attached
