"""GPU: the device-resident Catch (csrc/catch.hip; include/asyncrl_hip.h "device environment")
against the NumPy restatement catch_ref.py, bit for bit -- the granular step, the closed
actor-learner loop through arl_run_window, the Python chains, an LSTM net, a replayed graph and
the detached net -- and, last, whether the learner learns the game from pixels.

Every comparison but the learning test's is exact: the game is integer arithmetic, and the
learner's own buffers are compared between two runs of the same kernels."""
import numpy as np
import pytest
import torch

import catch_ref as C
import device_env_loop as loop
from device_env_loop import dev, run_windows
from episode_replay import same_bits

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. granular parity
@pytest.mark.parametrize("n", [1, 35])
def test_granular_step_matches_the_restatement(gpu, n):
    """30 steps (two episodes and the start of a third) of scripted actions: env 0 always left
    and env 1 always right (both paddle clamps), the rest random in 0..5 (the >= 4 no-ops);
    env_offset 7, a seed above 2^32.  Pairs, rewards, dones and the state half after every step."""
    from asyncrl_amd import DeviceCatch
    seed, off, steps = (9 << 32) | 12345, 7, 30
    rng = np.random.default_rng(n)
    actions = rng.integers(0, 6, (steps, n)).astype(np.int32)
    actions[:, 0] = 3
    if n > 1:
        actions[:, 1] = 2
    ref = C.CatchRef(n, seed=seed, env_offset=off)
    env = DeviceCatch(n, device=gpu, seed=seed, env_offset=off)
    want, got = ref.reset(), env.reset()
    px_seen = {int(ref.state[0, 3])}
    for t in range(steps + 1):
        for w, g, what in zip(want, got, ("pairs", "rewards", "dones")):
            assert same_bits(g.cpu().numpy(), w), (what, t)
        assert same_bits(env.state[env.parity].cpu().numpy(), ref.state), t
        if t == steps:
            break
        want, got = ref.step(actions[t]), env.step(dev(actions[t], gpu))
        px_seen.update(int(x) for x in ref.state[:2, 3])
    # the script exercised what it claims, on the restatement
    assert 0 in px_seen and (n == 1 or 144 in px_seen)
    assert (ref.state[:, 4] == 2).all() and (ref.state[:, 5] == steps - 2 * C.EPISODE_STEPS).all()
    if n > 1:
        assert ref.bounced[:, 0].any() and ref.bounced[:, 1].any() and ref.catches >= 1
    # a second reset starts over in half 0
    got = env.reset()
    assert same_bits(got[0].cpu().numpy(), C.CatchRef(n, seed=seed, env_offset=off).reset()[0])


# ---------------------------------------------------------------- 2 - 4. the closed loop
def make_agent(*args, **kw):
    from asyncrl_amd import DeviceCatch
    return loop.make_agent(DeviceCatch, *args, **kw)


def LoopCheck(n, seed=5):
    """Every env finishes an episode each EPISODE_STEPS env-steps."""
    return loop.LoopCheck(C.CatchRef(n, seed=seed), lambda k: n * (k // C.EPISODE_STEPS))


def test_closed_loop_window_one_call(gpu):
    """FF, A = 4, 33 envs, t_max 5, pool_len 2, 6 windows through A3C.run_window (arl_run_window)."""
    n, T, P = 33, 5, 2
    agent, net, catch, pools = make_agent("ff", 4, n, T, P, gpu)
    check = LoopCheck(n)
    run_windows(agent, pools, P, 6, check)
    check.end(net, catch, pools, P)
    assert check.ref.state[:, 4].min() == 2                   # 30 steps: every env is in its third episode


@pytest.mark.parametrize("kind,A,n,P,kw", [("ff", 4, 64, 7, dict(env_groups=2)), ("lstm", 6, 33, 7, {})])
def test_closed_loop_python_chains(gpu, kind, A, n, P, kw):
    """The Python chains (_chain_steps): two env groups on two streams at 64 envs, and an LSTM net
    (A = 6) on the single chain; the parameters after 6 windows equal the one-call path's bit for bit."""
    T = 5
    one, one_net, _, one_pools = make_agent(kind, A, n, T, P, gpu)
    check = LoopCheck(n)
    run_windows(one, one_pools, P, 6, check if kind == "lstm" else None)
    if kind == "lstm":
        check.end(one_net, one_net.env, one_pools, P)
    agent, net, catch, pools = make_agent(kind, A, n, T, P, gpu)
    agent.window_c = False                                    # (the single chain from Python)
    init = net.params.clone()
    check = LoopCheck(n)
    run_windows(agent, pools, P, 6, check, **kw)
    check.end(net, catch, pools, P)
    torch.cuda.synchronize()
    assert torch.equal(net.params.view(torch.int32), one_net.params.view(torch.int32))
    assert torch.equal(catch.state, one_net.env.state)
    assert not torch.equal(net.params, init)                  # (and the six updates moved them)


def test_closed_loop_graph_replay(gpu):
    """Window 0 eagerly with first=True, one window captured on a single stream and replayed 5
    times == 6 eager windows: parameters, env state, episode statistics."""
    n, T, P = 33, 5, 2
    eager, enet, ecatch, epools = make_agent("ff", 4, n, T, P, gpu)
    run_windows(eager, epools, P, 6)
    agent, net, catch, pools = make_agent("ff", 4, n, T, P, gpu)
    agent.run_window(*pools, P, first=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        agent.run_window(*pools, P, first=False, stream=s)
    torch.cuda.synchronize()
    # (a capture launches nothing: the 5 replays are windows 1..5)
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(net.params.view(torch.int32), enet.params.view(torch.int32))
    assert torch.equal(catch.state, ecatch.state)
    assert same_bits(net.episode_stats_raw(), enet.episode_stats_raw())
    assert net.episode_stats()["episodes"] == 2 * n
    for a, b in zip(pools, epools):
        assert torch.equal(a, b)


def test_detached_net_leaves_the_env_alone(gpu):
    """After set_env(None) a window over the same pools writes neither the pools nor the env
    state, and its parameters equal those of a net that never had an env."""
    n, T, P = 33, 5, 3
    agent, net, catch, pools = make_agent("ff", 4, n, T, P, gpu)
    net.set_env(None)
    torch.cuda.synchronize()
    before = [p.clone() for p in pools] + [catch.state.clone()]
    assert int(before[0][0].max()) == 236                        # the reset rendered entry 0
    plain, pnet, _, _ = make_agent("ff", 4, n, T, P, gpu, env=False)
    ppools = [p.clone() for p in pools]
    run_windows(agent, pools, P, 2)
    run_windows(plain, ppools, P, 2)
    torch.cuda.synchronize()
    for a, b in zip(list(pools) + [catch.state], before):
        assert torch.equal(a, b)
    assert torch.equal(net.params.view(torch.int32), pnet.params.view(torch.int32))
    with pytest.raises(Exception):
        net.env_step(0, *pools, P)                                # ARL_ESTATE: no env attached


# ---------------------------------------------------------------- 6. learning
LEARN_WINDOWS = 2400      # twice the most any of three seeds needed on the MI355X (DESIGN.md "Device environment")


def learn_run(gpu, lr):
    from asyncrl_amd import DeviceCatch
    return loop.learn_run(DeviceCatch, gpu, lr, LEARN_WINDOWS)


def test_the_learner_learns_catch(gpu):
    """The mean return of the episodes completed in the last tenth of 2,400 windows is at least
    +0.15, the midpoint between a random policy (catch_ref.RANDOM_MEAN, -0.70) and the optimum
    (+1); the same run from the same seed with lr0 = 0 stays below it (and near the random mean).
    A consistently flipped policy gradient would pass every parity test and fail here."""
    st, params = learn_run(gpu, 7e-4)
    print("learned: mean return %+.4f over %d episodes" % (st["mean"], st["episodes"]))
    frozen, params0 = learn_run(gpu, 0.0)
    print("lr0 = 0: mean return %+.4f over %d episodes" % (frozen["mean"], frozen["episodes"]))
    assert st["episodes"] >= 256 * (LEARN_WINDOWS // 10) * 5 // C.EPISODE_STEPS - 256
    assert st["mean"] >= C.LEARNED, st
    assert frozen["mean"] < C.LEARNED and abs(frozen["mean"] - C.RANDOM_MEAN) < 0.05, frozen
    assert not torch.equal(params, params0)
