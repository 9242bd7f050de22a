"""GPU: the device-resident Breakout (csrc/breakout.hip; include/asyncrl_hip.h "device
environment") against the NumPy restatement breakout_ref.py, bit for bit -- the granular step
from crafted states, the closed actor-learner loop through arl_run_window with terminals out of
phase, the Python chains, an LSTM net, a replayed graph, the two done modes, raw against clipped
rewards, the batched evaluation and the detached net -- and, last, whether the learner learns
the game from pixels.

Every comparison but the learning test's is exact: the game is integer arithmetic, and the learner's own buffers are
compared between two runs of the same kernels."""
import numpy as np
import pytest
import torch

import breakout_ref as B
import device_env_loop as loop
from device_env_loop import dev, run_windows
from episode_replay import same_bits

pytestmark = pytest.mark.gpu


def plant(env, ref, rows, half=None):
    """Crafted states {env index: row} into the device half the next step reads and the
    restatement (the state is caller-owned memory)."""
    half = env.parity if half is None else half
    for e, row in rows.items():
        env.state[half, e] = dev(row, env.state.device)
        ref.state[e] = row


# ---------------------------------------------------------------- 1. granular parity
@pytest.mark.parametrize("n", [1, 35])
def test_granular_step_matches_the_restatement(gpu, n):
    """120 steps of breakout_ref.script_policies: env 0 always left and env 1 always right (both
    paddle clamps), 11 envs from crafted states (a column cleared up to the ceiling, one brick
    left, game_steps = 998, the last life on a certain miss, bricks of rows 0, 2 and 3 about to be
    hit, the paddle's outer segments, both walls), 8 tracking envs, the rest random in 0..5;
    env_offset 7, a seed above 2^32.  Pairs, rewards, dones and the state half after every step;
    then the restatement's counters show that every event class occurred."""
    from asyncrl_amd import DeviceBreakout
    seed, off, steps = (9 << 32) | 12345, 7, 120
    rng = np.random.default_rng(n)
    ref = B.BreakoutRef(n, seed=seed, env_offset=off)
    env = DeviceBreakout(n, device=gpu, seed=seed, env_offset=off)
    want, got = ref.reset(), env.reset()
    policies, rows = B.script_policies(n)
    px_seen = set()
    for t in range(steps + 1):
        for w, g, what in zip(want, got, ("pairs", "rewards", "dones")):
            assert same_bits(g.cpu().numpy(), w), (what, t)
        assert same_bits(env.state[env.parity].cpu().numpy(), ref.state), t
        if t == steps:
            break
        if t == 0:
            plant(env, ref, rows)
        actions = B.script_actions(ref.state, policies, rng)
        want, got = ref.step(actions), env.step(dev(actions, gpu))
        px_seen.update(int(x) for x in ref.state[:2, B.PX])
    # the script exercised what it claims, on the restatement
    assert 0 in px_seen and ref.life_losses > 0 and ref.game_overs["lives"] > 0
    if n > 1:
        assert 144 in px_seen
        B.assert_every_event_class(ref)
    # a second reset starts over in half 0
    got = env.reset()
    assert same_bits(got[0].cpu().numpy(), B.BreakoutRef(n, seed=seed, env_offset=off).reset()[0])
    assert same_bits(env.state[0].cpu().numpy(), fresh_state(n, seed, off))


def fresh_state(n, seed, off):
    ref = B.BreakoutRef(n, seed=seed, env_offset=off)
    ref.reset()
    return ref.state


# ---------------------------------------------------------------- 2 - 4. the closed loop
def make_agent(*args, **kw):
    from asyncrl_amd import DeviceBreakout
    return loop.make_agent(DeviceBreakout, *args, **kw)


def LoopCheck(n, seed=5, life_loss_terminal=True, keep=8):
    """A life lasts 6 env-steps or more: the runs here are long enough for one to end."""
    return loop.LoopCheck(B.BreakoutRef(n, seed=seed, life_loss_terminal=life_loss_terminal), lambda k: 1, keep=keep)


def test_closed_loop_window_one_call(gpu):
    """FF, A = 4, 33 envs, t_max 5, pool_len 2, 12 windows through A3C.run_window (arl_run_window).
    What Catch cannot show: the terminals fall in at least three different window slots, and in
    one window two envs terminate in different slots."""
    n, T, P = 33, 5, 2
    agent, net, game, pools = make_agent("ff", 4, n, T, P, gpu)
    check = LoopCheck(n)
    run_windows(agent, pools, P, 12, check)
    check.end(net, game, pools, P)
    slots_used = {t for d in check.slots for t in range(T) if d[t].any()}
    assert len(slots_used) >= 3, slots_used
    assert any(sum(bool(d[t].any()) for t in range(T)) >= 2 for d in check.slots)
    assert check.ref.life_losses >= n                          # 60 steps of lives that last 6 steps and more


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
    agent, net, game, pools = make_agent(kind, A, n, T, P, gpu)
    agent.window_c = False                                    # (the single chain from Python)
    init = net.params.clone()
    check = LoopCheck(n)
    run_windows(agent, pools, P, 6, check, **kw)
    check.end(net, game, pools, P)
    torch.cuda.synchronize()
    assert torch.equal(net.params.view(torch.int32), one_net.params.view(torch.int32))
    assert torch.equal(game.state, one_net.env.state)
    assert not torch.equal(net.params, init)                  # (and the six updates moved them)


def test_closed_loop_graph_replay(gpu):
    """Window 0 eagerly with first=True, one window captured on a single stream and replayed 5
    times == 6 eager windows: parameters, env state (with `serves` advancing), episode statistics."""
    n, T, P = 33, 5, 2
    eager, enet, egame, epools = make_agent("ff", 4, n, T, P, gpu)
    run_windows(eager, epools, P, 6)
    agent, net, game, pools = make_agent("ff", 4, n, T, P, gpu)
    agent.run_window(*pools, P, first=True)
    torch.cuda.synchronize()
    serves_before = game.state[T & 1, :, B.SERVES].clone()
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
    assert torch.equal(game.state, egame.state)
    assert same_bits(net.episode_stats_raw(), enet.episode_stats_raw())
    assert net.episode_stats()["episodes"] >= n
    serves_after = game.state[(6 * T) & 1, :, B.SERVES]
    assert int((serves_after > serves_before).sum()) >= n // 2   # 25 replayed steps: most envs served again
    for a, b in zip(pools, epools):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 5. the two done modes
def test_done_modes_differ_only_in_done(gpu):
    """The same scripted actions through life_loss_terminal=True and False, 35 envs (the last
    life and the step cap crafted in), 60 steps: pairs, rewards and every state word but
    steps_in_episode are identical; the dones of the False arm are exactly the game overs."""
    from asyncrl_amd import DeviceBreakout
    n, steps, seed = 35, 60, 77
    rng = np.random.default_rng(5)
    arms = [DeviceBreakout(n, device=gpu, seed=seed, life_loss_terminal=flag) for flag in (True, False)]
    ref = B.BreakoutRef(n, seed=seed, life_loss_terminal=False)
    ref.reset()
    policies, rows = B.script_policies(n)
    for env in arms:
        env.reset()
        plant(env, ref, rows)
    keep = [i for i in range(B.STATE_INTS) if i != B.STEPS]
    life_only = game_overs = 0
    for t in range(steps):
        actions = B.script_actions(ref.state, policies, rng)
        _, want_r, want_d = ref.step(actions, render_pairs=False)
        (pa, ra, da), (pb, rb, db) = (env.step(dev(actions, gpu)) for env in arms)
        assert torch.equal(pa, pb) and torch.equal(ra.view(torch.int32), rb.view(torch.int32)), t
        sa, sb = (env.state[env.parity].cpu().numpy() for env in arms)
        assert same_bits(sa[:, keep], sb[:, keep]) and same_bits(sb, ref.state), t
        da, db = da.cpu().numpy(), db.cpu().numpy()
        assert same_bits(db, want_d) and same_bits(db, ref.over.astype(np.uint8)), t
        assert same_bits(da, (ref.lost | ref.over).astype(np.uint8)), t
        life_only += int((da & ~db & 1).sum())
        game_overs += int(db.sum())
    assert life_only > 0 and game_overs > 0
    assert all(v > 0 for v in ref.game_overs.values())         # by lives, by a cleared board, by the cap
    assert (sa[:, B.STEPS] != sb[:, B.STEPS]).any()


# ---------------------------------------------------------------- 6. raw and clipped rewards
def test_clipping_is_the_learners_not_the_envs(gpu):
    """Every env starts under a 7-point brick (breakout_ref.seven_point_state): after one window the
    pool holds the raw 7.0, the episode statistics' reward_sum counts 7 for it and the window
    record's reward_sum (field 4, the reward as the learner uses it) counts 1."""
    n, T, P = 33, 5, 7
    agent, net, game, pools = make_agent("ff", 4, n, T, P, gpu, window_stats=True)
    check = LoopCheck(n)
    row = B.seven_point_state()
    torch.cuda.synchronize()
    plant(game, check.ref, {e: row for e in range(n)}, half=0)
    run_windows(agent, pools, P, 1, check)
    torch.cuda.synchronize()
    rew = check.rewards[0].astype(np.float64)
    assert (rew[0] == 7.0).all() and same_bits(pools[1][1].cpu().numpy(), np.full(n, 7.0, np.float32))
    stats, record = net.episode_stats_raw(), net.window_stats_raw(1)[0]
    assert same_bits(stats, check.rp.reduce())
    assert stats[7] == rew.sum() and stats[7] >= 7 * n
    assert record[2] == T * n                                   # every sample live
    assert record[4] == np.minimum(rew, 1.0).sum() and record[4] <= stats[7] - 6 * n


# ---------------------------------------------------------------- 7. evaluation
@pytest.mark.parametrize("scores", ["host", "device"])
def test_run_episodes_takes_a_game_over_only_breakout(gpu, scores):
    """evaluation.run_episodes over DeviceBreakout(life_loss_terminal=False), unchanged: 12 greedy
    runs over 8 envs; the traced actions replayed through the restatement give the same scores."""
    from asyncrl_amd import A3CFF, DeviceBreakout, run_episodes
    n, n_runs, seed, off = 8, 12, 21, 3
    model = A3CFF(4, n_envs=n, t_max=5, seed=2, init_seed=1, device=gpu, frames="pairs")
    env = DeviceBreakout(n, device=gpu, seed=seed, env_offset=off, life_loss_terminal=False)
    got, trace = run_episodes(model, env, n_runs, deterministic=True, max_steps=2 * B.STEP_CAP + 10, scores=scores)
    ref = B.BreakoutRef(n, seed=seed, env_offset=off, life_loss_terminal=False)
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
    assert sum(ref.game_overs.values()) >= n_runs and ref.life_losses > sum(ref.game_overs.values())   # whole games


# ---------------------------------------------------------------- 8. detached
def test_detached_net_leaves_the_env_alone(gpu):
    """After set_env(None) a window over the same pools writes neither the pools nor the env
    state, and its parameters equal those of a net that never had an env."""
    n, T, P = 33, 5, 3
    agent, net, game, pools = make_agent("ff", 4, n, T, P, gpu)
    net.set_env(None)
    torch.cuda.synchronize()
    before = [p.clone() for p in pools] + [game.state.clone()]
    assert int(before[0][0].max()) == 236                        # the reset rendered entry 0
    plain, pnet, _, _ = make_agent("ff", 4, n, T, P, gpu, env=False)
    ppools = [p.clone() for p in pools]
    run_windows(agent, pools, P, 2)
    run_windows(plain, ppools, P, 2)
    torch.cuda.synchronize()
    for a, b in zip(list(pools) + [game.state], before):
        assert torch.equal(a, b)
    assert torch.equal(net.params.view(torch.int32), pnet.params.view(torch.int32))
    with pytest.raises(Exception):
        net.env_step(0, *pools, P)                                # ARL_ESTATE: no env attached


# ---------------------------------------------------------------- 9. learning
def learn_run(gpu, lr, windows):
    from asyncrl_amd import DeviceBreakout
    return loop.learn_run(DeviceBreakout, gpu, lr, windows, raw=True)


def test_the_learner_learns_breakout(gpu):
    """The mean raw return per life over the last tenth of 17,802 windows is at least 91.3, the
    midpoint between the lr0 = 0 arm (0.148) and the lowest of three seeds at that length (182.4);
    the three seeds first crossed the mark after at most 8,901 windows, and the test runs twice
    that.  The lr0 = 0 arm estimates a constant: it runs a quarter of the length and stays within
    5 of its own standard errors of the recorded 0.1480.  A consistently flipped policy gradient,
    or rewards that reach the learner unclipped, would pass every parity test and fail here."""
    import time
    t0 = time.perf_counter()
    st, params = learn_run(gpu, 7e-4, B.LEARN_WINDOWS)
    mean = st[1] / st[0]
    print("learned: mean return per life %.2f over %d lives" % (mean, st[0]))
    frozen, params0 = learn_run(gpu, 0.0, B.LEARN_WINDOWS // 4)
    n0, mean0 = frozen[0], frozen[1] / frozen[0]
    se0 = np.sqrt((frozen[2] / n0 - mean0 * mean0) / (n0 - 1))
    print("lr0 = 0: mean return per life %.4f +- %.4f over %d lives; both arms %.1f s"
          % (mean0, se0, n0, time.perf_counter() - t0))
    assert st[0] >= 256 and n0 >= 256 * (B.LEARN_WINDOWS // 40) * 5 // 45
    assert mean >= B.LEARNED, st
    assert mean0 < B.LEARNED and abs(mean0 - B.LR0_MEAN_PER_LIFE) <= 5 * se0, frozen
    assert not torch.equal(params, params0)
