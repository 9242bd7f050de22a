"""GPU: the device-resident T-maze (csrc/tmaze.hip; include/asyncrl_hip.h "device environment")
against the NumPy restatement tmaze_ref.py, bit for bit -- the granular reset and step with every
action value at the junctions, the one-launch step + screen against the two calls it replaces, the
closed actor-learner loop through arl_run_window against the same windows driven through host pools
from the restatement, direct mode against the pairs path eagerly and as a replayed graph, the
batched evaluation -- and the result no other device env can give: the LSTM learns the task while the
FF model, blind to the cue at the junction (test_tmaze.py), stays at an expected return of exactly 0.

Every comparison but the learning one is exact: the game is integer arithmetic, and the learner's
own buffers are compared between two runs of the same kernels."""
import os
import sys

import numpy as np
import pytest
import torch

import device_env_loop as loop
import tmaze_ref as M
from device_env_loop import dev, run_windows
from episode_replay import same_bits

pytestmark = pytest.mark.gpu


def compare(env, ref, want, got, where):
    for w, g, what in zip(want, got, ("pairs", "rewards", "dones")):
        assert same_bits(g.cpu().numpy(), w), (what, where)
    assert same_bits(env.state[env.parity].cpu().numpy(), ref.state), where


# ---------------------------------------------------------------- 1. granular parity
@pytest.mark.parametrize("n,length,off", [(1, 1, 0), (1, 4, 0), (33, 1, 0), (33, 4, 7), (33, 8, 0), (75, 4, 0),
                                          (75, 8, 0)])
def test_granular_matches_the_restatement(gpu, n, length, off):
    """reset + 3 (L + 1) steps, a seed above 2^32: pairs, rewards, dones and both state halves after every
    call.  The actions cycle 0..5 with an offset per env, so with 6 or more envs both arms and the lapse occur
    at junctions, for both cues.  A second reset starts over in half 0."""
    from asyncrl_amd import DeviceTMaze
    seed = (9 << 32) | 12345
    ref = M.TMazeRef(n, seed=seed, env_offset=off, length=length)
    env = DeviceTMaze(n, device=gpu, seed=seed, env_offset=off, length=length)
    want, got = ref.reset(), env.reset()
    compare(env, ref, want, got, "reset")
    for t in range(3 * (length + 1)):
        before = ref.state.copy()
        actions = M.cycle_actions(n, t)
        want, got = ref.step(actions), env.step(dev(actions, gpu))
        compare(env, ref, want, got, t)
        assert same_bits(env.state[env.parity ^ 1].cpu().numpy(), before), t    # the half read is left alone
    assert sum(ref.junctions.values()) == 3 * n and ref.corridor_steps == 3 * length * n
    if n >= 33:
        assert min(ref.junctions.values()) > 0, ref.junctions
        assert {(c, a) for c in (0, 1) for a in range(6)} <= set(ref.choices), ref.choices
    got = env.reset()
    fresh = M.TMazeRef(n, seed=seed, env_offset=off, length=length)
    assert same_bits(got[0].cpu().numpy(), fresh.reset()[0])
    assert same_bits(env.state[0].cpu().numpy(), fresh.state)


# ---------------------------------------------------------------- 2. the one-launch step + screen
@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("length", [1, 8])
def test_step_screen_equals_step_then_current_screen(gpu, length, mode):
    """n = 33, 2 (L + 1) + 1 steps from the reset on: arl_env_step_screen's screens, rewards, dones and both
    state halves equal arl_tmaze_step followed by arl_current_screen of the pair it wrote, byte for byte, in all
    four resize modes -- the steps that show a cue (the one after each terminal) and the steps after them
    included."""
    from asyncrl_amd import DeviceTMaze, current_screen
    n, seed, off = 33, (4 << 32) | 321, 6
    a = DeviceTMaze(n, device=gpu, seed=seed, env_offset=off, length=length)
    b = DeviceTMaze(n, device=gpu, seed=seed, env_offset=off, length=length)
    a.reset()
    b.reset()
    bare = None
    shown = after = 0
    for t in range(2 * (length + 1) + 1):
        act = dev(M.cycle_actions(n, t), gpu)
        pairs, r, d = a.step(act)
        want = current_screen(pairs[:, 0].contiguous(), pairs[:, 1].contiguous(), mode)
        screens, r2, d2 = b.step_screen(act, mode)
        torch.cuda.synchronize()
        assert torch.equal(screens, want), (t, int((screens != want).sum()))
        assert torch.equal(r.view(torch.int32), r2.view(torch.int32)) and torch.equal(d, d2), t
        assert a.parity == b.parity and torch.equal(a.state, b.state), t
        if bool(d.all()):                                     # the next episode's first screen: its cue is on it
            shown += 1
            cues = a.state[a.parity, :, M.CUE_BIT].cpu().numpy()
            up, down = screens[int(np.flatnonzero(cues == 0)[0])], screens[int(np.flatnonzero(cues == 1)[0])]
            assert not torch.equal(up, down)
            bare = t
        elif bare == t - 1:                                   # the step after it: no cue, all envs alike
            after += 1
            assert all(torch.equal(screens[0], screens[e]) for e in range(1, n))
    assert shown == 2 and after == 2 and int(screens.max()) > 0


# ---------------------------------------------------------------- 3. the closed loop
def make_agent(*args, length=4, **kw):
    from asyncrl_amd import DeviceTMaze
    return loop.make_agent(DeviceTMaze, *args, length=length, **kw)


def LoopCheck(n, length, seed=5, keep=8):
    return loop.LoopCheck(M.TMazeRef(n, seed=seed, length=length), lambda k: n * (k // (length + 1)), keep=keep)


def window_state(net, kind):
    T, n = net.t_max, net.n_envs
    out = {"frames": net.buffer("frames"), "nvalid": net.buffer("nvalid"), "reset": net.buffer("reset"),
           "rewards": net.buffer("rewards", torch.int32), "dones": net.buffer("dones"),
           "actions": net.buffer("actions", torch.int32, (T + 1, n))[:T], "ctl": net.buffer("ctl", torch.int64),
           "params": net.params.view(torch.int32), "ms": net.ms.view(torch.int32)}
    if kind == "lstm":
        out["hbuf"], out["cbuf"] = net.buffer("hbuf", torch.int32), net.buffer("cbuf", torch.int32)
    return out


@pytest.mark.parametrize("length", [4, 3])
@pytest.mark.parametrize("kind,A,n,kw", [("ff", 4, 64, dict(env_groups=2)), ("lstm", 6, 33, {})])
def test_closed_loop_equals_host_driven_windows(gpu, kind, A, n, kw, length):
    """7 windows of t_max 5 through A3C.run_window (arl_run_window) with the T-maze attached -- at L = 4 every
    window is one episode, at L = 3 the terminals do not align with the windows -- replayed through the
    restatement (rewards and dones rows, the state half, the pool entries, the episode statistics), and against
    a second net WITHOUT an env whose pools the host fills from the restatement's pairs, rewards and dones: the
    ring, the window buffers, the sampled actions and the parameters agree bit for bit after every window.  FF
    with A = 4 at 64 envs (and once more as two env groups on two streams), LSTM with A = 6 at 33."""
    closed_loop(gpu, kind, A, n, kw, length)


def closed_loop(gpu, kind, A, n, kw, length, T=5, windows=7):
    """The body of the test above at a window length of T (pools of T + 2 entries: a window's T + 1 observations
    fit, and the host's fill of window w + 1 does not reach back into them)."""
    Pl = T + 2
    agent, net, game, pools = make_agent(kind, A, n, T, Pl, gpu, length=length)
    host, hnet, _, hpools = make_agent(kind, A, n, T, Pl, gpu, length=length, env=False)
    check = LoopCheck(n, length, keep=T + 3)
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
    assert int(don.sum()) == n * (windows * T // (length + 1))
    if length == 3:
        assert {int(t) for t in np.flatnonzero(don.reshape(windows, T, n)[:, :, 0].any(0))} == set(range(T))
    rew = np.concatenate(check.rewards)
    assert set(np.unique(rew)) <= {-1.0, 0.0, 1.0} and (rew != 0).any() and (rew[don == 0] == 0).all()
    if kw:                                                    # the same windows as env-group chains from Python
        chains, cnet, cgame, cpools = make_agent(kind, A, n, T, Pl, gpu, length=length)
        chains.window_c = False
        run_windows(chains, cpools, Pl, windows, **kw)
        torch.cuda.synchronize()
        assert cnet.env_groups(2) == [(0, 32), (32, 32)]
        assert torch.equal(cnet.params.view(torch.int32), net.params.view(torch.int32))
        assert torch.equal(cgame.state, game.state)


def build(kind, A, n, T, length, gpu, direct, seed=5, P=3):
    """An agent at the reference's hyperparameters with a T-maze attached, episode statistics on: over pools of P
    entries, reset -- or direct, with no pools at all.  The window that follows runs with first=True."""
    from asyncrl_amd import A3C, A3CFF, A3CLSTM, DeviceTMaze, GradientClipping, RMSpropAsync
    model = (A3CFF if kind == "ff" else A3CLSTM)(A, n_envs=n, t_max=T, seed=seed, init_seed=1, device=gpu,
                                                 frames="pairs")
    opt = RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99).setup(model)
    opt.add_hook(GradientClipping(40))
    agent = A3C(model, opt, T, 0.99)
    net = model.net
    net.set_episode_stats(True)
    env = DeviceTMaze(n, device=gpu, seed=seed, length=length)
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
@pytest.mark.parametrize("kind,A,n,length", [("ff", 4, 35, 4), ("lstm", 6, 33, 3)])
def test_direct_mode_equals_the_pairs_path(gpu, kind, A, n, length, graph):
    """7 windows of t_max 5 with the env direct-to-ring (no pools) beside the pairs path, compared after every
    window: the frame ring, nvalid and the reset flags, the rewards, dones and actions rows, the control block,
    both env state halves, the parameters and the RMSProp state after the update (and the LSTM's rows), then the
    episode statistics.  Eagerly, and with window 0 eager and ONE captured direct window replayed."""
    direct_mode(gpu, kind, A, n, length, graph)


def direct_mode(gpu, kind, A, n, length, graph, T=5, windows=7):
    pa, pnet, penv, ppools = build(kind, A, n, T, length, gpu, False)
    da, dnet, denv, dpools = build(kind, A, n, T, length, gpu, True)
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
    dones = []
    for w in range(1, windows):
        pa.run_window(*ppools)
        if graph:
            g.replay()
        else:
            da.run_window(*dpools)
        assert_same((pnet, penv), (dnet, denv), kind, w)
        dones.append(dnet.buffer("dones").clone())
    assert int(torch.stack(dones).sum()) >= n * ((windows - 1) * T // (length + 1) - 1)
    assert not torch.equal(pnet.params, init)
    assert np.array_equal(pnet.episode_stats_raw(), dnet.episode_stats_raw())
    assert dnet.episode_stats()["episodes"] == n * (windows * T // (length + 1))


# ---------------------------------------------------------------- 4. evaluation
@pytest.mark.parametrize("scores", ["host", "device"])
def test_run_episodes_takes_a_tmaze(gpu, scores):
    """evaluation.run_episodes over DeviceTMaze(length=3), unchanged: 20 runs of sampled actions over 8 envs (an
    untrained greedy policy makes the same choice every time); the traced actions replayed serially through the
    restatement give the same scores, each one episode's +1, -1 or 0, and more than one of the three occurs."""
    from asyncrl_amd import A3CLSTM, DeviceTMaze, run_episodes
    n, n_runs, seed, off, length = 8, 20, 21, 3, 3
    model = A3CLSTM(4, n_envs=n, t_max=5, seed=2, init_seed=1, device=gpu, frames="pairs")
    env = DeviceTMaze(n, device=gpu, seed=seed, env_offset=off, length=length)
    got, trace = run_episodes(model, env, n_runs, deterministic=False, max_steps=100, scores=scores)
    ref = M.TMazeRef(n, seed=seed, env_offset=off, length=length)
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
    assert sum(ref.junctions.values()) >= n_runs and set(got.tolist()) <= {-1.0, 0.0, 1.0}
    assert len(set(got.tolist())) >= 2
    assert len(trace["actions"]) >= 3 * (length + 1)


# ---------------------------------------------------------------- 5. learning
# By the rule of DESIGN.md "Device environment", from three seeds of 10,000 windows at K = 1 (DESIGN.md "T-maze,
# the fourth device environment", curves under profiles/tmaze/): the lr0 = 0 arm averages +0.002 and the lowest seed's
# last-tenth level is +1.000, so the mark is their midpoint; all three seeds first reported at or above it at 401
# windows, and twice that is 802.  (K = 1 clears the mark on all three seeds, so the test runs the K = 1 arm.)
LEARN_WINDOWS = 802
LEARN_MARK = 0.501


def test_the_lstm_learns_the_tmaze_and_the_ff_model_cannot(gpu):
    """scripts/train_catch.py's train() at --env tmaze --length 4, 256 envs, t_max 5, the reference's
    hyperparameters (RMSpropAsync lr 7e-4, alpha 0.99, eps 0.1, clip 40, beta 0.01), seed 0.  --arch lstm: the
    episodes of the last tenth of LEARN_WINDOWS windows average at least LEARN_MARK (measured: +0.99).  --arch ff,
    the same settings and length: the last-tenth mean lies within 5 / sqrt(n) of 0, n the episodes of that tenth
    -- returns lie in [-1, 1] and the expectation is exactly 0, whatever the FF model learns, because its input at
    the junction is the same for both cues (test_tmaze.py test_ff_blindness_from_length_four_on): a condition, not
    a measurement.  The LSTM with lr0 = 0 gets the same bound."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import train_catch
    # (window 0 runs eagerly before the first report: reports of 81 windows leave the last one 72, the last tenth)
    kw = dict(env="tmaze", length=4, envs=256, windows=LEARN_WINDOWS, report=LEARN_WINDOWS // 10 + 1, seed=0,
              device=str(gpu), log=lambda *a: None)
    last = train_catch.train(arch="lstm", lr=7e-4, **kw)[-1]
    ff = train_catch.train(arch="ff", lr=7e-4, **kw)[-1]
    frozen = train_catch.train(arch="lstm", lr=0.0, **kw)[-1]
    print("T-maze, L = 4: LSTM %+.4f over %d episodes; FF %+.4f over %d; LSTM at lr0 = 0 %+.4f over %d"
          % (last["mean_return"], last["episodes"], ff["mean_return"], ff["episodes"], frozen["mean_return"],
             frozen["episodes"]))
    assert last["windows"] == LEARN_WINDOWS and last["episodes"] == 72 * 256 == ff["episodes"] == frozen["episodes"]
    assert last["mean_return"] >= LEARN_MARK, last
    for arm in (ff, frozen):
        assert abs(arm["mean_return"]) <= 5.0 / arm["episodes"] ** 0.5, arm
