"""GPU: device-side episode statistics (arl_net_set_episode_stats / arl_episode_stats_reset /
arl_episode_stats; a3c_ale.py:95-96,114-124 episode_r, total_r) against the NumPy float64
replay of episode_replay.py, bit for bit: the per-env arrays every ring kernel accumulates,
the fixed-order reduce, clear, env-range launches, force_reset, graph replay, the feature
off, and run_episodes(scores="device").

Every comparison is exact: all sums are f64 round-to-nearest ops in env-step order on both
sides, integers are int64."""
import numpy as np
import pytest
import torch

from episode_replay import BUFFERS, CLEARED, F64, LOG, Replay, case_pools, same_bits

pytestmark = pytest.mark.gpu

ESTATE = 3
HYPER = dict(resize_mode=0, gamma=0.99, beta=0.01, v_loss_coef=0.5, clip_reward=True, lr0=7e-4, total_steps=0,
             n_total=0, alpha=0.99, eps=0.1, clip=40.0)
_PAIRS = {}


def dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def pair_pool(P, n, gpu):
    """(P, n, 2, 210, 160, 3) uint8 frame pairs, made once per shape and shared (read only)."""
    if (P, n) not in _PAIRS:
        g = torch.Generator(device="cpu").manual_seed(P * 1000 + n)
        _PAIRS[P, n] = torch.randint(0, 256, (P, n, 2, 210, 160, 3), dtype=torch.uint8, generator=g).to(gpu)
    return _PAIRS[P, n]


def make_net(arch, A, n, T, gpu, seed=3):
    from asyncrl_amd import DeviceNet, init_like_torch
    net = DeviceNet(arch, A, n, T, seed=seed, device=gpu)
    net.load_params(init_like_torch(arch, A, np.random.default_rng(seed)))
    net.reset()
    return net


def ep_buffers(net):
    torch.cuda.synchronize()
    out = {}
    for k in BUFFERS:
        shape = (LOG, net.n_envs) if k in ("ep_log_ret", "ep_log_len", "ep_log_step") else (net.n_envs,)
        out[k] = net.buffer(k, torch.float64 if k in F64 else torch.int64, shape).cpu().numpy()
    return out


def reduce_raw(net, clear=0):
    from asyncrl_amd._lib import lib, ptr, stream_handle
    out = torch.full((8,), 123.0, dtype=torch.float64, device=net.device)
    assert lib.arl_episode_stats(net.handle, ptr(out), clear, stream_handle()) == 0
    return out.cpu().numpy()


def assert_matches(net, rp):
    """Every ep_* buffer and the reduce equal the replay bit for bit; then clear=1: the same
    values once more, a second read gives zeros and +-inf, the running episode and the log stay."""
    got = ep_buffers(net)
    bad = [k for k in BUFFERS if not same_bits(got[k], rp.b[k])]
    assert not bad, {k: (got[k], rp.b[k]) for k in bad}
    want = rp.reduce()
    assert same_bits(reduce_raw(net), want), (reduce_raw(net), want)
    assert same_bits(reduce_raw(net, clear=1), want)
    rp.reduce(clear=True)
    zero = np.array([0, 0, 0, np.inf, -np.inf, 0, 0, 0], np.float64)
    assert same_bits(reduce_raw(net), zero)
    after = ep_buffers(net)
    bad = [k for k in BUFFERS if not same_bits(after[k], rp.b[k])]
    assert not bad, bad
    assert all(same_bits(after[k], got[k]) for k in BUFFERS if k not in CLEARED)


def manual_windows(net, pools, P, w0, windows, observe=None, act=True):
    """Windows w0 .. w0 + windows - 1 from observe / act / advance (slot 0 of a continuing
    window is the previous window's bootstrap observation)."""
    T = net.t_max
    observe = observe or (lambda t, k: net.observe(t, *pools, P, force_reset=(k == 0)))
    for w in range(w0, w0 + windows):
        for t in range(0 if w == 0 else 1, T + 1):
            observe(t, w * T + t)
            if act:
                net.act(t, mode=1 if t < T else 0)
        net.advance()


def test_bitwise_against_replay_ff(gpu):
    """FF, 40 envs (a ragged second 32-env group), t_max 5, pool of 7 (out of phase with the
    window): 6 windows from observe / act / advance, then 6 through arl_run_window."""
    from asyncrl_amd._lib import ARCH_FF
    n, T, P = 40, 5, 7
    rewards, dones = case_pools(1, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    net = make_net(ARCH_FF, 4, n, T, gpu)
    net.set_episode_stats(True)
    manual_windows(net, pools, P, 0, 6)
    rp = Replay(n).run(rewards, dones, 1, 6 * T + 1)
    got = ep_buffers(net)
    assert all(same_bits(got[k], rp.b[k]) for k in BUFFERS), [k for k in BUFFERS if not same_bits(got[k], rp.b[k])]
    for _ in range(6):
        net.run_window(*pools, P, first=False, **HYPER)
    rp.run(rewards, dones, 6 * T + 1, 12 * T + 1)
    assert rp.b["ep_count"][0] == 0 and rp.b["ep_count"][1] == 60 and rp.b["ep_count"][2] > LOG
    assert_matches(net, rp)
    # the Python surface on the same state: one 64-byte copy, host-derived figures; the log views
    net.run_window(*pools, P, first=False, **HYPER)
    rp.run(rewards, dones, 12 * T + 1, 13 * T + 1)
    want = rp.reduce()
    st = net.episode_stats()
    assert st["episodes"] == int(want[0]) and st["return_sum"] == want[1] and st["steps"] == n * T
    assert st["mean"] == want[1] / want[0] and st["mean_length"] == want[5] / want[0]
    log = net.episode_log()
    assert same_bits(log["ret"].cpu().numpy(), rp.b["ep_log_ret"])
    assert same_bits(log["count"].cpu().numpy(), rp.b["ep_log_count"])
    # arl_episode_stats_reset: the whole block as arl_net_reset leaves it
    net.episode_stats_reset()
    fresh = Replay(n)
    got = ep_buffers(net)
    assert all(same_bits(got[k], fresh.b[k]) for k in BUFFERS)


@pytest.mark.parametrize("kind", ["rgb", "stack", "states", "nature", "lstm"])
def test_other_observation_kernels(gpu, kind):
    """rgb_ring_kernel, stack_ring_kernel (uint8 stacks and f32 states, with a bookkeeping-only
    observation from a null pool), and phi_ring_kernel under the Nature-head and LSTM nets:
    33 envs, t_max 2, 4 windows."""
    from asyncrl_amd._lib import ARCH_FF, ARCH_FF_NATURE, ARCH_LSTM, ARCH_RGB, ARCH_STACK, ARCH_STATES
    n, T, P, W = 33, 2, 5, 4
    rewards, dones = case_pools(2, P, n)
    dr, dd = dev(rewards, gpu), dev(dones, gpu)
    arch = {"rgb": ARCH_FF | ARCH_RGB, "stack": ARCH_FF | ARCH_STACK, "states": ARCH_FF | ARCH_STATES,
            "nature": ARCH_FF_NATURE, "lstm": ARCH_LSTM}[kind]
    g = torch.Generator(device="cpu").manual_seed(5)
    if kind == "rgb":
        frames = torch.randint(0, 256, (P, n, 16, 16, 3), dtype=torch.uint8, generator=g).to(gpu)
    elif kind == "stack":
        frames = torch.randint(0, 256, (P, n, 4, 84, 84), dtype=torch.uint8, generator=g).to(gpu)
    elif kind == "states":
        frames = torch.rand((P, n, 4, 84, 84), dtype=torch.float32, generator=g).to(gpu)
    else:
        frames = pair_pool(P, n, gpu)
    net = make_net(arch, 3, n, T, gpu)
    net.set_episode_stats(True)
    last = (W - 1) * T + T

    def observe(t, k):
        if kind in ("stack", "states") and k == last:      # reward / done only: no frame, no forward after it
            net.observe_stack(t, None, dr, dd, P)
        else:
            net.observe(t, frames, dr, dd, P, force_reset=(k == 0))

    manual_windows(net, None, P, 0, W - 1, observe)
    for t in range(1, T + 1):                              # the last window, without the forward of a frameless slot
        observe(t, (W - 1) * T + t)
        if (W - 1) * T + t != last or kind not in ("stack", "states"):
            net.act(t, mode=1 if t < T else 0)
    rp = Replay(n).run(rewards, dones, 1, W * T + 1)
    assert rp.b["ep_count"][1] == W * T and rp.b["ep_count"][0] == 0
    assert_matches(net, rp)


def test_env_range_launches_on_two_streams(gpu):
    """arl_observe_envs over [0, 32) and [32, 40) on two streams == the whole-range launch."""
    from asyncrl_amd._lib import ARCH_FF
    n, T, P, W = 40, 5, 7, 3
    rewards, dones = case_pools(3, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    whole = make_net(ARCH_FF, 4, n, T, gpu)
    split = make_net(ARCH_FF, 4, n, T, gpu)
    for net in (whole, split):
        net.set_episode_stats(True)
    manual_windows(whole, pools, P, 0, W, act=False)
    main = torch.cuda.current_stream()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def observe(t, k):
        for s, envs in ((s1, (0, 32)), (s2, (32, 8))):
            s.wait_stream(main)
            split.observe(t, *pools, P, force_reset=(k == 0), stream=s, envs=envs)
            main.wait_stream(s)

    manual_windows(split, pools, P, 0, W, observe, act=False)
    a, b = ep_buffers(whole), ep_buffers(split)
    assert all(same_bits(a[k], b[k]) for k in BUFFERS)
    assert_matches(split, Replay(n).run(rewards, dones, 1, W * T + 1))


def test_off_means_off(gpu):
    """Never enabled: arl_episode_stats is ARL_ESTATE, the block stays as arl_net_reset left
    it, and logits, gradients and parameters of 2 windows at 33 envs are bit-identical to a
    run with the feature on."""
    from asyncrl_amd._lib import ARCH_FF, lib, ptr, stream_handle
    n, T, P = 33, 5, 7
    rewards, dones = case_pools(4, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    outs = []
    for on in (False, True):
        net = make_net(ARCH_FF, 4, n, T, gpu)
        if on:
            net.set_episode_stats(True)
        grads = []
        for w in range(2):
            for t in range(0 if w == 0 else 1, T + 1):
                net.observe(t, *pools, P, force_reset=(w == 0 and t == 0))
                net.act(t, mode=1 if t < T else 0)
            net.learn()
            grads.append(net.grads.clone())
            net.optimize(advance=True)
        torch.cuda.synchronize()
        outs.append((net.buffer("logits", torch.float32, (T + 1, n, 4)).clone(), grads[0], grads[1],
                     net.params.clone(), net.ms.clone()))
        if not on:
            out = torch.zeros(8, dtype=torch.float64, device=gpu)
            assert lib.arl_episode_stats(net.handle, ptr(out), 0, stream_handle()) == ESTATE
            got, fresh = ep_buffers(net), Replay(n)
            assert all(same_bits(got[k], fresh.b[k]) for k in BUFFERS)
        else:
            assert_matches(net, Replay(n).run(rewards, dones, 1, 2 * T + 1))
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert float(outs[0][1].abs().max()) > 0


def test_force_reset_abandons_the_running_episode(gpu):
    from asyncrl_amd._lib import ARCH_FF
    n, T, P = 4, 5, 6
    rewards = np.full((P, n), 0.3, np.float32)
    rewards[4] = 2.0
    dones = np.zeros((P, n), np.uint8)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    net = make_net(ARCH_FF, 4, n, T, gpu)
    net.set_episode_stats(True)
    rp = Replay(n)
    for t in range(5):
        net.observe(t, *pools, P, force_reset=(t in (0, 3)))
        if t >= 1:
            rp.step(rewards[t], dones[t], t)
        if t in (0, 3):
            rp.force_reset()
    got = ep_buffers(net)
    assert (got["ep_count"] == 0).all() and (got["ep_log_count"] == 0).all()     # not an episode
    assert (got["ep_run_ret"] == 2.0).all() and (got["ep_run_len"] == 1).all()   # only the step after it
    assert (got["ep_steps"] == 4).all()                                          # total_r still has every reward
    x = np.float64(np.float32(0.3))
    assert (got["ep_total"] == ((x + x) + x) + 2.0).all()
    assert_matches(net, rp)


def test_graph_replay(gpu):
    """A window captured with the feature on, replayed 3 times: the statistics of 3 windows."""
    from asyncrl_amd._lib import ARCH_FF
    n, T, P = 8, 5, 7
    rewards, dones = case_pools(5, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    net = make_net(ARCH_FF, 4, n, T, gpu)
    net.set_episode_stats(True)
    net.run_window(*pools, P, first=True, **HYPER)
    net.episode_stats_reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        net.run_window(*pools, P, first=False, **HYPER)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert_matches(net, Replay(n).run(rewards, dones, T + 1, 4 * T + 1))


def test_device_scored_evaluation(gpu):
    """run_episodes(scores="device") == scores="host" bit for bit (greedy play on the stub
    emulator of test_gpu_eval), and more than ARL_EPISODE_LOG episodes per env is refused."""
    from fake_ale import FakeALEActions
    from asyncrl_amd import A3CFF, run_episodes
    from asyncrl_amd.envs import VecALE
    n_envs, n_runs, seed, nullops = 3, 5, 5, 4
    model, res = None, {}
    for how in ("host", "device"):
        vec = VecALE([FakeALEActions() for _ in range(n_envs)], device=gpu, seed=seed, max_start_nullops=nullops)
        if model is None:
            model = A3CFF(vec.number_of_actions, n_envs=n_envs, t_max=5, seed=3, init_seed=7, frames="pairs")
        model.net.reset()
        res[how] = run_episodes(model, vec, n_runs, deterministic=True, max_steps=500, scores=how)
        vec.close()
    (hs, ht), (ds, dt) = res["host"], res["device"]
    assert (ht["actions"] == dt["actions"]).all() and (ht["dones"] == dt["dones"]).all()
    assert same_bits(hs, ds), (hs, ds)
    assert np.abs(hs).max() > 0
    assert not model.net.episode_stats_on                     # left as it was found
    vec = VecALE([FakeALEActions() for _ in range(n_envs)], device=gpu, seed=seed, max_start_nullops=nullops)
    with pytest.raises(ValueError):
        run_episodes(model, vec, n_envs * LOG + 1, deterministic=True, max_steps=500, scores="device")
    with pytest.raises(ValueError):
        run_episodes(model, vec, n_runs, deterministic=True, scores="gpu")
    vec.close()
