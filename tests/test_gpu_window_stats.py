"""GPU: device-side window statistics (arl_net_set_window_stats / arl_window_stats_reset;
a3c.py:123-124,136-141,161-163: losses, gradient norm, entropy, value per update) against the
NumPy float64 replay of window_replay.py and the oracle.

After each window the test synchronises and snapshots the workspace arrays the record was
computed from (they stay valid until the next window's first launch).  Fields 0..13 are
compared bit for bit: f64 round-to-nearest sums in one fixed order on both sides."""
import numpy as np
import pytest
import torch

import oracle as O
from window_replay import FIELDS, LOG, NAMES, case_pools, replay, same_bits

pytestmark = pytest.mark.gpu

F = {k: i for i, k in enumerate(NAMES)}
LR0, TOTAL = 7e-4, 10_000
HYPER = dict(resize_mode=0, gamma=0.99, beta=0.01, v_loss_coef=0.5, clip_reward=True, lr0=LR0, total_steps=TOTAL,
             n_total=40, alpha=0.99, eps=0.1, clip=40.0)
_PAIRS = {}


def dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def pair_pool(P, n, gpu):
    """(P, n, 2, 210, 160, 3) uint8 frame pairs, made once per shape and shared (read only)."""
    if (P, n) not in _PAIRS:
        g = torch.Generator(device="cpu").manual_seed(P * 1000 + n)
        _PAIRS[P, n] = torch.randint(0, 256, (P, n, 2, 210, 160, 3), dtype=torch.uint8, generator=g).to(gpu)
    return _PAIRS[P, n]


def make_net(arch, A, n, T, gpu, seed=3, on=True):
    from asyncrl_amd import DeviceNet, init_like_torch
    net = DeviceNet(arch, A, n, T, seed=seed, device=gpu)
    net.load_params(init_like_torch(arch, A, np.random.default_rng(seed)))
    net.reset()
    if on:
        net.set_window_stats(True)
    return net


def snapshot(net):
    """Host copies of what the last window left: the record's inputs, the learner's other inputs and the gradient."""
    torch.cuda.synchronize()
    T, n, A, f32 = net.t_max, net.n_envs, net.n_actions, torch.float32
    b = lambda name, dt, shape: net.buffer(name, dt, shape).cpu().numpy()   # noqa: E731
    return dict(rewards=b("rewards", f32, (T, n)), dones=b("dones", torch.uint8, (T, n)), v=b("v", f32, (T + 1, n)),
                entropy=b("entropy", f32, (T + 1, n)), loss=b("loss", f32, (n, 2)), probs=b("probs", f32, (T + 1, n, A)),
                logp=b("logp", f32, (T + 1, n, A)), actions=b("actions", torch.int32, (T + 1, n)),
                grads=net.grads.cpu().numpy())


def log_and_count(net):
    torch.cuda.synchronize()
    return (net.buffer("win_log", torch.float64, (LOG, FIELDS)).cpu().numpy(),
            int(net.buffer("win_count", torch.int64, (1,)).cpu().numpy()[0]))


def check_replay(rec, snap, window, step, gamma=0.99, clip_reward=True):
    """Fields 0..13 of one record, bit for bit."""
    want = np.concatenate([[float(window), float(step)],
                           replay(snap["rewards"], snap["dones"], snap["v"], snap["entropy"], snap["loss"], gamma,
                                  clip_reward)])
    bad = [(NAMES[i], rec[i], want[i]) for i in range(14) if not same_bits(np.float64(rec[i]), np.float64(want[i]))]
    assert not bad, bad


def check_norm(rec, snap):
    """Field 14 within 1e-5 relative of the f64 squared norm of the gradient (the partials are f32 per thread)."""
    g = snap["grads"].astype(np.float64)
    sq = float((g * g).sum())
    assert sq > 0 and abs(rec[F["grad_sqnorm"]] - sq) <= 1e-5 * sq, (rec[F["grad_sqnorm"]], sq)


def manual_window(net, w, observe, learn, **opt):
    T = net.t_max
    for t in range(0 if w == 0 else 1, T + 1):
        observe(t, w * T + t)
        net.act(t, mode=1 if t < T else 0)
    learn()
    net.optimize(advance=True, **opt)


def test_ff_against_replay_and_oracle(gpu):
    """FF, 40 envs (a ragged second 32-env group), t_max 5, pool of 7: 6 windows from observe /
    act / learn / optimize(advance), then 6 through arl_run_window (the returns fused into the
    bootstrap launch, the clip norm folded into the conv reduce)."""
    from asyncrl_amd._lib import ARCH_FF
    n, T, P, A = 40, 5, 7, 4
    rewards, dones = case_pools(1, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    net = make_net(ARCH_FF, A, n, T, gpu)
    observe = lambda t, k: net.observe(t, *pools, P, force_reset=(k == 0))   # noqa: E731
    for w in range(12):
        if w < 6:
            manual_window(net, w, observe, net.learn, lr0=LR0, total_steps=TOTAL, n_total=n, clip=40.0)
        else:
            net.set_norm_fold(True)
            net.run_window(*pools, P, first=False, **HYPER)
        s = snapshot(net)
        rec = net.window_stats_raw()[0]
        check_replay(rec, s, w, w * T)
        assert rec[F["samples"]] == T * n and rec[F["terminals"]] >= T           # env 1 terminates at every step
        _, _, _, _, pi, vl = O.returns_and_lossgrad(s["rewards"], s["dones"], s["v"][:T], s["v"][T], s["probs"][:T],
                                                    s["logp"][:T], s["actions"][:T], gamma=0.99, beta=0.01,
                                                    v_loss_coef=0.5, clip_reward=True)
        for name, want in (("pi_loss", pi), ("v_loss", vl)):
            got = rec[F[name]]
            print(f"window {w} {name}: device {got!r} oracle {want!r}")
            assert abs(got - want) <= 1e-5 * max(abs(got), abs(want)), (w, name, got, want)
        check_norm(rec, s)
        assert rec[F["clip_scale"]] == 1.0 or rec[F["grad_sqnorm"]] > 1600.0
        lr = np.float32(O.annealed_lr(LR0, TOTAL, (w * T + T) * n))
        assert rec[F["lr"]] == float(lr) and np.float32(rec[F["lr"]]) == lr, (rec[F["lr"]], lr)
    d = net.window_stats(last=2)
    assert [x["window"] for x in d] == [10, 11] and d[1]["samples"] == T * n and d[1]["grad_norm"] > 0


def test_striding_past_256_envs(gpu):
    """300 envs: threads 0..43 own two envs each.  ARCH_STACK observations (25 MB of stacks)."""
    from asyncrl_amd._lib import ARCH_FF, ARCH_STACK
    n, T, P = 300, 2, 3
    rewards, dones = case_pools(6, P, n)
    g = torch.Generator(device="cpu").manual_seed(11)
    stacks = torch.randint(0, 256, (P, n, 4, 84, 84), dtype=torch.uint8, generator=g).to(gpu)
    dr, dd = dev(rewards, gpu), dev(dones, gpu)
    net = make_net(ARCH_FF | ARCH_STACK, 3, n, T, gpu)
    observe = lambda t, k: net.observe(t, stacks, dr, dd, P, force_reset=(k == 0))   # noqa: E731
    for w in range(2):
        manual_window(net, w, observe, net.learn)
        s = snapshot(net)
        rec = net.window_stats_raw()[0]
        check_replay(rec, s, w, w * T)
        check_norm(rec, s)
        assert rec[F["samples"]] == T * n


def test_window_longer_than_the_register_path(gpu):
    """t_max 9: the kernel keeps windows up to 8 steps in registers and loops over longer ones.
    5 envs, 2 windows, the second truncated to 7 steps (arl_truncate_window)."""
    from asyncrl_amd._lib import ARCH_FF
    n, T, P = 5, 9, 4
    rewards, dones = case_pools(8, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    net = make_net(ARCH_FF, 4, n, T, gpu)
    observe = lambda t, k: net.observe(t, *pools, P, force_reset=(k == 0))   # noqa: E731

    def learn_truncated():
        net.truncate_window(7)
        net.learn()

    for w in range(2):
        manual_window(net, w, observe, net.learn if w == 0 else learn_truncated)
        s = snapshot(net)
        rec = net.window_stats_raw()[0]
        check_replay(rec, s, w, w * T)
        check_norm(rec, s)
        assert rec[F["samples"]] == (T if w == 0 else 7) * n


@pytest.mark.parametrize("kind,gamma,clip_reward", [("lstm", 0.99, True), ("nature", 0.9, False),
                                                    ("states", 0.95, False), ("rgb", 0.99, True)])
def test_other_nets(gpu, kind, gamma, clip_reward):
    """LSTM, the Nature head (its own learner), f32 states and RGB screens: 33 envs, t_max 2,
    3 windows; gamma and clip_reward as the learn call gave them."""
    from asyncrl_amd._lib import ARCH_FF, ARCH_FF_NATURE, ARCH_LSTM, ARCH_RGB, ARCH_STATES
    n, T, P = 33, 2, 5
    rewards, dones = case_pools(2, P, n)
    dr, dd = dev(rewards, gpu), dev(dones, gpu)
    arch = {"lstm": ARCH_LSTM, "nature": ARCH_FF_NATURE, "states": ARCH_FF | ARCH_STATES, "rgb": ARCH_FF | ARCH_RGB}[kind]
    g = torch.Generator(device="cpu").manual_seed(5)
    if kind == "rgb":
        frames = torch.randint(0, 256, (P, n, 16, 16, 3), dtype=torch.uint8, generator=g).to(gpu)
    elif kind == "states":
        frames = torch.rand((P, n, 4, 84, 84), dtype=torch.float32, generator=g).to(gpu)
    else:
        frames = pair_pool(P, n, gpu)
    net = make_net(arch, 3, n, T, gpu)
    observe = lambda t, k: net.observe(t, frames, dr, dd, P, force_reset=(k == 0))   # noqa: E731
    learn = lambda: net.learn(gamma=gamma, clip_reward=clip_reward)                   # noqa: E731
    for w in range(3):
        manual_window(net, w, observe, learn)
        s = snapshot(net)
        rec = net.window_stats_raw()[0]
        check_replay(rec, s, w, w * T, gamma, clip_reward)
        check_norm(rec, s)
        assert rec[F["lr"]] == float(np.float32(LR0))                                 # no anneal without a step budget
    if not clip_reward:
        assert abs(rec[F["reward_sum"]]) > 0 and np.abs(s["rewards"]).max() > 1


def test_truncated_window_of_the_dropin(gpu):
    """The one-env A3C.act drop-in (phi = dqn_phi, keep_loss_scale_same): an episode that ends
    3 steps into a window gives a record of 3 live samples and 1 terminal; the next full
    window one of 5."""
    from asyncrl_amd import A3C, A3CFF, GradientClipping, RMSpropAsync, dqn_phi
    T, A = 5, 4
    model = A3CFF(A, n_envs=1, t_max=T, seed=4, init_seed=2, device=gpu)
    opt = RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99).setup(model)
    opt.add_hook(GradientClipping(40.0))
    agent = A3C(model, opt, T, 0.99, phi=dqn_phi, keep_loss_scale_same=True)
    net = model.net
    net.set_window_stats(True)
    rng = np.random.default_rng(9)
    state = lambda: list(rng.integers(0, 256, (4, 84, 84), dtype=np.uint8))   # noqa: E731
    rewards = [0.0, 2.0, -0.3, 0.7]
    for k in range(3):
        assert isinstance(agent.act(state(), rewards[k], False), int)
    assert agent.act(state(), rewards[3], True) is None          # terminal: the update of a 3-step window
    s = snapshot(net)
    rec = agent.window_stats()[0]
    assert rec["samples"] == 3 and rec["terminals"] == 1 and rec["window"] == 0
    assert (s["dones"][:, 0] == [0, 0, 1, 2, 2]).all()
    check_replay(net.window_stats_raw()[0], s, 0, 0)
    assert rec["reward_sum"] == (1.0 + float(np.float32(-0.3))) + float(np.float32(0.7))   # 2.0 clipped
    # a full window's act goes on to slot 0 of the next window with the new parameters: snapshot between the two
    snaps, update = [], agent._update
    agent._update = lambda *a, **k: (update(*a, **k), snaps.append(snapshot(net)))
    for k in range(5):
        assert isinstance(agent.act(state(), 0.5, False), int)
    assert not snaps
    assert isinstance(agent.act(state(), 0.5, False), int)       # the bootstrap observation: a full window's update
    s, = snaps
    raw = net.window_stats_raw(last=5)
    assert raw.shape == (2, FIELDS) and raw[1, F["samples"]] == 5 and raw[1, F["terminals"]] == 0
    assert raw[1, F["window"]] == 1
    check_replay(raw[1], s, 1, raw[1, F["step"]])
    assert (s["dones"][:, 0] == 0).all()


def real_params(net, flat):
    """The unpadded parameters of a flat array, in layout order."""
    return np.concatenate([flat[off:off + int(np.prod(shape))] for off, shape in net.layout.values()])


@pytest.mark.parametrize("clip", [0.5, 0.0])
def test_recorded_scale_and_lr_are_the_ones_applied(gpu, clip):
    """clip 0.5 (it clips) and clip 0 (disabled: scale 1, the norm still recorded): params and ms after the update
    equal oracle.rmsprop_update on the gradient scaled by the recorded clip_scale at the recorded lr, bit for bit."""
    from asyncrl_amd._lib import ARCH_FF
    n, T, P = 33, 5, 7
    rewards, dones = case_pools(4, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    net = make_net(ARCH_FF, 4, n, T, gpu)
    for t in range(T + 1):
        net.observe(t, *pools, P, force_reset=(t == 0))
        net.act(t, mode=1 if t < T else 0)
    net.learn()
    torch.cuda.synchronize()
    p0, ms0, g = net.params.cpu().numpy(), net.ms.cpu().numpy() + np.float32(0.25), net.grads.cpu().numpy()
    net.ms.copy_(dev(ms0, gpu))                                   # a non-trivial second moment
    net.optimize(lr0=LR0, total_steps=TOTAL, n_total=n, clip=clip, advance=True)
    s = snapshot(net)
    rec = net.window_stats_raw()[0]
    check_norm(rec, s)
    scale, lr = rec[F["clip_scale"]], rec[F["lr"]]
    if clip > 0:
        assert 0 < scale < 1 and abs(scale - clip / np.sqrt(rec[F["grad_sqnorm"]])) <= 1e-6 * scale   # an f32 of it
    else:
        assert scale == 1.0
    assert lr == float(np.float32(O.annealed_lr(LR0, TOTAL, T * n)))
    gs = (g * np.float32(scale)).astype(np.float32)
    p1, ms1 = O.rmsprop_update(p0, ms0, gs, lr)
    assert same_bits(real_params(net, net.params.cpu().numpy()).view(np.int32), real_params(net, p1).view(np.int32))
    assert same_bits(real_params(net, net.ms.cpu().numpy()).view(np.int32), real_params(net, ms1).view(np.int32))
    assert not same_bits(real_params(net, p1).view(np.int32), real_params(net, p0).view(np.int32))


def test_ring_wrap(gpu):
    """70 windows through a ring of 64: slot k % 64 holds window k."""
    from asyncrl_amd._lib import ARCH_FF
    n, T, P, W = 8, 2, 3, 70
    rewards, dones = case_pools(7, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    net = make_net(ARCH_FF, 4, n, T, gpu)
    hyper = dict(HYPER, n_total=n)
    for w in range(W):
        net.run_window(*pools, P, first=(w == 0), **hyper)
    s = snapshot(net)
    log, count = log_and_count(net)
    assert count == W
    for k in range(W - LOG, W):
        assert log[k % LOG, F["window"]] == k and log[k % LOG, F["step"]] == k * T and log[k % LOG, F["samples"]] == T * n
    raw = net.window_stats_raw(last=LOG)
    assert raw.shape == (LOG, FIELDS) and (raw[:, F["window"]] == np.arange(W - LOG, W)).all()
    assert net.window_stats_raw(last=100).shape == (LOG, FIELDS)
    assert same_bits(net.window_stats_raw(last=100), raw)
    assert net.window_stats_raw(last=3)[:, F["window"]].tolist() == [67.0, 68.0, 69.0]
    assert net.window_stats_raw(last=0).shape == (0, FIELDS)
    check_replay(raw[-1], s, W - 1, (W - 1) * T)


def test_off_means_off(gpu):
    """Two nets, one with the feature on: logits, both gradients, params and ms of 2 windows
    at 33 envs are bit-identical; the off net's log and count stay zero and reading it raises."""
    from asyncrl_amd._lib import ARCH_FF
    n, T, P = 33, 5, 7
    rewards, dones = case_pools(4, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    outs = []
    for on in (False, True):
        net = make_net(ARCH_FF, 4, n, T, gpu, on=on)
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
        log, count = log_and_count(net)
        if on:
            assert count == 2 and log[1, F["window"]] == 1 and (log[2:] == 0).all()
        else:
            assert count == 0 and not log.view(np.uint64).any()
            with pytest.raises(ValueError):
                net.window_stats_raw()
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert float(outs[0][1].abs().max()) > 0


def test_graph_replay(gpu):
    """A window captured with the feature on and replayed 3 times: 3 new records, each equal
    to the replay of the buffers its window left."""
    from asyncrl_amd._lib import ARCH_FF
    n, T, P = 8, 5, 7
    rewards, dones = case_pools(5, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    net = make_net(ARCH_FF, 4, n, T, gpu)
    hyper = dict(HYPER, n_total=n)
    net.run_window(*pools, P, first=True, **hyper)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        net.run_window(*pools, P, first=False, **hyper)
    _, c0 = log_and_count(net)
    for i in range(3):
        g.replay()
        snap = snapshot(net)
        log, count = log_and_count(net)
        assert count == c0 + i + 1
        rec = log[(count - 1) % LOG]
        check_replay(rec, snap, rec[F["window"]], rec[F["window"]] * T)
        check_norm(rec, snap)
        assert rec[F["lr"]] == float(np.float32(O.annealed_lr(LR0, TOTAL, (rec[F["step"]] + T) * n)))
    assert log[(count - 1) % LOG, F["window"]] == log[(count - 3) % LOG, F["window"]] + 2


def test_window_stats_reset(gpu):
    from asyncrl_amd._lib import ARCH_FF
    n, T, P = 8, 2, 3
    rewards, dones = case_pools(7, P, n)
    pools = (pair_pool(P, n, gpu), dev(rewards, gpu), dev(dones, gpu))
    net = make_net(ARCH_FF, 4, n, T, gpu)
    for w in range(2):
        net.run_window(*pools, P, first=(w == 0), **dict(HYPER, n_total=n))
    log, count = log_and_count(net)
    assert count == 2 and log[:2].any(axis=1).all()
    net.window_stats_reset()
    log, count = log_and_count(net)
    assert count == 0 and not log.view(np.uint64).any()
    assert net.window_stats_raw(last=4).shape == (0, FIELDS)
    net.run_window(*pools, P, first=False, **dict(HYPER, n_total=n))
    assert net.window_stats_raw(last=4)[:, F["window"]].tolist() == [2.0]   # the control block is not the log's
    net.reset()                                                              # arl_net_reset zeroes them too
    log, count = log_and_count(net)
    assert count == 0 and not log.view(np.uint64).any()
