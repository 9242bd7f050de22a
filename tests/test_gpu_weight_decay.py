"""GPU: NonbiasWeightDecay folded into the RMSProp update kernel
(optim.hip rmsprop_kernel<DecayArgs>, arl_net_set_weight_decay, arl_rmsprop_wd)
against the NumPy restatement of the reference's update
(test_weight_decay.reference_update, itself checked against the fixture
recorded from the reference's hook).

Tolerances: without a triggering clip every op of the update is an
elementwise round-to-nearest f32 op in the reference's order, so results are
compared bit for bit.  With a triggering clip the scale is one f32 rounding of
an f64 norm on both sides, summed in different orders: rtol 1e-6, atol 1e-7
(p) / 1e-9 (ms), the bound test_rmsprop_tiny_arrays_match_oracle uses."""
import numpy as np
import pytest
import torch

import oracle as O
from sim import make_pools
from test_weight_decay import close, is_bias, reference_update

pytestmark = pytest.mark.gpu

RATE = 0.3
HYPER = dict(lr=7e-4, alpha=0.99, eps=0.1)


def dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise (torch.equal would take -0.0 for +0.0)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def np_bits_equal(a, b) -> bool:
    return bool((np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32)).all())


def _opt(clip=0.0, rate=0.0):
    from asyncrl_amd import GradientClipping, NonbiasWeightDecay, RMSpropAsync
    o = RMSpropAsync(**HYPER)
    if clip > 0:
        o.add_hook(GradientClipping(clip))
    if rate > 0:
        o.add_hook(NonbiasWeightDecay(rate))
    return o


def _arrays(n, gscale=1.0):
    rng = np.random.default_rng(200 + n)
    p = rng.standard_normal(n).astype(np.float32)
    ms = (np.abs(rng.standard_normal(n)) * 0.01).astype(np.float32)
    g = (rng.standard_normal(n) * gscale).astype(np.float32)
    return p, ms, g


# tail only, tail of 3, one exact float4, float4 + tail, more than one block (1027 = 256 float4 + 1 float4 + 3);
# the last: one full pass of the launch's cap (2,048 x 256 float4), so that threads take a second pass (the
# loop's reload branch), plus a float4 and a tail of 3
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 2048 * 256 * 4 + 1027])
def test_update_arrays_decay_bit_exact(gpu, n):
    p, ms, g = _arrays(n)
    opt = _opt(rate=RATE)
    P, M, G = dev(p, gpu), dev(ms, gpu), dev(g, gpu)
    opt.update_arrays(P, M, G, nonbias=True)
    p1, m1 = reference_update({"W": p}, {"W": ms}, {"W": g}, RATE, 0.0, **HYPER)
    assert np_bits_equal(P.cpu().numpy(), p1["W"]) and np_bits_equal(M.cpu().numpy(), m1["W"])
    assert np_bits_equal(G.cpu().numpy(), g)          # the gradient array is read, not written
    p0, m0 = O.rmsprop_update(p, ms, g, HYPER["lr"])
    assert not (p1["W"] == p0).all()                  # (the decay moves the result)
    # nonbias=False with the hook installed: today's arl_rmsprop
    P, M = dev(p, gpu), dev(ms, gpu)
    opt.update_arrays(P, M, G)
    assert np_bits_equal(P.cpu().numpy(), p0) and np_bits_equal(M.cpu().numpy(), m0)
    P2, M2 = dev(p, gpu), dev(ms, gpu)
    _opt().update_arrays(P2, M2, G, nonbias=True)     # nonbias=True without the hook: the same
    assert bits_equal(P, P2) and bits_equal(M, M2)


def test_update_arrays_decay_after_triggering_clip(gpu):
    """The clip scales by the norm of the gradient BEFORE the decay.  With rate
    0.3 and |p| ~ 1 the wrong order (decay, then clip by the decayed norm) is
    far outside the tolerance -- asserted on the CPU with the same comparison."""
    n = 1027
    p, ms, g = _arrays(n, gscale=10.0)
    assert np.sqrt((g.astype(np.float64) ** 2).sum()) > 80.0
    P, M, G = dev(p, gpu), dev(ms, gpu), dev(g, gpu)
    _opt(clip=40.0, rate=RATE).update_arrays(P, M, G, nonbias=True)
    a = ({"W": p}, {"W": ms}, {"W": g}, RATE, 40.0)
    p1, m1 = reference_update(*a, exact_norm=True, **HYPER)
    got_p, got_m = P.cpu().numpy(), M.cpu().numpy()
    assert close("p", got_p, p1["W"]) and close("ms", got_m, m1["W"])
    pw, mw = reference_update(*a, exact_norm=True, decay_first=True, **HYPER)
    assert not close("p", pw["W"], p1["W"]) and not close("ms", mw["W"], m1["W"])
    assert not close("p", got_p, pw["W"]) and not close("ms", got_m, mw["W"])


def _rgb_pools(rng, P, N):
    pairs = rng.integers(0, 256, size=(P, N, 120, 160, 3), dtype=np.uint8)
    rewards = rng.choice([-1.0, 0.0, 1.0], p=[0.05, 0.9, 0.05], size=(P, N)).astype(np.float32)
    dones = (rng.random((P, N)) < 0.1).astype(np.uint8)
    return pairs, rewards, dones


def _agent(kind, gpu, N, T, A, opt, seed=5, init_seed=6):
    from asyncrl_amd import A3C, A3CFF, A3CFFNature, A3CLSTM, DoomA3CFF
    Model = {"ff": A3CFF, "lstm": A3CLSTM, "nature": A3CFFNature, "doom_ff": DoomA3CFF}[kind]
    m = Model(A, n_envs=N, t_max=T, seed=seed, init_seed=init_seed, frames="pairs", device=gpu)
    opt.setup(m)
    return A3C(m, opt, T, 0.99)


def _window_up_to_learn(kind, gpu, N=32, T=2, A=4, seed=91):
    """One window up to and including learn; ms gets non-zero statistics."""
    rng = np.random.default_rng(seed)
    P = T + 2
    pools = _rgb_pools(rng, P, N) if kind == "doom_ff" else make_pools(rng, P, N, "uniform", p_done=0.1)
    ag = _agent(kind, gpu, N, T, A, _opt())
    net = ag.net
    net.set_norm_fold(False)       # the tests below rescale the gradient after learn
    ag.run_window(*(dev(x, gpu) for x in pools), P, first=True, split_update=True)
    for name in net.layout:
        v = net.view(net.ms, name)
        v.copy_(dev((np.abs(rng.standard_normal(tuple(v.shape))) * 0.01).astype(np.float32), gpu))
    torch.cuda.synchronize()
    return ag


@pytest.mark.parametrize("kind,A", [("ff", 4), ("lstm", 6), ("nature", 4), ("doom_ff", 3)])
def test_net_update_matches_restatement(gpu, kind, A):
    """arl_optimize with a weight decay on the real layouts: every named tensor
    against the restatement (clip 0 bit-exact, a triggering clip 40 within the
    clipped tolerance), biases bit-equal to a decay-free update of the same
    inputs, the 64-float padding between tensors untouched."""
    ag = _window_up_to_learn(kind, gpu, A=A)
    net = ag.net
    biases = [n for n in net.layout if is_bias(n)]
    assert len(biases) == {"ff": 5, "lstm": 6, "nature": 6, "doom_ff": 5}[kind]
    assert ("1/lateral/W" in net.layout) == (kind == "lstm")
    pad = torch.ones(net.param_floats, dtype=torch.bool, device=gpu)
    for name in net.layout:
        net.view(pad, name).fill_(False)
    assert int(pad.sum()) > 0
    p_flat, ms_flat = net.params.clone(), net.ms.clone()
    p, ms = net.state_dict(p_flat), net.state_dict(ms_flat)
    for clip in (0.0, 40.0):
        if clip > 0:      # make the clip trigger: scale the gradient to a norm of 200
            net.params.copy_(p_flat)
            net.ms.copy_(ms_flat)
            net.params_changed()
            net.grads.mul_(200.0 / float(net.grads.double().norm()))
        g = net.state_dict(net.grads)
        g_flat = net.grads.clone()
        norm = np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values()))
        assert (norm > 2 * clip) if clip > 0 else norm > 0
        net.set_weight_decay(RATE)
        net.optimize(lr0=HYPER["lr"], alpha=HYPER["alpha"], eps=HYPER["eps"], clip=clip)
        torch.cuda.synchronize()
        got_p, got_ms = net.state_dict(), net.state_dict(net.ms)
        want_p, want_ms = reference_update(p, ms, g, RATE, clip, exact_norm=True, **HYPER)
        free_p, free_ms = reference_update(p, ms, g, 0.0, clip, exact_norm=True, **HYPER)
        for n in net.layout:
            if clip > 0:
                assert close("p", got_p[n], want_p[n]) and close("ms", got_ms[n], want_ms[n]), (clip, n)
            else:
                assert np_bits_equal(got_p[n], want_p[n]) and np_bits_equal(got_ms[n], want_ms[n]), (clip, n)
            assert is_bias(n) or not (want_p[n] == free_p[n]).all(), n     # the decay shows in every weight
        # biases: the decay-free update of the same inputs, run by the decay-free kernel
        net.params.copy_(p_flat)
        net.ms.copy_(ms_flat)
        net.params_changed()
        net.set_weight_decay(0.0)
        net.optimize(lr0=HYPER["lr"], alpha=HYPER["alpha"], eps=HYPER["eps"], clip=clip)
        torch.cuda.synchronize()
        plain_p, plain_ms = net.state_dict(), net.state_dict(net.ms)
        for n in biases:
            assert np_bits_equal(got_p[n], plain_p[n]) and np_bits_equal(got_ms[n], plain_ms[n]), (clip, n)
        assert bits_equal(net.params[pad], p_flat[pad]) and bits_equal(net.ms[pad], ms_flat[pad])
        assert bits_equal(net.grads, g_flat)


def test_fc_planes_follow_decayed_weights(gpu):
    """The update kernel rewrites the FC weight's split planes from the decayed
    W: a forward right after it equals the same forward after the planes are
    rebuilt from the f32 W (params_changed + prepare)."""
    ag = _window_up_to_learn("ff", gpu)
    net = ag.net
    w0 = net.param("0/2/W").clone()
    net.set_weight_decay(RATE)
    net.optimize(lr0=HYPER["lr"], alpha=HYPER["alpha"], eps=HYPER["eps"], clip=40.0)
    assert net.param_generation()[0] == net.param_generation()[1]
    assert not torch.equal(net.param("0/2/W"), w0)
    outs = []
    for rebuild in (False, True):
        if rebuild:
            net.params_changed()
            net.prepare()
        net.act(0, mode=0)
        torch.cuda.synchronize()
        o = net.step_outputs(0)
        outs.append((o["logits"].clone(), o["v"].clone()))
    assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1])


def test_fused_paths_agree_bitwise(gpu):
    """arl_run_window, the step-by-step observe / act / learn / optimize_advance
    calls and a captured-graph replay of the window apply the same decayed
    update: params, ms and actions identical after two windows."""
    rng = np.random.default_rng(93)
    N, T, P, A, rate = 33, 5, 7, 4, 0.01
    pairs, rewards, dones = make_pools(rng, P, N, "uniform", p_done=0.1)
    dp, dr, dd = dev(pairs, gpu), dev(rewards, gpu), dev(dones, gpu)

    def mk():
        o = _opt(clip=40.0, rate=rate)
        o.anneal_total_steps, o.n_total_envs = 10 ** 6, N
        return _agent("ff", gpu, N, T, A, o, seed=3, init_seed=4)

    a, b, c, plain = mk(), mk(), mk(), mk()
    plain.optimizer.hooks.pop()                 # the same windows without the decay
    for w in range(2):
        a.run_window(dp, dr, dd, P, first=(w == 0))            # one arl_run_window call a window
        plain.run_window(dp, dr, dd, P, first=(w == 0))
    net = b.net
    for w in range(2):
        for t in range(T + 1):
            if t > 0 or w == 0:
                net.observe(t, dp, dr, dd, P, force_reset=(t == 0), resize_mode=b.resize_mode)
            net.act(t)
        net.learn(b.gamma, b.beta, b._vcoef, b.clip_reward)
        net.optimize(advance=True, **b.optimizer.update_args())
    c.run_window(dp, dr, dd, P, first=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.run_window(dp, dr, dd, P, first=False)
    g.replay()
    torch.cuda.synchronize()
    acts = lambda ag: ag.net.buffer("actions", torch.int32, (T + 1, N))[:T]   # noqa: E731
    for other in (b, c):
        assert bits_equal(a.net.params, other.net.params)
        assert bits_equal(a.net.ms, other.net.ms)
        assert torch.equal(acts(a), acts(other))
    assert not torch.equal(a.net.params, plain.net.params)      # and the decay was in them


def test_rate_zero_is_todays_update(gpu):
    """set_weight_decay(0.0) and a NonbiasWeightDecay-free optimizer launch the
    decay-free kernel: bitwise the params and ms of an untouched net after two
    windows, with a -0.0 gradient element on a zero ms planted in the first."""
    rng = np.random.default_rng(95)
    N, T, P, A = 32, 2, 4, 4
    pools = [dev(x, gpu) for x in make_pools(rng, P, N, "uniform", p_done=0.1)]
    agents = [_agent("ff", gpu, N, T, A, _opt(clip=40.0), seed=3, init_seed=4) for _ in range(2)]
    agents[0].net.set_weight_decay(0.0)
    idx = agents[0].net.layout["0/2/W"][0] + 12345
    for w in range(2):
        for ag in agents:
            ag.run_window(*pools, P, first=(w == 0), split_update=True)
            if w == 0:
                ag.net.grads[idx] = -0.0
                ag.net.ms[idx] = 0.0
                assert int(ag.net.grads[idx].view(torch.int32)) == -2 ** 31
            ag.finish_window()
        if w == 0:
            torch.cuda.synchronize()
            for ag in agents:
                assert int(ag.net.ms[idx].view(torch.int32)) == 0       # +0.0 * alpha + (c * -0.0) * -0.0
    torch.cuda.synchronize()
    assert bits_equal(agents[0].net.params, agents[1].net.params)
    assert bits_equal(agents[0].net.ms, agents[1].net.ms)
