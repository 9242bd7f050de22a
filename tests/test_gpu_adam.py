"""GPU: Adam as the second fused update kernel (optim.hip adam_kernel, arl_adam,
arl_net_set_adam, asyncrl_amd.Adam) against the NumPy float32 restatement in
adam_ref.py.

Tolerances: every elementwise operation of the update is an explicit
round-to-nearest f32 operation in the oracle's order, so p, m and v are compared
bit for bit wherever the two sides use the same clip scale and step size: the
granular entry computes lr_t with the host's libm (Python's), and the net tests
replay with the clip scale and lr of the update's window-statistics record,
which come from the kernel's own device functions.  That recorded lr_t is held
to 1 f32 ulp of Python's value (beta**t by f64 binary exponentiation on the
device against the host's pow, a relative difference near 1e-13 in lr_t against
an f32 half ulp of 3e-8; equal at t = 1, where both are exact).  Only the granular clipped case compares across a
clip scale computed on both sides -- one f32 rounding of an f64 norm summed in
different orders: rtol 1e-6, atol 1e-7 (p) / 1e-9 (m, v), the bound of
test_update_arrays_decay_after_triggering_clip."""
import numpy as np
import pytest
import torch

from adam_ref import F32, adam_arrays, annealed_alpha, bits_equal, hooked_grad, lr_t, ulp_apart
from sim import make_pools
from test_weight_decay import close, is_bias

pytestmark = pytest.mark.gpu

HYPER = dict(alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
B1, B2, EPS = HYPER["beta1"], HYPER["beta2"], HYPER["eps"]
RATE, CLIP = 0.3, 40.0
N, T, P = 32, 2, 7
CTL_STEP, CTL_WINDOW, CTL_ADAM_T = 0, 1, 3


def dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def tbits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise (torch.equal would take -0.0 for +0.0)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _opt(clip=0.0, rate=0.0, adam=True, **kw):
    from asyncrl_amd import Adam, GradientClipping, NonbiasWeightDecay, RMSpropAsync
    o = Adam(**dict(HYPER, **kw)) if adam else RMSpropAsync(lr=7e-4, eps=0.1, alpha=0.99)
    if clip > 0:
        o.add_hook(GradientClipping(clip))
    if rate > 0:
        o.add_hook(NonbiasWeightDecay(rate))
    return o


_POOLS = {}


def pools(gpu):
    """The seeded frame-pair / reward / done pools every window test reads (made once, never written)."""
    if "p" not in _POOLS:
        _POOLS["p"] = tuple(dev(x, gpu) for x in make_pools(np.random.default_rng(77), P, N, "uniform", p_done=0.1))
    return _POOLS["p"]


def _agent(kind, gpu, opt, A=4, stats=False):
    from asyncrl_amd import A3C, A3CFF, A3CFFNature, A3CLSTM
    Model = {"ff": A3CFF, "lstm": A3CLSTM, "nature": A3CFFNature}[kind]
    m = Model(A, n_envs=N, t_max=T, seed=5, init_seed=6, frames="pairs", device=gpu)
    opt.setup(m)
    ag = A3C(m, opt, T, 0.99)
    if stats:
        ag.net.set_window_stats(True)
    return ag


def decay_mask(net):
    """True where NonbiasWeightDecay applies in the flat layout: everything but the bias tensors (the padding
    between tensors included: 0 + rate * 0 there)."""
    mask = np.ones(net.param_floats, bool)
    for name, (off, shape) in net.layout.items():
        if is_bias(name):
            mask[off:off + int(np.prod(shape))] = False
    return mask


def padding(net, gpu):
    pad = torch.ones(net.param_floats, dtype=torch.bool, device=gpu)
    for name in net.layout:
        net.view(pad, name).fill_(False)
    assert int(pad.sum()) > 0
    return pad


def state(net):
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (net.params, net.adam_m, net.ms)]


def replay(before, g, rec, rate, mask):
    """NumPy Adam on the flat buffers with the clip scale (field 15) and the lr (field 16) of the update's record."""
    p, m, v = before
    return adam_arrays(p, m, v, hooked_grad(p, g, scale=rec[15], rate=rate, decay=mask), F32(rec[16]), B1, B2, EPS)


def assert_state(net, want, what):
    for name, got, w in zip(("params", "adam_m", "ms"), state(net), want):
        assert bits_equal(got, w), (what, name)


# ------------------------------------------------------------------ 1. the granular entry, bit for bit
# tail only, a tail of 3, one exact float4, a float4 + tail, more than one block; the last: past the 2,048-workgroup
# cap of the launch (2,048 x 256 float4), so that threads take a second pass, plus a float4 and a tail of 3
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 2048 * 256 * 4 + 1027])
def test_arl_adam_arrays_bit_exact(gpu, n):
    rng = np.random.default_rng(300 + n % 9973)
    p = rng.standard_normal(n).astype(F32)
    gs = []
    for t in (1, 2, 3):                                               # normal-range gradients with a few exact +-0
        g = rng.standard_normal(n).astype(F32)
        z = rng.integers(0, n, min(n, 6))
        g[z[::2]], g[z[1::2]] = 0.0, -0.0
        gs.append(g)
    for rate in (0.0, RATE):
        opt = _opt(rate=rate)
        want = (p, np.zeros(n, F32), np.zeros(n, F32))
        Pd, Md, Vd = (dev(x, gpu) for x in want)
        for t, g in zip((1, 2, 3), gs):
            Gd = dev(g, gpu)
            opt.update_arrays(Pd, Md, Vd, Gd, t=t, nonbias=True)
            want = adam_arrays(*want, hooked_grad(want[0], g, rate=rate), lr_t(HYPER["alpha"], B1, B2, t), B1, B2, EPS)
            torch.cuda.synchronize()
            for name, got, w in zip("pmv", (Pd, Md, Vd), want):
                assert bits_equal(got.cpu().numpy(), w), (n, rate, t, name)
            assert bits_equal(Gd.cpu().numpy(), g)                  # the gradient is read, not written
        if rate > 0 and n > 1:                                        # (the decay moved the result)
            assert not bits_equal(want[0], free_p)
        free_p = want[0]
    o = _opt()
    o.update_arrays(Pd, Md, Vd, Gd)                                   # t=None counts the optimizer's own t
    assert o.t == 1


# ------------------------------------------------------------------ 2. a triggering clip, then the decay
def test_arl_adam_decay_after_triggering_clip(gpu):
    """The clip scales by the norm of the gradient BEFORE the decay; m and v start non-zero, so that the wrong
    order (decay, then clip by the decayed norm) is far outside the tolerance -- asserted with the same comparison."""
    n = 1027
    rng = np.random.default_rng(200 + n)
    p = rng.standard_normal(n).astype(F32)
    m = (rng.standard_normal(n) * 0.1).astype(F32)
    v = (np.abs(rng.standard_normal(n)) * 0.01).astype(F32)
    g = (rng.standard_normal(n) * 10.0).astype(F32)
    norm = np.sqrt((g.astype(np.float64) ** 2).sum())
    assert norm > 80.0
    Pd, Md, Vd, Gd = (dev(x, gpu) for x in (p, m, v, g))
    _opt(clip=CLIP, rate=RATE).update_arrays(Pd, Md, Vd, Gd, t=3, nonbias=True)
    lr = lr_t(HYPER["alpha"], B1, B2, 3)
    want = adam_arrays(p, m, v, hooked_grad(p, g, scale=CLIP / norm, rate=RATE), lr, B1, B2, EPS)
    gw = hooked_grad(p, g, rate=RATE)                                 # the wrong order
    gw = hooked_grad(p, gw, scale=CLIP / np.sqrt((gw.astype(np.float64) ** 2).sum()))
    wrong = adam_arrays(p, m, v, gw, lr, B1, B2, EPS)
    got = [x.cpu().numpy() for x in (Pd, Md, Vd)]
    for kind, a, w, x in zip(("p", "ms", "ms"), got, want, wrong):
        assert close(kind, a, w)
        assert not close(kind, x, w) and not close(kind, a, x)


# ------------------------------------------------------------------ 3. the net update
@pytest.mark.parametrize("kind,A", [("ff", 4), ("lstm", 6), ("nature", 4)])
def test_net_update_matches_the_replay(gpu, kind, A):
    """Three arl_optimize_advance updates on seeded gradients with the clip at 40 (triggering in the second) and
    NonbiasWeightDecay(0.3): params, adam_m and ms against the NumPy replay bit for bit, biases undecayed, padding
    untouched, the control block advanced, and the FC weight's split planes rewritten by the update."""
    from asyncrl_amd._lib import ARCH_FF_NATURE
    opt = _opt(clip=CLIP, rate=RATE)
    ag = _agent(kind, gpu, opt, A=A, stats=True)
    net = ag.net
    mask, pad = decay_mask(net), padding(net, gpu)
    assert net.adam_m is not None and net.adam_betas == (B1, B2)
    rng = np.random.default_rng(41)
    ctl = net.buffer("ctl", torch.int64)
    for t in (1, 2, 3):
        for name in net.layout:                                       # seeded gradients; the padding stays 0
            gv = net.view(net.grads, name)
            gv.copy_(dev((rng.standard_normal(tuple(gv.shape)) * (1.0 if t == 2 else 0.01)).astype(F32), gpu))
        before, g = state(net), net.grads.cpu().numpy()
        net.optimize(advance=True, **opt.update_args())
        rec = net.window_stats_raw(1)[0]
        assert (rec[15] < 1) == (t == 2)
        assert rec[14] == pytest.approx(float((g.astype(np.float64) ** 2).sum()), rel=1e-5)
        want_lr = F32(lr_t(HYPER["alpha"], B1, B2, t))
        assert F32(rec[16]) == rec[16] and ulp_apart(rec[16], want_lr) <= (0 if t == 1 else 1), (t, rec[16], want_lr)
        want = replay(before, g, rec, RATE, mask)
        assert_state(net, want, (kind, t))
        free = replay(before, g, rec, 0.0, mask)                      # biases: the decay-free update
        for name, (off, shape) in net.layout.items():
            sl = slice(off, off + int(np.prod(shape)))
            assert bits_equal(want[0][sl], free[0][sl]) == is_bias(name), name
        for flat in (net.params, net.adam_m, net.ms, net.grads):
            assert not flat[pad].any()
        assert ctl[[CTL_STEP, CTL_WINDOW, CTL_ADAM_T]].tolist() == [t * T, t, t]
    assert net.adam_t() == 3 and opt.t == 3
    if kind != "nature":                                              # the planes count as current: the update wrote them
        assert net.param_generation()[0] == net.param_generation()[1]
    # a forward on this net (planes from the update kernel) and on a twin that rebuilds them from the same f32 W
    net.observe(0, *pools(gpu), P, force_reset=True)
    twin = _agent(kind, gpu, _opt(), A=A).net
    twin.workspace.copy_(net.workspace)
    twin.load_params(net.state_dict())
    assert twin.param_generation()[0] != twin.param_generation()[1] or net.arch == ARCH_FF_NATURE
    outs = []
    for x in (net, twin):
        x.act(0, mode=0)
        torch.cuda.synchronize()
        o = x.step_outputs(0)
        outs.append((o["logits"].clone(), o["v"].clone()))
    assert tbits(outs[0][0], outs[1][0]) and tbits(outs[0][1], outs[1][1])
    assert outs[0][0].abs().max() > 0


# ------------------------------------------------------------------ 4. A3C(model, Adam(...))
@pytest.mark.parametrize("kind", ["ff", "lstm"])
def test_a3c_windows_one_call_and_split(gpu, kind):
    """Two windows through arl_run_window and through run_window(split_update=True) + finish_window: the same
    parameters and state bit for bit; the split run's updates equal the NumPy replay on (state before, net.grads)."""
    pl = pools(gpu)
    one = _agent(kind, gpu, _opt(clip=CLIP, rate=RATE))
    split = _agent(kind, gpu, _opt(clip=CLIP, rate=RATE), stats=True)
    mask = decay_mask(split.net)
    for w in range(2):
        one.run_window(*pl, P, first=(w == 0))
        split.run_window(*pl, P, first=(w == 0), split_update=True)
        before, g = state(split.net), split.net.grads.cpu().numpy()
        assert np.abs(g).max() > 0
        split.finish_window()
        rec = split.net.window_stats_raw(1)[0]
        assert ulp_apart(rec[16], F32(lr_t(HYPER["alpha"], B1, B2, w + 1))) <= (0 if w == 0 else 1)
        want = replay(before, g, rec, RATE, mask)
        assert_state(split.net, want, (kind, w))
        assert not bits_equal(want[0], before[0])
        for a, b in zip(state(one.net), state(split.net)):
            assert bits_equal(a, b), (kind, w)
    assert one.net.adam_t() == split.net.adam_t() == 2 and one.t == split.t == 2 * T


# ------------------------------------------------------------------ 5. graph replay: the device counter
def test_captured_window_counts_its_updates(gpu):
    """One eager window, run_window(first=False) captured on one stream and replayed twice, against three eager
    windows on a twin: params, adam_m, ms and the counter bit for bit -- each replay read its own t from the device."""
    pl = pools(gpu)
    eager = _agent("ff", gpu, _opt(clip=CLIP, rate=RATE))
    for w in range(3):
        eager.run_window(*pl, P, first=(w == 0))
    ag = _agent("ff", gpu, _opt(clip=CLIP, rate=RATE))
    ag.run_window(*pl, P, first=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ag.run_window(*pl, P, first=False)
    torch.cuda.synchronize()
    assert ag.net.adam_t() == 1                                       # (the capture ran nothing)
    g.replay()
    g.replay()
    for a, b in zip(state(ag.net), state(eager.net)):
        assert bits_equal(a, b)
    assert ag.net.adam_t() == eager.net.adam_t() == 3
    # the bias correction matters at these t: a twin held at t = 1 by the host ends elsewhere
    stuck = _agent("ff", gpu, _opt(clip=CLIP, rate=RATE))
    for w in range(3):
        stuck.run_window(*pl, P, first=(w == 0))
        stuck.net.set_adam_t(0 if w < 2 else 3)
    assert not bits_equal(state(stuck.net)[0], state(eager.net)[0])


# ------------------------------------------------------------------ 6. the on-device anneal
def test_annealed_alpha(gpu):
    """anneal_total_steps = 150 with 32 envs and t_max 2: global_t is 64, 128 and 192 at the three updates, so
    alpha_a is 85/150 and 21/150 of alpha, then 0.  The recorded lr within 1 ulp of the host formula (equal at
    t = 1), exactly 0 past the budget, where the parameters stop and the moments go on."""
    pl = pools(gpu)
    opt = _opt(clip=CLIP)
    opt.anneal_total_steps, opt.n_total_envs = 150, N
    ag = _agent("ff", gpu, opt, stats=True)
    lrs = []
    for w in range(3):
        before = state(ag.net)
        ag.run_window(*pl, P, first=(w == 0))
        rec = ag.net.window_stats_raw(1)[0]
        a = annealed_alpha(HYPER["alpha"], 150, (w * T + T) * N)
        want = F32(lr_t(a, B1, B2, w + 1))
        assert ulp_apart(rec[16], want) <= (0 if w == 0 else 1), (w, rec[16], want)
        lrs.append(rec[16])
    after = state(ag.net)
    assert lrs[0] > lrs[1] > 0 and lrs[2] == 0.0 and a == 0.0
    assert bits_equal(after[0], before[0]) and not bits_equal(after[1], before[1]) and not bits_equal(after[2], before[2])
    assert ag.net.adam_t() == 3


# ------------------------------------------------------------------ 7. checkpoints
def test_checkpoint_round_trip(gpu, tmp_path):
    from asyncrl_amd import read_hdf5
    pl = pools(gpu)
    a = _agent("lstm", gpu, _opt(clip=CLIP, rate=RATE), A=6)
    for w in range(2):
        a.run_window(*pl, P, first=(w == 0))
    a.optimizer.t = 99                                                # the file's t is the device's count
    f = str(tmp_path / "model.h5")
    a.save_model(f)
    names = set(a.net.layout)
    data = read_hdf5(f + ".opt")
    assert set(data) == {"t", "epoch"} | {n + "/m" for n in names} | {n + "/v" for n in names}
    assert int(data["t"]) == 2
    b = _agent("lstm", gpu, _opt(clip=CLIP, rate=RATE), A=6)
    assert b.net.adam_t() == 0
    b.load_model(f)
    assert b.net.adam_t() == 2 and b.optimizer.t == 2                 # written back by load (arl_net_set_adam_t)
    for x, y in zip(state(a.net), state(b.net)):
        assert bits_equal(x, y) and np.abs(x).max() > 0
    b.net.workspace.copy_(a.net.workspace)                            # the envs' state: rings, LSTM carry, step counters
    for ag in (a, b):
        ag.run_window(*pl, P, first=False)
    for x, y in zip(state(a.net), state(b.net)):
        assert bits_equal(x, y)
    assert a.net.adam_t() == b.net.adam_t() == 3


# ------------------------------------------------------------------ 8. the default path
def test_default_is_untouched(gpu):
    """An RMSpropAsync net that never saw Adam and one switched to Adam and back before any update: params, ms,
    gradients and the window records of two windows, bit for bit; and RMSpropAsync.setup switches a net back."""
    pl = pools(gpu)
    outs = []
    for touch in (False, True):
        ag = _agent("ff", gpu, _opt(clip=CLIP, adam=False), stats=True)
        if touch:
            ag.net.set_adam(B1, B2)
            ag.net.adam_m.fill_(7.0)
            ag.net.set_adam(None)
        for w in range(2):
            ag.run_window(*pl, P, first=(w == 0))
        torch.cuda.synchronize()
        outs.append([ag.net.params.cpu().numpy(), ag.net.ms.cpu().numpy(), ag.net.grads.cpu().numpy(),
                     ag.net.window_stats_raw(2)])
        assert ag.net.adam_t() == 0
        if touch:
            assert bool((ag.net.adam_m == 7.0).all())
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes() and np.abs(x).max() > 0
    assert outs[0][3][1][16] == F32(7e-4)                             # the record's lr is RMSProp's
    from asyncrl_amd import A3CFF
    m = A3CFF(4, n_envs=N, t_max=T, frames="pairs", device=gpu)
    _opt().setup(m)
    assert m.net.adam_betas == (B1, B2)
    _opt(adam=False).setup(m)
    assert m.net.adam_betas is None
