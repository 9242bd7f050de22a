"""GPU: clipped-surrogate (PPO) epochs (arl_ppo_snapshot, arl_ppo_lossgrad, arl_net_set_ppo / arl_ppo_begin /
arl_ppo_learn, A3C(ppo_epochs=)) against the NumPy restatement ppo_ref.py.

Tolerances: the snapshot and the loss gradient are explicit round-to-nearest operations in the restatement's
order, so they are compared bit for bit -- the loss gradient with the device's ratio handed to the restatement,
because the ratio's float64 exp is the device's there and the C library's here; the two may differ in the last
float64 bit, which after the rounding to f32 is at most 1 f32 ulp (the Adam lr_t precedent).  Whole-window
gradients against the oracle: conftest.grads_match at the project's 1e-5."""
import ctypes

import numpy as np
import pytest
import torch

import catch_ref
import oracle as O
import ppo_ref
from conftest import grads_match
from gae_replay import window_case
from sim import OracleStatesView, make_pools, make_state_pools

pytestmark = pytest.mark.gpu

F32 = np.float32
GAMMA, BETA, VCOEF, EPS = 0.99, 0.01, 0.5, 0.2
GRID = np.array([-0.6, -0.35, -0.1, 0.1, 0.35, 0.6], F32)
# (T, n, A): EB = 51 envs a block at T = 5, so 75 envs leave a partial second block; T = 9 takes the looped path
# past RW = 8; one env and the widest action set the register forms are built for; T = 8, the last length the
# register windows (RW, PO_RW) hold; A = 16, at the edge of the heads' 16-column tiles
SHAPES = [(5, 75, 4), (9, 33, 6), (5, 1, 18), (8, 33, 6), (5, 33, 16)]


def dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def tbits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ulps_apart(a, b):
    """Distance in f32 representations (both arrays positive or zero)."""
    return np.abs(np.asarray(a, F32).view(np.int32).astype(np.int64) - np.asarray(b, F32).view(np.int32).astype(np.int64))


def P(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


_CASES = {}


def case(i):
    if i not in _CASES:
        T, n, A = SHAPES[i]
        _CASES[i] = window_case(60 + i, T, n, A, truncate=True)
    return _CASES[i]


# ------------------------------------------------------------------ 1. the granular snapshot
def device_snapshot(c, T, n, A, gpu, lam, clip_reward):
    from asyncrl_amd._lib import lib
    t = {k: dev(v, gpu) for k, v in c.items()}
    out = [torch.full((T, n), float("nan"), device=gpu) for _ in range(3)]
    rc = lib.arl_ppo_snapshot(P(t["rewards"]), P(t["dones"]), P(t["v"]), P(t["logp"]), P(t["actions"]), T, n, A, GAMMA,
                              float(lam), int(clip_reward), *(P(o) for o in out), None)
    assert rc == 0, lib.arl_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("clip_reward", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_granular_snapshot_is_the_restatement(gpu, i, lam, clip_reward):
    T, n, A = SHAPES[i]
    c = case(i)
    want = ppo_ref.snapshot(c["rewards"], c["dones"], c["v"], c["logp"], c["actions"], GAMMA, lam, clip_reward)
    got = device_snapshot(c, T, n, A, gpu, lam, clip_reward)
    live = (c["dones"] & 2) == 0
    assert (~live).sum() == 2
    for name, g, w in zip(("logp_old", "adv", "ret"), got, want):
        assert bits_equal(g, w), name
        assert (g[~live] == 0).all() and (np.abs(g[live]).max() > 0 or n == 1)   # (n = 1: three live samples)


# ------------------------------------------------------------------ 2. the granular loss gradient
def shifted(i, lam=1.0, zero=False):
    """case i with its snapshot moved off the current policy: logp_old = logp_new[ac] + delta, delta from GRID
    (fixed seed); zero: delta = 0."""
    T, n, A = SHAPES[i]
    c = case(i)
    lpo, adv, ret = ppo_ref.snapshot(c["rewards"], c["dones"], c["v"], c["logp"], c["actions"], GAMMA, lam, True)
    live = (c["dones"] & 2) == 0
    if not zero:
        delta = np.random.default_rng(100 + i).choice(GRID, (T, n)).astype(F32)
        lpo = np.where(live, (lpo + delta).astype(F32), F32(0)).astype(F32)
    return c, lpo, adv, ret, live


def device_lossgrad(c, lpo, adv, ret, T, n, A, gpu, keep, pcoef=0.5):
    from asyncrl_amd._lib import lib
    t = {k: dev(v, gpu) for k, v in c.items()}
    s = [dev(x, gpu) for x in (lpo, adv, ret)]
    dl = torch.full((T, n, A), float("nan"), device=gpu)
    dv = torch.full((T, n), float("nan"), device=gpu)
    loss = torch.full((n, 2), float("nan"), device=gpu)
    ratio = torch.full((T, n), float("nan"), device=gpu)
    rc = lib.arl_ppo_lossgrad(P(t["dones"]), P(t["v"]), P(t["probs"]), P(t["logp"]), P(t["actions"]), *(P(x) for x in s),
                              T, n, A, EPS, BETA, pcoef, VCOEF, int(keep), P(dl), P(dv), P(loss), P(ratio), None)
    assert rc == 0, lib.arl_last_error()
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dv.cpu().numpy(), loss.cpu().numpy(), ratio.cpu().numpy()


def check_inputs(refs):
    """On the CPU, before the device is touched.  No reference ratio within 2 f32 ulps of lo or hi, in any case.
    Each of the four (sign of adv x active / inactive) classes holds at least 10 % of the live samples: of every
    case that has 40 or more of them, and of all cases together -- the (5, 1, 18) case has 3 live samples, which
    cannot hold four classes."""
    lo, hi = ppo_ref.clip_range(EPS)
    total = np.zeros(4)
    for o, adv in refs:
        live = o["live"]
        rho = o["own_ratio"][live]
        assert ulps_apart(rho, np.full_like(rho, lo)).min() > 2 and ulps_apart(rho, np.full_like(rho, hi)).min() > 2
        pos, act = adv >= 0, o["active"]
        counts = np.array([(live & (pos == s) & (act == a)).sum() for s in (True, False) for a in (True, False)])
        if live.sum() >= 40:
            assert (counts >= 0.1 * live.sum()).all(), counts
        total += counts
    assert (total >= 0.1 * total.sum()).all(), total


@pytest.mark.parametrize("keep", [False, True])
def test_granular_lossgrad_is_the_restatement(gpu, keep):
    cases = [shifted(i) for i in range(len(SHAPES))]
    refs = [ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, EPS, BETA, 0.5,
                             VCOEF, keep) for c, lpo, adv, ret, _ in cases]
    check_inputs([(o, cs[2]) for o, cs in zip(refs, cases)])
    for i, ((c, lpo, adv, ret, live), ref) in enumerate(zip(cases, refs)):
        T, n, A = SHAPES[i]
        dl, dv, loss, ratio = device_lossgrad(c, lpo, adv, ret, T, n, A, gpu, keep)
        apart = ulps_apart(ratio, ref["own_ratio"])
        print(f"case {i} keep {keep}: ratio differs from libm's in {int((apart > 0).sum())} of {ratio.size} samples, "
              f"max {int(apart.max())} ulp")
        assert apart.max() <= 1 and (ratio[~live] == 0).all()
        o = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, EPS, BETA, 0.5,
                             VCOEF, keep, rho=ratio)
        assert bits_equal(o["active"], ref["active"])            # (no ratio near enough to the clip to flip)
        for name, got, want in (("dlogits", dl, o["dlogits"]), ("dv", dv, o["dv"]), ("loss", loss, o["loss"])):
            assert bits_equal(got, want), (i, name)
        assert (dl[~live] == 0).all() and np.abs(dl).max() > 0 and np.isfinite(loss).all()


def device_returns(c, T, n, A, gpu, lam, keep, pcoef=0.5):
    from asyncrl_amd._lib import lib
    t = {k: dev(v, gpu) for k, v in c.items()}
    dl = torch.full((T, n, A), float("nan"), device=gpu)
    dv = torch.full((T, n), float("nan"), device=gpu)
    head = [P(t[k]) for k in ("rewards", "dones", "v", "probs", "logp", "actions")] + [T, n, A, GAMMA]
    tail = [BETA, pcoef, VCOEF, int(keep), 1, P(dl), P(dv), None, None]
    rc = lib.arl_returns_lossgrad(*head, *tail) if lam == 1.0 else lib.arl_returns_lossgrad_gae(*head, lam, *tail)
    assert rc == 0, lib.arl_last_error()
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dv.cpu().numpy()


@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("keep", [False, True])
def test_at_delta_zero_the_epoch_is_the_returns_launch(gpu, keep, lam):
    for i, (T, n, A) in enumerate(SHAPES):
        c = case(i)
        lpo, adv, ret = device_snapshot(c, T, n, A, gpu, lam, True)
        dl, dv, _, ratio = device_lossgrad(c, lpo, adv, ret, T, n, A, gpu, keep)
        dl_w, dv_w = device_returns(c, T, n, A, gpu, lam, keep)
        live = (c["dones"] & 2) == 0
        assert (ratio[live] == 1).all()
        assert bits_equal(dl, dl_w) and bits_equal(dv, dv_w) and np.abs(dl).max() > 0, i


# ------------------------------------------------------------------ 3, 4. a net's epochs
N, T, A, PL = 64, 5, 4, 6
LR2 = 8e-3     # the update between the epochs: see test_epoch_two_against_the_oracle


# (N, T, A) of the nets whose first epoch is compared with the A3C learn: one for each shape the loss-gradient
# launch's register forms are built for -- A <= 4, A <= 8, wider (all T <= 8), and T > 8
# (both 32 rows a pass: the memory form); T = 33 and 64, a second pass over rows with one row and with all 32
NET_SHAPES = [(64, 5, 4), (5, 5, 6), (5, 5, 18), (5, 9, 4), (5, 33, 6), (3, 64, 4)]


def state_pools(shape=(N, T, A)):
    return make_state_pools(np.random.default_rng(sum(shape)), PL, shape[0], p_done=0.2)


def rollout(gpu, pools, lam, ppo, shape=(N, T, A)):
    from asyncrl_amd import A3CFF
    n, t_max, n_actions = shape
    model = A3CFF(n_actions, n_envs=n, t_max=t_max, seed=99, init_seed=3, frames="states", device=gpu)
    net = model.net
    net.reset()
    net.set_gae(lam)
    if ppo:
        net.set_ppo(EPS)
    for t in range(t_max + 1):
        net.observe_act(t, *pools, PL, force_reset=(t == 0))
    return net


def learner_outputs(net):
    torch.cuda.synchronize()
    # (not the loss buffer: its policy term is the surrogate rho * adv here and lp[ac] * adv there, by definition)
    out = {k: net.buffer(k, torch.float32).clone() for k in ("dlogits", "dv", "dfc")}
    out["grads"] = net.grads.clone()
    return out


def dev_acts(net, shape=(N, T, A)):
    N, T, _ = shape
    a1 = net.buffer("a1", torch.float32, (T + 1, N, 16, 20, 20))[:T].cpu().numpy()
    a2 = net.buffer("a2", torch.float32, (T + 1, N, 32, 9, 9))[:T].cpu().numpy()
    h = net.buffer("hfc", torch.float32, (T + 1, N, 256))[:T].cpu().numpy()
    return a1.reshape(T * N, 16, 20, 20), a2.reshape(T * N, 32, 9, 9), h.reshape(T * N, 256)


@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("shape", NET_SHAPES, ids=lambda sh: "N%d-T%d-A%d" % sh)
def test_epoch_one_is_the_a3c_gradient(gpu, shape, lam):
    n, t_max, _ = shape
    pools = tuple(dev(x, gpu) for x in state_pools(shape))
    a3c = rollout(gpu, pools, lam, False, shape)
    a3c.learn(GAMMA, BETA, VCOEF, True)
    want = learner_outputs(a3c)
    ppo = rollout(gpu, pools, lam, True, shape)
    with pytest.raises(Exception, match="arl_ppo_begin"):
        ppo.ppo_learn(BETA, VCOEF)
    ppo.ppo_begin(GAMMA, True)
    ppo.ppo_learn(BETA, VCOEF)
    got = learner_outputs(ppo)
    for k in want:
        assert tbits(got[k], want[k]), k
        assert float(want[k].abs().max()) > 0
    ratio = ppo.ppo_planes()["ratio"]
    dones = ppo.buffer("dones", torch.uint8, (t_max, n))
    assert bool((ratio == 1).all()) and int(dones.max()) <= 1
    ctl = ppo.buffer("ctl", torch.int64)
    assert int(ctl[2]) == int(ctl[0])                               # the step snapshot the fused advance reads


def test_epoch_two_against_the_oracle(gpu):
    """The PPO net after one RMSProp update (eps 0.1, clip 40) at lr LR2.  The lr is picked on the CPU oracle: its
    window on these pools with the Philox actions the device draws (seed 99), the GAE advantage, clip 40 and one
    oracle RMSProp step puts the ratios in 0.888 .. 1.188 at lr 2e-3 (none inactive; the device measured the
    same range), 0.762 .. 1.446 at 5e-3 (15 % inactive) and 0.635 .. 1.762 at 8e-3 (36 % inactive).  The
    reference asserts that share below, before the gradient is compared."""
    epoch_two_against_the_oracle(gpu, (N, T, A), LR2)


def epoch_two_against_the_oracle(gpu, shape, lr):
    from asyncrl_amd import A3CFF
    lam = 0.95
    N, T, A = shape
    states, rewards, dones = state_pools(shape)
    pools = tuple(dev(x, gpu) for x in (states, rewards, dones))
    net = rollout(gpu, pools, lam, True, shape)
    net.ppo_begin(GAMMA, True)
    net.ppo_learn(BETA, VCOEF)
    torch.cuda.synchronize()
    snap = {k: v.clone() for k, v in net.ppo_planes().items()}
    acts_t = net.buffer("actions", torch.int32, (T + 1, N)).clone()
    boot = {k: v.clone() for k, v in net.step_outputs(T).items()}
    step0 = int(net.buffer("ctl", torch.int64)[0])
    net.optimize(lr0=lr, alpha=0.99, eps=0.1, clip=40.0)
    for t in range(T):
        net.act(t, mode=0)
    net.ppo_learn(BETA, VCOEF)
    torch.cuda.synchronize()
    # what must not have moved
    assert tbits(net.buffer("actions", torch.int32, (T + 1, N)), acts_t)
    for k, v in net.step_outputs(T).items():
        assert tbits(v.float(), boot[k].float()), k
    for k in ("logp_old", "adv", "ret"):
        assert tbits(net.ppo_planes()[k], snap[k]), k
    assert int(net.buffer("ctl", torch.int64)[0]) == step0
    # the re-forward: a fresh net with the updated parameters on the same pool entries
    params = net.state_dict()
    fresh = A3CFF(A, n_envs=N, t_max=T, seed=99, init_seed=None, frames="states", device=gpu).net
    fresh.reset()
    fresh.load_params(params)
    for t in range(T):
        fresh.observe_act(t, *pools, PL, force_reset=(t == 0), mode=0)
    torch.cuda.synchronize()
    for k in ("logits", "v"):
        a = net.buffer(k, torch.float32)[:T * N * (A if k == "logits" else 1)]
        b = fresh.buffer(k, torch.float32)[:T * N * (A if k == "logits" else 1)]
        assert tbits(a, b) and float(a.abs().max()) > 0, k
    # the gradient: the oracle's window at the updated parameters, its loss gradient the restatement's on the
    # snapshot with the device's ratio
    view = OracleStatesView(states, dones)
    x, bstate = view.states_f32(0, T)
    r, d = view.window_rd(rewards, 0, T)
    acts = acts_t[:T].cpu().numpy()
    lpo, adv, ret, ratio = (snap[k].cpu().numpy() if k != "ratio" else net.ppo_planes()[k].cpu().numpy()
                            for k in ("logp_old", "adv", "ret", "ratio"))
    with ppo_ref.patched(lpo, adv, ret, EPS, rho=ratio):
        g, aux = O.ff_window_grads(params, x, acts, r, d, bstate, gamma=GAMMA, beta=BETA, v_loss_coef=VCOEF,
                                   dev_acts=dev_acts(net, shape))
    lg = aux["logits"].reshape(T * N, A)
    own = ppo_ref.lossgrad(d, aux["v"], O.softmax(lg).reshape(T, N, A), O.log_softmax(lg).reshape(T, N, A), acts, lpo, adv,
                           ret, EPS, BETA, 1.0, VCOEF)
    inactive = (~own["active"]).sum()
    print(f"epoch 2: reference ratios {own['own_ratio'].min():.3f} .. {own['own_ratio'].max():.3f}, "
          f"{int(inactive)} of {T * N} samples inactive")
    assert 0 < inactive < T * N
    assert np.allclose(ratio, own["own_ratio"], rtol=1e-4)           # (the oracle's forward, not the device's)
    grads_match(net.state_dict(net.grads), g, aux["grad_mag"], 1e-5)


# ------------------------------------------------------------------ 5. the whole agent
NA, TA, PA = 32, 5, 7


def agent(gpu, epochs, adam=True, env=False, seed=5):
    from asyncrl_amd import A3C, A3CFF, Adam, DeviceCatch, GradientClipping, RMSpropAsync
    m = A3CFF(4, n_envs=NA, t_max=TA, seed=seed, init_seed=6, frames="pairs", device=gpu)
    opt = (Adam(alpha=1e-3) if adam else RMSpropAsync(lr=7e-4, eps=0.1, alpha=0.99)).setup(m)
    opt.add_hook(GradientClipping(40))
    kw = {} if epochs is None else dict(ppo_epochs=epochs)
    ag = A3C(m, opt, TA, GAMMA, gae_lambda=0.95, **kw)
    pools = None
    if env:
        game = DeviceCatch(NA, device=gpu, seed=seed)
        pools = game.make_pools(2)
        m.net.set_env(game)
        m.net.env_reset(*pools, 2)
    return ag, pools


_POOLS = {}


def pair_pools(gpu):
    if "p" not in _POOLS:
        _POOLS["p"] = tuple(dev(x, gpu) for x in make_pools(np.random.default_rng(77), PA, NA, "uniform", p_done=0.1))
    return _POOLS["p"]


def test_one_epoch_is_the_default_agent(gpu):
    pl = pair_pools(gpu)
    outs = []
    for epochs in (None, 1):
        ag, _ = agent(gpu, epochs, adam=False)
        for w in range(2):
            ag.run_window(*pl, PA, first=(w == 0))
        torch.cuda.synchronize()
        assert ag.net.ppo_snap is None
        outs.append((ag.net.params.clone(), ag.net.ms.clone()))
    assert tbits(outs[0][0], outs[1][0]) and tbits(outs[0][1], outs[1][1])


@pytest.mark.parametrize("env", [False, True])
def test_three_epochs_eager_and_replayed(gpu, env):
    K = 3
    states = []
    for graph in (False, True):
        ag, own = agent(gpu, K, env=env)
        pl, PLEN = (own, 2) if env else (pair_pools(gpu), PA)
        net = ag.net
        ag.run_window(*pl, PLEN, first=True)
        torch.cuda.synchronize()
        ctl = net.buffer("ctl", torch.int64)
        assert int(ctl[0]) == TA and int(ctl[1]) == 1 and net.adam_t() == K
        if graph:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                ag.run_window(*pl, PLEN, first=False, stream=s)
            torch.cuda.synchronize()
            assert net.adam_t() == K
            g.replay()
        else:
            ag.run_window(*pl, PLEN, first=False)
        torch.cuda.synchronize()
        assert int(ctl[0]) == 2 * TA and int(ctl[1]) == 2 and net.adam_t() == 2 * K
        st = ag.ppo_stats()
        assert set(st) == {"clip_fraction", "approx_kl", "ratio_max"}
        assert 0.0 <= st["clip_fraction"] <= 1.0 and st["ratio_max"] >= 1 - 1e-6 and np.isfinite(st["approx_kl"])
        keep = [net.params.clone(), net.adam_m.clone(), net.ms.clone(), net.ppo_snap.clone()]
        if env:
            # the env stepped T times a window, not T times an epoch: 2 T steps an env after two windows
            keep.append(net.env.state.clone().float())
            st = net.env.state[(2 * TA) & 1].cpu().numpy()            # [.., episode, steps_in_episode, ..]
            assert ((st[:, 4] * catch_ref.EPISODE_STEPS + st[:, 5]) == 2 * TA).all(), st[:4]
        states.append(keep)
    for a, b in zip(*states):
        assert tbits(a, b)
    assert float((states[0][3][3] - 1).abs().max()) > 0            # the last epoch's ratios left 1


# ------------------------------------------------------------------ 6. learning
LEARN_WINDOWS = 1000     # twice the most any of three seeds needed to cross the mark (DESIGN.md "PPO epochs")
LEARN_MARK = 0.108       # midpoint of the lr0 = 0 mean (-0.70) and the lowest seed's last-tenth level (+0.916)


def test_three_epochs_learn_catch(gpu):
    """scripts/train_catch.py's train() at --ppo-epochs 3, everything else the reference's hyperparameters
    (RMSpropAsync lr 7e-4, clip 40, ppo_clip 0.2), seed 0: the episodes of the last tenth of 1,000 windows average
    at least LEARN_MARK; the same run with lr0 = 0 stays at the random mean, within 5 standard errors (an episode's
    return is +1 or -1, so its variance is 1 - mean^2)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import train_catch
    kw = dict(envs=256, windows=LEARN_WINDOWS, report=LEARN_WINDOWS // 10, seed=0, ppo_epochs=3, device=str(gpu),
              log=lambda *a: None)
    last = train_catch.train(lr=7e-4, **kw)[-1]
    frozen = train_catch.train(lr=0.0, **kw)[-1]
    print("K = 3: mean return %+.4f over %d episodes (clip fraction %.3f); lr0 = 0: %+.4f over %d"
          % (last["mean_return"], last["episodes"], last["clip_fraction"], frozen["mean_return"], frozen["episodes"]))
    assert last["windows"] == LEARN_WINDOWS and last["episodes"] >= 8000
    assert last["mean_return"] >= LEARN_MARK, last
    se = ((1.0 - frozen["mean_return"] ** 2) / frozen["episodes"]) ** 0.5
    assert abs(frozen["mean_return"] - catch_ref.RANDOM_MEAN) <= 5 * se, (frozen, se)
