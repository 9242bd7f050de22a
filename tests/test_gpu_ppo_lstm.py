"""GPU: clipped-surrogate (PPO) epochs on the LSTM (arl_net_set_ppo_state; include/asyncrl_hip.h, "The LSTM"):
the re-forward from the window's own initial recurrent state, truncated BPTT on the re-forwarded rows, and the
carry -- the next window starts from the rollout's (h_T, c_T) whatever the epoch count.

Every net test runs on the SECOND window of its net, after one plain A3C update: h_0 != 0 there and some reset
flags are set.  Tolerances: as test_gpu_ppo.py -- explicit round-to-nearest kernels against their restatements
bit for bit, whole-window gradients against the oracle with conftest.grads_match at the project's 1e-5."""
import numpy as np
import pytest
import torch

import catch_ref
import oracle as O
import ppo_options_ref as R
import ppo_ref
import test_gpu_ppo as G
from conftest import grads_match
from sim import OracleStatesView
from test_gpu_ppo import bits_equal, dev, tbits, ulps_apart

pytestmark = pytest.mark.gpu

F32 = np.float32
GAMMA, BETA, VCOEF, EPS, PL = G.GAMMA, G.BETA, G.VCOEF, G.EPS, G.PL
HID, GATES = 256, 1024
LR1 = 7e-4      # the plain A3C update that ends the first window
LR2 = 2e-2      # the update between epochs 1 and 2: see test_epoch_two_against_the_oracle
# (N, T, A), the smallest that reach each path: a full 32-row tile plus a ragged row; wide heads; the T > 8 memory
# forms; no BPTT step; one BPTT step; 32 and 63 BPTT steps with the loss-gradient launch's second row pass
SHAPES = [(33, 5, 6), (5, 5, 18), (5, 9, 4), (5, 1, 4), (64, 2, 4), (3, 33, 6), (2, 64, 4)]
N, T, A = SHAPES[0]
LONG = (3, 33, 6)   # the re-forward and the carry once more over 33 steps (hbuf / cbuf / the carry's rows 0 and 33)
LONG_TRUNCATE = 20

_POOLS = {}


def pools_of(gpu, shape):
    """(host pools, device pools) of a shape, as test_gpu_ppo.state_pools builds them; built once."""
    if shape not in _POOLS:
        host = G.state_pools(shape)
        _POOLS[shape] = (host, tuple(dev(x, gpu) for x in host))
    return _POOLS[shape]


def second_window(gpu, pools, lam, ppo, shape=SHAPES[0], truncate=None):
    """An LSTM net after one whole A3C window (learn + advancing update at LR1) and the rollout of the second;
    ppo: PPO (and so the carry buffer) set before that rollout; truncate: arl_truncate_window after it."""
    from asyncrl_amd import A3CLSTM
    n, t_max, n_actions = shape
    net = A3CLSTM(n_actions, n_envs=n, t_max=t_max, seed=99, init_seed=3, frames="states", device=gpu).net
    net.reset()
    net.set_gae(lam)
    for t in range(t_max + 1):
        net.observe_act(t, *pools, PL, force_reset=(t == 0))
    net.learn(GAMMA, BETA, VCOEF, True)
    net.optimize(lr0=LR1, alpha=0.99, eps=0.1, clip=40.0, advance=True)
    if ppo:
        net.set_ppo(EPS)
    for t in range(t_max + 1):
        net.observe_act(t, *pools, PL)
    if truncate is not None:
        net.truncate_window(truncate)
    return net


def rows(net, name, width=HID):
    return net.buffer(name, torch.float32, (net.t_max + 2, net.n_envs, width))


def reset_rows(net):
    return net.buffer("reset", torch.uint8, (net.t_max + 1, net.n_envs))


def learner_outputs(net):
    torch.cuda.synchronize()
    out = {k: net.buffer(k, torch.float32).clone() for k in ("dlogits", "dv", "dh", "dG", "dfc")}
    out["grads"] = net.grads.clone()
    return out


# ------------------------------------------------------------------ 1. epoch one
@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "N%d-T%d-A%d" % sh)
def test_epoch_one_is_the_a3c_lstm_gradient(gpu, shape, lam):
    n, t_max, _ = shape
    _, pools = pools_of(gpu, shape)
    a3c = second_window(gpu, pools, lam, False, shape)
    assert a3c.ppo_snap is None and a3c.ppo_carry is None
    a3c.learn(GAMMA, BETA, VCOEF, True)
    want = learner_outputs(a3c)
    ppo = second_window(gpu, pools, lam, True, shape)
    assert tuple(ppo.ppo_carry.shape) == (2, n, HID)
    with pytest.raises(Exception, match="arl_ppo_begin"):
        ppo.ppo_learn(BETA, VCOEF)
    ppo.ppo_begin(GAMMA, True)
    ppo.ppo_learn(BETA, VCOEF)
    got = learner_outputs(ppo)
    # the second window: a carried state, and (but for the smallest windows' few samples) some episode ended
    assert float(rows(ppo, "hbuf")[0].abs().max()) > 0 and float(rows(ppo, "cbuf")[0].abs().max()) > 0
    assert n * t_max < 25 or bool(reset_rows(ppo)[:t_max].any())
    for k in want:
        assert tbits(got[k], want[k]), k
        assert float(want[k].abs().max()) > 0, k
    ratio = ppo.ppo_planes()["ratio"]
    dones = ppo.buffer("dones", torch.uint8, (t_max, n))
    assert bool((ratio == 1).all()) and int(dones.max()) <= 1
    ctl = ppo.buffer("ctl", torch.int64)
    assert int(ctl[2]) == int(ctl[0]) == t_max
    # the save: the carry buffer holds the rollout's rows T
    assert tbits(ppo.ppo_carry[0], rows(ppo, "hbuf")[t_max]) and tbits(ppo.ppo_carry[1], rows(ppo, "cbuf")[t_max])


# ------------------------------------------------------------------ 2, 3. epoch two
_E2 = {}


def epoch_two(gpu, shape=SHAPES[0]):
    """The net of tests 2 and 3, run once a shape: epoch 1, an RMSProp update at LR2, the re-forward and epoch 2 on
    the second window of a (33, 5, 6) net at lambda 0.95; with what has to be compared later, cloned at its time."""
    if shape in _E2:
        return _E2[shape]
    N, T, A = shape
    _, pools = pools_of(gpu, shape)
    net = second_window(gpu, pools, 0.95, True, shape)
    net.ppo_begin(GAMMA, True)
    net.ppo_learn(BETA, VCOEF)
    torch.cuda.synchronize()
    k = _E2[shape] = {}
    k["net"] = net
    k["snap"] = {n_: v.clone() for n_, v in net.ppo_planes().items()}
    k["actions"] = net.buffer("actions", torch.int32, (T + 1, N)).clone()
    k["boot"] = {n_: v.clone() for n_, v in net.step_outputs(T).items()}
    k["step0"] = int(net.buffer("ctl", torch.int64)[0])
    k["h0"], k["c0"] = rows(net, "hbuf")[0].clone(), rows(net, "cbuf")[0].clone()
    k["hT"], k["cT"] = rows(net, "hbuf")[T].clone(), rows(net, "cbuf")[T].clone()
    k["reset"] = reset_rows(net).clone()
    k["v1"] = net.buffer("v", torch.float32, (T + 1, N)).clone()
    net.optimize(lr0=LR2, alpha=0.99, eps=0.1, clip=40.0)
    for t in range(T):
        net.act(t, mode=0)
    torch.cuda.synchronize()
    k["fwd"] = {"logits": net.buffer("logits", torch.float32, (T + 1, N, A))[:T].clone(),
                "v": net.buffer("v", torch.float32, (T + 1, N))[:T].clone(),
                "hbuf": rows(net, "hbuf")[1:T + 1].clone(),
                "gates": net.buffer("gates", torch.float32, (T + 1, N, GATES))[:T].clone()}
    net.ppo_learn(BETA, VCOEF)
    torch.cuda.synchronize()
    return k


def test_the_reforward_is_the_forward(gpu):
    reforward_is_the_forward(gpu, SHAPES[0])


def reforward_is_the_forward(gpu, shape):
    from asyncrl_amd import A3CLSTM
    N, T, A = shape
    k = epoch_two(gpu, shape)
    net = k["net"]
    _, pools = pools_of(gpu, shape)
    # what must not have moved
    assert tbits(net.buffer("actions", torch.int32, (T + 1, N)), k["actions"])
    for name, v in net.step_outputs(T).items():
        assert tbits(v.float(), k["boot"][name].float()), name
    for name in ("logp_old", "adv", "ret"):
        assert tbits(net.ppo_planes()[name], k["snap"][name]), name
    assert int(net.buffer("ctl", torch.int64)[0]) == k["step0"] == T
    assert tbits(rows(net, "hbuf")[0], k["h0"]) and tbits(rows(net, "cbuf")[0], k["c0"])
    assert torch.equal(reset_rows(net), k["reset"])
    # ... and what must have: the update at LR2 moved the slots' values
    assert not tbits(k["fwd"]["v"], k["v1"][:T])
    # a fresh net with the updated parameters, the same initial state and reset rows, on the same pool entries
    fresh = A3CLSTM(A, n_envs=N, t_max=T, seed=99, init_seed=None, frames="states", device=gpu).net
    fresh.reset()
    fresh.load_params(net.state_dict())
    torch.cuda.synchronize()
    fresh.buffer("ctl", torch.int64)[0] = k["step0"]
    rows(fresh, "hbuf")[0] = k["h0"]
    rows(fresh, "cbuf")[0] = k["c0"]
    reset_rows(fresh).copy_(k["reset"])
    for t in range(T):
        fresh.observe_act(t, *pools, PL, mode=0)
    torch.cuda.synchronize()
    assert torch.equal(reset_rows(fresh)[:T], k["reset"][:T])              # (the observations rewrote the same flags)
    got = {"logits": fresh.buffer("logits", torch.float32, (T + 1, N, A))[:T],
           "v": fresh.buffer("v", torch.float32, (T + 1, N))[:T],
           "hbuf": rows(fresh, "hbuf")[1:T + 1],
           "gates": fresh.buffer("gates", torch.float32, (T + 1, N, GATES))[:T]}
    for name, want in k["fwd"].items():
        assert tbits(got[name], want), name
        assert float(want.abs().max()) > 0, name


def test_epoch_two_against_the_oracle(gpu):
    """The LSTM twin of test_gpu_ppo.py's test: the second window of the (33, 5, 6) net after epoch 1 and one
    RMSProp update (eps 0.1, clip 40) at lr LR2, against oracle.lstm_window at the updated parameters, started
    from the window's own rows 0 and reset row, its loss gradient the restatement's on the snapshot with the
    device's ratio.  The lr is picked on the CPU oracle (the whole chain replayed in NumPy: the first window with
    the Philox actions the device draws at seed 99, its RMSProp step at LR1, the second window's GAE gradient,
    clip 40 -- the norm is 14.0 -- and one RMSProp step): the ratios of the re-forward lie in 0.883 .. 1.170 at
    lr 8e-3, the FF test's (none of 165 inactive), 0.830 .. 1.258 at 1.2e-2 (17 inactive, 10.3 %) and 0.729 ..
    1.448 at 2e-2 (39 inactive, 23.6 %): the LSTM's policy moves less per step than the FF net's, so LR2 is 2e-2
    here.  The oracle's own share is asserted below, inside 5 % .. 50 %, before anything is compared."""
    k = epoch_two(gpu)
    net = k["net"]
    (states, rewards, dones), _ = pools_of(gpu, SHAPES[0])
    params = net.state_dict()
    view = OracleStatesView(states, dones)
    x, bstate = view.states_f32(T, T)                    # the second window: pool entries T .. 2 T
    r, d = view.window_rd(rewards, T, T)
    dprev = k["reset"][:T].cpu().numpy()
    assert bits_equal(dprev, np.concatenate([dones[T % PL][None], d[:-1]], 0)) and dprev.any()
    st0 = O.LSTMState(h=k["h0"].cpu().numpy(), c=k["c0"].cpu().numpy(), has=np.ones(N, bool))
    acts = k["actions"][:T].cpu().numpy()
    lpo, adv, ret = (k["snap"][n_].cpu().numpy() for n_ in ("logp_old", "adv", "ret"))
    ratio = net.ppo_planes()["ratio"].cpu().numpy()
    with ppo_ref.patched(lpo, adv, ret, EPS, rho=ratio):
        g, aux = O.lstm_window(params, x, acts, r, dprev, d, bstate, st0, gamma=GAMMA, beta=BETA, v_loss_coef=VCOEF,
                               dev_acts=lstm_dev_acts(net))
    lg = aux["logits"].reshape(T * N, A)
    own = ppo_ref.lossgrad(d, aux["v"], O.softmax(lg).reshape(T, N, A), O.log_softmax(lg).reshape(T, N, A), acts, lpo,
                           adv, ret, EPS, BETA, 1.0, VCOEF)
    inactive = int((~own["active"]).sum())
    print(f"epoch 2: reference ratios {own['own_ratio'].min():.3f} .. {own['own_ratio'].max():.3f}, "
          f"{inactive} of {T * N} samples inactive")
    assert 0.05 * T * N <= inactive <= 0.5 * T * N
    assert np.allclose(ratio, own["own_ratio"], rtol=1e-4)           # (the oracle's forward, not the device's)
    grads_match(net.state_dict(net.grads), g, aux["grad_mag"], 1e-5)


def lstm_dev_acts(net):
    """The window's post-ReLU activations on the device, for the oracle's tie-aware ReLU masks."""
    n, t = net.n_envs, net.t_max
    a1 = net.buffer("a1", torch.float32, (t + 1, n, 16, 20, 20))[:t].cpu().numpy()
    a2 = net.buffer("a2", torch.float32, (t + 1, n, 32, 9, 9))[:t].cpu().numpy()
    h = net.buffer("hfc", torch.float32, (t + 1, n, 256))[:t].cpu().numpy()
    return a1.reshape(t * n, 16, 20, 20), a2.reshape(t * n, 32, 9, 9), h.reshape(t * n, 256)


# ------------------------------------------------------------------ 4. the carry
def two_epochs(net):
    """K = 2 up to (not including) the last update; -> the rollout's rows T, cloned before ppo_begin."""
    t_max = net.t_max
    torch.cuda.synchronize()
    hT, cT = rows(net, "hbuf")[t_max].clone(), rows(net, "cbuf")[t_max].clone()
    net.ppo_begin(GAMMA, True)
    net.ppo_learn(BETA, VCOEF)
    net.optimize(lr0=LR2, alpha=0.99, eps=0.1, clip=40.0)
    for t in range(t_max):
        net.act(t, mode=0)
    net.ppo_learn(BETA, VCOEF)
    torch.cuda.synchronize()
    # the re-forward did overwrite rows T: without this the test could not tell restore from no restore
    assert not tbits(rows(net, "hbuf")[t_max], hT) and not tbits(rows(net, "cbuf")[t_max], cT)
    return hT, cT


@pytest.mark.parametrize("fused", [True, False], ids=["optimize_advance", "optimize-then-advance"])
def test_the_carry_is_the_rollouts_state(gpu, fused):
    carry_is_the_rollouts_state(gpu, fused, SHAPES[0])


def carry_is_the_rollouts_state(gpu, fused, shape):
    T = shape[1]
    _, pools = pools_of(gpu, shape)
    net = second_window(gpu, pools, 0.95, True, shape)
    hT, cT = two_epochs(net)
    rsT = reset_rows(net)[T].clone()
    if fused:
        net.optimize(lr0=LR2, alpha=0.99, eps=0.1, clip=40.0, advance=True)
    else:
        net.optimize(lr0=LR2, alpha=0.99, eps=0.1, clip=40.0)
        net.advance()
    torch.cuda.synchronize()
    assert tbits(rows(net, "hbuf")[0], hT) and tbits(rows(net, "cbuf")[0], cT)
    assert torch.equal(reset_rows(net)[0], rsT) and torch.equal(reset_rows(net)[0], reset_rows(net)[T])
    ctl = net.buffer("ctl", torch.int64)
    assert int(ctl[0]) == 2 * T and int(ctl[1]) == 2
    with pytest.raises(Exception, match="arl_ppo_begin"):            # the advance cleared the window's snapshot
        net.ppo_learn(BETA, VCOEF)


def test_the_carry_after_a_truncated_window(gpu):
    carry_after_a_truncated_window(gpu, SHAPES[0], 2)                 # two live steps, three past the window's end


def carry_after_a_truncated_window(gpu, shape, tr):
    _, pools = pools_of(gpu, shape)
    one = second_window(gpu, pools, 0.95, False, shape, truncate=tr)
    one.learn(GAMMA, BETA, VCOEF, True)
    one.optimize(lr0=LR2, alpha=0.99, eps=0.1, clip=40.0, advance=True)
    net = second_window(gpu, pools, 0.95, True, shape, truncate=tr)
    hT, cT = two_epochs(net)
    live = net.ppo_planes()["ratio"] > 0
    assert bool(live[:tr].all()) and not bool(live[tr:].any())        # tr live steps, the rest past the window's end
    net.optimize(lr0=LR2, alpha=0.99, eps=0.1, clip=40.0, advance=True)
    torch.cuda.synchronize()
    for name in ("hbuf", "cbuf"):
        assert tbits(rows(net, name)[0], rows(one, name)[0]), name
    assert tbits(rows(net, "hbuf")[0], hT) and tbits(rows(net, "cbuf")[0], cT)
    assert torch.equal(reset_rows(net)[0], reset_rows(one)[0])
    assert torch.equal(net.buffer("ctl", torch.int64)[:2], one.buffer("ctl", torch.int64)[:2])


# ------------------------------------------------------------------ 5. the options
def test_options_on_the_lstm(gpu):
    """norm_adv + vclip 0.2 on the (33, 5, 6) net's second window, as test_gpu_ppo_options.py's net tests on FF:
    adv', the moments, epoch 2's dlogits / dv and the records against ppo_options_ref.py, bit for bit."""
    VEPS, lam = 0.2, 0.95
    _, pools = pools_of(gpu, SHAPES[0])
    net = second_window(gpu, pools, lam, True)
    net.set_ppo_options(True, VEPS)
    f32 = torch.float32

    def ws():
        b = {"rewards": net.buffer("rewards", f32, (T, N)), "dones": net.buffer("dones", torch.uint8, (T, N)),
             "v": net.buffer("v", f32, (T + 1, N)), "probs": net.buffer("probs", f32, (T + 1, N, A)),
             "logp": net.buffer("logp", f32, (T + 1, N, A)), "actions": net.buffer("actions", torch.int32, (T + 1, N)),
             "dlogits": net.buffer("dlogits", f32)[:T * N * A], "dv": net.buffer("dv", f32)[:T * N]}
        return {n_: x.cpu().numpy() for n_, x in b.items()}

    net.ppo_begin(GAMMA, True)
    torch.cuda.synchronize()
    w = ws()
    lpo, adv, ret = ppo_ref.snapshot(w["rewards"], w["dones"], w["v"], w["logp"], w["actions"], GAMMA, lam, True)
    adv_n, moments = R.normalize_adv(w["dones"], adv)
    planes = {n_: v.cpu().numpy() for n_, v in net.ppo_planes().items()}
    assert bits_equal(planes["adv"], adv_n) and not bits_equal(adv_n, adv)
    assert bits_equal(planes["ret"], ret) and bits_equal(planes["logp_old"], lpo)
    count, m, _ = net.ppo_aux_raw()
    assert count == 0 and bits_equal(np.array(m, np.float64), np.array(moments, np.float64)) and m[0] == T * N
    assert bits_equal(net.ppo_v_old.cpu().numpy(), w["v"][:T])
    net.ppo_learn(BETA, VCOEF)
    net.optimize(lr0=LR2, alpha=0.99, eps=0.1, clip=40.0)
    for t in range(T):
        net.act(t, mode=0)
    net.ppo_learn(BETA, VCOEF)
    torch.cuda.synchronize()
    w = ws()
    pl = {n_: v.cpu().numpy() for n_, v in net.ppo_planes().items()}
    vo = net.ppo_v_old.cpu().numpy()
    assert bits_equal(pl["adv"], adv_n)
    o = R.lossgrad_vclip(w["dones"], w["v"], w["probs"], w["logp"], w["actions"], pl["logp_old"], pl["adv"], pl["ret"], vo,
                         EPS, VEPS, BETA, 1.0, VCOEF, False, rho=pl["ratio"])
    assert ulps_apart(pl["ratio"], o["own_ratio"]).max() <= 1
    assert bits_equal(w["dlogits"].reshape(T, N, A), o["dlogits"]) and bits_equal(w["dv"].reshape(T, N), o["dv"])
    window = int(net.buffer("ctl", torch.int64)[1])
    want = R.epoch_record(w["dones"], w["v"], w["logp"], w["actions"], pl["logp_old"], pl["adv"], pl["ret"], pl["ratio"],
                          vo, EPS, VEPS, window, 2)
    print("epoch 2: " + "  ".join(f"{n_} {x:.6g}" for n_, x in zip(R.FIELDS, want)))
    count, _, ring = net.ppo_aux_raw()
    assert window == 1 and count == 2 and bits_equal(ring[1], want) and ring[0][1] == 1 and ring[0][2] == T * N
    assert want[5] > 1 > want[6] > 0                                 # the update moved the ratios both ways


# ------------------------------------------------------------------ 6. the whole agent
NA, TA, PA = G.NA, G.TA, G.PA
WINDOWS = 4


def agent(gpu, epochs, env=False, seed=5):
    from asyncrl_amd import A3C, A3CLSTM, Adam, DeviceCatch, GradientClipping
    m = A3CLSTM(4, n_envs=NA, t_max=TA, seed=seed, init_seed=6, frames="pairs", device=gpu)
    opt = Adam(alpha=1e-3).setup(m)
    opt.add_hook(GradientClipping(40))
    ag = A3C(m, opt, TA, GAMMA, gae_lambda=0.95, ppo_epochs=epochs)
    m.net.set_episode_stats(True)
    pools = None
    if env:
        game = DeviceCatch(NA, device=gpu, seed=seed)
        pools = game.make_pools(2)
        m.net.set_env(game)
        m.net.env_reset(*pools, 2)
    return ag, pools


@pytest.mark.parametrize("env", [False, True])
def test_three_epochs_eager_and_replayed(gpu, env):
    K = 3
    states = []
    for graph in (False, True):
        ag, own = agent(gpu, K, env=env)
        pl, PLEN = (own, 2) if env else (G.pair_pools(gpu), PA)
        net = ag.net
        assert net.ppo_carry is not None
        ag.run_window(*pl, PLEN, first=True)
        torch.cuda.synchronize()
        if graph:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                ag.run_window(*pl, PLEN, first=False, stream=s)
            torch.cuda.synchronize()
            assert net.adam_t() == K                                   # (the capture ran nothing)
            for _ in range(WINDOWS - 1):
                g.replay()
        else:
            for _ in range(WINDOWS - 1):
                ag.run_window(*pl, PLEN, first=False)
        torch.cuda.synchronize()
        ctl = net.buffer("ctl", torch.int64)
        assert int(ctl[0]) == WINDOWS * TA and int(ctl[1]) == WINDOWS and net.adam_t() == WINDOWS * K
        es = ag.episode_stats()
        assert es["episodes"] > 0
        keep = [net.params.clone(), net.adam_m.clone(), net.ms.clone(), rows(net, "hbuf")[0].clone(),
                rows(net, "cbuf")[0].clone()]
        # rows 0 are the last rollout's (h_T, c_T), as the carry buffer still holds them
        assert tbits(keep[3], net.ppo_carry[0]) and tbits(keep[4], net.ppo_carry[1])
        assert float(keep[3].abs().max()) > 0
        if env:
            st = net.env.state[(WINDOWS * TA) & 1].cpu().numpy()
            assert ((st[:, 4] * catch_ref.EPISODE_STEPS + st[:, 5]) == WINDOWS * TA).all(), st[:4]
        states.append((keep, es, np.asarray(net.episode_stats_raw(), np.float64)))
    for a, b in zip(states[0][0], states[1][0]):
        assert tbits(a, b)
    assert states[0][1] == states[1][1] and bits_equal(states[0][2], states[1][2])
    assert float((net.ppo_snap[3] - 1).abs().max()) > 0             # the last epoch's ratios left 1


def test_one_epoch_never_touches_the_ppo_state(gpu):
    pl = G.pair_pools(gpu)
    ag, _ = agent(gpu, 1)
    for w in range(2):
        ag.run_window(*pl, PA, first=(w == 0))
    torch.cuda.synchronize()
    assert ag.net.ppo_snap is None and ag.net.ppo_carry is None and ag.net.ppo_clip is None


# ------------------------------------------------------------------ 7. learning
# By the rule of DESIGN.md "Device environment", from three seeds of 4,000 windows (DESIGN.md "PPO epochs on the
# LSTM"): the lr0 = 0 arm averages -0.699 and the lowest seed's last-tenth level is +0.961, so the mark is their
# midpoint; the seeds first reported at or above it at 701, 701 and 601 windows, and twice the most is 1,402.
LEARN_WINDOWS = 1402
LEARN_MARK = 0.131


def test_three_epochs_learn_catch_on_the_lstm(gpu):
    """scripts/train_catch.py's train() at --arch lstm --ppo-epochs 3, everything else the reference's
    hyperparameters (RMSpropAsync lr 7e-4, clip 40, ppo_clip 0.2), seed 0: the episodes of the last tenth of
    LEARN_WINDOWS windows average at least LEARN_MARK; the same run with lr0 = 0 stays at the random mean, within 5
    standard errors (an episode's return is +1 or -1, so its variance is 1 - mean^2)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import train_catch
    # (window 0 runs eagerly before the first report: reports of 141 windows leave the last one 132, the last tenth)
    kw = dict(arch="lstm", envs=256, windows=LEARN_WINDOWS, report=LEARN_WINDOWS // 10 + 1, seed=0, ppo_epochs=3,
              device=str(gpu), log=lambda *a: None)
    last = train_catch.train(lr=7e-4, **kw)[-1]
    frozen = train_catch.train(lr=0.0, **kw)[-1]
    print("LSTM, K = 3: mean return %+.4f over %d episodes (clip fraction %.3f); lr0 = 0: %+.4f over %d"
          % (last["mean_return"], last["episodes"], last["clip_fraction"], frozen["mean_return"], frozen["episodes"]))
    assert last["windows"] == LEARN_WINDOWS and last["episodes"] >= 8000
    assert last["mean_return"] >= LEARN_MARK, last
    se = ((1.0 - frozen["mean_return"] ** 2) / frozen["episodes"]) ** 0.5
    assert abs(frozen["mean_return"] - catch_ref.RANDOM_MEAN) <= 5 * se, (frozen, se)
