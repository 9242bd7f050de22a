"""GPU: the PPO epochs' options (arl_net_set_ppo_options: advantage normalisation, the clipped value loss, the
per-epoch record; A3C(ppo_norm_adv=, ppo_vclip=)) against the NumPy restatement ppo_options_ref.py.

Tolerances: every kernel here is explicit round-to-nearest operations in the restatement's order (the float64
sums in the one-workgroup kernels' thread order, the device's float64 divide and sqrt correctly rounded), so
everything is compared bit for bit -- the loss gradient with the device's ratio handed to the restatement, as in
test_gpu_ppo.py."""
import ctypes

import numpy as np
import pytest
import torch

import ppo_options_ref as R
import ppo_ref
import test_gpu_ppo as G
from gae_replay import window_case
from test_gpu_ppo import P, bits_equal, dev, tbits, ulps_apart

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GAMMA, BETA, VCOEF, EPS, VEPS = 0.99, 0.01, 0.5, 0.2, 0.1
# test_gpu_ppo.py's three (a partial second block, the looped path past RW = 8, one env) and one whose 600 envs make
# a thread of the single workgroup walk three envs, the last pass ragged (600 = 2 * 256 + 88); and T = 8, the last
# length the one-workgroup kernels' register window (PO_RW) holds
SHAPES = [(5, 75, 4), (9, 33, 6), (5, 1, 18), (4, 600, 4), (8, 33, 6), (5, 33, 16)]   # the last: A at the 16-column edge
VGRID = np.array([-0.3, -0.15, -0.05, 0.05, 0.15, 0.3], F32)

_CASES = {}


def case(i):
    if i not in _CASES:
        T, n, A = SHAPES[i]
        _CASES[i] = window_case(60 + i, T, n, A, truncate=True)
    return _CASES[i]


def snapshot(i, lam=1.0):
    c = case(i)
    return ppo_ref.snapshot(c["rewards"], c["dones"], c["v"], c["logp"], c["actions"], GAMMA, lam, True)


# ------------------------------------------------------------------ 1. normalisation, granular
def device_normalize(dones, adv, gpu):
    from asyncrl_amd._lib import lib
    T, n = adv.shape
    d, a = dev(dones, gpu), dev(adv, gpu)
    m = torch.full((3,), float("nan"), dtype=torch.float64, device=gpu)
    rc = lib.arl_ppo_normalize_adv(P(d), P(a), T, n, P(m), None)
    assert rc == 0, lib.arl_last_error()
    torch.cuda.synchronize()
    return a.cpu().numpy(), m.cpu().numpy()


@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_granular_normalisation_is_the_restatement(gpu, i, lam):
    c = case(i)
    _, adv, _ = snapshot(i, lam)
    live = (c["dones"] & 2) == 0
    want, moments = R.normalize_adv(c["dones"], adv)
    got, m = device_normalize(c["dones"], adv, gpu)
    print(f"case {i} lam {lam}: n_live {m[0]:.0f} mean {m[1]:+.6f} std {m[2]:.6f}")
    assert bits_equal(m, np.array(moments, F64))
    assert bits_equal(got, want) and (got[~live] == 0).all() and not bits_equal(got, adv)


def test_granular_normalisation_edge_cases(gpu):
    c = case(0)
    _, adv, _ = snapshot(0)
    none = np.full_like(c["dones"], 2)                       # every sample past the window's end
    got, m = device_normalize(none, adv, gpu)
    assert bits_equal(got, adv) and bits_equal(m, np.zeros(3, F64))
    live = (c["dones"] & 2) == 0
    flat = np.where(live, F32(0.37), F32(0)).astype(F32)     # all live advantages equal
    got, m = device_normalize(c["dones"], flat, gpu)
    assert bits_equal(got, np.zeros_like(flat)) and bits_equal(m, np.array([live.sum(), F64(F32(0.37)), 0.0], F64))


# ------------------------------------------------------------------ 2. value clip, granular
def vclip_case(i):
    """case i with logp_old moved off the policy as test_gpu_ppo.shifted does and v_old = f32(v + delta)."""
    T, n, A = SHAPES[i]
    c = case(i)
    lpo, adv, ret = snapshot(i)
    live = (c["dones"] & 2) == 0
    shift = np.random.default_rng(100 + i).choice(G.GRID, (T, n)).astype(F32)
    lpo = np.where(live, (lpo + shift).astype(F32), F32(0)).astype(F32)
    delta = np.random.default_rng(200 + i).choice(VGRID, (T, n)).astype(F32)
    v_old = (c["v"][:T] + delta).astype(F32)
    return c, lpo, adv, ret, v_old, live


def device_lossgrad_vclip(c, lpo, adv, ret, v_old, T, n, A, gpu, keep, veps=VEPS, pcoef=0.5):
    from asyncrl_amd._lib import lib
    t = {k: dev(v, gpu) for k, v in c.items()}
    s = [dev(x, gpu) for x in (lpo, adv, ret, v_old)]
    dl = torch.full((T, n, A), float("nan"), device=gpu)
    dv = torch.full((T, n), float("nan"), device=gpu)
    loss = torch.full((n, 2), float("nan"), device=gpu)
    ratio = torch.full((T, n), float("nan"), device=gpu)
    rc = lib.arl_ppo_lossgrad_vclip(P(t["dones"]), P(t["v"]), P(t["probs"]), P(t["logp"]), P(t["actions"]),
                                    *(P(x) for x in s), T, n, A, EPS, veps, BETA, pcoef, VCOEF, int(keep), P(dl), P(dv),
                                    P(loss), P(ratio), None)
    assert rc == 0, lib.arl_last_error()
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dv.cpu().numpy(), loss.cpu().numpy(), ratio.cpu().numpy()


def check_vclip_inputs(refs):
    """On the CPU, before the device is touched.  Each of the three classes (inside; outside and taken; outside and
    not taken) holds at least 10 % of the live samples, of every case with 40 or more of them and of all cases
    together; no live sample outside has lc == lu; no |do| lies within 2 f32 ulps of ev."""
    total = np.zeros(3)
    ev = F32(VEPS)
    for o in refs:
        live, vc = o["live"], o["vc"]
        counts = np.array([o["inside"].sum(), o["taken"].sum(), o["outside_kept"].sum()])
        assert counts.sum() == live.sum()
        if live.sum() >= 40:
            assert (counts >= 0.1 * live.sum()).all(), counts
        total += counts
        outside = live & ~vc["inside"]
        assert not (vc["lc"] == vc["lu"])[outside].any()
        ado = np.abs(vc["do"][live])
        assert ulps_apart(ado, np.full_like(ado, ev)).min() > 2
    assert (total >= 0.1 * total.sum()).all(), total


@pytest.mark.parametrize("keep", [False, True])
def test_granular_value_clip_is_the_restatement(gpu, keep):
    cases = [vclip_case(i) for i in range(len(SHAPES))]
    refs = [R.lossgrad_vclip(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, v_old, EPS, VEPS,
                             BETA, 0.5, VCOEF, keep) for c, lpo, adv, ret, v_old, _ in cases]
    check_vclip_inputs(refs)
    for i, ((c, lpo, adv, ret, v_old, live), ref) in enumerate(zip(cases, refs)):
        T, n, A = SHAPES[i]
        dl, dv, loss, ratio = device_lossgrad_vclip(c, lpo, adv, ret, v_old, T, n, A, gpu, keep)
        assert ulps_apart(ratio, ref["own_ratio"]).max() <= 1 and (ratio[~live] == 0).all()
        o = R.lossgrad_vclip(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, v_old, EPS, VEPS,
                             BETA, 0.5, VCOEF, keep, rho=ratio)
        print(f"case {i} keep {keep}: inside {int(o['inside'].sum())} taken {int(o['taken'].sum())} "
              f"outside, not taken {int(o['outside_kept'].sum())}")
        for name, got, want in (("dlogits", dl, o["dlogits"]), ("dv", dv, o["dv"]), ("loss", loss, o["loss"])):
            assert bits_equal(got, want), (i, name)
        assert (dv[o["taken"]] == 0).all() and np.abs(dv).max() > 0 and np.isfinite(loss).all()


@pytest.mark.parametrize("keep", [False, True])
def test_value_clip_at_v_old_equal_to_v_is_the_plain_lossgrad(gpu, keep):
    for i, (T, n, A) in enumerate(SHAPES):
        c, lpo, adv, ret, _, live = vclip_case(i)
        got = device_lossgrad_vclip(c, lpo, adv, ret, c["v"][:T].copy(), T, n, A, gpu, keep)
        want = G.device_lossgrad(c, lpo, adv, ret, T, n, A, gpu, keep)
        for name, g, w in zip(("dlogits", "dv", "loss", "ratio"), got, want):
            assert bits_equal(g, w), (i, name)
        assert np.abs(got[1]).max() > 0


# ------------------------------------------------------------------ 3. epoch record, granular
def device_epoch_stats(c, lpo, adv, ret, ratio, v_old, T, n, A, gpu, window, epoch):
    from asyncrl_amd._lib import lib
    t = {k: dev(v, gpu) for k, v in c.items()}
    s = [dev(x, gpu) for x in (lpo, adv, ret, ratio)]
    vo = None if v_old is None else dev(v_old, gpu)
    rec = torch.full((R.PPO_STAT_FIELDS,), float("nan"), dtype=torch.float64, device=gpu)
    rc = lib.arl_ppo_epoch_stats(P(t["dones"]), P(t["v"]), P(t["logp"]), P(t["actions"]), *(P(x) for x in s), P(vo), T, n,
                                 A, EPS, VEPS if v_old is not None else 0.0, float(window), float(epoch), P(rec), None)
    assert rc == 0, lib.arl_last_error()
    torch.cuda.synchronize()
    return rec.cpu().numpy()


@pytest.mark.parametrize("with_v_old", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_granular_epoch_record_is_the_restatement(gpu, i, with_v_old):
    T, n, A = SHAPES[i]
    c, lpo, adv, ret, v_old, live = vclip_case(i)
    adv, _ = R.normalize_adv(c["dones"], adv)                # (the advantage as an epoch with normalisation uses it)
    ratio = G.device_lossgrad(c, lpo, adv, ret, T, n, A, gpu, False)[3]
    vo = v_old if with_v_old else None
    want = R.epoch_record(c["dones"], c["v"], c["logp"], c["actions"], lpo, adv, ret, ratio, vo, EPS, VEPS, 3 + i, 2)
    got = device_epoch_stats(c, lpo, adv, ret, ratio, vo, T, n, A, gpu, 3 + i, 2)
    print(f"case {i} v_old {with_v_old}: " + "  ".join(f"{k} {x:.6g}" for k, x in zip(R.FIELDS, got)))
    assert bits_equal(got, want), dict(zip(R.FIELDS, zip(got, want)))
    assert got[2] == live.sum() and (with_v_old or got[7] == 0)
    assert live.sum() < 40 or (got[3] > 0 and (got[7] > 0) == with_v_old)


# ------------------------------------------------------------------ 4, 5. a net's epochs
def net_rollout(gpu, pools, lam, norm_adv, vclip, shape=(G.N, G.T, G.A)):
    net = G.rollout(gpu, pools, lam, True, shape)
    if norm_adv or vclip is not None:
        net.set_ppo_options(norm_adv, vclip)
    return net


@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("shape", G.NET_SHAPES, ids=lambda sh: "N%d-T%d-A%d" % sh)
def test_epoch_one_with_value_clip_is_the_plain_epoch(gpu, shape, lam):
    """The net-level counterpart of test_value_clip_at_v_old_equal_to_v_is_the_plain_lossgrad, at every shape the
    loss-gradient launch has a register form for: in epoch one v == v_old on every live sample, so the value-clipped
    form takes the unclipped square and leaves the plain form's gradient, bit for bit."""
    pools = tuple(dev(x, gpu) for x in G.state_pools(shape))
    outs = []
    for vclip in (None, 0.2):
        net = net_rollout(gpu, pools, lam, False, vclip, shape)
        assert (net.ppo_v_old is None) == (vclip is None)
        net.ppo_begin(GAMMA, True)
        net.ppo_learn(BETA, VCOEF)
        outs.append(G.learner_outputs(net))
    want, got = outs
    for k in want:
        assert tbits(got[k], want[k]), k
        assert float(want[k].abs().max()) > 0


@pytest.mark.parametrize("lam", [1.0, 0.95])
def test_net_epoch_one(gpu, lam):
    N, T = G.N, G.T
    pools = tuple(dev(x, gpu) for x in G.state_pools())
    plain = net_rollout(gpu, pools, lam, False, None)
    plain.ppo_begin(GAMMA, True)
    plain.ppo_learn(BETA, VCOEF)
    want = G.learner_outputs(plain)
    snap = {k: v.cpu().numpy() for k, v in plain.ppo_planes().items()}
    assert plain.ppo_aux is None and plain.ppo_v_old is None
    # value clipping on: v_old is the rollout's v, every sample inside, the gradient bit for bit the plain one
    vc = net_rollout(gpu, pools, lam, False, VEPS)
    vc.ppo_begin(GAMMA, True)
    vc.ppo_learn(BETA, VCOEF)
    got = G.learner_outputs(vc)
    for k in want:
        assert tbits(got[k], want[k]), k
        assert float(want[k].abs().max()) > 0
    dones = vc.buffer("dones", torch.uint8, (T, N)).cpu().numpy()
    v = vc.buffer("v", torch.float32, (T + 1, N)).cpu().numpy()
    assert bits_equal(vc.ppo_v_old.cpu().numpy(), np.where((dones & 2) == 0, v[:T], F32(0)).astype(F32))
    count, _, ring = vc.ppo_aux_raw()
    assert count == 1 and ring[0][1] == 1 and ring[0][2] == T * N and ring[0][7] == 0
    # normalisation on: the adv plane is the plain snapshot's, normalised; the other planes and the target stay
    na = net_rollout(gpu, pools, lam, True, None)
    na.ppo_begin(GAMMA, True)
    torch.cuda.synchronize()
    planes = {k: v.cpu().numpy() for k, v in na.ppo_planes().items()}
    adv, moments = R.normalize_adv(dones, snap["adv"])
    assert bits_equal(planes["adv"], adv) and not bits_equal(adv, snap["adv"])
    assert bits_equal(planes["ret"], snap["ret"]) and bits_equal(planes["logp_old"], snap["logp_old"])
    count, m, _ = na.ppo_aux_raw()
    assert count == 0 and bits_equal(np.array(m, F64), np.array(moments, F64)) and m[0] == T * N


def test_net_epoch_two(gpu):
    """Both options on; one RMSProp update at test_gpu_ppo.py's LR2 between the epochs, which moves the ratios to
    0.64 .. 1.76 there.  The workspace's dlogits / dv of epoch 2 against the restatement on the workspace's own v /
    probs / log_probs, the snapshot, v_old and the device's ratio; the record of epoch 2 likewise."""
    net_epoch_two(gpu, (G.N, G.T, G.A), G.LR2)


def net_epoch_two(gpu, shape, lr):
    N, T, A = shape
    pools = tuple(dev(x, gpu) for x in G.state_pools(shape))
    net = net_rollout(gpu, pools, 0.95, True, VEPS, shape)
    net.ppo_begin(GAMMA, True)
    net.ppo_learn(BETA, VCOEF)
    torch.cuda.synchronize()
    snap = {k: v.clone() for k, v in net.ppo_planes().items()}
    v_old = net.ppo_v_old.clone()
    net.optimize(lr0=lr, alpha=0.99, eps=0.1, clip=40.0)
    for t in range(T):
        net.act(t, mode=0)
    net.ppo_learn(BETA, VCOEF)
    torch.cuda.synchronize()
    for k in ("logp_old", "adv", "ret"):
        assert tbits(net.ppo_planes()[k], snap[k]), k
    assert tbits(net.ppo_v_old, v_old)
    f32 = torch.float32
    ws = {"dones": net.buffer("dones", torch.uint8, (T, N)), "v": net.buffer("v", f32, (T + 1, N)),
          "probs": net.buffer("probs", f32, (T + 1, N, A)), "logp": net.buffer("logp", f32, (T + 1, N, A)),
          "actions": net.buffer("actions", torch.int32, (T + 1, N)), "dlogits": net.buffer("dlogits", f32)[:T * N * A],
          "dv": net.buffer("dv", f32)[:T * N]}
    ws = {k: x.cpu().numpy() for k, x in ws.items()}
    pl = {k: x.cpu().numpy() for k, x in net.ppo_planes().items()}
    vo = v_old.cpu().numpy()
    assert np.abs(ws["v"][:T] - vo).max() > VEPS                 # the update moved some value out of the clip range
    o = R.lossgrad_vclip(ws["dones"], ws["v"], ws["probs"], ws["logp"], ws["actions"], pl["logp_old"], pl["adv"],
                         pl["ret"], vo, EPS, VEPS, BETA, 1.0, VCOEF, False, rho=pl["ratio"])
    assert ulps_apart(pl["ratio"], o["own_ratio"]).max() <= 1
    assert bits_equal(ws["dlogits"].reshape(T, N, A), o["dlogits"]) and bits_equal(ws["dv"].reshape(T, N), o["dv"])
    window = int(net.buffer("ctl", torch.int64)[1])
    want = R.epoch_record(ws["dones"], ws["v"], ws["logp"], ws["actions"], pl["logp_old"], pl["adv"], pl["ret"],
                          pl["ratio"], vo, EPS, VEPS, window, 2)
    print("epoch 2: " + "  ".join(f"{k} {x:.6g}" for k, x in zip(R.FIELDS, want)))
    assert 0 < want[7] < want[2] and 0 < want[3] < want[2]
    count, _, ring = net.ppo_aux_raw()
    assert count == 2 and bits_equal(ring[1], want) and ring[0][1] == 1
    assert net.ppo_epoch_log(5) == [list(ring[0]), list(ring[1])]


# ------------------------------------------------------------------ 6, 7. the whole agent
NA, TA, PA = G.NA, G.TA, G.PA


def agent(gpu, env=False, seed=5, **kw):
    from asyncrl_amd import A3C, A3CFF, Adam, DeviceCatch, GradientClipping
    m = A3CFF(4, n_envs=NA, t_max=TA, seed=seed, init_seed=6, frames="pairs", device=gpu)
    opt = Adam(alpha=1e-3).setup(m)
    opt.add_hook(GradientClipping(40))
    ag = A3C(m, opt, TA, GAMMA, gae_lambda=0.95, ppo_epochs=3, **kw)
    pools = None
    if env:
        game = DeviceCatch(NA, device=gpu, seed=seed)
        pools = game.make_pools(2)
        m.net.set_env(game)
        m.net.env_reset(*pools, 2)
    return ag, pools


@pytest.mark.parametrize("env", [False, True])
def test_three_epochs_with_options_eager_and_replayed(gpu, env):
    K = 3
    states = []
    for graph in (False, True):
        ag, own = agent(gpu, env=env, ppo_norm_adv=True, ppo_vclip=0.2)
        pl, PLEN = (own, 2) if env else (G.pair_pools(gpu), PA)
        net = ag.net
        ag.run_window(*pl, PLEN, first=True)
        torch.cuda.synchronize()
        assert net.ppo_aux_raw()[0] == K
        if graph:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                ag.run_window(*pl, PLEN, first=False, stream=s)
            torch.cuda.synchronize()
            assert net.ppo_aux_raw()[0] == K                 # (the capture ran nothing)
            g.replay()
        else:
            ag.run_window(*pl, PLEN, first=False)
        torch.cuda.synchronize()
        count, m, ring = net.ppo_aux_raw()
        assert count == 2 * K and net.adam_t() == 2 * K
        assert [int(r[1]) for r in ring[:2 * K]] == [1, 2, 3, 1, 2, 3] and [int(r[0]) for r in ring[:2 * K]] == [0] * 3 + [1] * 3
        assert not ring[2 * K:].any() and m[0] == ring[K][2] > 0 and m[2] > 0
        st = ag.ppo_epoch_stats(last=2 * K)
        assert [d["epoch"] for d in st] == [1, 2, 3, 1, 2, 3] and ag.ppo_epoch_stats()[0] == st[-1]
        assert set(st[0]) == {"window", "epoch", "samples", "clip_fraction", "approx_kl", "ratio_max", "ratio_min",
                              "vclip_fraction", "adv_mean", "adv_std"}
        assert st[3]["clip_fraction"] == 0 and st[3]["vclip_fraction"] == 0 and st[3]["ratio_max"] == 1   # epoch 1
        assert abs(st[-1]["adv_mean"]) < 1e-6 and abs(st[-1]["adv_std"] - 1) < 1e-5    # (f32 roundings of adv')
        states.append([net.params.clone(), net.adam_m.clone(), net.ms.clone(), net.ppo_snap.clone(),
                       net.ppo_v_old.clone(), net.ppo_aux.clone()])
    for a, b in zip(*states):
        assert tbits(a, b)
    assert float((states[0][3][3] - 1).abs().max()) > 0            # the last epoch's ratios left 1


def test_default_options_are_untouched(gpu):
    pl = G.pair_pools(gpu)
    outs = []
    for kw in ({}, dict(ppo_norm_adv=False, ppo_vclip=None), "back to the defaults", dict(ppo_norm_adv=True, ppo_vclip=0.2)):
        ag, _ = agent(gpu, **(kw if isinstance(kw, dict) else {}))
        if not isinstance(kw, dict):                          # options set on the handle, then taken back
            ag.net.set_ppo_options(True, 0.2)
            ag.net.set_ppo_options()
        elif not kw.get("ppo_norm_adv"):
            assert ag.net.ppo_aux is None and ag.net.ppo_v_old is None
        for w in range(2):
            ag.run_window(*pl, PA, first=(w == 0))
        torch.cuda.synchronize()
        outs.append((ag.net.params.clone(), ag.net.adam_m.clone(), ag.net.ms.clone(), ag.net.ppo_snap.clone()))
    for other in outs[1:3]:
        for a, b in zip(outs[0], other):
            assert tbits(a, b)
    assert not tbits(outs[0][0], outs[3][0])                   # (the options do change the update)


# ------------------------------------------------------------------ 8. learning
# By the rule of test_gpu_ppo.py's LEARN_MARK / LEARN_WINDOWS, from three seeds of 2,000 windows (DESIGN.md "PPO
# options"): the lowest seed's last-tenth level is +0.216, so the mark is the midpoint of that and the random mean
# -0.70; the seeds first reported at or above it at 901, 901 and 1,201 windows, and twice the most is 2,402.
LEARN_WINDOWS = 2402
LEARN_MARK = -0.242


def test_three_epochs_with_options_learn_catch(gpu):
    """scripts/train_catch.py's train() at --ppo-epochs 3 --ppo-norm-adv --ppo-vclip 0.2, everything else the
    reference's hyperparameters as in test_gpu_ppo.py's learn test, seed 0: the episodes of the last tenth of
    LEARN_WINDOWS windows average at least LEARN_MARK; the same run with lr0 = 0 stays at the random mean, within 5
    standard errors (an episode's return is +1 or -1, so its variance is 1 - mean^2)."""
    import os
    import sys
    import catch_ref
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import train_catch
    # (window 0 runs eagerly before the first report: reports of 241 windows leave the last one 232, the last tenth)
    kw = dict(envs=256, windows=LEARN_WINDOWS, report=LEARN_WINDOWS // 10 + 1, seed=0, ppo_epochs=3, ppo_norm_adv=True,
              ppo_vclip=0.2, device=str(gpu), log=lambda *a: None)
    last = train_catch.train(lr=7e-4, **kw)[-1]
    frozen = train_catch.train(lr=0.0, **kw)[-1]
    print("options on: mean return %+.4f over %d episodes (%s); lr0 = 0: %+.4f over %d"
          % (last["mean_return"], last["episodes"], last["ppo_epoch"], frozen["mean_return"], frozen["episodes"]))
    assert last["windows"] == LEARN_WINDOWS and last["episodes"] >= 8000
    assert last["ppo_epoch"]["epoch"] == 3 and last["ppo_epoch"]["window"] == LEARN_WINDOWS - 1
    assert last["mean_return"] >= LEARN_MARK, last
    se = ((1.0 - frozen["mean_return"] ** 2) / frozen["episodes"]) ** 0.5
    assert abs(frozen["mean_return"] - catch_ref.RANDOM_MEAN) <= 5 * se, (frozen, se)
