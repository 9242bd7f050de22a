"""CPU: the long-window cases of tests/test_gpu_long_windows.py and tests/test_gpu_stages.py on the reference
alone, in the manner of tests/test_stage_ref.py: the inputs hold the conditions the cases exist for, the float32
rounding of a 33- and 64-step BPTT chain is measured, and each mistake the cases are meant to catch misses the
GPU tests' tolerance (1e-5 of the scale; bit for bit for the statistics) by more than 10x."""
import functools
import inspect

import numpy as np
import pytest

import long_cases as L
import oracle as O
import stage_ref as R
from conftest import close_grad, close_normscaled
from window_replay import case_pools, replay, same_bits

RTOL = 1e-5
F32 = np.float32


def in_bounds(got, want):
    """close_normscaled's error in units of the GPU tests' bound (> 1: the check fails)."""
    return close_normscaled(got, want, RTOL)[1] / RTOL


# ------------------------------------------------------------------ the input conditions
@pytest.mark.parametrize("n_envs,t_max", R.BPTT_LONG_CASES)
def test_chain_cases_have_long_chains(n_envs, t_max):
    d = R.bptt_chain_data(n_envs, t_max)
    rs = d["reset"][:t_max]
    assert R.crafted_flags_hold(rs)
    assert not rs[:, 0].any()                                         # env 0: one chain over the whole window
    assert rs[0, 1] and rs[t_max - 1, 1] and rs[:, 1].sum() == 2      # env 1: reset at step 0 and at step T - 1
    assert rs[32:, 2].sum() == 1 and rs[:, 2].sum() == 1              # env 2: once, past step 32
    assert n_envs == 3 or 0 < rs[:, 3:].mean() < 0.06
    assert (d["reset"][t_max] == 1).all()                             # (the slot past the window: lstm_data's)
    # the short cases keep the drawn flags, and with them their data
    old = R.bptt_chain_data(37, 5)
    assert old["reset"][0, 0] == 1 and 0.1 < old["reset"][:5].mean() < 0.35
    assert np.array_equal(old["reset"], R.lstm_data(37, 5)["reset"])


@pytest.mark.parametrize("kind,N,T,windows", [(c[7], c[2], c[3], c[6]) for c in L.FF_CASES]
                         + [("palette", c[1], c[2], c[5]) for c in L.LSTM_CASES])
def test_window_cases_have_the_crafted_terminals(kind, N, T, windows):
    dones = L.pool_dones(T, N)
    P = dones.shape[0]
    assert P == T + 2 and (T + 4) % P and P % (T + 4)                 # neither a multiple nor a divisor of R
    d = L.window_dones(dones, 0, T)
    assert R.crafted_flags_hold(d)
    assert not d[:, 0].any() and d[0, 1] and d[T - 1, 1] and d[32:].any()
    if N > 2:
        assert d[32:, 2].sum() == 1 and d[:32, 2].sum() == 0
    if windows > 1:                                                   # window two wraps the pool
        d2 = L.window_dones(dones, 1, T)
        assert max((T + t + 1) // P for t in range(T)) == 1 and (2 * T) % P == T - 2
        assert not d2[:, 0].any() and np.array_equal(d2[2:], d[:T - 2]) and not d2[:2].any()


def test_the_pools_are_the_gpu_cases_pools():
    obs, rewards, dones = L.pools("states", 5, 33)
    assert obs.shape == (35, 5, 4, 84, 84) and rewards.shape == (35, 5) and np.array_equal(dones, L.pool_dones(33, 5))
    assert not obs.flags.writeable and L.pools("states", 5, 33)[0] is obs


# ------------------------------------------------------------------ the float32 rounding of a long chain
def _sig32(x):
    return (F32(1) / (F32(1) + np.exp(-x))).astype(F32)


def chain32(Wl, reset, gates, cbuf, dH, cut=None):
    """stage_ref.lstm_bptt_chain_ref restated in float32 throughout (NumPy's matmul, exp and tanh), as a device
    kernel computes it.  cut: the mistake of a carry (dh and dc) dropped on the way from step cut to cut - 1."""
    T, n = dH.shape[0], gates.shape[1]
    dG = np.empty((T,) + gates.shape[1:], F32)
    dcn = None
    for t in range(T - 1, -1, -1):
        dh = dH[t].astype(F32)
        if t < T - 1 and t + 1 != cut:
            dh = dh + (dG[t + 1] @ Wl).astype(F32) * (reset[t + 1] == 0)[:, None].astype(F32)
        g = gates[t].reshape(n, R.HID, 4)
        a, i, f, o = np.tanh(g[..., 0]), _sig32(g[..., 1]), _sig32(g[..., 2]), _sig32(g[..., 3])
        rp = (reset[t] != 0)[:, None]
        tc, cp = np.tanh(cbuf[t + 1]), np.where(rp, F32(0), cbuf[t])
        dc = dh * o * (F32(1) - tc * tc)
        if dcn is not None and t + 1 != cut:
            dc = dc + dcn
        dG[t] = np.stack([dc * i * (F32(1) - a * a), dc * a * i * (F32(1) - i), dc * cp * f * (F32(1) - f),
                          dh * tc * o * (F32(1) - o)], -1).reshape(n, R.GATES)
        dcn = np.where(rp, F32(0), dc * f).astype(F32)
    return dG


@functools.lru_cache(maxsize=None)
def chain_case(n_envs, t_max):
    d = R.bptt_chain_data(n_envs, t_max)
    return d, R.lstm_bptt_chain_ref(d["Wl"], d["reset"], d["gates"], d["cbuf"], d["dh"])


CHAIN32_MAX = 2.5e-6   # a quarter of the suite's 1e-5: below it the issue's 4x allowance raises no bound


@pytest.mark.parametrize("n_envs,t_max", R.BPTT_LONG_CASES)
def test_float32_chain_against_float64(n_envs, t_max):
    """The reference-alone rounding error of the long chains: the float32 restatement against the float64
    reference, over the whole dG and per step.  Measured: 1.8e-7 of the scale at (3, 64), 2.0e-7 at (33, 33)
    (worst single step 2.9e-7 and 2.5e-7); 4x that is below the suite's 1e-5, so test_lstm_bptt_chain keeps 1e-5."""
    d, ref = chain_case(n_envs, t_max)
    g32 = chain32(d["Wl"], d["reset"], d["gates"], d["cbuf"], d["dh"])
    whole = close_normscaled(g32, ref, RTOL)[1]
    per = max(close_normscaled(g32[t], ref[t], RTOL)[1] for t in range(t_max))
    print(f"chain ({n_envs}, {t_max}): float32 against float64 {whole:.3g} of the scale, worst step {per:.3g}; "
          f"resets {d['reset'][:t_max].mean():.3f}")
    assert whole <= CHAIN32_MAX and per <= CHAIN32_MAX, (whole, per)
    assert np.abs(ref[0, 0]).max() > 0


@pytest.mark.parametrize("n_envs,t_max", R.BPTT_LONG_CASES)
def test_chain_tolerance_catches_a_dropped_carry(n_envs, t_max):
    """The carry dropped on one step past 9 and on one past 32 (there is none at T = 33: its last step, 32)."""
    d, ref = chain_case(n_envs, t_max)
    for cut in (10, 33 if t_max > 33 else 32):
        pert = chain32(d["Wl"], d["reset"], d["gates"], d["cbuf"], d["dh"], cut=cut)
        f, f_env0 = in_bounds(pert, ref), in_bounds(pert[:cut, 0], ref[:cut, 0])
        print(f"chain ({n_envs}, {t_max}) carry dropped from step {cut}: {f:.3g} x the bound, env 0's chain "
              f"{f_env0:.3g} x")
        assert f >= 10 and f_env0 >= 10, (cut, f, f_env0)
        assert np.array_equal(pert[cut:], chain32(d["Wl"], d["reset"], d["gates"], d["cbuf"], d["dh"])[cut:])


# ------------------------------------------------------------------ the oracle's LSTM window: carry mistakes, sized
def _lstm_window_cut():
    """oracle.lstm_window with the BPTT carry zeroed after step CUT (from its source, one statement added)."""
    src = inspect.getsource(O.lstm_window).replace("def lstm_window(", "def lstm_window_cut(CUT, ")
    line = '        dh_next = ((dg @ params["1/lateral/W"]) * m).astype(np.float32)\n'
    assert src.count(line) == 1
    src = src.replace(line, line + "        if t == CUT:\n            dh_next, dc_next = dh_next * 0, dc_next * 0\n")
    ns = dict(vars(O))
    exec(src, ns)
    return ns["lstm_window_cut"]


@functools.lru_cache(maxsize=None)
def lstm_case():
    """Window one and two of the (3, 64, 6) LSTM case's terminals on random uint8 stacks (the mistakes below
    do not depend on what the screens show), at init_like_torch weights: window one's run, and its state."""
    _, N, T, A, _, _, _ = L.LSTM_CASES[0]
    rng = np.random.default_rng(1)
    params = O.init_like_torch(O.ARCH_LSTM, A, rng)
    dones = L.pool_dones(T, N)
    x = O.PHI_LUT[rng.integers(0, 256, (2 * T + 1, N, 4, 84, 84), dtype=np.uint8)]
    acts = rng.integers(0, A, (2 * T, N)).astype(np.int32)
    r = rng.choice(np.array([-1, 0, 1], F32), (2 * T, N))
    d1 = L.window_dones(dones, 0, T)
    st0 = O.LSTMState(h=np.zeros((N, 256), F32), c=np.zeros((N, 256), F32), has=np.zeros(N, bool))
    dprev1 = np.concatenate([np.ones((1, N), np.uint8), d1[:-1]])
    args1 = (params, x[:T], acts[:T], r[:T], dprev1, d1, x[T], st0)
    g1, aux1 = O.lstm_window(*args1)
    return dict(N=N, T=T, params=params, x=x, acts=acts, r=r, dones=dones, args1=args1, g1=g1, aux1=aux1)


def _tensor_shift(g, ref):
    return {k: close_normscaled(g[k], ref[k], RTOL)[1] for k in ref}


def test_oracle_window_carry_dropped_inside_the_window():
    """The oracle's BPTT carry zeroed at step 55 and at step 32 of the 64-step window (env 0's chain runs over
    all of it): every gradient tensor the chain feeds moves by >= 0.04 of its scale, 4,000 x the 1e-5 bound
    (the heads' tensors do not depend on the chain)."""
    c = lstm_case()
    cut = _lstm_window_cut()
    chain_fed = [k for k in c["g1"] if not k.startswith(("2/", "3/"))]
    for CUT in (55, 32):
        g, _ = cut(CUT, *c["args1"])
        shift = _tensor_shift(g, c["g1"])
        print(f"carry zeroed at step {CUT}: " + " ".join(f"{k} {shift[k]:.2g}" for k in chain_fed))
        assert min(shift[k] for k in chain_fed) >= 0.04, shift
        assert all(shift[k] == 0 for k in c["g1"] if k not in chain_fed)


def test_oracle_window_two_without_the_carried_state():
    """Row T of h / c not carried into window two (it starts from zeros on the envs that go on): v and every
    gradient tensor but the value head's bias miss the bound by more than 10x; that bias, a plain sum of dv, by
    6.9x.  (hbuf[T] of window two is no witness: 64 steps on, the cell has forgotten how it started, 7e-8.)"""
    c = lstm_case()
    N, T = c["N"], c["T"]
    d1, d2 = L.window_dones(c["dones"], 0, T), L.window_dones(c["dones"], 1, T)
    dprev2 = np.concatenate([d1[-1:], d2[:-1]])
    assert dprev2[0, 1] and not dprev2[0, 0]                          # env 1 starts reset, env 0 goes on
    a = c["aux1"]
    def args(st):
        return c["params"], c["x"][T:2 * T], c["acts"][T:], c["r"][T:], dprev2, d2, c["x"][2 * T], st

    g, aux = O.lstm_window(*args(O.LSTMState(h=a["h_last"], c=a["c_last"], has=np.ones(N, bool))))
    gz, auxz = O.lstm_window(*args(O.LSTMState(h=np.zeros_like(a["h_last"]), c=np.zeros_like(a["c_last"]),
                                               has=np.ones(N, bool))))
    shift = _tensor_shift(gz, g)
    shift["v"] = close_normscaled(auxz["v"], aux["v"], RTOL)[1]
    print("window two from zeros: " + " ".join(f"{k} {e:.2g}" for k, e in shift.items())
          + f"; h_last {close_normscaled(auxz['h_last'], aux['h_last'], RTOL)[1]:.2g}")
    assert min(e for k, e in shift.items() if k != "3/0/b") >= 10 * RTOL and shift["3/0/b"] > RTOL, shift
    assert np.array_equal(auxz["v"][:, 1], aux["v"][:, 1])            # the env that starts reset never saw the carry


# ------------------------------------------------------------------ the returns scan
@pytest.mark.parametrize("T,A,N,lam", [(64, 4, 3, 1.0), (33, 6, 5, 0.95), (64, 4, 2, 0.95), (33, 6, 3, 1.0)])
def test_returns_tolerance_catches_a_scan_that_stops_after_32_rows(T, A, N, lam):
    """A returns scan that covers rows 0 .. 31 only (the bootstrap value taken as row 32's, rows >= 32 left
    without a gradient) on returns_data's operands under the case's crafted terminals."""
    d = R.returns_data(T, A, N)
    dones = L.window_dones(L.pool_dones(T, N), 0, T)
    ref = R.returns_heads_ref(d["rewards"], dones, d["v"], d["probs"], d["logp"], d["actions"], d["Wpi"], d["Wv"],
                              d["hfc"][:T], lam=lam)
    v32 = np.concatenate([d["v"][:32], d["v"][T:]])
    part = R.returns_heads_ref(d["rewards"][:32], dones[:32], v32, d["probs"][:32], d["logp"][:32], d["actions"][:32],
                               d["Wpi"], d["Wv"], d["hfc"][:32], lam=lam)
    for what, got, want in zip(("dlogits", "dv", "loss", "dfc"), part, ref):
        pert = want.copy()
        if what == "loss":
            pert = got
        else:
            pert[:32], pert[32:] = got, 0.0
        f, f_head = in_bounds(pert, want), (in_bounds(pert[:32, 0], want[:32, 0]) if what != "loss" else np.inf)
        print(f"returns T={T} A={A} N={N} lambda={lam} {what}: {f:.3g} x the bound, env 0's rows 0..31 {f_head:.3g} x")
        assert f >= 10 and f_head >= 10, (what, f, f_head)


# ------------------------------------------------------------------ the ring residue
def test_conv_tolerance_catches_a_ring_of_9_slots():
    """The ring residue taken with R = 9 (every ring case before these) instead of T + 4: conv_fwd at slots 0 and
    63 of the (3, 64) case, conv_bwd's gradient over its 192 samples, and slot 0 of a T = 33 net under each of
    ring_starts(33)."""
    n_envs, t_max, slots = R.CONV_FWD_LONG_CASE
    d = R.conv_fwd_data(n_envs, "ring", t_max=t_max)
    assert d["R"] == 68 and d["frames"].shape[0] == 68 and slots == (0, 63, 64)
    bad = R.RingX(d["frames"], d["nvalid"], n_envs, t_max, steps=t_max + 1)
    bad.R = 9
    for t in slots[:2]:
        sl = slice(t * n_envs, (t + 1) * n_envs)
        ref = R.conv_fwd_ref(d["x"][sl], d["W1"], d["b1"], d["W2"], d["b2"])
        pert = R.conv_fwd_ref(bad[sl], d["W1"], d["b1"], d["W2"], d["b2"])
        f = min(in_bounds(pert[0], ref[0]), in_bounds(pert[1], ref[1]))
        print(f"conv_fwd (3, 64) slot {t} with R = 9: {f:.3g} x the bound")
        assert f >= 10, (t, f)
    c = R.conv_data(3, 64)
    assert c["R"] == 68 and (3, 64) in R.CONV_CASES
    a1 = c["a1"][:64].reshape(192, 16, 20, 20)
    ref, mag = R.conv_bwd_ref(c["x"], a1, c["da2"], c["W2"])
    bad = R.RingX(c["frames"], c["nvalid"], 3, 64)
    bad.R = 9
    pert, _ = R.conv_bwd_ref(bad, a1, c["da2"], c["W2"])
    f = max(in_bounds(pert["c1W"], ref["c1W"]), close_grad(pert["c1W"], ref["c1W"], mag["c1W"], RTOL)[1] / RTOL)
    print(f"conv_bwd (3, 64) with R = 9: conv1's weight gradient {f:.3g} x the bound")
    assert f >= 10, f
    assert all(np.array_equal(pert[k], ref[k]) for k in ("c1b", "c2W", "c2b"))   # (nothing else reads the ring)
    T = R.CONV_FWD_RING_T
    rng = np.random.default_rng(33)
    frames = rng.integers(0, 256, (T + 4, 2, 84, 84), dtype=np.uint8)
    nvalid = np.full((T + 4, 2), 4, np.uint8)
    for start in R.ring_starts(T):
        assert start % (T + 4) != start % 9
        good = R.RingX(frames, nvalid, 2, T, start=start)[:2]
        bad = R.RingX(frames, nvalid, 2, T, start=start)
        bad.R = 9
        f = in_bounds(bad[:2], good)
        print(f"state of slot 0, T = 33, start {start}, with R = 9: {f:.3g} x the bound")
        assert f >= 10, (start, f)


# ------------------------------------------------------------------ the window record past 256 envs
def test_window_record_notices_skipped_envs_past_256():
    """A statistics scan that stops at env 255 of 260 (t_max 10, the GPU case's pools): every sum field of the
    record differs from the replay's in its bits; the sample count by 40."""
    n, T = 260, 10
    rewards, dones = case_pools(10, T + 2, n)
    rng = np.random.default_rng(10)
    idx = [(t + 1) % (T + 2) for t in range(T)]
    r, d = rewards[idx], dones[idx]
    v, ent = rng.standard_normal((T + 1, n)).astype(F32), rng.random((T + 1, n)).astype(F32)
    loss = rng.standard_normal((n, 2)).astype(F32)
    full = replay(r, d, v, ent, loss)
    short = replay(r[:, :256], d[:, :256], v[:, :256], ent[:, :256], loss[:256])
    assert full[0] - short[0] == 4 * T
    same = [i for i in range(12) if same_bits(np.float64(full[i]), np.float64(short[i]))]
    assert not same, same


# ------------------------------------------------------------------ the clip + RMSProp delta check, clip active
def test_delta_check_floor_of_the_nature_gae_case():
    """_run_ff's last check holds new - old parameters to 1e-5 of the largest step of their tensor.  On the Nature
    (2, 64, 4) GAE case the oracle's own gradient has norm 41.3, the first whole-window case of the suite where the
    clip at 40 is active, and the clipped steps are small: conv2's largest is 2.68e-4 while one float32 ulp of its
    largest parameter is 3.7e-9, 1.39e-5 of that step.  The oracle's update with a clip scale one float32 ulp off
    (an f64 norm against one from f32 partial sums differ by that) moves 101 of conv2's 32,768 parameters by one
    ulp: a delta error of 1.39e-5 on the reference alone, above the bound.  Printed for every tensor.  So the
    update's norm has to give the f32 scale the f64 norm gives: grad_sqnorm_kernel sums in f64."""
    from sim import OracleEnvView
    from gae_replay import patched
    _, arch, N, T, A, lam, _, kind = L.FF_CASES[3]
    assert (arch, N, T, A, lam) == (O.ARCH_FF_NATURE, 2, 64, 4, 0.95)
    pairs, rewards, dones = L.pools(kind, N, T)
    params = O.init_like_torch(arch, A, np.random.default_rng(60 + T))      # the GPU case's init_seed
    view = OracleEnvView(pairs, dones)
    x, boot = view.states_f32(0, T)
    r, d = view.window_rd(rewards, 0, T)
    lo, _, _ = O.pi_and_v_ff(params, x.reshape(T * N, 4, 84, 84), arch)
    p0 = O.softmax(lo).reshape(T, N, A)
    acts = np.stack([O.sample_from_uniform(p0[t], O.sample_uniforms(99, np.arange(N, dtype=np.uint64), t))
                     for t in range(T)]).astype(np.int32)
    with patched(lam):
        g, _ = O.ff_window_grads(params, x, acts, r, d, boot, arch=arch)
    names = list(g)
    gl, norm = O.clip_grads([g[k] for k in names], 40.0, exact_norm=True)
    assert norm > 40.0
    rate = np.nextafter(F32(40.0 / norm), F32(0))
    worst = {}
    for k, gk in zip(names, gl):
        p1, _ = O.rmsprop_update(params[k], np.zeros_like(params[k]), gk, 7e-4)
        p2, _ = O.rmsprop_update(params[k], np.zeros_like(params[k]), (g[k] * rate).astype(F32), 7e-4)
        step = float(np.abs(p1 - params[k]).max())
        worst[k] = close_normscaled(p2 - params[k], p1 - params[k], RTOL)[1]
        print(f"{k}: gradient norm {norm:.4g}, largest step {step:.3g}, ulp(max |p|) / step "
              f"{float(np.spacing(np.abs(p1).max())) / step:.3g}, delta error with the clip scale one ulp off "
              f"{worst[k]:.3g}, {int((p1 != p2).sum())} of {p1.size} parameters differ")
    assert worst["0/1/W"] > RTOL and max(worst.values()) < 2e-5
