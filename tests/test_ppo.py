"""CPU: the clipped-surrogate (PPO) epochs' reference (ppo_ref.py) pinned against what it must reduce
to and against finite differences, and the host-side validation of the new entry points -- no kernel
launches."""
import ctypes
import math

import numpy as np
import pytest

import oracle as O
import ppo_ref
from gae_replay import gae_adv, returns_and_lossgrad_gae, window_case

F32 = np.float32
GAMMA, BETA, VCOEF = 0.99, 0.01, 0.5
GRID = np.array([-0.6, -0.35, -0.1, 0.1, 0.35, 0.6], F32)     # logp_old - logp_new: ratios 1.82 .. 0.55


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_on_live(got, want, live):
    """Bit for bit on the live samples; a sample that is not live is zero (the oracle leaves +-0 there)."""
    return bits_equal(got[live], want[live]) and (got[~live] == 0).all() and (want[~live] == 0).all()


def oracle_args(c, T):
    d = c["dones"]
    return (c["rewards"], d & 1, c["v"][:T], c["v"][T], c["probs"][:T], c["logp"][:T], c["actions"][:T])


# A in {4, 6}: NumPy sums rows under 8 elements serially, as the device and ppo_ref do
@pytest.mark.parametrize("T,n,A", [(5, 75, 4), (9, 33, 6)])
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("clip_reward", [True, False])
def test_at_ratio_one_the_epoch_is_the_a3c_gradient(T, n, A, keep, clip_reward):
    c = window_case(7 + T, T, n, A, truncate=True)
    live = (c["dones"] & 2) == 0
    kw = dict(gamma=GAMMA, beta=BETA, v_loss_coef=VCOEF, clip_reward=clip_reward, pi_loss_coef=0.5,
              keep_loss_scale_same=keep, t_max=T, valid=live)
    # n-step
    lpo, adv, ret = ppo_ref.snapshot(c["rewards"], c["dones"], c["v"], c["logp"], c["actions"], GAMMA, 1.0, clip_reward)
    R_w, adv_w, dl_w, dv_w, _, _ = O.returns_and_lossgrad(*oracle_args(c, T), **kw)
    assert same_on_live(ret, R_w * live, live) and same_on_live(adv, adv_w * live, live)
    o = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, 0.2, BETA, 0.5, VCOEF, keep)
    assert (o["ratio"][live] == 1).all() and o["active"][live].all()
    assert same_on_live(o["dlogits"], dl_w, live) and same_on_live(o["dv"], dv_w, live)
    assert np.abs(dl_w).max() > 0
    # GAE: the snapshot's adv is gae_adv's
    lam = 0.95
    lpo, adv, ret2 = ppo_ref.snapshot(c["rewards"], c["dones"], c["v"], c["logp"], c["actions"], GAMMA, lam, clip_reward)
    assert bits_equal(ret2, ret)
    assert same_on_live(adv, gae_adv(c["rewards"], c["dones"], c["v"][:T], c["v"][T], GAMMA, lam, clip_reward) * live, live)
    _, _, dl_g, dv_g, _, _ = returns_and_lossgrad_gae(*oracle_args(c, T), lam=lam, **kw)
    o = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret2, 0.2, BETA, 0.5, VCOEF, keep)
    assert same_on_live(o["dlogits"], dl_g, live) and same_on_live(o["dv"], dv_g, live)
    assert not bits_equal(dl_g, dl_w)


def shifted_case(seed, T, n, A):
    """A window_case whose snapshot's logp_old is moved off the current policy by the grid."""
    c = window_case(seed, T, n, A, truncate=True)
    lpo, adv, ret = ppo_ref.snapshot(c["rewards"], c["dones"], c["v"], c["logp"], c["actions"], GAMMA, 1.0, True)
    delta = np.random.default_rng(seed).choice(GRID, (T, n)).astype(F32)
    live = (c["dones"] & 2) == 0
    lpo = np.where(live, (lpo + delta).astype(F32), F32(0)).astype(F32)
    return c, lpo, adv, ret, live


def classes(o, adv):
    """The four (sign of adv x active / inactive) classes of the live samples."""
    live, act, pos = o["live"], o["active"], adv >= 0
    return {(s, a): live & (pos == s) & (act == a) for s in (True, False) for a in (True, False)}


def f64_loss(z, v, ac, lpo, adv, ret, lo, hi, beta, pf, vf):
    """pf * (-min(rho A, clip(rho, lo, hi) A) - beta H(z)) + vf * (v - R)^2 / 2 of one sample, float64."""
    m = z.max()
    lp = z - (m + math.log(np.exp(z - m).sum()))
    p = np.exp(lp)
    rho = math.exp(lp[ac] - lpo)
    surr = min(rho * adv, min(max(rho, lo), hi) * adv)
    H = -(p * lp).sum()
    return pf * (-surr - beta * H) + vf * 0.5 * (v - ret) ** 2


def test_gradient_formula_against_finite_differences():
    """The reference's dlogits / dv are the derivative of the clipped surrogate + entropy + value loss: central
    differences in float64 (h = 1e-5, truncation error ~1e-10) against the f32 formula on f32 softmax outputs.
    Bound 2e-5: the inputs carry 6e-8 relative rounding, |adv| <= 6 here and the formula is ~10 f32 operations,
    so its error stays under 1e-5; the rest is margin for the larger coefficients.  15 samples of each class."""
    T, n, A = 5, 75, 4
    c, lpo, adv, ret, live = shifted_case(3, T, n, A)
    rng = np.random.default_rng(0)
    logits = rng.standard_normal((T + 1, n, A)).astype(F32)
    c["probs"] = O.softmax(logits.reshape(-1, A)).reshape(T + 1, n, A)
    c["logp"] = O.log_softmax(logits.reshape(-1, A)).reshape(T + 1, n, A)
    lpa = np.take_along_axis(c["logp"][:T], c["actions"][:T, :, None].astype(np.int64), 2)[..., 0]
    delta = rng.choice(GRID, (T, n)).astype(F32)
    lpo = np.where(live, (lpa + delta).astype(F32), F32(0)).astype(F32)
    pcoef, eps = 0.7, 0.2
    o = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, eps, BETA, pcoef, VCOEF)
    lo, hi = (float(x) for x in ppo_ref.clip_range(eps))
    h, worst = 1e-5, 0.0
    for key, mask in classes(o, adv).items():
        idx = np.argwhere(mask)
        assert len(idx) >= 15, key
        for t, e in idx[:15]:
            z, v = logits[t, e].astype(np.float64), float(c["v"][t, e])
            args = (int(c["actions"][t, e]), float(lpo[t, e]), float(adv[t, e]), float(ret[t, e]), lo, hi, BETA, pcoef,
                    VCOEF)
            for k in range(A):
                dz = np.zeros(A)
                dz[k] = h
                fd = (f64_loss(z + dz, v, *args) - f64_loss(z - dz, v, *args)) / (2 * h)
                worst = max(worst, abs(fd - float(o["dlogits"][t, e, k])))
            fd = (f64_loss(z, v + h, *args) - f64_loss(z, v - h, *args)) / (2 * h)
            worst = max(worst, abs(fd - float(o["dv"][t, e])))
            if not key[1]:      # an inactive sample: the policy term has no gradient, only the entropy's is left
                w0 = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv * 0, ret, eps,
                                      BETA, pcoef, VCOEF)["dlogits"][t, e]
                assert bits_equal(o["dlogits"][t, e], w0)
    print(f"finite differences: worst abs err {worst:.3e}")
    assert worst < 2e-5


def test_rho_argument_replaces_the_ratio():
    c, lpo, adv, ret, live = shifted_case(5, 5, 33, 6)
    a = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret)
    b = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, rho=a["own_ratio"])
    assert all(bits_equal(a[k], b[k]) for k in ("dlogits", "dv", "loss", "ratio"))
    one = np.ones_like(lpo)
    b = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, rho=one)
    assert not bits_equal(a["dlogits"], b["dlogits"]) and bits_equal(a["dv"], b["dv"])


def test_patched_oracle_window_uses_the_snapshot():
    T, n, A = 5, 8, 4
    c, lpo, adv, ret, live = shifted_case(11, T, n, A)
    want = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, 0.2, BETA, 1.0, VCOEF)
    before = O.returns_and_lossgrad
    with ppo_ref.patched(lpo, adv, ret, 0.2):
        R, a, dl, dv, pl, vl = O.returns_and_lossgrad(*oracle_args(c, T), GAMMA, BETA, VCOEF, valid=live)
    assert O.returns_and_lossgrad is before
    assert bits_equal(dl, want["dlogits"]) and bits_equal(dv, want["dv"]) and bits_equal(R, ret) and bits_equal(a, adv)
    assert pl == float(want["loss"][:, 0].sum()) and vl == float(want["loss"][:, 1].sum())


# ------------------------------------------------------------------ the C ABI, no device
OK, EINVAL, ESTATE = 0, 1, 3
FAKE = 1 << 40            # 256-byte aligned, never dereferenced


def make(lib, arch, bind=False):
    h = ctypes.c_void_p()
    assert lib.arl_net_create(ctypes.byref(h), arch, 4, 32, 5, 0, 0) == 0
    if bind:
        assert lib.arl_net_bind(h, FAKE, FAKE, FAKE, FAKE) == 0
    return h


def test_set_ppo_validation():
    from asyncrl_amd._lib import lib
    snap = FAKE + (1 << 30)
    for arch, want in ((0, OK), (16, OK), (32, OK), (64, OK), (1, ESTATE), (1 | 16, ESTATE), (2, ESTATE)):
        h = make(lib, arch)
        try:
            assert lib.arl_net_set_ppo(h, snap, 0.2) == want, arch
            if want == ESTATE:
                assert b"FF" in lib.arl_last_error()
            assert lib.arl_net_set_ppo(h, None, 0.2) == OK           # off: always
            for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
                assert lib.arl_net_set_ppo(h, snap, bad) == EINVAL, bad
            assert lib.arl_net_set_ppo(h, snap + 4, 0.2) == EINVAL   # 16-byte alignment
        finally:
            lib.arl_net_destroy(h)
    assert lib.arl_net_set_ppo(None, snap, 0.2) == EINVAL


def test_ppo_calls_need_a_bound_net_with_ppo_on_and_a_snapshot():
    from asyncrl_amd._lib import lib
    snap = FAKE + (1 << 30)
    h = make(lib, 0)
    try:
        assert lib.arl_net_set_ppo(h, snap, 0.2) == OK
        assert lib.arl_ppo_begin(h, GAMMA, 1, None) == ESTATE and b"bound" in lib.arl_last_error()
        assert lib.arl_ppo_learn(h, BETA, VCOEF, None) == ESTATE and b"bound" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)
    h = make(lib, 0, bind=True)
    try:
        assert lib.arl_ppo_begin(h, GAMMA, 1, None) == ESTATE and b"off" in lib.arl_last_error()
        assert lib.arl_ppo_learn(h, BETA, VCOEF, None) == ESTATE and b"off" in lib.arl_last_error()
        assert lib.arl_net_set_ppo(h, snap, 0.2) == OK
        assert lib.arl_ppo_learn(h, BETA, VCOEF, None) == ESTATE and b"arl_ppo_begin" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)


def test_run_window_refuses_while_ppo_is_set():
    from asyncrl_amd._lib import lib
    h = make(lib, 0, bind=True)
    try:
        args = (FAKE + (2 << 30), None, None, 8, 1, 0, GAMMA, BETA, VCOEF, 1, 7e-4, 0, 0, 0.99, 0.1, 40.0, None)
        assert lib.arl_run_window(h, *args) == EINVAL                 # (PPO off: the unregistered pool, no launch)
        assert lib.arl_net_set_ppo(h, FAKE + (1 << 30), 0.2) == OK
        assert lib.arl_run_window(h, *args) == ESTATE and b"epochs" in lib.arl_last_error()
        assert lib.arl_net_set_ppo(h, None, 0.0) == OK
        assert lib.arl_run_window(h, *args) == EINVAL
    finally:
        lib.arl_net_destroy(h)


def test_granular_entries_validate_before_any_launch():
    from asyncrl_amd._lib import lib
    p = FAKE
    assert lib.arl_ppo_snapshot(p, p, p, p, p, 5, 4, 4, GAMMA, 1.5, 1, p, p, p, None) == EINVAL      # lambda
    assert lib.arl_ppo_snapshot(p, p, p, p, p, 0, 4, 4, GAMMA, 1.0, 1, p, p, p, None) == EINVAL      # t_max
    assert lib.arl_ppo_snapshot(p, p, p, p, p, 5, 4, 4, GAMMA, 1.0, 1, p, None, p, None) == EINVAL   # null
    assert lib.arl_ppo_snapshot(None, None, None, None, None, 5, 0, 4, GAMMA, 1.0, 1, None, None, None, None) == OK
    tail = (BETA, 1.0, VCOEF, 0, p, p, None, None, None)
    assert lib.arl_ppo_lossgrad(p, p, p, p, p, p, p, p, 5, 4, 4, 0.0, *tail) == EINVAL              # clip_eps
    assert lib.arl_ppo_lossgrad(p, p, p, p, p, p, p, p, 5, 4, 4, float("nan"), *tail) == EINVAL
    assert lib.arl_ppo_lossgrad(p, p, p, p, p, p, p, p, 5, 4, 33, 0.2, *tail) == EINVAL             # n_actions
    assert lib.arl_ppo_lossgrad(p, p, p, p, p, None, p, p, 5, 4, 4, 0.2, *tail) == EINVAL           # null
    assert lib.arl_ppo_lossgrad(p, p, p, p, p, p, p, p, 5, 0, 4, 0.2, *tail) == OK                  # n == 0


# ------------------------------------------------------------------ A3C's arguments, no device
class FakeNet:
    """What A3C.__init__ and run_window's argument checks touch, without a device."""
    t_max, n_envs, stack, states, arch, base_arch, env = 5, 32, False, False, 0, 0, None

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a))


class FakeModel:
    frames = "pairs"

    def __init__(self):
        self.net = FakeNet()


class FakeOpt:
    target = None

    def setup(self, model):
        self.target = model


def test_a3c_validates_the_ppo_arguments():
    from asyncrl_amd import A3C
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="ppo_epochs"):
            A3C(FakeModel(), FakeOpt(), 5, GAMMA, ppo_epochs=bad)
    for bad in (0.0, 1.0, -0.2, float("nan")):
        with pytest.raises(ValueError, match="ppo_clip"):
            A3C(FakeModel(), FakeOpt(), 5, GAMMA, ppo_epochs=2, ppo_clip=bad)
    with pytest.raises(ValueError, match="one rank"):
        A3C(FakeModel(), FakeOpt(), 5, GAMMA, ppo_epochs=2, collectives=True)
    m = FakeModel()
    agent = A3C(m, FakeOpt(), 5, GAMMA, ppo_epochs=3, ppo_clip=0.1)
    assert ("set_ppo", (0.1,)) in m.net.calls
    with pytest.raises(ValueError, match="split_update"):
        agent.run_window(None, None, None, 6, first=True, split_update=True)
    m = FakeModel()
    A3C(m, FakeOpt(), 5, GAMMA)                                        # the default never touches set_ppo
    assert not [c for c in m.net.calls if c[0] == "set_ppo"]
