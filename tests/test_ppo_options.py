"""CPU: the PPO epochs' options (arl_net_set_ppo_options: advantage normalisation, the clipped value
loss, the per-epoch record) -- the restatement's own invariants (ppo_options_ref.py) and the
host-side validation of the new entry points; no kernel launches."""
import ctypes

import numpy as np
import pytest

import ppo_options_ref as R
import ppo_ref
from gae_replay import window_case
from test_ppo import FAKE, FakeModel, FakeOpt, bits_equal, make

F32, F64 = np.float32, np.float64
GAMMA, BETA, VCOEF = 0.99, 0.01, 0.5
OK, EINVAL, ESTATE = 0, 1, 3
SHAPES = [(5, 75, 4), (9, 33, 6), (5, 1, 18), (4, 600, 4)]


def snap(i, lam=1.0):
    T, n, A = SHAPES[i]
    c = window_case(60 + i, T, n, A, truncate=True)
    return c, ppo_ref.snapshot(c["rewards"], c["dones"], c["v"], c["logp"], c["actions"], GAMMA, lam, True)


# ------------------------------------------------------------------ the restatement's invariants
@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("i", [0, 1, 3])
def test_normalised_advantages_have_mean_zero_and_std_one(i, lam):
    c, (lpo, adv, ret) = snap(i, lam)
    live = (c["dones"] & 2) == 0
    out, (n_live, mean, std) = R.normalize_adv(c["dones"], adv)
    assert n_live == live.sum() and out.dtype == F32
    x = out[live].astype(F64)
    assert abs(x.mean()) < 1e-6 and abs(x.std() - 1.0) < 1e-6            # (population std, as the kernel's)
    assert abs(mean - adv[live].astype(F64).mean()) < 1e-12 and abs(std - adv[live].astype(F64).std()) < 1e-12
    assert (out[~live] == 0).all() and (~live).sum() == 2


def test_equal_advantages_normalise_to_exactly_zero():
    c, (lpo, adv, ret) = snap(0)
    live = (c["dones"] & 2) == 0
    flat = np.where(live, F32(0.37), F32(0)).astype(F32)
    out, (n_live, mean, std) = R.normalize_adv(c["dones"], flat)
    assert (out == 0).all() and std == 0 and mean == F64(F32(0.37))
    none = np.full_like(c["dones"], 2)                                   # no live sample: nothing is rewritten
    out, m = R.normalize_adv(none, adv)
    assert bits_equal(out, adv) and m == (0, 0, 0)


def test_ordered_sum_is_the_threads_order():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((4, 600))
    live = rng.random((4, 600)) < 0.9
    part = [0.0] * 256
    for j in range(256):
        for e in range(j, 600, 256):
            for t in range(4):
                part[j] = part[j] + (float(x[t, e]) if live[t, e] else 0.0)
    total = part[0]
    for q in range(1, 256):
        total = total + part[q]
    assert R.ordered_sum(x, live) == total


@pytest.mark.parametrize("keep", [False, True])
def test_value_clip_with_v_old_equal_to_v_is_the_plain_epoch(keep):
    for i in range(len(SHAPES)):
        T, n, A = SHAPES[i]
        c, (lpo, adv, ret) = snap(i)
        args = (c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret)
        want = ppo_ref.lossgrad(*args, 0.2, BETA, 0.5, VCOEF, keep)
        got = R.lossgrad_vclip(*args, c["v"][:T], 0.2, 0.1, BETA, 0.5, VCOEF, keep)
        assert not got["taken"].any() and bits_equal(got["inside"], got["live"])
        for k in ("dlogits", "dv", "loss", "lv", "lpi", "ratio"):
            assert bits_equal(got[k], want[k]), (i, k)


def test_value_clip_is_the_gradient_of_the_max():
    """0.5 * max((v - R)^2, (v_clip - R)^2) in float64 against the f32 restatement: the loss within f32 rounding,
    dv = vf * (v - R) where the unclipped square is the larger (or v is inside), else 0."""
    T, n, A = SHAPES[0]
    c, (lpo, adv, ret) = snap(0)
    delta = np.random.default_rng(1).choice(np.array([-0.3, -0.15, -0.05, 0.05, 0.15, 0.3], F32), (T, n))
    v_old = (c["v"][:T] + delta).astype(F32)
    o = R.lossgrad_vclip(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret, v_old, 0.2, 0.1, BETA,
                         1.0, VCOEF)
    live = o["live"]
    v, r, vo = (x.astype(F64) for x in (c["v"][:T], ret, v_old))
    vc = vo + np.clip(v - vo, -float(F32(0.1)), float(F32(0.1)))
    lu, lc = (v - r) ** 2, (vc - r) ** 2
    assert np.allclose(o["lv"][live], (VCOEF * 0.5 * np.maximum(lu, lc))[live], rtol=1e-5, atol=1e-7)
    kept = live & ~o["taken"]
    assert bits_equal(o["dv"][kept], (F32(VCOEF) * (c["v"][:T] - ret).astype(F32)).astype(F32)[kept])
    assert (o["dv"][o["taken"]] == 0).all() and (lc > lu)[o["taken"]].all() and o["taken"].sum() > 20


def test_epoch_record_fields():
    T, n, A = SHAPES[0]
    c, (lpo, adv, ret) = snap(0)
    o = ppo_ref.lossgrad(c["dones"], c["v"], c["probs"], c["logp"], c["actions"], lpo, adv, ret)
    rec = R.epoch_record(c["dones"], c["v"], c["logp"], c["actions"], lpo, adv, ret, o["ratio"], None, 0.2, 0.0, 7, 2)
    live = o["live"]
    assert rec.shape == (R.PPO_STAT_FIELDS,) and len(R.FIELDS) == R.PPO_STAT_FIELDS
    assert list(rec[:4]) == [7, 2, live.sum(), 0] and rec[4] == 0 and rec[5] == 1 and rec[6] == 1 and rec[7] == 0
    assert abs(rec[8] - adv[live].astype(F64).sum()) < 1e-9
    none = np.full_like(c["dones"], 2)
    assert not R.epoch_record(none, c["v"], c["logp"], c["actions"], lpo, adv, ret, o["ratio"])[2:].any()


# ------------------------------------------------------------------ the C ABI, no device
def test_new_symbols_exist():
    from asyncrl_amd import _lib
    for name in ("arl_net_set_ppo_options", "arl_ppo_normalize_adv", "arl_ppo_lossgrad_vclip", "arl_ppo_epoch_stats"):
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None
    assert _lib.PPO_AUX_DOUBLES == 8 + 16 * 10 == R.PPO_AUX_HEAD + R.PPO_LOG * R.PPO_STAT_FIELDS
    assert _lib.PPO_STAT_NAMES == R.FIELDS
    assert _lib.lib.arl_abi_version() == 4


def test_set_ppo_options_validation():
    from asyncrl_amd._lib import lib
    vo, aux = FAKE + (1 << 30), FAKE + (2 << 30)
    for arch, want in ((0, OK), (16, OK), (32, OK), (64, OK), (1, ESTATE), (1 | 16, ESTATE), (2, ESTATE)):
        h = make(lib, arch)                                            # (an unbound handle: host state only)
        try:
            assert lib.arl_net_set_ppo_options(h, 1, 0.1, vo, aux) == want, arch
            if want == ESTATE:
                assert b"FF" in lib.arl_last_error()
            assert lib.arl_net_set_ppo_options(h, 0, 0.0, None, None) == OK          # the defaults: always
            for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
                assert lib.arl_net_set_ppo_options(h, 0, bad, vo, aux) == EINVAL, bad
            assert lib.arl_net_set_ppo_options(h, 0, 0.1, None, aux) == EINVAL       # value clipping needs v_old
            assert lib.arl_net_set_ppo_options(h, 1, 0.0, None, None) == EINVAL      # normalisation needs aux
            assert lib.arl_net_set_ppo_options(h, 0, 0.1, vo + 4, aux) == EINVAL     # 16-byte alignment
            assert lib.arl_net_set_ppo_options(h, 1, 0.0, None, aux + 4) == EINVAL   # 8-byte alignment
            for args in ((0, 0.1, vo, None), (1, 0.0, None, aux), (0, 0.0, None, aux)):
                assert lib.arl_net_set_ppo_options(h, *args) == want, (arch, args)
            assert lib.arl_net_set_ppo_options(h, 0, 0.0, vo, None) == OK            # (v_old alone switches nothing on)
        finally:
            lib.arl_net_destroy(h)
    assert lib.arl_net_set_ppo_options(None, 0, 0.0, None, None) == EINVAL


def test_options_stay_inert_while_ppo_is_off():
    from asyncrl_amd._lib import lib
    h = make(lib, 0, bind=True)
    try:
        assert lib.arl_net_set_ppo_options(h, 1, 0.1, FAKE + (1 << 30), FAKE + (2 << 30)) == OK
        assert lib.arl_ppo_begin(h, GAMMA, 1, None) == ESTATE and b"off" in lib.arl_last_error()
        assert lib.arl_ppo_learn(h, BETA, VCOEF, None) == ESTATE and b"off" in lib.arl_last_error()
    finally:
        lib.arl_net_destroy(h)


def test_granular_entries_validate_before_any_launch():
    from asyncrl_amd._lib import lib
    p = FAKE
    # arl_ppo_normalize_adv(dones, adv, t_max, n, moments, stream)
    assert lib.arl_ppo_normalize_adv(p, p, 0, 4, p, None) == EINVAL                   # t_max
    assert lib.arl_ppo_normalize_adv(p, p, 257, 4, p, None) == EINVAL
    assert lib.arl_ppo_normalize_adv(p, p, 5, -1, p, None) == EINVAL
    assert lib.arl_ppo_normalize_adv(p, None, 5, 4, p, None) == EINVAL                # null
    assert lib.arl_ppo_normalize_adv(p, p, 5, 4, None, None) == EINVAL
    assert lib.arl_ppo_normalize_adv(p, p, 5, 4, p + 4, None) == EINVAL               # alignment
    assert lib.arl_ppo_normalize_adv(None, None, 5, 0, None, None) == OK              # n == 0
    # arl_ppo_lossgrad_vclip(.., ret, v_old, t_max, n, A, clip_eps, vclip_eps, ..)
    head = (p,) * 9
    tail = (BETA, 1.0, VCOEF, 0, p, p, None, None, None)
    assert lib.arl_ppo_lossgrad_vclip(*head, 5, 4, 4, 0.0, 0.1, *tail) == EINVAL      # clip_eps
    assert lib.arl_ppo_lossgrad_vclip(*head, 5, 4, 4, 0.2, 0.0, *tail) == EINVAL      # vclip_eps
    assert lib.arl_ppo_lossgrad_vclip(*head, 5, 4, 4, 0.2, float("nan"), *tail) == EINVAL
    assert lib.arl_ppo_lossgrad_vclip(*head, 5, 4, 4, 0.2, float("inf"), *tail) == EINVAL
    assert lib.arl_ppo_lossgrad_vclip(*head, 5, 4, 33, 0.2, 0.1, *tail) == EINVAL     # n_actions
    assert lib.arl_ppo_lossgrad_vclip(*head, 257, 4, 4, 0.2, 0.1, *tail) == EINVAL    # t_max
    assert lib.arl_ppo_lossgrad_vclip(*head[:8], None, 5, 4, 4, 0.2, 0.1, *tail) == EINVAL   # null v_old
    assert lib.arl_ppo_lossgrad_vclip(*head, 5, 0, 4, 0.2, 0.1, *tail) == OK          # n == 0
    # arl_ppo_epoch_stats(dones, v, logp, act, lpo, adv, ret, ratio, v_old, t_max, n, A, clip, vclip, window, epoch, rec)
    e8 = (p,) * 8
    assert lib.arl_ppo_epoch_stats(*e8, None, 0, 4, 4, 0.2, 0.0, 0.0, 1.0, p, None) == EINVAL     # t_max
    assert lib.arl_ppo_epoch_stats(*e8, None, 5, 4, 33, 0.2, 0.0, 0.0, 1.0, p, None) == EINVAL    # n_actions
    assert lib.arl_ppo_epoch_stats(*e8, None, 5, 4, 4, 1.0, 0.0, 0.0, 1.0, p, None) == EINVAL     # clip_eps
    assert lib.arl_ppo_epoch_stats(*e8, p, 5, 4, 4, 0.2, 0.0, 0.0, 1.0, p, None) == EINVAL        # v_old needs eps
    assert lib.arl_ppo_epoch_stats(*e8, p, 5, 4, 4, 0.2, -1.0, 0.0, 1.0, p, None) == EINVAL
    assert lib.arl_ppo_epoch_stats(*e8[:7], None, None, 5, 4, 4, 0.2, 0.0, 0.0, 1.0, p, None) == EINVAL   # null ratio
    assert lib.arl_ppo_epoch_stats(*e8, None, 5, 4, 4, 0.2, 0.0, 0.0, 1.0, None, None) == EINVAL  # null record
    assert lib.arl_ppo_epoch_stats(*e8, None, 5, 4, 4, 0.2, 0.0, 0.0, 1.0, p + 4, None) == EINVAL
    assert lib.arl_ppo_epoch_stats(*e8, p, 5, 0, 4, 0.2, 0.1, 0.0, 1.0, p, None) == OK            # n == 0


# ------------------------------------------------------------------ A3C / DeviceNet arguments, no device
def test_a3c_validates_the_option_arguments():
    from asyncrl_amd import A3C
    for kw in (dict(ppo_norm_adv=True), dict(ppo_vclip=0.2)):
        with pytest.raises(ValueError, match="ppo_epochs"):
            A3C(FakeModel(), FakeOpt(), 5, GAMMA, **kw)                  # ppo_epochs == 1
    for bad in (0.0, -0.2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ppo_vclip"):
            A3C(FakeModel(), FakeOpt(), 5, GAMMA, ppo_epochs=2, ppo_vclip=bad)
    m = FakeModel()
    agent = A3C(m, FakeOpt(), 5, GAMMA, ppo_epochs=3, ppo_norm_adv=True, ppo_vclip=0.2)
    assert ("set_ppo_options", (True, 0.2)) in m.net.calls
    assert agent.ppo_norm_adv is True and agent.ppo_vclip == 0.2
    m = FakeModel()
    agent = A3C(m, FakeOpt(), 5, GAMMA, ppo_epochs=3)                   # the default never touches set_ppo_options
    assert not [c for c in m.net.calls if c[0] == "set_ppo_options"]
    with pytest.raises(ValueError, match="ppo_epoch_stats"):
        agent.ppo_epoch_stats()


def test_device_net_validates_vclip():
    from asyncrl_amd.net import DeviceNet
    net = DeviceNet.__new__(DeviceNet)                                   # no handle: the check comes first
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="vclip"):
            net.set_ppo_options(False, bad)
    assert net.ppo_aux is None and net.ppo_v_old is None and net.ppo_options == (False, None)


def test_epoch_stats_dict_derives_from_the_sums():
    from asyncrl_amd import ppo_epoch_stats_dict
    d = ppo_epoch_stats_dict([3, 2, 10, 4, 0.5, 1.5, 0.5, 2, 1.0, 10.1])
    assert d == {"window": 3, "epoch": 2, "samples": 10, "clip_fraction": 0.4, "approx_kl": 0.05, "ratio_max": 1.5,
                 "ratio_min": 0.5, "vclip_fraction": 0.2, "adv_mean": 0.1, "adv_std": pytest.approx(1.0)}
    assert np.isnan(ppo_epoch_stats_dict([0] * 10)["clip_fraction"])
    with pytest.raises(ValueError):
        ppo_epoch_stats_dict([0] * 9)
