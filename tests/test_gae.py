"""CPU: the GAE(lambda) restatement of gae_replay.py (what the GPU tests replay) pinned by its two
closed forms and by autograd, and the host side of arl_net_set_gae / arl_returns_lossgrad_gae.
GAE has no reference counterpart, so there is no reference fixture to compare with."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import oracle as O
from conftest import ROOT, close_normscaled
from gae_replay import gae_adv, patched, returns_and_lossgrad_gae, window_case

HEADER = os.path.join(ROOT, "include", "asyncrl_hip.h")
GAMMA = 0.99
CASES = [(1, 3, 4), (5, 7, 4), (9, 6, 6)]          # (T, n, A): terminals at t = 0, T - 1, consecutive, none (envs 0..3)


def oracle_call(c, T, **kw):
    return O.returns_and_lossgrad(c["rewards"], c["dones"], c["v"][:T], c["v"][T], c["probs"][:T], c["logp"][:T],
                                  c["actions"][:T], gamma=GAMMA, **kw)


@pytest.mark.parametrize("T,n,A", CASES)
@pytest.mark.parametrize("clip_reward", [True, False])
def test_lambda_one_is_the_n_step_advantage(T, n, A, clip_reward):
    """sum_k gamma^(k - t) delta_k telescopes to R_t - v_t.  The oracle rounds R_t to f32 (half an
    f32 ulp of R), then the f32 difference (half an ulp of the advantage); the scan rounds its f64
    sum to f32 once (half an ulp of the advantage).  The two f64 sums themselves differ by at most a
    few f64 roundings of their partial sums, each below T (max|r| + max|v|): 4 T of them at 2^-52."""
    c = window_case(T * 100 + n, T, n, A)
    Rs, adv1, _, _, _, _ = oracle_call(c, T, clip_reward=clip_reward)
    adv = gae_adv(c["rewards"], c["dones"], c["v"][:T], c["v"][T], GAMMA, 1.0, clip_reward)
    mag = float(np.abs(c["rewards"]).max() + np.abs(c["v"]).max()) * T
    bound = (0.5 * np.spacing(np.abs(Rs)).astype(np.float64)
             + np.spacing(np.maximum(np.abs(adv), np.abs(adv1))).astype(np.float64) + 4 * T * mag * 2.0 ** -52)
    err = np.abs(adv.astype(np.float64) - adv1.astype(np.float64))
    assert (err <= bound).all(), float((err / bound).max())
    assert np.abs(adv).max() > 0


@pytest.mark.parametrize("T,n,A", CASES)
def test_lambda_zero_is_the_one_step_td_error(T, n, A):
    c = window_case(T * 100 + n + 1, T, n, A)
    adv = gae_adv(c["rewards"], c["dones"], c["v"][:T], c["v"][T], GAMMA, 0.0, True)
    r = np.clip(c["rewards"].astype(np.float64), -1, 1)
    vn = np.where(c["dones"] & 1, 0.0, c["v"][1:].astype(np.float64))
    want = ((r + GAMMA * vn) - c["v"][:T].astype(np.float64)).astype(np.float32)
    assert (adv == want).all()


def test_terminal_cuts_the_scan():
    """Whatever follows a terminal, a truncated window's tail included, does not reach the steps before it."""
    T, n, A = 5, 7, 4
    c = window_case(3, T, n, A, truncate=True)
    adv = gae_adv(c["rewards"], c["dones"], c["v"][:T], c["v"][T], GAMMA, 0.95)
    v2 = c["v"].copy()
    v2[T - 2:, 4] = 1e6                                 # env 4: terminal at T - 3, past the end from T - 2
    r2 = c["rewards"].copy()
    r2[T - 2:, 4] = -7.0
    adv2 = gae_adv(r2, c["dones"], v2[:T], v2[T], GAMMA, 0.95)
    assert (adv[:T - 2, 4].view(np.int32) == adv2[:T - 2, 4].view(np.int32)).all()


@pytest.mark.parametrize("T,n,A", CASES)
@pytest.mark.parametrize("lam", [0.0, 0.5, 0.95])
def test_gradient_is_the_gradient_of_the_loss(T, n, A, lam):
    """Torch float64 autograd of sum -logpi(a) adv.detach() - beta H + vcoef (v - R.detach())^2 / 2 with respect
    to the logits and v against the restatement's dlogits / dv, 1e-5 norm-scaled (the project's f32 parity bound;
    no CPU check of returns_and_lossgrad alone against autograd exists to take another from)."""
    beta, vcoef = 0.05, 0.5
    c = window_case(T * 10 + n, T, n, A)
    rng = np.random.default_rng(T)
    logits = rng.standard_normal((T, n, A)).astype(np.float32)
    probs = O.softmax(logits.reshape(-1, A)).reshape(T, n, A)
    logp = O.log_softmax(logits.reshape(-1, A)).reshape(T, n, A)
    R, adv, dlogits, dv, pi_loss, v_loss = returns_and_lossgrad_gae(
        c["rewards"], c["dones"], c["v"][:T], c["v"][T], probs, logp, c["actions"][:T], gamma=GAMMA, beta=beta,
        v_loss_coef=vcoef, lam=lam)
    z = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    v = torch.tensor(c["v"][:T], dtype=torch.float64, requires_grad=True)
    lp = torch.log_softmax(z, dim=2)
    H = -(lp.exp() * lp).sum(2)
    la = lp.gather(2, torch.tensor(c["actions"][:T, :, None], dtype=torch.int64))[..., 0]
    pil = (-(la * torch.tensor(adv, dtype=torch.float64)) - beta * H).sum()
    vl = (vcoef * (v - torch.tensor(R, dtype=torch.float64)) ** 2 / 2).sum()
    (pil + vl).backward()
    for name, got, want in (("dlogits", dlogits, z.grad.numpy()), ("dv", dv, v.grad.numpy())):
        ok, err = close_normscaled(got, want, 1e-5)
        assert ok, (name, err)
    assert abs(pi_loss - pil.item()) <= 1e-5 * max(abs(pil.item()), 1.0)
    assert abs(v_loss - vl.item()) <= 1e-5 * max(abs(vl.item()), 1.0)
    # only the policy term changed
    R1, _, _, dv1, _, v_loss1 = O.returns_and_lossgrad(c["rewards"], c["dones"], c["v"][:T], c["v"][T], probs, logp,
                                                       c["actions"][:T], gamma=GAMMA, beta=beta, v_loss_coef=vcoef)
    assert (R1.view(np.int32) == R.view(np.int32)).all() and (dv1.view(np.int32) == dv.view(np.int32)).all()
    assert v_loss1 == v_loss


def test_patched_oracle_window_uses_the_wrapper():
    c = window_case(2, 5, 7, 4)
    with patched(0.5):
        _, adv, dl, _, _, _ = oracle_call(c, 5)
    _, adv1, dl1, _, _, _ = oracle_call(c, 5)
    assert (adv == gae_adv(c["rewards"], c["dones"], c["v"][:5], c["v"][5], GAMMA, 0.5)).all()
    assert not (adv == adv1).all() and not (dl == dl1).all()


# ------------------------------------------------------------------ host side
def test_set_gae_validates_on_an_unbound_handle():
    from asyncrl_amd._lib import lib
    h = ctypes.c_void_p()
    assert lib.arl_net_create(ctypes.byref(h), 0, 4, 16, 5, 0, 0) == 0
    try:
        for lam in (0.0, 0.95, 1.0):
            assert lib.arl_net_set_gae(h, lam) == 0, lam
        for lam in (-0.1, 1.5, float("nan"), float("inf"), float("-inf")):
            assert lib.arl_net_set_gae(h, lam) == 1, lam            # ARL_EINVAL
            assert b"lambda" in lib.arl_last_error()
        assert lib.arl_net_set_gae(None, 0.5) == 1
    finally:
        lib.arl_net_destroy(h)
    assert lib.arl_abi_version() == 4


def test_granular_entry_validates_lambda_before_any_launch():
    from asyncrl_amd._lib import lib
    args = lambda lam: (None, None, None, None, None, None, 5, 0, 4, 0.99, lam, 0.01, 1.0, 0.5, 0, 1, None, None,  # noqa: E731
                        None, None)
    for lam in (-0.1, 1.5, float("nan"), float("inf")):
        assert lib.arl_returns_lossgrad_gae(*args(lam)) == 1, lam
    assert lib.arl_returns_lossgrad_gae(*args(0.95)) == 0           # n = 0: nothing to launch


def test_header_library_and_table_agree():
    from asyncrl_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s, nargs in (("arl_net_set_gae", 2), ("arl_returns_lossgrad_gae", 20)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, code)
        assert m, s
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[s][1]), s
        assert hasattr(_lib.lib, s), s
    assert "double lambda" in re.search(r"arl_returns_lossgrad_gae\s*\(([^)]*)\)", code).group(1)


def test_a3c_rejects_a_lambda_outside_the_unit_interval():
    from asyncrl_amd import A3C
    model = types.SimpleNamespace(net=types.SimpleNamespace(t_max=5))
    for lam in (2, -0.5, float("nan")):
        with pytest.raises(ValueError, match="gae_lambda"):
            A3C(model, None, 5, 0.99, gae_lambda=lam)
