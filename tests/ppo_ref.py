"""Test-side restatement of the clipped-surrogate (PPO) epochs (include/asyncrl_hip.h,
arl_net_set_ppo): the snapshot and the loss gradient of one epoch in NumPy, every operation in the
header's order and precision, so both are bit-identical to the kernels' -- except the ratio, whose
float64 exp comes from the C library here and from the device's there (1 f32 ulp at most); `rho=`
takes the device's instead.

PPO has no reference counterpart.  `patched` swaps a wrapper with oracle.returns_and_lossgrad's
signature into the oracle module for the whole-window functions that call it (ff_window_grads);
nothing under oracle/ is edited."""
import contextlib

import numpy as np

import oracle as O
from gae_replay import gae_adv

F32 = np.float32
_ORIGINAL = O.returns_and_lossgrad


def clip_range(clip_eps):
    """lo, hi as the host forms them: one float64 operation each, rounded to f32."""
    return F32(1.0 - float(clip_eps)), F32(1.0 + float(clip_eps))


def snapshot(rewards, dones, v, logp, actions, gamma, lam=1.0, clip_reward=True):
    """rewards (T, N); dones (T, N) with bit 0 = terminal, bit 1 = past the window's end; v (T + 1, N),
    logp (T + 1, N, A), actions (T + 1, N) with row T = the bootstrap slot.
    -> logp_old, adv, ret, each (T, N) f32, zero where a sample is not live."""
    rewards, v = np.asarray(rewards, F32), np.asarray(v, F32)
    dones = np.asarray(dones).astype(np.int64)
    T, N = rewards.shape
    term, live = (dones & 1) != 0, (dones & 2) == 0
    r = rewards.astype(np.float64)
    if clip_reward:
        r = np.clip(r, -1.0, 1.0)
    gamma = float(gamma)
    R = v[T].astype(np.float64)
    ret = np.zeros((T, N), F32)
    for t in reversed(range(T)):
        R = np.where(term[t], 0.0, R)
        R = R * gamma + r[t]
        ret[t] = R.astype(F32)
    if float(lam) == 1.0:
        adv = (ret - v[:T]).astype(F32)
    else:
        adv = gae_adv(rewards, term, v[:T], v[T], gamma, lam, clip_reward)
    lpo = np.take_along_axis(np.asarray(logp, F32)[:T], np.asarray(actions)[:T, :, None].astype(np.int64), 2)[..., 0]
    z = F32(0)
    return np.where(live, lpo, z).astype(F32), np.where(live, adv, z).astype(F32), np.where(live, ret, z).astype(F32)


def lossgrad(dones, v, probs, logp, actions, logp_old, adv, ret, clip_eps=0.2, beta=0.01, pi_loss_coef=1.0,
             v_loss_coef=0.5, keep_loss_scale_same=False, rho=None):
    """One epoch's loss gradient.  dones (T, N) (both bits); v, probs, logp, actions: the current
    policy's, rows 0 .. T - 1 are read; logp_old, adv, ret (T, N): the snapshot.  rho: the ratio to
    use instead of this function's own (float)exp((double)d).
    -> dict(dlogits (T, N, A), dv (T, N), loss (N, 2), ratio (T, N), active (T, N) bool, lpi, lv (T, N))."""
    dones = np.asarray(dones).astype(np.int64)
    T, N = dones.shape
    pr, lp = np.asarray(probs, F32)[:T], np.asarray(logp, F32)[:T]
    vi = np.asarray(v, F32)[:T]
    ac = np.asarray(actions)[:T].astype(np.int64)
    lpo, adv, Rf = np.asarray(logp_old, F32), np.asarray(adv, F32), np.asarray(ret, F32)
    A = pr.shape[2]
    live = (dones & 2) == 0
    scale = O.segment_scale(dones & 1, T, live) if keep_loss_scale_same else np.ones((T, N))
    pf = (F32(pi_loss_coef) * scale.astype(F32)).astype(F32)
    vf = (F32(v_loss_coef) * scale.astype(F32)).astype(F32)
    beta = F32(beta)
    lpa = np.take_along_axis(lp, ac[..., None], 2)[..., 0]
    d = (lpa - lpo).astype(F32)
    own = np.exp(d.astype(np.float64)).astype(F32)
    rho = own if rho is None else np.asarray(rho, F32)
    lo, hi = clip_range(clip_eps)
    pos = adv >= 0
    active = np.where(pos, rho <= hi, rho >= lo)
    w = np.where(active, (rho * adv).astype(F32), F32(0)).astype(F32)
    surr = np.where(active, w, (np.where(pos, hi, lo).astype(F32) * adv).astype(F32)).astype(F32)
    H = np.zeros((T, N), F32)
    for k in range(A):                                   # serial, k ascending
        H = (H + (pr[..., k] * lp[..., k]).astype(F32)).astype(F32)
    H = -H
    dl = np.zeros((T, N, A), F32)
    for k in range(A):
        oh = (ac == k).astype(F32)
        t1 = ((-w) * (oh - pr[..., k]).astype(F32)).astype(F32)
        t2 = ((beta * pr[..., k]).astype(F32) * (lp[..., k] + H).astype(F32)).astype(F32)
        dl[..., k] = (pf * (t1 + t2).astype(F32)).astype(F32)
    dvv = (vi - Rf).astype(F32)
    dv = (vf * dvv).astype(F32)
    lpi = (pf * (surr + (beta * H).astype(F32)).astype(F32)).astype(F32)
    lv = (vf * ((dvv * dvv).astype(F32) * F32(0.5)).astype(F32)).astype(F32)
    z = F32(0)
    dl = np.where(live[..., None], dl, z).astype(F32)
    dv, lpi, lv = (np.where(live, x, z).astype(F32) for x in (dv, lpi, lv))
    loss = np.zeros((N, 2), F32)
    for t in reversed(range(T)):                          # env_loss's order
        loss[:, 0] = (loss[:, 0] - lpi[t]).astype(F32)
        loss[:, 1] = (loss[:, 1] + lv[t]).astype(F32)
    return dict(dlogits=dl, dv=dv, loss=loss, ratio=np.where(live, rho, z).astype(F32), active=active & live,
                lpi=lpi, lv=lv, live=live, own_ratio=np.where(live, own, z).astype(F32))


@contextlib.contextmanager
def patched(logp_old, adv, ret, clip_eps, rho=None):
    """oracle.returns_and_lossgrad -> one PPO epoch on this snapshot, for the oracle's window
    functions: the forward is the oracle's own (the current parameters), rewards / gamma are not
    read (ret and adv are fixed).  Returns the original's tuple (R, adv, dlogits, dv, pi_loss, v_loss)."""
    def wrapper(rewards, dones, values, vboot, probs, logp, actions, gamma=0.99, beta=0.01, v_loss_coef=0.5,
                clip_reward=True, pi_loss_coef=1.0, keep_loss_scale_same=False, t_max=None, valid=None):
        dn = (np.asarray(dones) != 0).astype(np.int64)
        if valid is not None:
            dn = dn | np.where(np.asarray(valid, bool), 0, 2)
        o = lossgrad(dn, values, probs, logp, actions, logp_old, adv, ret, clip_eps, beta, pi_loss_coef, v_loss_coef,
                     keep_loss_scale_same, rho)
        return (np.asarray(ret, F32), np.asarray(adv, F32), o["dlogits"], o["dv"], float(o["loss"][:, 0].sum()),
                float(o["loss"][:, 1].sum()))
    O.returns_and_lossgrad = wrapper
    try:
        yield
    finally:
        O.returns_and_lossgrad = _ORIGINAL
