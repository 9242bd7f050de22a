"""Test-side restatement of the PPO epochs' options (include/asyncrl_hip.h, arl_net_set_ppo_options):
advantage normalisation, the clipped value loss and the per-epoch record in NumPy, every operation in
the header's order and precision, so all three are bit-identical to the kernels'.

The float64 sums follow the one-workgroup kernels' ordering rule (`ordered_sum`): thread j of 256 owns
envs j, j + 256, ... ascending and per env the steps t ascending; its partial starts at +0.0, a sample
that is not live adds +0.0; partial 0, then partials 1 .. 255 are added in order.  NumPy's float64
scalar and array operations are unfused round-to-nearest ones, as the kernels'."""
import numpy as np

import oracle as O
import ppo_ref

F32, F64 = np.float32, np.float64
PPO_LOG, PPO_STAT_FIELDS, PPO_AUX_HEAD = 16, 10, 8
FIELDS = ("window", "epoch", "samples", "clipped", "kl_sum", "ratio_max", "ratio_min", "vclipped", "adv_sum",
          "adv_sumsq")


def ordered_sum(x, live):
    """x (T, n) float64, live (T, n) bool -> the kernels' total, a float64 scalar."""
    x = np.where(live, np.asarray(x, F64), 0.0)
    T, n = x.shape
    part = np.zeros(256, F64)
    for base in range(0, n, 256):                 # every thread's next env
        w = min(256, n - base)
        for t in range(T):
            part[:w] = part[:w] + x[t, base:base + w]
    total = part[0]
    for q in range(1, 256):
        total = total + part[q]
    return F64(total)


def normalize_adv(dones, adv):
    """-> adv' (T, n) f32 and the moments (n_live, mean, std) as float64."""
    adv = np.asarray(adv, F32)
    live = (np.asarray(dones).astype(np.int64) & 2) == 0
    n_live = int(live.sum())
    if n_live == 0:
        return adv.copy(), (F64(0), F64(0), F64(0))
    a = adv.astype(F64)
    nl = F64(n_live)
    mean = ordered_sum(a, live) / nl
    dd = a - mean
    std = np.sqrt(ordered_sum(dd * dd, live) / nl)
    out = (dd / (std + F64(1e-8))).astype(F32)
    return np.where(live, out, adv).astype(F32), (nl, mean, std)


def vclip(vi, vold, Rf, ev):
    """The value-clip decision of one epoch (the kernels' shared device function), elementwise f32:
    -> taken (bool), lsq = the square the value loss takes, inside (bool), lu, lc."""
    vi, vold, Rf, ev = np.asarray(vi, F32), np.asarray(vold, F32), np.asarray(Rf, F32), F32(ev)
    dvv = (vi - Rf).astype(F32)
    do = (vi - vold).astype(F32)
    inside = np.abs(do) <= ev
    vc = (vold + np.where(do > 0, ev, -ev).astype(F32)).astype(F32)
    dvc = (vc - Rf).astype(F32)
    lu = (dvv * dvv).astype(F32)
    lc = (dvc * dvc).astype(F32)
    taken = ~inside & (lc > lu)
    return dict(taken=taken, lsq=np.where(taken, lc, lu).astype(F32), inside=inside, lu=lu, lc=lc, do=do)


def lossgrad_vclip(dones, v, probs, logp, actions, logp_old, adv, ret, v_old, clip_eps=0.2, vclip_eps=0.1, beta=0.01,
                   pi_loss_coef=1.0, v_loss_coef=0.5, keep_loss_scale_same=False, rho=None):
    """ppo_ref.lossgrad with the clipped value loss: only dv and the value loss differ."""
    o = ppo_ref.lossgrad(dones, v, probs, logp, actions, logp_old, adv, ret, clip_eps, beta, pi_loss_coef, v_loss_coef,
                         keep_loss_scale_same, rho)
    dn = np.asarray(dones).astype(np.int64)
    T, N = dn.shape
    live = o["live"]
    scale = O.segment_scale(dn & 1, T, live) if keep_loss_scale_same else np.ones((T, N))
    vf = (F32(v_loss_coef) * scale.astype(F32)).astype(F32)
    vi, Rf = np.asarray(v, F32)[:T], np.asarray(ret, F32)
    c = vclip(vi, v_old, Rf, F32(vclip_eps))
    dvv = (vi - Rf).astype(F32)
    z = F32(0)
    dv = np.where(c["taken"], z, (vf * dvv).astype(F32)).astype(F32)
    lv = (vf * (c["lsq"] * F32(0.5)).astype(F32)).astype(F32)
    dv, lv = (np.where(live, x, z).astype(F32) for x in (dv, lv))
    loss = o["loss"].copy()
    loss[:, 1] = 0
    for t in reversed(range(T)):
        loss[:, 1] = (loss[:, 1] + lv[t]).astype(F32)
    out = dict(o)
    out.update(dv=dv, lv=lv, loss=loss, taken=c["taken"] & live, inside=c["inside"] & live,
               outside_kept=~c["inside"] & ~c["taken"] & live, vc=c)
    return out


def epoch_record(dones, v, logp, actions, logp_old, adv, ret, ratio, v_old=None, clip_eps=0.2, vclip_eps=0.0,
                 window=0.0, epoch=1.0):
    """The ten fields of one epoch's record, float64."""
    dn = np.asarray(dones).astype(np.int64)
    T, N = dn.shape
    live = (dn & 2) == 0
    lp = np.asarray(logp, F32)[:T]
    ac = np.asarray(actions)[:T].astype(np.int64)
    lpa = np.take_along_axis(lp, ac[..., None], 2)[..., 0]
    d = (lpa - np.asarray(logp_old, F32)).astype(F32)
    rho, adv = np.asarray(ratio, F32), np.asarray(adv, F32)
    lo, hi = ppo_ref.clip_range(clip_eps)
    cut = ~np.where(adv >= 0, rho <= hi, rho >= lo)
    taken = np.zeros((T, N), bool)
    if v_old is not None:
        taken = vclip(np.asarray(v, F32)[:T], v_old, ret, F32(vclip_eps))["taken"]
    ad = adv.astype(F64)
    one = np.ones((T, N), F64)
    any_live = bool(live.any())
    rec = [F64(window), F64(epoch), ordered_sum(one, live), ordered_sum(one, live & cut),
           ordered_sum(-d.astype(F64), live),
           F64(rho[live].max()) if any_live else F64(0), F64(rho[live].min()) if any_live else F64(0),
           ordered_sum(one, live & taken), ordered_sum(ad, live), ordered_sum(ad * ad, live)]
    return np.array(rec, F64)
