"""Test-side restatement of the GAE(lambda) advantage (include/asyncrl_hip.h, arl_net_set_gae):
NumPy float64, elementwise operations in the header's order, each one IEEE round-to-nearest
operation as on the device, so `gae_adv` is bit-identical to the kernels' adv_t.

GAE has no reference counterpart.  Only the policy term changes: R, dv and v_loss come from
oracle.returns_and_lossgrad unchanged, and dlogits / pi_loss are recomputed with that
function's own formula and the new advantage.  `patched` swaps the wrapper into the oracle
module for the whole-window functions that call it (ff_window_grads, lstm_window); nothing
under oracle/ is edited."""
import contextlib

import numpy as np

import oracle as O

F32 = np.float32
_ORIGINAL = O.returns_and_lossgrad


def gae_adv(rewards, dones, values, vboot, gamma, lam, clip_reward=True):
    """rewards (T, N), dones (T, N) with bit 0 = terminal, values (T, N) f32, vboot (N,) f32 ->
    adv (T, N) f32."""
    rewards, values, vboot = np.asarray(rewards, F32), np.asarray(values, F32), np.asarray(vboot, F32)
    T, N = rewards.shape
    r = rewards.astype(np.float64)
    if clip_reward:
        r = np.clip(r, -1.0, 1.0)
    gamma = float(gamma)
    gl = gamma * float(lam)                            # one f64 product, on the host
    v = np.concatenate([values, vboot[None]]).astype(np.float64)
    term = (np.asarray(dones).astype(np.int64) & 1) != 0
    G = np.zeros(N, np.float64)
    adv = np.zeros((T, N), F32)
    for k in reversed(range(T)):
        vn = np.where(term[k], 0.0, v[k + 1])
        d = (r[k] + gamma * vn) - v[k]
        G = np.where(term[k], 0.0, G)
        G = d + gl * G
        adv[k] = G.astype(F32)
    return adv


def returns_and_lossgrad_gae(rewards, dones, values, vboot, probs, logp, actions, gamma=0.99, beta=0.01,
                             v_loss_coef=0.5, clip_reward=True, pi_loss_coef=1.0, keep_loss_scale_same=False,
                             t_max=None, valid=None, lam=0.95, per_env=False):
    """oracle.returns_and_lossgrad's arguments and results with the GAE advantage in the policy
    term.  per_env: pi_loss / v_loss as (N,) float64 sums per env instead of the window's."""
    Rs, _, _, dv, _, v_loss = _ORIGINAL(rewards, dones, values, vboot, probs, logp, actions, gamma, beta, v_loss_coef,
                                        clip_reward, pi_loss_coef, keep_loss_scale_same, t_max, valid)
    T, N = rewards.shape
    t_max = T if t_max is None else t_max
    valid = np.ones((T, N), bool) if valid is None else np.asarray(valid, bool)
    adv = gae_adv(rewards, dones, values, vboot, gamma, lam, clip_reward)
    H = O.entropy(probs, logp)
    onehot = np.zeros_like(probs)
    np.put_along_axis(onehot, actions[..., None].astype(np.int64), 1.0, axis=2)
    scale = O.segment_scale(dones, t_max, valid) if keep_loss_scale_same else np.ones((T, N))
    pf = (F32(pi_loss_coef) * scale.astype(F32)).astype(F32) * valid
    vf = (F32(v_loss_coef) * scale.astype(F32)).astype(F32) * valid
    dlogits = (pf[..., None] * (-adv[..., None] * (onehot - probs)
               + F32(beta) * probs * (logp + H[..., None]))).astype(F32)
    logp_a = np.take_along_axis(logp, actions[..., None].astype(np.int64), 2)[..., 0]
    pi_terms = -(pf * (logp_a * adv + F32(beta) * H))
    if per_env:
        v_terms = vf * (((values - Rs) ** 2) / 2)
        return Rs, adv, dlogits, dv, pi_terms.astype(np.float64).sum(0), v_terms.astype(np.float64).sum(0)
    return Rs, adv, dlogits, dv, float(pi_terms.sum()), v_loss


@contextlib.contextmanager
def patched(lam):
    """oracle.returns_and_lossgrad -> the GAE wrapper at this lambda, for the oracle's window functions."""
    def wrapper(*args, **kw):
        return returns_and_lossgrad_gae(*args, lam=lam, **kw)
    O.returns_and_lossgrad = wrapper
    try:
        yield
    finally:
        O.returns_and_lossgrad = _ORIGINAL


def replay_adv_sums(adv, dones, threads=256):
    """Fields 12, 13 of a window-statistics record over this advantage, in the record's order (window_replay.py):
    thread j walks envs j, j + threads, ... and t ascending; the threads' partials are then added in order."""
    T, n = adv.shape
    parts = []
    for j in range(min(threads, n)):
        s = q = 0.0
        for e in range(j, n, threads):
            for t in range(T):
                if int(dones[t, e]) & 2:
                    continue
                a = float(adv[t, e])
                s = s + a
                q = q + a * a
        parts.append((s, q))
    s, q = parts[0]
    for ps, pq in parts[1:]:
        s, q = s + ps, q + pq
    return s, q


def window_case(seed, T, n, A, truncate=False):
    """A seeded random window for the granular entry.  Terminals in every position class in fixed
    columns (mod n): env 0 at t = 0, env 1 at T - 1, env 2 at two consecutive steps, env 3 none;
    truncate: env 4 % n ended at t = T - 3 and is past the window's end from there (dones 2,
    rewards 0, as arl_truncate_window leaves them).  Rewards reach outside [-1, 1]."""
    rng = np.random.default_rng(seed)
    rewards = rng.choice(np.array([-2.5, -1.0, -0.3, 0.0, 0.0, 0.7, 1.0, 3.0], F32), (T, n)).astype(F32)
    dones = (rng.random((T, n)) < 0.15).astype(np.uint8)
    dones[:, :min(n, 4)] = 0
    dones[0, 0] = 1
    if n > 1:
        dones[T - 1, 1] = 1
    if n > 2:
        dones[min(1, T - 1), 2] = dones[min(2, T - 1), 2] = 1
    if truncate:
        assert T >= 4
        e = 4 % n
        dones[:, e] = 0
        dones[T - 3, e] = 1
        dones[T - 2:, e] = 2
        rewards[T - 2:, e] = 0.0
    v = rng.standard_normal((T + 1, n)).astype(F32)
    logits = rng.standard_normal((T + 1, n, A)).astype(F32)
    probs, logp = O.softmax(logits.reshape(-1, A)), O.log_softmax(logits.reshape(-1, A))
    actions = rng.integers(0, A, (T + 1, n)).astype(np.int32)
    return dict(rewards=rewards, dones=dones, v=v, probs=probs.reshape(T + 1, n, A).astype(F32),
                logp=logp.reshape(T + 1, n, A).astype(F32), actions=actions)
