"""Test-side restatement of the device-side window statistics (include/asyncrl_hip.h, "window
statistics"): a NumPy float64 replay of fields 2..13 of one record from the workspace arrays
of one window, in the order the header fixes -- thread j of 256 walks envs j, j + 256, ...
ascending, each env t = 0 .. T - 1 ascending after one reverse scan for the returns; thread 0
then adds partials 1 .. 255 to its own in order.  Nothing here imports the package under test."""
import numpy as np

from episode_replay import REWARD_VALUES, case_pools, same_bits  # noqa: F401  (shared with the tests)

LOG = 64                     # ARL_WINDOW_LOG
FIELDS = 17                  # ARL_WINDOW_STAT_FIELDS
NAMES = ("window", "step", "samples", "terminals", "reward_sum", "pi_loss", "v_loss", "entropy_sum", "value_sum",
         "value_sumsq", "return_sum", "return_sumsq", "adv_sum", "adv_sumsq", "grad_sqnorm", "clip_scale", "lr")
SUMS = NAMES[2:14]           # what replay() returns, in order
THREADS = 256


def clip64(r, clip_reward):
    """The reward as the learner uses it: (double)r, clipped to [-1, 1] iff clip_reward."""
    x = float(np.float32(r))
    return min(max(x, -1.0), 1.0) if clip_reward else x


def env_returns(rewards, dones, vboot, gamma, clip_reward):
    """One env's (float)R_t, t = 0 .. T - 1: the f64 recurrence from v[T], R = 0 at bit-0
    terminals, R = R * gamma + clip(r) (Python floats: unfused IEEE f64 ops)."""
    T = len(rewards)
    R = float(np.float32(vboot))
    out = np.zeros(T, np.float32)
    for t in reversed(range(T)):
        if int(dones[t]) & 1:
            R = 0.0
        R = R * float(gamma) + clip64(rewards[t], clip_reward)
        out[t] = np.float32(R)
    return out


def replay(rewards, dones, v, entropy, loss, gamma=0.99, clip_reward=True):
    """rewards (T, n) f32, dones (T, n) uint8, v and entropy (T + 1, n) f32 (row T of v = the
    bootstrap value), loss (n, 2) f32 -> the 12 doubles of fields 2..13 (SUMS order)."""
    rewards, dones = np.asarray(rewards, np.float32), np.asarray(dones, np.uint8)
    v, entropy, loss = np.asarray(v, np.float32), np.asarray(entropy, np.float32), np.asarray(loss, np.float32)
    T, n = rewards.shape
    assert dones.shape == (T, n) and v.shape == (T + 1, n) and entropy.shape[1] == n and loss.shape == (n, 2)
    parts = []
    for j in range(min(THREADS, n)):
        a = [0.0] * 12
        for e in range(j, n, THREADS):
            Rf = env_returns(rewards[:, e], dones[:, e], v[T, e], gamma, clip_reward)
            a[3] = a[3] + float(loss[e, 0])
            a[4] = a[4] + float(loss[e, 1])
            for t in range(T):
                d = int(dones[t, e])
                if d & 2:
                    continue
                vd, rd, ad = float(v[t, e]), float(Rf[t]), float(np.float32(Rf[t] - v[t, e]))
                a[0] = a[0] + 1.0
                if d & 1:
                    a[1] = a[1] + 1.0
                a[2] = a[2] + clip64(rewards[t, e], clip_reward)
                a[5] = a[5] + float(entropy[t, e])
                a[6] = a[6] + vd
                a[7] = a[7] + vd * vd
                a[8] = a[8] + rd
                a[9] = a[9] + rd * rd
                a[10] = a[10] + ad
                a[11] = a[11] + ad * ad
        parts.append(a)
    out = list(parts[0])
    for q in parts[1:]:          # (threads n .. 255 hold zeros: x + 0.0 == x)
        for f in range(12):
            out[f] = out[f] + q[f]
    return np.array(out, np.float64)


def window_case(seed, T=5, n=7, A=4):
    """A seeded random window with the edge cases in fixed columns: env 0 terminal at t = 0,
    env 1 at T - 1, env 2 at two consecutive steps, env 3 truncated from t = 3 (its episode
    ended at t = 2: dones 2 and rewards 0 from there, as arl_truncate_window leaves them);
    rewards from REWARD_VALUES (values outside [-1, 1]).  Returns a dict of arrays."""
    rng = np.random.default_rng(seed)
    rewards = rng.choice(REWARD_VALUES, (T, n)).astype(np.float32)
    dones = (rng.random((T, n)) < 0.15).astype(np.uint8)
    dones[:, :4] = 0
    dones[0, 0] = 1
    dones[T - 1, 1] = 1
    dones[1, 2] = dones[2, 2] = 1
    dones[2, 3] = 1
    dones[3:, 3] = 2
    rewards[3:, 3] = 0.0
    v = rng.standard_normal((T + 1, n)).astype(np.float32)
    logits = rng.standard_normal((T, n, A)).astype(np.float32)
    actions = rng.integers(0, A, (T, n)).astype(np.int32)
    entropy = rng.random((T + 1, n)).astype(np.float32)
    loss = rng.standard_normal((n, 2)).astype(np.float32)
    return dict(rewards=rewards, dones=dones, v=v, logits=logits, actions=actions, entropy=entropy, loss=loss)
