"""Test-side restatement of the device-side episode statistics (include/asyncrl_hip.h,
"episode statistics"): a NumPy float64 replay of the per-env bookkeeping in env-step order,
the fixed-order reduce of arl_episode_stats, and the inputs of the main GPU case.  Nothing
here imports the package under test."""
import numpy as np

LOG = 8                      # ARL_EPISODE_LOG
REWARD_VALUES = np.array([-1.5, 0.1, 0.3, 2.0, 7.0], np.float32)   # sums not representable, values outside [-1, 1]
F64 = ("ep_run_ret", "ep_total", "ep_sum", "ep_sumsq", "ep_min", "ep_max", "ep_log_ret")
I64 = ("ep_run_len", "ep_steps", "ep_count", "ep_len_sum", "ep_log_count", "ep_log_len", "ep_log_step")
BUFFERS = ("ep_run_ret", "ep_run_len", "ep_total", "ep_steps", "ep_count", "ep_sum", "ep_sumsq", "ep_min", "ep_max",
           "ep_len_sum", "ep_log_count", "ep_log_ret", "ep_log_len", "ep_log_step")
CLEARED = ("ep_count", "ep_sum", "ep_sumsq", "ep_min", "ep_max", "ep_len_sum", "ep_steps", "ep_total")


class Replay:
    """State of n envs; step() ingests what one observation at window slot t >= 1 carries."""

    def __init__(self, n):
        self.n = n
        self.b = {k: np.zeros((LOG, n) if "_log_" in k and k != "ep_log_count" else n,
                              np.float64 if k in F64 else np.int64) for k in BUFFERS}
        self.b["ep_min"][:] = np.inf
        self.b["ep_max"][:] = -np.inf

    def step(self, r, d, k, envs=None):
        """r (n,) float32, d (n,) uint8 of global observation index k (envs: a slice)."""
        b = self.b
        sl = slice(None) if envs is None else envs
        idx = np.arange(self.n)[sl]
        r64 = np.asarray(r, np.float32)[sl].astype(np.float64)
        term = np.asarray(d)[sl] != 0
        G = b["ep_run_ret"][sl] + r64
        L = b["ep_run_len"][sl] + 1
        b["ep_total"][sl] += r64
        b["ep_steps"][sl] += 1
        e = idx[term]
        Gt, Lt = G[term], L[term]
        c = b["ep_count"][e].copy()
        b["ep_count"][e] = c + 1
        b["ep_sum"][e] += Gt
        b["ep_sumsq"][e] += Gt * Gt
        b["ep_len_sum"][e] += Lt
        b["ep_min"][e] = np.where(Gt < b["ep_min"][e], Gt, b["ep_min"][e])
        b["ep_max"][e] = np.where(Gt > b["ep_max"][e], Gt, b["ep_max"][e])
        b["ep_log_ret"][c % LOG, e] = Gt
        b["ep_log_len"][c % LOG, e] = Lt
        b["ep_log_step"][c % LOG, e] = k
        b["ep_log_count"][e] += 1
        b["ep_run_ret"][sl] = np.where(term, 0.0, G)
        b["ep_run_len"][sl] = np.where(term, 0, L)

    def force_reset(self):
        """What force_reset adds after the step: the running episode is abandoned."""
        self.b["ep_run_ret"][:] = 0.0
        self.b["ep_run_len"][:] = 0

    def run(self, rewards, dones, k0, k1):
        """Observations k0 .. k1 - 1 of pools (P, n): entry k % P."""
        P = rewards.shape[0]
        for k in range(k0, k1):
            self.step(rewards[k % P], dones[k % P], k)
        return self

    def reduce(self, clear=False):
        """arl_episode_stats: thread j of 256 sums envs j, j + 256, ... ascending; thread 0 then
        combines partials 0..255 in order.  float64 scalar adds, integers exact."""
        b = self.b
        parts = []
        for j in range(256):
            s = ss = tot = np.float64(0.0)
            mn, mx = np.float64(np.inf), np.float64(-np.inf)
            cnt = ln = st = 0
            for e in range(j, self.n, 256):
                cnt += int(b["ep_count"][e])
                s = s + b["ep_sum"][e]
                ss = ss + b["ep_sumsq"][e]
                mn = b["ep_min"][e] if b["ep_min"][e] < mn else mn
                mx = b["ep_max"][e] if b["ep_max"][e] > mx else mx
                ln += int(b["ep_len_sum"][e])
                st += int(b["ep_steps"][e])
                tot = tot + b["ep_total"][e]
            parts.append((cnt, s, ss, mn, mx, ln, st, tot))
        cnt, s, ss, mn, mx, ln, st, tot = parts[0]
        for q in parts[1:]:
            cnt += q[0]
            s = s + q[1]
            ss = ss + q[2]
            mn = q[3] if q[3] < mn else mn
            mx = q[4] if q[4] > mx else mx
            ln += q[5]
            st += q[6]
            tot = tot + q[7]
        if clear:
            for k in CLEARED:
                b[k][:] = np.inf if k == "ep_min" else -np.inf if k == "ep_max" else 0
        return np.array([cnt, s, ss, mn, mx, ln, st, tot], np.float64)


def serial_reference(rewards, dones):
    """The reference's train_loop bookkeeping, literally, for one env's stream of (r, terminal):
    episode_r += r; at a terminal record it and start again (a3c_ale.py:114-124), total_r the
    sum of all.  Returns (episode returns, episode lengths, indices, running episode_r, total_r)."""
    episode_r, total_r, length = 0.0, 0.0, 0
    rets, lens, at = [], [], []
    for i, (r, terminal) in enumerate(zip(rewards, dones)):
        episode_r += float(r)
        total_r += float(r)
        length += 1
        if terminal:
            rets.append(episode_r)
            lens.append(length)
            at.append(i)
            episode_r, length = 0.0, 0
    return rets, lens, at, episode_r, total_r


def case_pools(seed, P, n, p_done=0.3, special=True):
    """rewards (P, n) f32 from REWARD_VALUES, dones (P, n) uint8; with special: env 0 never
    terminates, env 1 terminates every step, env 2 at every pool entry but one."""
    rng = np.random.default_rng(seed)
    rewards = rng.choice(REWARD_VALUES, (P, n)).astype(np.float32)
    dones = (rng.random((P, n)) < p_done).astype(np.uint8)
    if special:
        dones[:, 0] = 0
        dones[:, 1] = 1
        dones[:, 2] = 1
        dones[0, 2] = 0
    return rewards, dones


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())
