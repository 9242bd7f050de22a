"""The whole-window cases at long t_max (33 and 64 steps) and their pools, shared by tests/test_gpu_long_windows.py
(the device against the oracle) and tests/test_long_windows_ref.py (the input conditions and, on the reference
alone, the size of the mistakes the cases exist for).  Nothing here touches a device.

A pool has T + 2 entries: neither a multiple nor a divisor of the ring's R = T + 4, and the second window wraps it.
The transition into observation k carries pool entry k % P, so window one's terminal flags are entries 1 .. T:
they are stage_ref.crafted_flags (env 0 never ends an episode, env 1 at steps 0 and T - 1, env 2 once past step
32, the others at about 3 % a step); entries 0 and T + 1 are 0, so window two sees the same flags two steps later
and env 0's chain is unbroken in both windows."""
import functools

import numpy as np

import oracle as O
import stage_ref as R
from sim import make_pools, make_state_pools

# (id, net, N, T, A, lambda or None for n-step, windows, observation kind)
FF_CASES = [("ff-ring-N3-T64-A4-nstep", O.ARCH_FF, 3, 64, 4, None, 2, "uniform"),
            ("ff-states-N5-T33-A6-gae", O.ARCH_FF, 5, 33, 6, 0.95, 1, "states"),
            ("nature-N3-T33-A6-nstep", O.ARCH_FF_NATURE, 3, 33, 6, None, 2, "palette"),
            ("nature-N2-T64-A4-gae", O.ARCH_FF_NATURE, 2, 64, 4, 0.95, 1, "palette")]
# (id, N, T, A, lambda, windows, lateral weight scale)
LSTM_CASES = [("lstm-N3-T64-A6-nstep", 3, 64, 6, None, 2, None),
              ("lstm-N5-T33-A6-gae", 5, 33, 6, 0.95, 1, None),
              ("lstm-N3-T33-A6-lateral-x4", 3, 33, 6, None, 1, 4.0)]
# whole windows at the 16-column head tiles' edges: (id, net, N, T, A)
EDGE_CASES = [("ff-A16", "ff", 3, 3, 16), ("ff-A31", "ff", 3, 2, 31), ("lstm-A17", "lstm", 4, 2, 17),
              ("nature-A15", "nature", 3, 2, 15)]


def pool_dones(T, N, seed=0):
    """(T + 2, N) uint8: entries 1 .. T are crafted_flags, entries 0 and T + 1 are 0."""
    dones = np.zeros((T + 2, N), np.uint8)
    dones[1:T + 1] = R.crafted_flags(np.random.default_rng([seed, T, N, 16]), T, N)
    return dones


def window_dones(dones, w, T):
    """The (T, N) terminal flags of window w, as sim.OracleEnvView.window_rd reads them."""
    P = dones.shape[0]
    return dones[[(w * T + t + 1) % P for t in range(T)]]


@functools.lru_cache(maxsize=None)
def pools(kind, N, T, seed=0):
    """(observations, rewards, dones) of T + 2 entries: sim.make_pools / make_state_pools with the crafted flags.
    Made once per shape, shared, read only."""
    rng = np.random.default_rng([seed, T, N, 17])
    make = make_state_pools if kind == "states" else lambda r, P, n, p_done: make_pools(r, P, n, kind, p_done=p_done)
    obs, rewards, _ = make(rng, T + 2, N, p_done=0.0)
    out = (obs, rewards, pool_dones(T, N, seed))
    for a in out:
        a.setflags(write=False)
    return out
