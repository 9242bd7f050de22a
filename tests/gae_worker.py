"""Runs one FF window per case of CASES with A3C(gae_lambda=argv[2]) through A3C.run_window (one env
group) and saves what the learner's first kernel and the learner left to an .npz (argv[1]).
test_gpu_gae runs it in its own process (the window as one C call, the returns inside the bootstrap
policy launch) and in a child under ARL_WINDOW_C=0 ARL_FUSE_RETURNS=0 (step by step, the separate
returns launch; both are read once per process) and compares the files bitwise."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "async-rl_amd"), os.path.join(HERE, "..", "oracle"), HERE]
from sim import make_pools  # noqa: E402

CASES = [(33, 5, 4), (33, 9, 6), (5, 5, 18), (5, 33, 6)]   # (n, T, A); T = 33: a second pass over rows
KEYS = ("dlogits", "dv", "loss", "dfc", "v")


def main(out, lam):
    from asyncrl_amd import A3C, A3CFF, GradientClipping, RMSpropAsync
    dev = torch.device("cuda:0")
    res = {}
    for n, T, A in CASES:
        rng = np.random.default_rng(n * 100 + T)
        P = T + 1
        pairs, rewards, dones = make_pools(rng, P, n, "uniform", p_done=0.2)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        m = A3CFF(A, n_envs=n, t_max=T, seed=9, init_seed=10, frames="pairs", device=dev)
        o = RMSpropAsync(lr=7e-4, eps=0.1, alpha=0.99).setup(m)
        o.add_hook(GradientClipping(40))
        ag = A3C(m, o, T, 0.99, gae_lambda=lam)
        ag.run_window(t(pairs), t(rewards), t(dones), P, first=True, env_groups=1)
        torch.cuda.synchronize()
        net = ag.net
        pre = f"{n}_{T}_{A}_"
        for k in KEYS:
            res[pre + k] = net.buffer(k, torch.float32).cpu().numpy()
        res[pre + "grads"] = net.grads.detach().cpu().numpy()
        res[pre + "params"] = net.params.detach().cpu().numpy()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], float(sys.argv[2]))
