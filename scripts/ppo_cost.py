#!/usr/bin/env python
"""What PPO epochs (A3C(ppo_epochs=K)) cost a window.

C4 shape: A3C-FF NIPS head, 512 envs, t_max 5.  One agent per arm -- K = 1 (today's window, one C
call), 2 and 4 -- each with its window captured as a graph; the graphs are replayed alternately:
ROUNDS rounds of WINDOWS replays per arm, the device synchronised around each round.  Reports each
arm's median window time over the rounds.  Also the plain loss-gradient launches alone on the same
shape, through the granular entries (arl_returns_lossgrad against arl_ppo_lossgrad, 512 x 5 samples,
timed with events over REPS launches, interleaved the same way).  One JSON line (and --out FILE).

    python scripts/ppo_cost.py [--windows 200] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "async-rl_amd"))

import asyncrl_amd as pkg  # noqa: E402
from asyncrl_amd._lib import lib  # noqa: E402

ARMS = (1, 2, 4)
N, T, A, P = 512, 5, 4, 8


def pools(dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    pairs = torch.randint(0, 256, (P, N, 2, 210, 160, 3), dtype=torch.uint8, device=dev, generator=g)
    rng = np.random.default_rng(2)
    rewards = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), (P, N), p=[0.025, 0.95, 0.025])
    dones = (rng.random((P, N)) < 1 / 500).astype(np.uint8)
    return pairs, torch.from_numpy(rewards).to(dev), torch.from_numpy(dones).to(dev)


def windows_cost(windows, rounds, dev):
    pl = pools(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graphs, agents = {}, {}
    for K in ARMS:
        model = pkg.A3CFF(A, n_envs=N, t_max=T, seed=1234, init_seed=0, device=dev, frames="pairs")
        opt = pkg.Adam(alpha=1e-4).setup(model)
        opt.add_hook(pkg.GradientClipping(40))
        agents[K] = agent = pkg.A3C(model, opt, T, 0.99, beta=1e-2, collectives=False, gae_lambda=0.95, ppo_epochs=K)
        with torch.cuda.stream(stream):
            agent.run_window(*pl, P, first=True, stream=stream)
            stream.synchronize()
            graphs[K] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[K], stream=stream):
                agent.run_window(*pl, P, stream=stream)
            for _ in range(20):
                graphs[K].replay()
    times = {K: [] for K in ARMS}
    for _ in range(rounds):
        for K in ARMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for _ in range(windows):
                    graphs[K].replay()
            torch.cuda.synchronize()
            times[K].append(1e3 * (time.perf_counter() - t0) / windows)
    out = {f"k{K}_ms": [round(x, 5) for x in times[K]] for K in ARMS}
    out.update({f"median_k{K}_ms": round(float(np.median(times[K])), 5) for K in ARMS})
    out["params_finite"] = all(bool(torch.isfinite(a.net.params).all()) for a in agents.values())
    return out


def launch_cost(reps, rounds, dev):
    """The two plain loss-gradient kernels on one window's worth of arrays (values do not matter to the time)."""
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    f = lambda *s: torch.rand(*s, device=dev, generator=g)                       # noqa: E731
    rewards, v, probs = f(T, N), f(T + 1, N), torch.softmax(f(T + 1, N, A), -1)
    logp, dones = torch.log(probs), torch.zeros(T, N, dtype=torch.uint8, device=dev)
    act = torch.zeros(T + 1, N, dtype=torch.int32, device=dev)
    lpo, adv, ret = logp[:T, :, 0].contiguous(), f(T, N) - 0.5, f(T, N)
    dl, dv, loss, ratio = f(T, N, A), f(T, N), f(N, 2), f(T, N)
    p = lambda x: ctypes.c_void_p(x.data_ptr())                                   # noqa: E731

    def a3c():
        return lib.arl_returns_lossgrad(p(rewards), p(dones), p(v), p(probs), p(logp), p(act), T, N, A, 0.99, 0.01, 1.0,
                                        0.5, 0, 1, p(dl), p(dv), p(loss), None)

    def ppo():
        return lib.arl_ppo_lossgrad(p(dones), p(v), p(probs), p(logp), p(act), p(lpo), p(adv), p(ret), T, N, A, 0.2, 0.01,
                                    1.0, 0.5, 0, p(dl), p(dv), p(loss), p(ratio), None)

    times = {"returns": [], "ppo": []}
    for fn in (a3c, ppo):
        assert fn() == 0
    for _ in range(rounds):
        for name, fn in (("returns", a3c), ("ppo", ppo)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / reps)
    return {"returns_lossgrad_us": round(float(np.median(times["returns"])), 3),
            "ppo_lossgrad_us": round(float(np.median(times["ppo"])), 3), "launch_reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"n_envs": N, "t_max": T, "windows_per_round": a.windows, "rounds": a.rounds}
    out.update(windows_cost(a.windows, a.rounds, dev))
    out.update(launch_cost(500, a.rounds, dev))
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
