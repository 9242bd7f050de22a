#!/usr/bin/env python
"""What PPO epochs (A3C(ppo_epochs=K)) cost a window of the LSTM model.

C3 shape: A3C-LSTM NIPS head, 1,024 envs, t_max 5, Adam, GAE lambda 0.95.  One agent per arm -- K = 1
(today's window), 2 and 4 -- each with its window captured as a graph; the graphs are replayed
alternately: ROUNDS rounds of WINDOWS replays per arm, the device synchronised around each round.
Reports each arm's median window time over the rounds and the cost of an epoch after the first,
(K4 - K2) / 2.  An epoch after the first is t_max forward steps over all envs on one stream (conv,
FC, LSTM gates, policy), the PPO loss gradient, BPTT and the rest of the learner, and one update; the
carry (ppo_carry_kernel: one save and one restore a window, whatever K >= 2) is in every K >= 2 arm.
--arms picks the arms (e.g. --arms 2 under a kernel trace).  One JSON line (and --out FILE).

    python scripts/ppo_lstm_cost.py [--windows 200] [--rounds 5] [--arms 1,2,4] [--envs 1024] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "async-rl_amd"))

import asyncrl_amd as pkg  # noqa: E402

T, A, P = 5, 4, 8


def pools(n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    pairs = torch.randint(0, 256, (P, n, 2, 210, 160, 3), dtype=torch.uint8, device=dev, generator=g)
    rng = np.random.default_rng(2)
    rewards = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), (P, n), p=[0.025, 0.95, 0.025])
    dones = (rng.random((P, n)) < 1 / 500).astype(np.uint8)
    return pairs, torch.from_numpy(rewards).to(dev), torch.from_numpy(dones).to(dev)


def windows_cost(arms, n, windows, rounds, dev):
    pl = pools(n, dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graphs, agents = {}, {}
    for K in arms:
        model = pkg.A3CLSTM(A, n_envs=n, t_max=T, seed=1234, init_seed=0, device=dev, frames="pairs")
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
    times = {K: [] for K in arms}
    for _ in range(rounds):
        for K in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for _ in range(windows):
                    graphs[K].replay()
            torch.cuda.synchronize()
            times[K].append(1e3 * (time.perf_counter() - t0) / windows)
    out = {f"k{K}_ms": [round(x, 5) for x in times[K]] for K in arms}
    med = {K: float(np.median(times[K])) for K in arms}
    out.update({f"median_k{K}_ms": round(med[K], 5) for K in arms})
    if 2 in med and 4 in med:
        out["epoch_after_first_ms"] = round((med[4] - med[2]) / 2, 5)
        if 1 in med:   # what K = 2 costs beyond K = 1 and one more epoch: the carry, the snapshot, the unfused window
            out["first_epoch_overhead_ms"] = round(med[2] - med[1] - (med[4] - med[2]) / 2, 5)
    out["params_finite"] = all(bool(torch.isfinite(a.net.params).all()) for a in agents.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arms", default="1,2,4")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arms = tuple(int(k) for k in a.arms.split(","))
    dev = torch.device("cuda:0")
    out = {"arch": "lstm", "n_envs": a.envs, "t_max": T, "windows_per_round": a.windows, "rounds": a.rounds}
    out.update(windows_cost(arms, a.envs, a.windows, a.rounds, dev))
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
