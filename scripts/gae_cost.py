#!/usr/bin/env python
"""What GAE(lambda) advantages (A3C(gae_lambda=) / DeviceNet.set_gae) cost a window when on.

For each shape -- C4: A3C-FF NIPS head, 512 envs; C3: A3C-LSTM, 1,024 envs; t_max 5 -- one model's
window is captured as a graph twice, at lambda = 1 (the n-step kernels) and at lambda = 0.95 (the GAE
form of the returns kernel), and the two graphs are replayed alternately: ROUNDS rounds of WINDOWS
replays per arm, the device synchronised around each round.  Reports each arm's median window time
over the rounds and the difference, one JSON line per shape (and --out FILE: the list as JSON).
Under `rocprofv3 --kernel-trace --stats` the same run gives the two forms' kernel times: they are
different instantiations, so the statistics list them apart.

    python scripts/gae_cost.py [--windows 200] [--rounds 5] [--shapes c4,c3] [--out FILE]
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

SHAPES = {"c4": ("ff", 512, 4), "c3": ("lstm", 1024, 6)}
ARMS = {"nstep": 1.0, "gae": 0.95}


def pools(n, P, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    pairs = torch.randint(0, 256, (P, n, 2, 210, 160, 3), dtype=torch.uint8, device=dev, generator=g)
    rng = np.random.default_rng(2)
    rewards = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), (P, n), p=[0.025, 0.95, 0.025])
    dones = (rng.random((P, n)) < 1 / 500).astype(np.uint8)
    return pairs, torch.from_numpy(rewards).to(dev), torch.from_numpy(dones).to(dev)


def measure(shape, windows, rounds, dev, T=5, P=8):
    arch, N, A = SHAPES[shape]
    Model = pkg.A3CLSTM if arch == "lstm" else pkg.A3CFF
    model = Model(A, n_envs=N, t_max=T, seed=1234, init_seed=0, device=dev, frames="pairs")
    opt = pkg.RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99).setup(model)
    opt.add_hook(pkg.GradientClipping(40))
    opt.anneal_total_steps, opt.n_total_envs = 8 * 10 ** 7, N
    agent = pkg.A3C(model, opt, T, 0.99, beta=1e-2, collectives=False)
    net = model.net
    pairs, rewards, dones = pools(N, P, dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graphs = {}
    with torch.cuda.stream(stream):
        agent.run_window(pairs, rewards, dones, P, first=True, stream=stream)
        agent.run_window(pairs, rewards, dones, P, stream=stream)   # (creates the env-group side streams)
        for arm, lam in ARMS.items():
            net.set_gae(lam)                                         # gl is an argument of the captured launch
            stream.synchronize()
            graphs[arm] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[arm], stream=stream):
                agent.run_window(pairs, rewards, dones, P, stream=stream)
        for arm in ARMS:                                             # warm both
            for _ in range(20):
                graphs[arm].replay()
    times = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for _ in range(windows):
                    graphs[arm].replay()
            torch.cuda.synchronize()
            times[arm].append(1e3 * (time.perf_counter() - t0) / windows)
    a, b = float(np.median(times["nstep"])), float(np.median(times["gae"]))
    out = {"shape": shape, "arch": arch, "n_envs": N, "t_max": T, "windows_per_round": windows, "rounds": rounds,
           "lambda": ARMS["gae"], "nstep_ms": [round(x, 5) for x in times["nstep"]],
           "gae_ms": [round(x, 5) for x in times["gae"]], "median_nstep_ms": round(a, 5), "median_gae_ms": round(b, 5),
           "difference_us": round(1e3 * (b - a), 3), "params_finite": bool(torch.isfinite(net.params).all())}
    del graphs, agent, opt, model, pairs
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="c4,c3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for shape in a.shapes.split(","):
        res.append(measure(shape, a.windows, a.rounds, dev))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
