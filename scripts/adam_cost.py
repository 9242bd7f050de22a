#!/usr/bin/env python
"""What the Adam update kernel costs in a window against the RMSProp one.

C4's shape (A3C-FF NIPS head, 512 envs, t_max 5, clip 40, on-device anneal), one net whose optimizer is
switched between the two (DeviceNet.set_adam) in alternation, two measurements per arm and round:
  stage_us   the window timeline's interval that the update kernel closes (arl_stamps_*, stage "rmsprop":
             from the conv reduce's stamp to the update's), median over the eager windows of the round;
  window_ms  a whole window as a captured graph, the mean over WINDOWS replays of the round.
Reports the medians over the rounds and the Adam / RMSProp ratio of the stage; one JSON line (and --out FILE).

    python scripts/adam_cost.py [--windows 200] [--rounds 5] [--out FILE]
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


def pools(n, P, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    pairs = torch.randint(0, 256, (P, n, 2, 210, 160, 3), dtype=torch.uint8, device=dev, generator=g)
    rng = np.random.default_rng(2)
    rewards = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), (P, n), p=[0.025, 0.95, 0.025])
    dones = (rng.random((P, n)) < 1 / 500).astype(np.uint8)
    return pairs, torch.from_numpy(rewards).to(dev), torch.from_numpy(dones).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, T, A, P = 512, 5, 4, 8
    model = pkg.A3CFF(A, n_envs=N, t_max=T, seed=1234, init_seed=0, device=dev, frames="pairs")
    opts = {"rmsprop": pkg.RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99), "adam": pkg.Adam(alpha=1e-4)}
    for o in opts.values():
        o.add_hook(pkg.GradientClipping(40))
        o.anneal_total_steps, o.n_total_envs = 8 * 10 ** 7, N
        o.target = model
    agent = pkg.A3C(model, opts["rmsprop"], T, 0.99, beta=1e-2, collectives=False)
    net = model.net
    pairs, rewards, dones = pools(N, P, dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())

    def arm(name):
        agent.optimizer = opts[name]
        net.set_adam(*((opts["adam"].beta1, opts["adam"].beta2) if name == "adam" else (None,)))

    graphs = {}
    with torch.cuda.stream(stream):
        agent.run_window(pairs, rewards, dones, P, first=True, stream=stream)
        for name in opts:
            arm(name)
            agent.run_window(pairs, rewards, dones, P, stream=stream)
            stream.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name], stream=stream):
                agent.run_window(pairs, rewards, dones, P, stream=stream)
            for _ in range(20):
                graphs[name].replay()
    stage = {k: [] for k in opts}
    window = {k: [] for k in opts}
    eager = min(a.windows, 50)
    for _ in range(a.rounds):
        for name in opts:
            arm(name)
            with torch.cuda.stream(stream):
                net.stamps_begin(eager * 64)
                for _ in range(eager):
                    agent.run_window(pairs, rewards, dones, P, stream=stream)
                ms, st = net.stamps_end()
            us = [1e3 * m for m, s in zip(ms, st) if s == "rmsprop"]
            assert len(us) == eager
            stage[name].append(float(np.median(us)))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for _ in range(a.windows):
                    graphs[name].replay()
            torch.cuda.synchronize()
            window[name].append(1e3 * (time.perf_counter() - t0) / a.windows)
    med = lambda xs: float(np.median(xs))   # noqa: E731
    out = {"shape": "c4", "n_envs": N, "t_max": T, "param_floats": net.param_floats, "rounds": a.rounds,
           "eager_windows_per_round": eager, "replays_per_round": a.windows,
           "stage_us": {k: [round(x, 3) for x in v] for k, v in stage.items()},
           "window_ms": {k: [round(x, 5) for x in v] for k, v in window.items()},
           "median_stage_us": {k: round(med(v), 3) for k, v in stage.items()},
           "median_window_ms": {k: round(med(v), 5) for k, v in window.items()},
           "stage_ratio_adam_over_rmsprop": round(med(stage["adam"]) / med(stage["rmsprop"]), 3),
           "window_difference_us": round(1e3 * (med(window["adam"]) - med(window["rmsprop"])), 3),
           "adam_t": net.adam_t(), "params_finite": bool(torch.isfinite(net.params).all())}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
