#!/usr/bin/env python
"""What the direct-to-ring device env saves: the fused env-step + observation launch against the two launches it
replaces, and the closed-loop window with and without the frame pools.

Two measurements per shape -- C4 (FF, 512 envs, t_max 5) and C3's frames (LSTM, 1,024 envs) -- arms interleaved
within every round (one process, one device), after a warm-up, medians over the rounds:
  launch   microseconds per launch over back-to-back launches between two events: arl_env_step(0) ("env_step"),
           arl_observe(1) ("observe"), the two in turn ("env_step_then_observe") and arl_env_step_observe(0)
           ("env_step_observe"), all on one net and one env whose direct mode is switched between the arms;
  window   the captured closed-loop window replayed: "pairs" (set_env(env), pools) against "direct" (set_env(env,
           direct=True), no pools read), both graphs over the same net, for Catch and Breakout.
The acceptance line: the direct window's median lies below the pairs window's by at least 5 x the env_step time of
the same run (the fused launch costs no more than the observation alone); the margin is the round-to-round spread
(max - min) of the pairs arm.
One JSON line (and --out FILE).

    python scripts/env_direct_cost.py [--envs catch,breakout] [--rounds 7] [--launches 40] [--windows 200]
                                      [--shapes c4,c3]
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

SHAPES = {"c4": ("ff", 512), "c3": ("lstm", 1024)}
GAMES = {"catch": pkg.DeviceCatch, "breakout": pkg.DeviceBreakout, "pong": pkg.DevicePong, "tmaze": pkg.DeviceTMaze,
         "maze": pkg.DeviceMaze}
P = 2


def timed_us(fn, launches, stream):
    """Microseconds per call of `launches` back-to-back calls of fn on stream (two events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        fn()
        a.record(stream)
        for _ in range(launches):
            fn()
        b.record(stream)
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / launches


def setup(kind, n, dev, stream, game):
    T, A = 5, 4
    model = (pkg.A3CFF if kind == "ff" else pkg.A3CLSTM)(A, n_envs=n, t_max=T, seed=1234, init_seed=0, device=dev,
                                                         frames="pairs")
    opt = pkg.RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99).setup(model)
    opt.add_hook(pkg.GradientClipping(40))
    opt.anneal_total_steps, opt.n_total_envs = 8 * 10 ** 7, n
    agent = pkg.A3C(model, opt, T, 0.99, beta=1e-2, collectives=False)
    env = GAMES[game](n, device=dev, seed=1234)
    pools = env.make_pools(P)
    net = model.net
    net.set_env(env)
    with torch.cuda.stream(stream):
        net.env_reset(*pools, P, stream=stream)
        agent.run_window(*pools, P, first=True, stream=stream)
        for _ in range(3):                      # a few windows on: sprites away from their start positions
            agent.run_window(*pools, P, stream=stream)
    stream.synchronize()
    return agent, net, env, pools


def measure(shape, game, dev, stream, rounds, launches, windows):
    kind, n = SHAPES[shape]
    agent, net, env, pools = setup(kind, n, dev, stream, game)
    mode = agent.resize_mode

    def pairs_on():
        net.set_env(env)

    def direct_on():
        net.set_env(env, direct=True)

    def step():
        net.env_step(0, *pools, P, stream=stream)

    def observe():
        net.observe(1, *pools, P, resize_mode=mode, stream=stream)

    def both():
        step()
        observe()

    def fused():
        net.env_step_observe(0, mode, stream=stream)

    arms = {"env_step": (pairs_on, step), "observe": (pairs_on, observe), "env_step_then_observe": (pairs_on, both),
            "env_step_observe": (direct_on, fused)}
    us = {k: [] for k in arms}
    for r in range(rounds + 1):                 # round 0 is the warm-up
        for k, (switch, fn) in arms.items():
            switch()
            v = timed_us(fn, launches, stream)
            if r:
                us[k].append(v)
    lmed = {k: float(np.median(v)) for k, v in us.items()}

    graphs = {}
    for name, switch, wp in (("pairs", pairs_on, pools + (P,)), ("direct", direct_on, (None, None, None, 0))):
        switch()
        with torch.cuda.stream(stream):
            agent.run_window(*wp, stream=stream)
            stream.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name], stream=stream):
                agent.run_window(*wp, stream=stream)
            for _ in range(20):
                graphs[name].replay()
    ms = {k: [] for k in graphs}
    for r in range(rounds + 1):
        for name, g in graphs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for _ in range(windows):
                    g.replay()
            torch.cuda.synchronize()
            if r:
                ms[name].append(1e3 * (time.perf_counter() - t0) / windows)
    wmed = {k: float(np.median(v)) for k, v in ms.items()}
    saved = 1e3 * (wmed["pairs"] - wmed["direct"])
    need = net.t_max * lmed["env_step"]
    spread = 1e3 * (max(ms["pairs"]) - min(ms["pairs"]))
    return {"shape": shape, "kind": kind, "n_envs": n, "env": game,
            "launch_median_us": {k: round(v, 2) for k, v in lmed.items()},
            "fused_minus_observe_us": round(lmed["env_step_observe"] - lmed["observe"], 2),
            "window_median_ms": {k: round(v, 5) for k, v in wmed.items()},
            "window_saved_us": round(saved, 2), "needed_us_5x_env_step": round(need, 2),
            "pairs_spread_us": round(spread, 2), "accepted": bool(saved >= need - spread),
            "pool_bytes_not_allocated": int(sum(p.numel() * p.element_size() for p in pools)),
            "launch_us": {k: [round(x, 2) for x in v] for k, v in us.items()},
            "window_ms": {k: [round(x, 5) for x in v] for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="catch,breakout")
    ap.add_argument("--shapes", default="c4,c3")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be >= 5 (medians)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    out = {"lib": os.path.relpath(pkg.LIB_PATH, ROOT), "rounds": a.rounds, "launches": a.launches,
           "windows_per_round": a.windows, "results": []}
    for shape in a.shapes.split(","):
        for game in a.envs.split(","):
            out["results"].append(measure(shape, game, dev, stream, a.rounds, a.launches, a.windows))
            torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
