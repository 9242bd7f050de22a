#!/usr/bin/env python
"""What the device-resident envs cost: the env-step kernel as a store stream, and the closed loop in a window.

Three measurements, arms interleaved within every round (one process, one device):
  step     arl_env_step alone, Catch's ("env_step"), Breakout's ("breakout_step", from the reset state: all 120
           bricks to render), Pong's ("pong_step", from the reset state), the T-maze's ("tmaze_step") and the maze's ("maze_step",
           rooms 3, view 0) at 512 envs (C4, FF) and 1,024 envs (C3's frames, LSTM): microseconds per launch
           over back-to-back launches between two events, and the store rate on the 201,600 x n bytes it writes;
           beside it arl_stream_copy of the same byte count, every mode, whose best is the yardstick
           (a copy moves each byte twice, so its rate is quoted on bytes written, as the env's is);
  window   the captured C4 window with the env attached (closed loop) against the same net with the env
           detached over the pools the env left (the difference is the 5 env launches);
  handoff  env_step(t) followed by the observation that reads it, arl_observe(t + 1): the pair's time and the
           observation's share.  Run once per library build (ASYNCRL_HIP_LIB), processes alternating, to A/B a
           change of the render's stores with the launch that reads them timed in both arms (how plain stores
           were chosen over non-temporal ones: DESIGN.md, "Device environment").
--env breakout / --env pong / --env tmaze / --env maze attach DeviceBreakout / DevicePong / DeviceTMaze / DeviceMaze instead of DeviceCatch
in the window and handoff measurements.
One JSON line (and --out FILE).

    python scripts/device_env_cost.py [--env catch|breakout|pong|tmaze|maze] [--rounds 5] [--launches 40] [--windows 200]
                                      [--only step,window,handoff]
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
from asyncrl_amd._lib import check, lib, ptr, stream_handle  # noqa: E402

PAIR = 2 * 210 * 160 * 3


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


def setup(kind, n, dev, stream, P=2, game="catch"):
    T, A = 5, 4
    model = (pkg.A3CFF if kind == "ff" else pkg.A3CLSTM)(A, n_envs=n, t_max=T, seed=1234, init_seed=0, device=dev,
                                                         frames="pairs")
    opt = pkg.RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99).setup(model)
    opt.add_hook(pkg.GradientClipping(40))
    opt.anneal_total_steps, opt.n_total_envs = 8 * 10 ** 7, n
    agent = pkg.A3C(model, opt, T, 0.99, beta=1e-2, collectives=False)
    game_cls = {"catch": pkg.DeviceCatch, "breakout": pkg.DeviceBreakout, "pong": pkg.DevicePong,
                "tmaze": pkg.DeviceTMaze, "maze": pkg.DeviceMaze}[game]
    env = game_cls(n, device=dev, seed=1234)
    pools = env.make_pools(P)
    net = model.net
    net.set_env(env)
    with torch.cuda.stream(stream):
        net.env_reset(*pools, P, stream=stream)
        agent.run_window(*pools, P, first=True, stream=stream)
    stream.synchronize()
    return agent, net, env, pools


def measure_step(kind, n, dev, stream, rounds, launches):
    agent, net, env, pools = setup(kind, n, dev, stream)
    nbytes = PAIR * n
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    h = stream_handle(stream)
    _, bnet, benv, bpools = setup(kind, n, dev, stream, game="breakout")
    _, pnet, penv, ppools = setup(kind, n, dev, stream, game="pong")
    _, tnet, tenv, tpools = setup(kind, n, dev, stream, game="tmaze")
    _, mnet, menv, mpools = setup(kind, n, dev, stream, game="maze")
    arms = {"env_step": lambda: net.env_step(0, *pools, 2, stream=stream),
            "breakout_step": lambda: bnet.env_step(0, *bpools, 2, stream=stream),
            "pong_step": lambda: pnet.env_step(0, *ppools, 2, stream=stream),
            "tmaze_step": lambda: tnet.env_step(0, *tpools, 2, stream=stream),
            "maze_step": lambda: mnet.env_step(0, *mpools, 2, stream=stream)}
    for mode, blocks in ((0, 2048), (1, 2048), (2, 1), (3, 1)):
        arms["copy_mode%d" % mode] = (lambda m=mode, b=blocks: check(
            lib.arl_stream_copy(ptr(src), ptr(dst), nbytes, b, m, h), "arl_stream_copy"))
    us = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            us[k].append(timed_us(fn, launches, stream))
    med = {k: float(np.median(v)) for k, v in us.items()}
    best = min((k for k in med if k.startswith("copy")), key=med.get)
    rate = {k: nbytes / (1e-6 * v) / 1e12 for k, v in med.items()}     # TB/s of bytes written
    return {"kind": kind, "n_envs": n, "bytes_written": nbytes, "median_us": {k: round(v, 2) for k, v in med.items()},
            "write_TBps": {k: round(v, 3) for k, v in rate.items()}, "best_copy": best,
            "env_over_best_copy_rate": round(rate["env_step"] / rate[best], 3),
            "breakout_over_best_copy_rate": round(rate["breakout_step"] / rate[best], 3),
            "breakout_over_catch_time": round(med["breakout_step"] / med["env_step"], 3),
            "pong_over_best_copy_rate": round(rate["pong_step"] / rate[best], 3),
            "pong_over_catch_time": round(med["pong_step"] / med["env_step"], 3),
            "tmaze_over_best_copy_rate": round(rate["tmaze_step"] / rate[best], 3),
            "tmaze_over_catch_time": round(med["tmaze_step"] / med["env_step"], 3),
            "maze_over_best_copy_rate": round(rate["maze_step"] / rate[best], 3),
            "maze_over_catch_time": round(med["maze_step"] / med["env_step"], 3),
            "us": {k: [round(x, 2) for x in v] for k, v in us.items()}}


def measure_window(dev, stream, rounds, windows, game="catch"):
    agent, net, env, pools = setup("ff", 512, dev, stream, game=game)
    graphs = {}
    for name in ("closed_loop", "detached"):
        net.set_env(env if name == "closed_loop" else None)
        with torch.cuda.stream(stream):
            agent.run_window(*pools, 2, stream=stream)
            stream.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name], stream=stream):
                agent.run_window(*pools, 2, stream=stream)
            for _ in range(20):
                graphs[name].replay()
    ms = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for _ in range(windows):
                    g.replay()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / windows)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"shape": "c4", "env": game, "n_envs": 512, "replays_per_round": windows,
            "median_window_ms": {k: round(v, 5) for k, v in med.items()},
            "env_cost_us_per_window": round(1e3 * (med["closed_loop"] - med["detached"]), 2),
            "window_ms": {k: [round(x, 5) for x in v] for k, v in ms.items()}}


def measure_handoff(dev, stream, rounds, launches, game="catch"):
    agent, net, env, pools = setup("ff", 512, dev, stream, game=game)

    def step():
        net.env_step(0, *pools, 2, stream=stream)

    def step_observe():
        net.env_step(0, *pools, 2, stream=stream)
        net.observe(1, *pools, 2, stream=stream)

    us = {"env_step": [], "env_step_then_observe": []}
    for _ in range(rounds):
        us["env_step"].append(timed_us(step, launches, stream))
        us["env_step_then_observe"].append(timed_us(step_observe, launches, stream))
    med = {k: float(np.median(v)) for k, v in us.items()}
    return {"env": game, "n_envs": 512, "median_us": {k: round(v, 2) for k, v in med.items()},
            "observe_after_env_us": round(med["env_step_then_observe"] - med["env_step"], 2),
            "us": {k: [round(x, 2) for x in v] for k, v in us.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", choices=("catch", "breakout", "pong", "tmaze", "maze"), default="catch")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--only", default="step,window,handoff")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    out = {"lib": os.path.relpath(pkg.LIB_PATH, ROOT), "rounds": a.rounds, "launches": a.launches}
    only = a.only.split(",")
    if "step" in only:
        out["step"] = [measure_step("ff", 512, dev, stream, a.rounds, a.launches),
                       measure_step("lstm", 1024, dev, stream, a.rounds, a.launches)]
    if "window" in only:
        out["window"] = measure_window(dev, stream, a.rounds, a.windows, a.env)
    if "handoff" in only:
        out["handoff"] = measure_handoff(dev, stream, a.rounds, a.launches, a.env)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
