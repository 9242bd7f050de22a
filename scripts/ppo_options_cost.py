#!/usr/bin/env python
"""What the PPO epochs' options (A3C(ppo_norm_adv=, ppo_vclip=)) cost a window.

C4 shape: A3C-FF NIPS head, 512 envs, t_max 5, K = 3 epochs, Adam, lambda 0.95.  Two arms, options off and on
(norm_adv and vclip 0.2), one agent each:
  * the window captured as a graph and replayed, arms alternating: ROUNDS rounds of WINDOWS replays, median ms;
  * the window timeline (arl_stamps_*) over eager windows: the median time of every stamp interval of a window,
    in order, so the intervals the options add (the "other" stamps after the snapshot's and after each epoch's
    "returns") stand beside the ones that were there.  Eager intervals include the launch gap;
  * the two one-workgroup kernels alone through the granular entries (events over REPS back-to-back launches).
--pkg DIR times another tree's package (an A/B against another commit; a tree without the options runs only
the off arm).  One JSON line (and --out FILE).

    python scripts/ppo_options_cost.py [--windows 200] [--rounds 5] [--pkg DIR] [--out FILE]
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
N, T, A, P, K = 512, 5, 4, 8, 3


def pools(dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    pairs = torch.randint(0, 256, (P, N, 2, 210, 160, 3), dtype=torch.uint8, device=dev, generator=g)
    rng = np.random.default_rng(2)
    rewards = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), (P, N), p=[0.025, 0.95, 0.025])
    dones = (rng.random((P, N)) < 1 / 500).astype(np.uint8)
    return pairs, torch.from_numpy(rewards).to(dev), torch.from_numpy(dones).to(dev)


def make_agent(pkg, dev, on):
    model = pkg.A3CFF(A, n_envs=N, t_max=T, seed=1234, init_seed=0, device=dev, frames="pairs")
    opt = pkg.Adam(alpha=1e-4).setup(model)
    opt.add_hook(pkg.GradientClipping(40))
    kw = dict(ppo_norm_adv=True, ppo_vclip=0.2) if on else {}
    return pkg.A3C(model, opt, T, 0.99, beta=1e-2, collectives=False, gae_lambda=0.95, ppo_epochs=K, **kw)


def windows_cost(pkg, arms, windows, rounds, dev):
    pl = pools(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    graphs, agents = {}, {}
    for arm in arms:
        agents[arm] = agent = make_agent(pkg, dev, arm == "on")
        with torch.cuda.stream(stream):
            agent.run_window(*pl, P, first=True, stream=stream)
            stream.synchronize()
            graphs[arm] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[arm], stream=stream):
                agent.run_window(*pl, P, stream=stream)
            for _ in range(20):
                graphs[arm].replay()
    times = {arm: [] for arm in arms}
    for _ in range(rounds):
        for arm in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for _ in range(windows):
                    graphs[arm].replay()
            torch.cuda.synchronize()
            times[arm].append(1e3 * (time.perf_counter() - t0) / windows)
    out = {f"window_{arm}_ms": [round(x, 5) for x in times[arm]] for arm in arms}
    out.update({f"median_window_{arm}_ms": round(float(np.median(times[arm])), 5) for arm in arms})
    # the timeline of eager windows, per arm
    for arm in arms:
        agent, net = agents[arm], agents[arm].net
        W = 40
        torch.cuda.synchronize()
        net.stamps_begin(W * 256)
        for _ in range(W):
            agent.run_window(*pl, P, first=False)
        ms, stages = net.stamps_end()
        per = len(ms) // W
        assert per * W == len(ms), (len(ms), W)
        rows = ms.reshape(W, per)[1:]                 # (the first window's first interval has no predecessor)
        med = np.median(rows, 0)
        out[f"timeline_{arm}"] = [[s, round(float(1e3 * x), 2)] for s, x in zip(stages[:per], med)]   # us
    out["params_finite"] = all(bool(torch.isfinite(a.net.params).all()) for a in agents.values())
    return out


def launch_cost(lib, reps, rounds, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    f = lambda *s: torch.rand(*s, device=dev, generator=g)                       # noqa: E731
    v, logp = f(T + 1, N), torch.log(torch.softmax(f(T + 1, N, A), -1))
    dones = torch.zeros(T, N, dtype=torch.uint8, device=dev)
    act = torch.zeros(T + 1, N, dtype=torch.int32, device=dev)
    lpo, adv, ret, ratio, vold = logp[:T, :, 0].contiguous(), f(T, N) - 0.5, f(T, N), f(T, N) + 0.5, f(T, N)
    adv0 = adv.clone()
    m = torch.zeros(3, dtype=torch.float64, device=dev)
    rec = torch.zeros(10, dtype=torch.float64, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())                                   # noqa: E731

    def norm():
        return lib.arl_ppo_normalize_adv(p(dones), p(adv), T, N, p(m), None)

    def stats():
        return lib.arl_ppo_epoch_stats(p(dones), p(v), p(logp), p(act), p(lpo), p(adv), p(ret), p(ratio), p(vold), T, N, A,
                                       0.2, 0.2, 0.0, 1.0, p(rec), None)

    times = {"normalize_adv": [], "epoch_stats": []}
    for _ in range(rounds):
        for name, fn in (("normalize_adv", norm), ("epoch_stats", stats)):
            adv.copy_(adv0)
            assert fn() == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / reps)
    return {f"{k}_us": round(float(np.median(x)), 3) for k, x in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "async-rl_amd"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import asyncrl_amd as pkg
    from asyncrl_amd._lib import lib
    has = hasattr(lib, "arl_net_set_ppo_options") and "arl_net_set_ppo_options" in pkg._lib.SIGNATURES
    dev = torch.device("cuda:0")
    out = {"pkg": os.path.relpath(a.pkg, ROOT), "n_envs": N, "t_max": T, "epochs": K, "windows_per_round": a.windows,
           "rounds": a.rounds}
    out.update(windows_cost(pkg, ("off", "on") if has else ("off",), a.windows, a.rounds, dev))
    if has:
        out.update(launch_cost(lib, 500, a.rounds, dev))
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
