#!/usr/bin/env python
"""Closed-loop training on a device-resident env (asyncrl_amd.DeviceCatch, DeviceBreakout with --env breakout,
DevicePong with --env pong --points P, DeviceTMaze with --env tmaze --length L, or DeviceMaze with --env maze
--rooms R --view V --levels L): the learner has to learn.

env -> phi -> forward -> sample -> env -> ... -> update runs on the device with no host work per step: window 0
eagerly (first=True), then one captured window replayed.  Every --report windows the learning curve is read
from the device-side episode statistics (A3C.episode_stats(clear=True): the episodes completed since the
last read) together with the newest per-window record (A3C.window_stats).  The optimum is +1 per episode, a
uniform random policy scores about -0.70.  With --env breakout an episode is a life (a life loss is terminal, as
the reference trains), the return is the raw, unclipped sum of its brick values, and a uniform random policy
scores about 0.14 per life.  With --env pong an episode is a game to --points points against the opponent's paddle,
the return is the agent's points minus the opponent's, and a uniform random policy scores about -0.36 at --points 1
and about -17 at 21.  With --env tmaze an episode is one cue, a corridor of --length steps and one choice (+1 for the
cue's arm, -1 for the other, 0 for none): any policy that does not remember the cue scores 0 on average, which from
--length 4 on is every policy of the FF model; --arch lstm can reach +1.  --t-max sets the window (default 5: with
--length 4 an episode is one window; a longer corridor needs memory across a window boundary).  With --env maze an
episode is one level of a grid maze over --rooms x --rooms rooms: +1 for reaching the goal within 8 rooms steps, else
0, so the mean return is the success rate; a uniform random policy scores 0.368 / 0.211 / 0.144 at --rooms 2 / 3 / 4.
--view 1 or 2 hides all but the tiles around the agent.  --levels L > 0 trains on levels 0..L-1 only; after training
the parameters are copied into an evaluation model that plays 2,048 sampled runs on DeviceMaze(levels=L) and on
DeviceMaze(levels=0), same seed: the two success rates ("eval_trained_levels", "eval_all_levels") are printed and
added to the JSON line, and their difference is the generalisation gap.

Defaults are the reference's hyperparameters (RMSpropAsync lr 7e-4, alpha 0.99, eps 0.1, clip 40, beta 0.01,
gamma 0.99) on the FF model with 256 envs; the batched learner sums the gradient of all envs, so --batch-loss
mean, --opt adam, --gae-lambda and --ppo-epochs (clipped-surrogate epochs on each window's rollout, with
--ppo-clip; each report row then carries A3C.ppo_stats of the last epoch; --ppo-norm-adv and --ppo-vclip X switch
the epochs' advantage normalisation and clipped value loss on, and each row then also carries the last epoch's
device-side record, A3C.ppo_epoch_stats) are there to try.  --direct runs the env direct-to-ring
(DeviceNet.set_env(env, direct=True)): no frame pools are allocated, the curve is bit-identical.  One JSON line at
the end (and --out FILE).

    python scripts/train_catch.py [--env catch|breakout|pong|tmaze|maze] [--points 21] [--length 4] [--t-max 5]
                                  [--rooms 3] [--view 0] [--levels 0]
                                  [--windows 4000] [--report 200]
                                  [--envs 256] [--seed 0]
                                  [--lr 7e-4] [--opt rmsprop|adam] [--batch-loss sum|mean] [--gae-lambda 1.0]
                                  [--arch ff|lstm] [--ppo-epochs 1] [--ppo-clip 0.2] [--ppo-norm-adv] [--ppo-vclip X]
                                  [--direct]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "async-rl_amd"))

import asyncrl_amd as pkg  # noqa: E402


def train(envs=256, windows=4000, report=200, seed=0, lr=7e-4, opt="rmsprop", batch_loss="sum", gae_lambda=1.0,
          arch="ff", beta=1e-2, eps=None, device="cuda:0", log=print, env="catch", ppo_epochs=1, ppo_clip=0.2, ppo_norm_adv=False,
          ppo_vclip=None, points=21, direct=False, length=4, t_max=5, rooms=3, view=0, levels=0, evaluation=None):
    """Returns the curve: one dict per report with the window count, the episodes completed since the last
    report and their mean return, and the newest window record's entropy / value / gradient norm.  evaluation: a
    dict that, with env="maze" and levels > 0, receives the trained model's success rates on the trained levels
    and on all levels (evaluate_maze)."""
    dev = torch.device(device)
    T, A, P = t_max, 4, 2
    model = (pkg.A3CFF if arch == "ff" else pkg.A3CLSTM)(A, n_envs=envs, t_max=T, seed=seed, init_seed=seed,
                                                         device=dev, frames="pairs")
    if opt == "adam":
        optimizer = pkg.Adam(alpha=lr, eps=1e-8 if eps is None else eps).setup(model)
    else:
        optimizer = pkg.RMSpropAsync(lr=lr, eps=1e-1 if eps is None else eps, alpha=0.99).setup(model)
    optimizer.add_hook(pkg.GradientClipping(40))
    agent = pkg.A3C(model, optimizer, T, 0.99, beta=beta, batch_loss=batch_loss, gae_lambda=gae_lambda,
                    collectives=False, ppo_epochs=ppo_epochs, ppo_clip=ppo_clip, ppo_norm_adv=ppo_norm_adv,
                    ppo_vclip=ppo_vclip)
    net = model.net
    net.set_episode_stats(True)
    net.set_window_stats(True)
    if env == "pong":
        game = pkg.DevicePong(envs, device=dev, seed=seed, points=points)
    elif env == "tmaze":
        game = pkg.DeviceTMaze(envs, device=dev, seed=seed, length=length)
    elif env == "maze":
        game = pkg.DeviceMaze(envs, device=dev, seed=seed, rooms=rooms, view=view, levels=levels)
    else:
        game = (pkg.DeviceBreakout if env == "breakout" else pkg.DeviceCatch)(envs, device=dev, seed=seed)
    pools = (None, None, None) if direct else game.make_pools(P)   # direct: the frame pairs never exist
    net.set_env(game, direct=direct)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        if not direct:   # (a direct window with first=True issues the reset itself)
            net.env_reset(*pools, P, stream=stream)
        agent.run_window(*pools, P, first=True, stream=stream)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            agent.run_window(*pools, P, stream=stream)
    curve, done = [], 1
    t0 = time.perf_counter()
    while done < windows:
        k = min(report, windows - done)
        with torch.cuda.stream(stream):
            for _ in range(k):
                graph.replay()
            done += k
            ep = agent.episode_stats(clear=True, stream=stream)
            ws = agent.window_stats(1, stream=stream)[0]
        row = {"windows": done, "episodes": ep["episodes"], "mean_return": ep["mean"], "entropy": ws["entropy"],
               "value_mean": ws["value_mean"], "grad_norm": ws["grad_norm"], "pi_loss": ws["pi_loss"],
               "v_loss": ws["v_loss"], "seconds": time.perf_counter() - t0}
        if ppo_epochs > 1:
            row.update(agent.ppo_stats(stream=stream))
        if ppo_norm_adv or ppo_vclip is not None:
            row["ppo_epoch"] = agent.ppo_epoch_stats(1, stream=stream)[0]
        curve.append(row)
        log("windows %6d  episodes %6d  return %+.3f  entropy %.3f  v %+.3f  |g| %9.3f  pi_loss %+10.3f  "
            "v_loss %9.3f  %.1fs" % (done, row["episodes"], row["mean_return"], row["entropy"], row["value_mean"],
                                     row["grad_norm"], row["pi_loss"], row["v_loss"], row["seconds"])
            + ("  clip %.3f  kl %+.4f  rho_max %.3f" % (row["clip_fraction"], row["approx_kl"], row["ratio_max"])
               if ppo_epochs > 1 else "")
            + ("  vclip %.3f  adv %+.3f +- %.3f" % tuple(row["ppo_epoch"][k] for k in ("vclip_fraction", "adv_mean",
                                                                                          "adv_std"))
               if "ppo_epoch" in row else ""))
    if env == "maze" and levels > 0 and evaluation is not None:
        with torch.cuda.stream(stream):
            evaluation.update(evaluate_maze(model, arch, dev, seed, rooms, view, levels, T, stream))
        log("success on the %d trained levels %.4f, on all levels %.4f (%d sampled runs each)"
            % (levels, evaluation["eval_trained_levels"], evaluation["eval_all_levels"], EVAL_RUNS))
    return curve


EVAL_RUNS, EVAL_ENVS = 2048, 256


def evaluate_maze(model, arch, dev, seed, rooms, view, levels, t_max, stream=None):
    """The trained parameters in an evaluation model of its own (the learner's games go on), EVAL_RUNS runs of the
    sampled policy through evaluation.run_episodes on the trained levels and on all of them, same seed: a run's
    score is 1 or 0, so the mean is the success rate."""
    ev = (pkg.A3CFF if arch == "ff" else pkg.A3CLSTM)(4, n_envs=EVAL_ENVS, t_max=t_max, seed=seed, init_seed=seed,
                                                      device=dev, frames="pairs")
    ev.net.copy_params_from(model.net)
    out = {}
    for key, lv in (("eval_trained_levels", levels), ("eval_all_levels", 0)):
        game = pkg.DeviceMaze(EVAL_ENVS, device=dev, seed=seed, rooms=rooms, view=view, levels=lv)
        scores, _ = pkg.run_episodes(ev, game, EVAL_RUNS, deterministic=False, stream=stream)
        out[key] = float(scores.mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", choices=("catch", "breakout", "pong", "tmaze", "maze"), default="catch")
    ap.add_argument("--points", type=int, default=21)
    ap.add_argument("--length", type=int, default=4)
    ap.add_argument("--t-max", type=int, default=5)
    ap.add_argument("--rooms", type=int, default=3)
    ap.add_argument("--view", type=int, default=0)
    ap.add_argument("--levels", type=int, default=0)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--windows", type=int, default=4000)
    ap.add_argument("--report", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=7e-4)
    ap.add_argument("--opt", choices=("rmsprop", "adam"), default="rmsprop")
    ap.add_argument("--batch-loss", choices=("sum", "mean"), default="sum")
    ap.add_argument("--gae-lambda", type=float, default=1.0)
    ap.add_argument("--beta", type=float, default=1e-2)
    ap.add_argument("--eps", type=float, default=None)
    ap.add_argument("--arch", choices=("ff", "lstm"), default="ff")
    ap.add_argument("--ppo-epochs", type=int, default=1)
    ap.add_argument("--ppo-clip", type=float, default=0.2)
    ap.add_argument("--ppo-norm-adv", action="store_true")
    ap.add_argument("--ppo-vclip", type=float, default=None)
    ap.add_argument("--direct", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = {k: v for k, v in vars(a).items() if k != "out"}
    evaluation = {}
    curve = train(evaluation=evaluation, **cfg)
    out = {"config": cfg, "curve": curve, "final_mean_return": curve[-1]["mean_return"] if curve else None}
    out.update(evaluation)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
