"""What the GPU tests of the device environments share (test_gpu_catch.py, test_gpu_breakout.py):
the closed actor-learner loop over a device env class, replayed through that game's NumPy
restatement and the episode replay.  The env class, the restatement instance and each game's own
bounds come from the test."""
import numpy as np
import torch

from episode_replay import Replay, same_bits


def dev(x, gpu, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(gpu)


def make_agent(game_cls, kind, A, n, T, P, gpu, seed=5, env=True, window_stats=False, **game_kw):
    """An agent at the reference's hyperparameters on `kind` ("ff" / "lstm"), its pools, and a
    game_cls(**game_kw) attached and reset (the window that follows runs with first=True)."""
    from asyncrl_amd import A3C, A3CFF, A3CLSTM, GradientClipping, RMSpropAsync
    model = (A3CFF if kind == "ff" else A3CLSTM)(A, n_envs=n, t_max=T, seed=seed, init_seed=1, device=gpu,
                                                 frames="pairs")
    opt = RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99).setup(model)
    opt.add_hook(GradientClipping(40))
    agent = A3C(model, opt, T, 0.99)
    net = model.net
    net.set_episode_stats(True)
    if window_stats:
        net.set_window_stats(True)
    game = game_cls(n, device=gpu, seed=seed, **game_kw)
    pools = game.make_pools(P)
    if env:
        net.set_env(game)
        net.env_reset(*pools, P)
    return agent, net, game, pools


class LoopCheck:
    """Replays the actions the policy sampled through `ref`, the game's restatement (not yet
    reset), and the episode replay.  min_episodes(k): the episodes the game must have completed
    after k env-steps."""

    def __init__(self, ref, min_episodes, keep=8):
        self.ref = ref
        self.obs = {0: self.ref.reset()}          # observation index -> (pairs, rewards, dones)
        self.rp = Replay(ref.n)
        self.k, self.keep, self.min_episodes = 0, keep, min_episodes
        self.slots = []                           # per window: (T, n) dones
        self.rewards = []

    def window(self, net):
        """The window that just ran: its rewards / dones rows are what the env answers to its actions."""
        T, n = net.t_max, net.n_envs
        torch.cuda.synchronize()
        acts = net.buffer("actions", torch.int32, (T + 1, n))[:T].cpu().numpy()
        rew = net.buffer("rewards", torch.float32, (T, n)).cpu().numpy()
        don = net.buffer("dones", torch.uint8, (T, n)).cpu().numpy()
        assert acts.min() >= 0 and acts.max() < net.n_actions
        for t in range(T):
            _, r, d = out = self.ref.step(acts[t])
            self.k += 1
            self.obs[self.k] = out
            self.obs.pop(self.k - self.keep, None)
            self.rp.step(r, d, self.k)
            assert same_bits(rew[t], r) and same_bits(don[t], d), (self.k, t)
        self.slots.append(don.copy())
        self.rewards.append(rew.copy())

    def end(self, net, game, pools, P):
        """The final state half, the pool entries left, the episode statistics."""
        torch.cuda.synchronize()
        assert same_bits(game.state[self.k & 1].cpu().numpy(), self.ref.state)
        for k in range(self.k - min(P, self.keep) + 1, self.k + 1):
            for pool, want in zip(pools, self.obs[k]):
                assert same_bits(pool[k % P].cpu().numpy(), want), k
        assert same_bits(net.episode_stats_raw(), self.rp.reduce())
        assert self.rp.reduce()[0] >= self.min_episodes(self.k)


def run_windows(agent, pools, P, windows, check=None, **kw):
    for w in range(windows):
        agent.run_window(*pools, P, first=(w == 0), **kw)
        if check is not None:
            check.window(agent.net)


def learn_run(game_cls, gpu, lr, windows, n=256, seed=0, raw=False):
    """A game from pixels, closed loop: FF, 256 envs, t_max 5, the reference's hyperparameters
    (RMSpropAsync alpha 0.99, eps 0.1, clip 40, beta 0.01, gamma 0.99, rewards clipped for the
    learner), window 0 eagerly and one captured window replayed.  Returns the episode statistics of
    the last tenth of the run (raw: the 8 sums, not the dict), and the parameters."""
    from asyncrl_amd import A3C, A3CFF, GradientClipping, RMSpropAsync
    T, P = 5, 2
    model = A3CFF(4, n_envs=n, t_max=T, seed=seed, init_seed=seed, device=gpu, frames="pairs")
    opt = RMSpropAsync(lr=lr, eps=1e-1, alpha=0.99).setup(model)
    opt.add_hook(GradientClipping(40))
    agent = A3C(model, opt, T, 0.99, beta=1e-2)
    net = model.net
    net.set_episode_stats(True)
    game = game_cls(n, device=gpu, seed=seed)
    pools = game.make_pools(P)
    net.set_env(game)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net.env_reset(*pools, P, stream=s)
        agent.run_window(*pools, P, first=True, stream=s)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            agent.run_window(*pools, P, stream=s)
        tail = windows // 10
        for _ in range(windows - 1 - tail):
            g.replay()
        net.episode_stats(clear=True, stream=s)
        for _ in range(tail):
            g.replay()
        st = net.episode_stats_raw(stream=s) if raw else net.episode_stats(stream=s)
    return st, net.params.clone()
