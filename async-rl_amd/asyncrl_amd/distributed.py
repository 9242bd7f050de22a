"""Env-sharded data parallelism for the lockstep actor-learner.

Replaces async.py:68-90 (fork P Hogwild processes sharing RawArray params)
with one process per GPU: rank r owns envs [r*n, (r+1)*n) -- frame ring,
LSTM state, rollout buffers and the Philox stream keyed by the global env id
-- and the ranks exchange one gradient per window, the SUM all-reduce of the
flat fp32 gradient (RCCL over xGMI with backend "nccl"; gloo works for CPU
tests), issued in two sections so the large FC / LSTM / heads part overlaps
the conv backward (A3C._reduce_and_step).  Every rank then applies the same clip + RMSProp to replicated
parameters, so replicas stay bitwise identical (checked by replica_checksum).
"""
from __future__ import annotations

import torch
import torch.distributed as dist


def dist_initialized() -> bool:
    return dist.is_available() and dist.is_initialized()


def world_info(group=None):
    if dist_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


def shard_envs(global_envs: int, world: int, rank: int):
    """(n_local, env_offset) for an even split of global_envs over ranks."""
    if global_envs % world:
        raise ValueError(f"{global_envs} envs do not split evenly over {world} ranks")
    n = global_envs // world
    return n, rank * n


def allreduce_grads(grads: torch.Tensor, group=None, async_op: bool = False, force: bool = False):
    """Sum (a contiguous section of) the flat gradient over ranks in place
    (2.71 MB FF / 4.81 MB LSTM per window, latency-bound ring all-reduces).
    async_op: return the work handle (None when nothing was issued); its
    wait() makes the current stream wait for the collective.  With one rank
    nothing is issued unless force=True (a one-rank process group still runs
    the collective: the RCCL path rehearsed on a single GPU)."""
    world, _ = world_info(group)
    if world > 1 or (force and dist.is_available() and dist.is_initialized()):
        return dist.all_reduce(grads, op=dist.ReduceOp.SUM, group=group, async_op=async_op)
    return None


def merge_episode_stats(vectors):
    """Merge the 8 doubles of arl_episode_stats of several ranks, in rank
    order: [episodes, return_sum, return_sumsq, return_min, return_max,
    length_sum, steps, reward_sum] -- SUM for the counts and sums, MIN / MAX
    for the extrema (a rank without an episode holds +inf / -inf there, the
    identities).  Pure host arithmetic; returns a list of 8 floats."""
    vs = [[float(x) for x in v] for v in vectors]
    if not vs or any(len(v) != 8 for v in vs):
        raise ValueError("merge_episode_stats: need at least one vector of 8 values")
    out = list(vs[0])
    for v in vs[1:]:
        for i in (0, 1, 2, 5, 6, 7):
            out[i] += v[i]
        out[3] = min(out[3], v[3])
        out[4] = max(out[4], v[4])
    return out


def _gather_doubles(v: torch.Tensor, group=None):
    """All-gather one rank's float64 tensor of any shape, the same on every
    rank (a device tensor for RCCL, a host one for gloo); returns the ranks'
    tensors in rank order as nested lists."""
    world, _ = world_info(group)
    out = [torch.zeros_like(v) for _ in range(world)]
    dist.all_gather(out, v, group=group)
    return [o.cpu().tolist() for o in out]


def gather_episode_stats(v: torch.Tensor, group=None):
    """All-gather one rank's 8 doubles (a device tensor for RCCL, a host one
    for gloo); returns the ranks' vectors in rank order as lists."""
    return _gather_doubles(v, group)


# fields of a window record (WINDOW_STAT_NAMES) every rank must agree on: window, step, and what the
# update computes from the all-reduced gradient (grad_sqnorm, clip_scale, lr); the rest are sums
_WINDOW_EQUAL = (0, 1, 14, 15, 16)
_WINDOW_FIELDS = 17


def merge_window_stats(rows):
    """Merge one window record (17 doubles, WINDOW_STAT_NAMES order) of
    several ranks that share their gradients: window, step, grad_sqnorm,
    clip_scale and lr must be equal on all ranks (ValueError otherwise);
    samples .. adv_sumsq are summed in rank order.  Pure host arithmetic;
    returns a list of 17 floats."""
    rs = [[float(x) for x in r] for r in rows]
    if not rs or any(len(r) != _WINDOW_FIELDS for r in rs):
        raise ValueError(f"merge_window_stats: need at least one record of {_WINDOW_FIELDS} values")
    out = list(rs[0])
    for k, r in enumerate(rs[1:], 1):
        for i in range(_WINDOW_FIELDS):
            if i in _WINDOW_EQUAL:
                if r[i] != out[i]:
                    raise ValueError(f"merge_window_stats: field {i} differs between rank 0 ({out[i]}) and rank {k} "
                                     f"({r[i]}): the ranks do not describe the same update")
            else:
                out[i] += r[i]
    return out


def gather_window_stats(rows: torch.Tensor, group=None):
    """All-gather one rank's (k, 17) records (k the same on every rank);
    returns the ranks' record lists in rank order."""
    return _gather_doubles(rows, group)


def replica_checksum(t: torch.Tensor) -> int:
    """Order-dependent 64-bit hash of the raw bits (equal iff bitwise equal,
    up to hash collisions)."""
    w = t.detach().contiguous().view(torch.int32).to(torch.int64)
    idx = torch.arange(1, w.numel() + 1, dtype=torch.int64, device=w.device)
    return int(((w * (idx * 2654435761 % 4294967291)) % 9223372036854775783).sum().item())


def replicas_identical(t: torch.Tensor, group=None) -> bool:
    """True iff every rank holds bitwise-identical `t` (all-gathers one int)."""
    world, _ = world_info(group)
    if world == 1:
        return True
    c = torch.tensor([replica_checksum(t)], dtype=torch.int64, device=t.device)
    out = [torch.zeros_like(c) for _ in range(world)]
    dist.all_gather(out, c, group=group)
    return all(int(o.item()) == int(c.item()) for o in out)
