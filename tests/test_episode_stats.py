"""CPU: the device-side episode statistics' host pieces -- the three C symbols and
ARL_EPISODE_LOG in the header and the ctypes table, the rank merge, the host-derived
figures, and the NumPy replay the GPU tests compare against (episode_replay.Replay) checked
against a literal serial restatement of the reference's episode_r / total_r loop."""
import ctypes
import math
import os
import re
import statistics

import numpy as np
import pytest

from conftest import ROOT
from episode_replay import LOG, REWARD_VALUES, Replay, case_pools, same_bits, serial_reference

HEADER = os.path.join(ROOT, "include", "asyncrl_hip.h")
SYMBOLS = ("arl_net_set_episode_stats", "arl_episode_stats_reset", "arl_episode_stats")


def test_symbols_declared_bound_and_exported():
    from asyncrl_amd import _lib
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert s in _lib.SIGNATURES and hasattr(_lib.lib, s), s
    assert re.search(r"#define\s+ARL_EPISODE_LOG\s+8\b", code)
    assert _lib.EPISODE_LOG == LOG == 8
    assert _lib.lib.arl_abi_version() == 4                      # additions to ABI 4
    assert "a3c_ale.py:95-96,114-124" in txt and "twice" in txt  # the semantics' source and the double-count note


def test_unbound_net_is_estate_and_workspace_names_the_arrays():
    from asyncrl_amd._lib import lib
    from episode_replay import BUFFERS
    n = 40
    h = ctypes.c_void_p()
    assert lib.arl_net_create(ctypes.byref(h), 0, 4, n, 5, 0, 0) == 0
    try:
        assert lib.arl_net_set_episode_stats(h, 1) == 3
        assert lib.arl_episode_stats_reset(h, None) == 3
        assert lib.arl_episode_stats(h, None, 0, None) == 3
        ws = lib.arl_net_workspace_bytes(h)
        off, nb = ctypes.c_int64(), ctypes.c_int64()
        prev_end = 0
        for name in BUFFERS:
            assert lib.arl_net_buffer(h, name.encode(), ctypes.byref(off), ctypes.byref(nb)) == 0, name
            logs = name in ("ep_log_ret", "ep_log_len", "ep_log_step")
            assert nb.value == 8 * n * (LOG if logs else 1)
            assert off.value % 256 == 0 and off.value >= prev_end
            prev_end = off.value + nb.value
        assert prev_end <= ws < prev_end + 256                   # the block ends the workspace
        fake = 1 << 40                                           # bound to fake memory: host checks only
        assert lib.arl_net_bind(h, fake, fake, fake, fake) == 0
        assert lib.arl_episode_stats(h, fake, 0, None) == 3      # the feature is off
        assert lib.arl_net_set_episode_stats(h, 1) == 0
        assert lib.arl_episode_stats(h, None, 0, None) == 1      # null out
        assert lib.arl_episode_stats(h, fake + 4, 0, None) == 1  # misaligned out
    finally:
        lib.arl_net_destroy(h)


def test_merge_episode_stats():
    from asyncrl_amd.distributed import merge_episode_stats
    inf = math.inf
    a = [3.0, 10.5, 50.25, -1.5, 7.0, 30.0, 100.0, 12.0]
    b = [0.0, 0.0, 0.0, inf, -inf, 0.0, 64.0, 0.3]             # a rank without an episode
    c = [2.0, -3.0, 4.5, -2.5, -0.5, 9.0, 64.0, -2.0]
    assert merge_episode_stats([a]) == a
    assert merge_episode_stats([b, b]) == [0.0, 0.0, 0.0, inf, -inf, 0.0, 128.0, 0.6]
    got = merge_episode_stats([a, b, c])
    assert got == [5.0, 7.5, 54.75, -2.5, 7.0, 39.0, 228.0, (12.0 + 0.3) + -2.0]
    assert merge_episode_stats([b, a])[3:5] == [-1.5, 7.0]
    assert merge_episode_stats([np.array(a), np.array(c)])[0] == 5.0
    with pytest.raises(ValueError):
        merge_episode_stats([])
    with pytest.raises(ValueError):
        merge_episode_stats([a[:7]])


RANK_VECTORS = ([3.0, 10.5, 50.25, -1.5, 7.0, 30.0, 100.0, 12.0],
                [0.0, 0.0, 0.0, math.inf, -math.inf, 0.0, 64.0, 0.3])


def _gather_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "async-rl_amd"))
    import torch
    import torch.distributed as dist
    from asyncrl_amd.distributed import gather_episode_stats, merge_episode_stats
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        vs = gather_episode_stats(torch.tensor(RANK_VECTORS[rank], dtype=torch.float64))
        q.put((rank, vs, merge_episode_stats(vs)))
    finally:
        dist.destroy_process_group()


def test_two_rank_gather_and_merge():
    """What A3C.episode_stats(reduce=True) does with a process group (gloo, world_size 2):
    every rank ends with all ranks' vectors in rank order and the same merge."""
    import socket
    import torch.multiprocessing as mp
    from asyncrl_amd.distributed import merge_episode_stats
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in ps:
        p.join(timeout=60)
    want = merge_episode_stats(RANK_VECTORS)
    assert want == [3.0, 10.5, 50.25, -1.5, 7.0, 30.0, 164.0, 12.3]
    for rank, vs, merged in res:
        assert vs == [list(v) for v in RANK_VECTORS] and merged == want, rank


def test_host_derived_figures():
    from asyncrl_amd.net import episode_stats_dict
    rets = [2.5, -1.0, 7.0, 0.5]
    v = [len(rets), sum(rets), sum(x * x for x in rets), min(rets), max(rets), 40.0, 55.0, 9.5]
    d = episode_stats_dict(v)
    assert d["episodes"] == 4 and d["steps"] == 55 and d["length_sum"] == 40
    assert d["mean"] == statistics.mean(rets) and d["mean_length"] == 10.0
    assert abs(d["stdev"] - statistics.stdev(rets)) < 1e-12
    assert d["return_min"] == -1.0 and d["return_max"] == 7.0 and d["reward_sum"] == 9.5
    e = episode_stats_dict([0, 0, 0, math.inf, -math.inf, 0, 3, 0.1])
    assert e["episodes"] == 0 and math.isnan(e["mean"]) and math.isnan(e["stdev"]) and math.isnan(e["mean_length"])
    assert math.isnan(episode_stats_dict([1, 2.0, 4.0, 2.0, 2.0, 5, 5, 2.0])["stdev"])


def test_replay_matches_serial_reference():
    """The vectorised replay == the literal per-env loop on random (r, d) streams, every field."""
    rng = np.random.default_rng(7)
    n, steps = 11, 90
    rewards = rng.choice(REWARD_VALUES, (steps, n)).astype(np.float32)
    dones = (rng.random((steps, n)) < 0.2).astype(np.uint8)
    dones[:, 3] = 0
    dones[:, 4] = 1
    rp = Replay(n)
    for k in range(steps):
        rp.step(rewards[k], dones[k], 100 + k)
    b = rp.b
    for e in range(n):
        rets, lens, at, running, total = serial_reference(rewards[:, e], dones[:, e])
        c = len(rets)
        assert b["ep_count"][e] == c == b["ep_log_count"][e]
        assert b["ep_steps"][e] == steps and b["ep_total"][e] == total and b["ep_run_ret"][e] == running
        assert b["ep_run_len"][e] == steps - sum(lens)
        s = ss = 0.0
        for g in rets:
            s += g
            ss += g * g
        assert b["ep_sum"][e] == s and b["ep_sumsq"][e] == ss and b["ep_len_sum"][e] == sum(lens)
        assert b["ep_min"][e] == (min(rets) if rets else np.inf)
        assert b["ep_max"][e] == (max(rets) if rets else -np.inf)
        for i in range(max(0, c - LOG), c):                      # the last LOG episodes, at i % LOG
            assert b["ep_log_ret"][i % LOG, e] == rets[i]
            assert b["ep_log_len"][i % LOG, e] == lens[i]
            assert b["ep_log_step"][i % LOG, e] == 100 + at[i]
    # the fixed-order reduce of so few envs is the plain left-to-right sum
    red = rp.reduce()
    assert red[0] == b["ep_count"].sum() and red[6] == n * steps
    s = 0.0
    for e in range(n):
        s += b["ep_sum"][e]
    assert red[1] == s and red[3] == b["ep_min"].min() and red[4] == b["ep_max"].max()
    # clear: the cumulative arrays only
    keep = {k: b[k].copy() for k in ("ep_run_ret", "ep_run_len", "ep_log_ret", "ep_log_count")}
    rp.reduce(clear=True)
    z = rp.reduce()
    assert same_bits(z, np.array([0, 0, 0, np.inf, -np.inf, 0, 0, 0], np.float64))
    assert all(same_bits(keep[k], b[k]) for k in keep)


def test_gpu_case_inputs_have_the_three_kinds():
    """The inputs of the main GPU case (40 envs, pool of 7, observations 1..60): an env that
    never terminates, one that terminates at every step, one whose log wraps; non-trivial sums."""
    rewards, dones = case_pools(1, 7, 40)
    rp = Replay(40).run(rewards, dones, 1, 61)
    c = rp.b["ep_count"]
    assert c[0] == 0 and rp.b["ep_run_len"][0] == 60 and rp.b["ep_min"][0] == np.inf
    assert c[1] == 60 and rp.b["ep_len_sum"][1] == 60
    assert LOG < c[2] < 60 and rp.b["ep_log_count"][2] == c[2]
    assert (c[3:] > 0).sum() > 30 and (rp.b["ep_run_len"][3:] > 0).any()   # the random envs: mid-episode too
    assert np.abs(rp.b["ep_log_ret"]).max() > 1.0                # a clipped reward would show
    f32 = np.zeros(40, np.float32)                               # an f32 accumulation would show too
    for k in range(1, 61):
        f32 += rewards[k % 7]
    assert (f32.astype(np.float64) != rp.b["ep_total"]).sum() > 20
