"""CPU: the device-side window statistics' host pieces -- the two C symbols and the two
constants in the header and the ctypes table, the workspace entries, the rank merge, the
host-derived figures, and the NumPy replay the GPU tests compare against
(window_replay.replay) checked against the oracle's returns and advantages."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from window_replay import FIELDS, LOG, NAMES, SUMS, replay, same_bits, window_case

HEADER = os.path.join(ROOT, "include", "asyncrl_hip.h")
SYMBOLS = ("arl_net_set_window_stats", "arl_window_stats_reset")


def test_symbols_declared_bound_and_exported():
    import asyncrl_amd
    from asyncrl_amd import _lib
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert s in _lib.SIGNATURES and hasattr(_lib.lib, s), s
    assert re.search(r"#define\s+ARL_WINDOW_LOG\s+64\b", code)
    assert re.search(r"#define\s+ARL_WINDOW_STAT_FIELDS\s+17\b", code)
    assert _lib.WINDOW_LOG == LOG == 64 and _lib.WINDOW_STAT_FIELDS == FIELDS == 17
    assert _lib.WINDOW_STAT_NAMES == NAMES and len(NAMES) == FIELDS
    assert _lib.lib.arl_abi_version() == 4                      # additions to ABI 4
    assert callable(asyncrl_amd.window_stats_dict)
    for m in ("set_window_stats", "window_stats_reset", "window_stats_raw"):
        assert callable(getattr(asyncrl_amd.DeviceNet, m)), m
    assert callable(asyncrl_amd.A3C.window_stats)


def test_unbound_net_is_estate_and_workspace_names_the_buffers():
    from asyncrl_amd._lib import lib
    h = ctypes.c_void_p()
    assert lib.arl_net_create(ctypes.byref(h), 0, 4, 40, 5, 0, 0) == 0
    try:
        assert lib.arl_net_set_window_stats(h, 1) == 3
        assert lib.arl_window_stats_reset(h, None) == 3
        off, nb = ctypes.c_int64(), ctypes.c_int64()
        where = {}
        for name in ("win_log", "win_count", "ep_run_ret"):
            assert lib.arl_net_buffer(h, name.encode(), ctypes.byref(off), ctypes.byref(nb)) == 0, name
            assert off.value % 256 == 0, name
            where[name] = (off.value, nb.value)
        assert where["win_log"][1] == LOG * FIELDS * 8 and where["win_count"][1] == 8
        assert where["win_log"][0] + where["win_log"][1] <= where["win_count"][0]
        assert where["win_count"][0] + 256 <= where["ep_run_ret"][0]      # its own 256-byte slot, before the episodes
        fake = 1 << 40                                                     # bound to fake memory: host checks only
        assert lib.arl_net_bind(h, fake, fake, fake, fake) == 0
        assert lib.arl_net_set_window_stats(h, 1) == 0 and lib.arl_net_set_window_stats(h, 0) == 0
    finally:
        lib.arl_net_destroy(h)


def test_merge_window_stats():
    from asyncrl_amd.distributed import merge_window_stats
    a = [3.0, 15.0, 200.0, 7.0, 12.5, 0.3, 0.7, 250.0, 10.0, 30.0, 11.0, 40.0, 1.0, 9.0, 1600.5, 0.75, 6.5e-4]
    b = [3.0, 15.0, 195.0, 0.0, -2.0, 0.1, 0.2, 240.0, -4.0, 20.0, -3.0, 25.0, 1.5, 6.0, 1600.5, 0.75, 6.5e-4]
    c = [3.0, 15.0, 200.0, 1.0, 0.3, -0.6, 0.4, 10.0, 0.5, 1.0, 0.25, 2.0, -0.5, 3.0, 1600.5, 0.75, 6.5e-4]
    assert merge_window_stats([a]) == a
    got = merge_window_stats([a, b, c])
    for i in (0, 1, 14, 15, 16):
        assert got[i] == a[i]
    for i in range(2, 14):
        assert got[i] == (a[i] + b[i]) + c[i], i                  # rank order
    assert got[2] == 595.0 and got[3] == 8.0
    assert merge_window_stats([np.array(a), np.array(b)])[2] == 395.0
    for i in (0, 1, 14, 15, 16):                                   # what every rank must agree on
        bad = list(b)
        bad[i] = bad[i] + 1.0
        with pytest.raises(ValueError):
            merge_window_stats([a, bad])
    with pytest.raises(ValueError):
        merge_window_stats([])
    with pytest.raises(ValueError):
        merge_window_stats([a[:16]])
    with pytest.raises(ValueError):
        merge_window_stats([a, b + [0.0]])


def test_host_derived_figures():
    from asyncrl_amd.net import window_stats_dict
    R = [1.0, 2.0, 4.0, -1.0]
    v = [0.5, 2.5, 3.0, 0.0]
    adv = [r - x for r, x in zip(R, v)]
    row = [9.0, 45.0, 4.0, 1.0, 2.5, 0.75, 0.5, 5.0, sum(v), sum(x * x for x in v), sum(R), sum(x * x for x in R),
           sum(adv), sum(x * x for x in adv), 6400.0, 0.5, 6e-4]
    d = window_stats_dict(row)
    for k in ("window", "step", "samples", "terminals"):
        assert type(d[k]) is int
    assert (d["window"], d["step"], d["samples"], d["terminals"]) == (9, 45, 4, 1)
    assert all(d[k] == x for k, x in zip(NAMES, row))
    assert d["entropy"] == 1.25 and d["value_mean"] == 1.5 and d["return_mean"] == 1.5 and d["adv_mean"] == 0.0
    var = lambda xs: sum((x - sum(xs) / 4) ** 2 for x in xs) / 4   # noqa: E731
    assert abs(d["explained_variance"] - (1 - var(adv) / var(R))) < 1e-12
    assert d["grad_norm"] == 80.0 and d["clipped"] is True and d["total_loss"] == 1.25
    same = list(row)                                               # every return equal: Var(R) = 0
    same[10], same[11] = 8.0, 16.0
    e = window_stats_dict(same)
    assert math.isnan(e["explained_variance"]) and e["return_mean"] == 2.0
    z = window_stats_dict([2.0, 10.0] + [0.0] * 12 + [4.0, 1.0, 7e-4])   # no live sample
    for k in ("entropy", "value_mean", "return_mean", "adv_mean", "explained_variance"):
        assert math.isnan(z[k]), k
    assert z["samples"] == 0 and z["clipped"] is False and z["grad_norm"] == 2.0
    with pytest.raises(ValueError):
        window_stats_dict(row[:16])


def ordered_sum(x, live):
    """sum over live (t, e) of x in the record's order for n <= 256 envs: one partial per
    env over t ascending from 0.0, the partials then added to env 0's in env order."""
    T, n = x.shape
    parts = []
    for e in range(n):
        s = 0.0
        for t in range(T):
            if live[t, e]:
                s = s + float(x[t, e])
        parts.append(s)
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


@pytest.mark.parametrize("clip_reward", [True, False])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_replay_against_the_oracle(seed, clip_reward):
    """T = 5, n = 7, rewards outside [-1, 1]; terminals at t = 0, at T - 1, consecutive, one
    column truncated from t = 3: the replay's return / advantage / reward sums equal the
    same-order f64 sums of oracle.returns_and_lossgrad's Rs and adv bit for bit."""
    import oracle as O
    T, n = 5, 7
    c = window_case(seed, T, n)
    live = (c["dones"] & 2) == 0
    assert not live[3:, 3].any() and live.sum() == T * n - 2
    probs, logp = O.softmax(c["logits"].reshape(T * n, -1)), O.log_softmax(c["logits"].reshape(T * n, -1))
    Rs, adv, *_ = O.returns_and_lossgrad(c["rewards"], c["dones"], c["v"][:T], c["v"][T], probs.reshape(T, n, -1),
                                         logp.reshape(T, n, -1), c["actions"], gamma=0.99, clip_reward=clip_reward,
                                         valid=live)
    assert Rs.dtype == np.float32 and adv.dtype == np.float32
    got = dict(zip(SUMS, replay(c["rewards"], c["dones"], c["v"], c["entropy"], c["loss"], 0.99, clip_reward)))
    r64 = c["rewards"].astype(np.float64)
    r64 = np.clip(r64, -1, 1) if clip_reward else r64
    Rd, ad = Rs.astype(np.float64), adv.astype(np.float64)
    want = {"reward_sum": ordered_sum(r64, live), "return_sum": ordered_sum(Rd, live),
            "return_sumsq": ordered_sum(Rd * Rd, live), "adv_sum": ordered_sum(ad, live),
            "adv_sumsq": ordered_sum(ad * ad, live)}
    for k, x in want.items():
        assert same_bits(np.float64(got[k]), np.float64(x)), (k, got[k], x)
    assert got["samples"] == live.sum() and got["terminals"] == (live & ((c["dones"] & 1) != 0)).sum() >= 5
    vd = c["v"][:T].astype(np.float64)
    assert same_bits(np.float64(got["value_sum"]), np.float64(ordered_sum(vd, live)))
    assert same_bits(np.float64(got["value_sumsq"]), np.float64(ordered_sum(vd * vd, live)))
    assert same_bits(np.float64(got["entropy_sum"]), np.float64(ordered_sum(c["entropy"][:T].astype(np.float64), live)))
    lo = c["loss"].astype(np.float64)
    assert got["pi_loss"] == sum(lo[1:, 0], lo[0, 0]) and got["v_loss"] == sum(lo[1:, 1], lo[0, 1])
    # the clip shows: without it some |r| > 1 enters the sum
    if not clip_reward:
        assert np.abs(c["rewards"]).max() > 1 and got["reward_sum"] != ordered_sum(np.clip(r64, -1, 1), live)


def test_replay_strides_past_256_envs():
    """n = 300: thread j's partial holds envs j and j + 256 before the combine."""
    rng = np.random.default_rng(5)
    T, n = 2, 300
    v = rng.standard_normal((T + 1, n)).astype(np.float32)
    ent = rng.random((T + 1, n)).astype(np.float32)
    loss = rng.standard_normal((n, 2)).astype(np.float32)
    rewards = rng.standard_normal((T, n)).astype(np.float32)
    dones = np.zeros((T, n), np.uint8)
    got = replay(rewards, dones, v, ent, loss)
    lo = loss[:, 0].astype(np.float64)
    parts = [(0.0 + lo[j]) + lo[j + 256] if j + 256 < n else 0.0 + lo[j] for j in range(256)]
    want = parts[0]
    for p in parts[1:]:
        want = want + p
    assert got[3] == want and got[0] == T * n
    plain = 0.0
    for e in range(n):
        plain = plain + lo[e]
    assert abs(got[3] - plain) < 1e-9
