"""GPU: whole windows at t_max = 33 and 64 and at the action counts on the edges of the heads' 16-column tiles,
through the helpers of the modules that hold the short cases (test_gpu_parity, test_gpu_gae, test_gpu_window_stats,
test_gpu_episode_stats) at their tolerances: 1e-5 norm-scaled and componentwise against the oracle, bit for bit
against the float64 replays.  tests/long_cases.py has the cases and their pools; tests/test_long_windows_ref.py
shows on the CPU that the inputs hold the conditions the cases exist for and that each mistake they are meant to
catch misses the tolerance by more than 10x on the reference alone.

| case                              | what only it reaches                                                          |
|-----------------------------------|-------------------------------------------------------------------------------|
| FF ring (3, 64, 4), 2 windows     | frame ring of R = 68 slots, conv_fwd / conv_bwd slot addressing to t = 64,    |
|                                   | policy_fc_returns_kernel's second row pass on a rollout's own operands        |
| FF f32 states (5, 33, 6), GAE     | the states ring of 37 slots, the 32-row GAE form with one row in pass two     |
| Nature (3, 33, 6), 2 windows      | returns_kernel at EB = 256 / 33 = 7 envs a workgroup                          |
| Nature (2, 64, 4), GAE            | returns_kernel at EB = 4, its GAE scan over 64 rows                           |
| LSTM (3, 64, 6), 2 windows        | 63 lstm_bptt launches, hbuf / cbuf of 66 rows, advance_kernel's row 64 -> 0,  |
|                                   | window two from the carried h, c and reset flags                              |
| LSTM (5, 33, 6), GAE              | returns_heads_kernel's 32-row GAE form feeding the BPTT chain                 |
| LSTM (3, 33, 6), lateral W x 4    | cell states up to 0.45 (0.1 at init_like_torch weights) through 32 steps      |
| window record (5, 64), (260, 10)  | window_stats_kernel's 65,536-byte LDS request; two envs a thread in the       |
|                                   | memory path                                                                   |
| A = 16, 31 (FF), 17 (LSTM),       | the value column alone in / at the end of the heads' second 16-column tile,   |
| 15 (Nature)                       | policy_rows16's second zs pass; the Nature heads GEMM's one exact M tile      |
"""
import numpy as np
import pytest
import torch

import long_cases as L
import oracle as O
import stage_ref as R
import test_gpu_episode_stats as EP
import test_gpu_gae as GAE
import test_gpu_parity as PAR
import test_gpu_ppo as PPO
import test_gpu_ppo_lstm as PPOL
import test_gpu_ppo_options as PPOO
import test_gpu_tmaze as TM
import test_gpu_window_stats as WS
from episode_replay import Replay
from gae_replay import gae_adv, replay_adv_sums
from window_replay import NAMES, case_pools, replay, same_bits

pytestmark = pytest.mark.gpu

F = {k: i for i, k in enumerate(NAMES)}


def ids(cases):
    return [c[0] for c in cases]


# ------------------------------------------------------------------ whole windows against the oracle
@pytest.mark.parametrize("case", L.FF_CASES, ids=ids(L.FF_CASES))
def test_ff_long_windows_match_oracle(gpu, case):
    """test_gpu_parity._run_ff's checks (logits, v, the bootstrap value, dlogits, dv, the actions against the
    Philox draws, every gradient tensor, the clip + RMSProp delta) on pools of T + 2 entries with crafted
    terminals: an env that never ends an episode, terminals at steps 0, T - 1 and past step 32.

    nature-N2-T64-A4-gae is the suite's first whole window in which the clip at 40 is active (gradient norm 41.34)
    on a net whose update takes the norm from grad_sqnorm_kernel.  With that kernel's per-thread sums in f32 the
    f32 clip scale came out one ulp from the oracle's (an f64 norm), 98 of conv2's 32,768 updated parameters
    landed one f32 ulp of the largest parameter away (3.7e-9), and that is 1.39e-5 of the tensor's largest step
    (2.68e-4): the delta check failed at 1.391e-5 on conv2's weight and 1.004e-5 on conv1's.  The kernel now sums
    in f64 (test_long_windows_ref.test_delta_check_floor_of_the_nature_gae_case sizes the effect on the oracle
    alone); this case is its regression test."""
    _, arch, N, T, A, lam, windows, kind = case
    pools = L.pools(kind, N, T)
    d = L.window_dones(pools[2], 0, T)
    assert R.crafted_flags_hold(d) and pools[0].shape[0] == T + 2 and (T + 4) % (T + 2) and (T + 2) % (T + 4)
    PAR._run_ff(gpu, N=N, T=T, A=A, seed=60 + T, kind=kind, windows=windows, arch=arch, pools=pools, lam=lam)


@pytest.mark.parametrize("case", L.LSTM_CASES, ids=ids(L.LSTM_CASES))
def test_lstm_long_windows_match_oracle(gpu, case):
    """test_gpu_parity._run_lstm's checks (v, the bootstrap value, hbuf[T], logits, dlogits, dv, the actions,
    every gradient tensor) on the crafted pools.  oracle.lstm_window runs its BPTT in float32; the float32
    restatement of the chain is within 2.9e-7 of the scale of the float64 one over 64 steps
    (tests/test_long_windows_ref.py), so the suite's 1e-5 is kept as it stands."""
    _, N, T, A, lam, windows, lateral = case
    pools = L.pools("palette", N, T)
    assert R.crafted_flags_hold(L.window_dones(pools[2], 0, T))
    if windows > 1:   # window two starts with a carried reset flag on env 1 and carried h, c on env 0
        assert L.window_dones(pools[2], 0, T)[T - 1, 1] and not L.window_dones(pools[2], 1, T)[:, 0].any()
    PAR._run_lstm(gpu, False, N, T, A, windows=windows, pools=pools, lam=lam, lateral_scale=lateral)


@pytest.mark.parametrize("case", L.EDGE_CASES, ids=ids(L.EDGE_CASES))
def test_windows_at_the_head_tile_edges(gpu, case):
    """One window each at A = 16 (the value column alone in the second 16-column tile; policy_rows16's zs loop
    takes its second pass, the bias read directly), A = 31 (value column 31 of the second tile), A = 17 on the
    LSTM and A = 15 on the Nature head (value column 15: the first tile exactly full)."""
    _, net, N, T, A = case
    if net == "lstm":
        PAR._run_lstm(gpu, False, N, T, A, windows=1)
    else:
        PAR._run_ff(gpu, N=N, T=T, A=A, seed=70 + A, kind="uniform", windows=1, p_done=0.2,
                    arch=O.ARCH_FF_NATURE if net == "nature" else O.ARCH_FF)


# ------------------------------------------------------------------ statistics
def _record_check(net, s, w, step, T, lam, samples):
    """Fields 0..13 bit for bit against the replay (12, 13 over the GAE advantage at lam), the norm against the
    float64 squared norm of the gradient."""
    rec = net.window_stats_raw()[0]
    want = np.concatenate([[float(w), float(step)],
                           replay(s["rewards"], s["dones"], s["v"], s["entropy"], s["loss"], GAE.GAMMA, True)])
    if lam is not None:
        adv = gae_adv(s["rewards"], s["dones"], s["v"][:T], s["v"][T], GAE.GAMMA, lam, True)
        want[12], want[13] = replay_adv_sums(adv, s["dones"])
    bad = [(NAMES[i], rec[i], want[i]) for i in range(14) if not same_bits(np.float64(rec[i]), np.float64(want[i]))]
    assert not bad, (w, lam, bad)
    WS.check_norm(rec, s)
    assert rec[F["samples"]] == samples


@pytest.mark.parametrize("lam", [None, 0.95], ids=["nstep", "gae"])
def test_window_record_at_64_steps(gpu, lam):
    """5 envs, t_max 64, two windows, the second truncated to 33 steps: window_stats_kernel's memory path with
    R_t columns of 64 x 256 floats, a dynamic LDS request of exactly 65,536 bytes, in both of its forms."""
    n, T, A, P = 5, 64, 4, 66
    rewards, dones = case_pools(9, P, n)
    pools = (GAE.pair_pool(P, n, gpu), GAE.dev(rewards, gpu), GAE.dev(dones, gpu))
    net = GAE.make_net(A, n, T, gpu, lam, stats=True)
    for w in range(2):
        GAE.manual_window(net, pools, P, w == 0, truncate=33 if w == 1 else None)
        _record_check(net, GAE.snapshot(net), w, w * T, T, lam, (T if w == 0 else 33) * n)


@pytest.mark.parametrize("lam", [None, 0.95], ids=["nstep", "gae"])
def test_window_record_memory_path_past_256_envs(gpu, lam):
    """260 envs, t_max 10 (the memory path), whole stacks as the observation: threads 0..3 own two envs each and
    reuse their LDS column for the second."""
    n, T, A, P = 260, 10, 4, 12
    rewards, dones = case_pools(10, P, n)
    g = torch.Generator(device="cpu").manual_seed(12)
    stacks = torch.randint(0, 256, (P, n, 4, 84, 84), dtype=torch.uint8, generator=g).to(gpu)
    pools = (stacks, GAE.dev(rewards, gpu), GAE.dev(dones, gpu))
    net = GAE.make_net(A, n, T, gpu, lam, stats=True, stack=True)
    for w in range(2):
        GAE.manual_window(net, pools, P, w == 0)
        _record_check(net, GAE.snapshot(net), w, w * T, T, lam, T * n)


def test_episode_statistics_over_33_step_windows(gpu):
    """The episode statistics over the two 33-step windows of the Nature case's pools (episodes that span a
    whole window on env 0, end at its first and last step on env 1), bit for bit against episode_replay."""
    from asyncrl_amd._lib import ARCH_FF_NATURE
    _, _, N, T, A, _, windows, kind = L.FF_CASES[2]
    assert T == 33 and windows == 2
    obs, rewards, dones = L.pools(kind, N, T)
    P = obs.shape[0]
    pools = (EP.dev(obs, gpu), EP.dev(rewards, gpu), EP.dev(dones, gpu))
    net = EP.make_net(ARCH_FF_NATURE, A, N, T, gpu)
    net.set_episode_stats(True)
    EP.manual_windows(net, pools, P, 0, windows)
    rp = Replay(N).run(rewards, dones, 1, windows * T + 1)
    assert rp.b["ep_count"][0] == 0 and rp.b["ep_count"][1] >= 3
    EP.assert_matches(net, rp)


# ------------------------------------------------------------------ PPO epochs and the drop-in at long windows
PPO_LONG = (5, 33, 6)
# The update between the epochs, picked on the CPU oracle as test_gpu_ppo.test_epoch_two_against_the_oracle's
# docstring describes (its window on these pools with the Philox actions at seed 99, the GAE advantage, clip 40 --
# the norm is 552 -- and one oracle RMSProp step): ratios 0.921 .. 1.132 at lr 2e-3 (none of 165 inactive), 0.806 ..
# 1.333 at 5e-3 (5.5 %), 0.629 .. 1.563 at 8e-3 (35.2 %), 0.060 .. 2.526 at 2e-2 (52.1 %): test_gpu_ppo's LR2 serves.
PPO_LONG_LR = PPO.LR2


def test_ppo_epoch_two_against_the_oracle_over_33_steps(gpu):
    """test_gpu_ppo.test_epoch_two_against_the_oracle's body at (5, 33, 6): the re-forward of 33 slots and the PPO
    form's second row pass on a rollout's snapshot; "some but not all samples inactive" asserted on the reference."""
    PPO.epoch_two_against_the_oracle(gpu, PPO_LONG, PPO_LONG_LR)


def test_ppo_options_epoch_two_over_33_steps(gpu):
    """test_gpu_ppo_options.test_net_epoch_two's body at (5, 33, 6), advantage normalisation and value clipping on."""
    PPOO.net_epoch_two(gpu, PPO_LONG, PPO_LONG_LR)


def test_ppo_lstm_reforward_over_33_steps(gpu):
    PPOL.reforward_is_the_forward(gpu, PPOL.LONG)


@pytest.mark.parametrize("fused", [True, False], ids=["optimize_advance", "optimize-then-advance"])
def test_ppo_lstm_carry_over_33_steps(gpu, fused):
    """ppo_state.hip's carry of rows 33 of hbuf / cbuf into rows 0."""
    PPOL.carry_is_the_rollouts_state(gpu, fused, PPOL.LONG)


def test_ppo_lstm_carry_after_a_window_truncated_to_20_of_33_steps(gpu):
    PPOL.carry_after_a_truncated_window(gpu, PPOL.LONG, PPOL.LONG_TRUNCATE)


def test_dropin_act_with_a_33_step_window_closed_at_step_20(gpu):
    """test_gpu_gae.test_dropin_act_with_a_truncated_window's body at t_max 33: a terminal 20 steps into the first
    window (13 rows past its end, the second row pass all dead), then a full window of 33."""
    GAE.dropin_truncated_window(gpu, T=33, cut=20)


# ------------------------------------------------------------------ the device env loop and a captured window
@pytest.mark.parametrize("what", ["closed_loop", "direct", "direct_graph"])
def test_tmaze_longest_corridor_in_windows_of_20(gpu, what):
    """T-maze of length 8, the longest DeviceTMaze builds (16 px a cell on a 160 px screen; it refuses more): an
    episode of 9 steps, t_max 20, so every window holds two terminals that move through it; LSTM with 6 actions,
    33 envs: the closed loop against host-driven windows over 3 windows, and the direct mode against the pairs
    path, eagerly and with one captured window replayed -- bit for bit, as at t_max 5."""
    if what == "closed_loop":
        TM.closed_loop(gpu, "lstm", 6, 33, {}, 8, T=20, windows=3)
    else:
        TM.direct_mode(gpu, "lstm", 6, 33, 8, what == "direct_graph", T=20, windows=3)


def test_tmaze_refuses_a_corridor_of_16(gpu):
    from asyncrl_amd import DeviceTMaze
    with pytest.raises(ValueError, match="length must be in 1..8"):
        DeviceTMaze(33, device=gpu, seed=5, length=16)


def test_graph_replay_equals_eager_at_64_steps(gpu):
    """test_gpu_parity.test_graph_replay_equals_eager's body on an FF net of 2 envs at t_max 64: one captured
    window of several hundred graph nodes, three replays."""
    PAR.graph_replay_equals_eager(gpu, 2, 64, 66)
