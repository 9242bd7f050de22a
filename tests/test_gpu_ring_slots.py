"""The ring and pool residues of the window's kernels against Python's own % on the same counter.

The kernels reduce the device step counter by host-precomputed constants (csrc/fastdiv.hpp) and wrap
window-local offsets with a compare.  Here the counter is written through the `ctl` buffer view to values on
both sides of 2^31, 2^32 and 2^40, and R + 1 windows run from each with pool lengths 3 and 7 (neither a power
of two, neither a divisor of R = 9: both residues wrap, at different steps).  After every window: the ring
planes and nvalid sit where k % R says, the rewards / dones / reset flags are those of pool entry k % P, and
the window's logits and values match the oracle fed the same frames; the first window's gradient matches the
oracle at the tolerances of test_gpu_stages.py.  Net: 3 envs, t_max 5, the smallest shape with a ring and a
window; one case each for the RGB (Doom, 160 wide) and the whole-stack layouts."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
from conftest import close_normscaled, grads_match
from sim import make_pools, make_rgb_pools
from stage_ref import ring_starts

pytestmark = pytest.mark.gpu

RTOL = 1e-5                    # test_gpu_stages.py's
N, T, A = 3, 5, 4
R = T + 4
PMAX = 7
CTL_STEP = 0
STARTS = [0, R - 1, 2 ** 31 - 2, 2 ** 32 - 3, (2 ** 40 + 1) // T * T]


@functools.lru_cache(maxsize=None)
def pools(layout):
    """The 7-entry pools of a layout (their first 3 entries serve pool_len 3) and each entry's uint8 planes as
    the ring should hold them: computed once, shared by every case, never written."""
    rng = np.random.default_rng({"ring": 5, "rgb": 6, "stack": 7}[layout])
    if layout == "rgb":
        obs, rewards, dones = make_rgb_pools(rng, PMAX, N, 120, 160, p_done=0.2)
        planes = np.stack([[O.rgb_screen_u8(obs[j, e]) for e in range(N)] for j in range(PMAX)])   # (P, N, 3, 84, 84)
        assert (O.PHI_LUT[planes[0, 0]] == O.rgb_phi(obs[0, 0])).all()   # the state the oracle's phi gives
    elif layout == "stack":
        rewards = rng.choice(np.array([-2.0, 0.0, 1.0, 3.5], np.float32), (PMAX, N))
        dones = (rng.random((PMAX, N)) < 0.2).astype(np.uint8)
        obs = rng.integers(0, 256, (PMAX, N, 4, 84, 84), dtype=np.uint8)
        planes = obs
    else:
        obs, rewards, dones = make_pools(rng, PMAX, N, "uniform", p_done=0.2)
        planes = np.stack([[O.current_screen(obs[j, e, 0], obs[j, e, 1]) for e in range(N)] for j in range(PMAX)])
    for a in (obs, rewards, dones, planes):
        a.setflags(write=False)
    return obs, rewards, dones, planes


def make_net(layout, T=T):
    from asyncrl_amd import A3CFF, DoomA3CFF
    if layout == "rgb":
        return DoomA3CFF(A, n_envs=N, t_max=T, seed=11, init_seed=3).net
    return A3CFF(A, n_envs=N, t_max=T, seed=11, init_seed=3, frames="stacks" if layout == "stack" else "pairs").net


def dev_acts(net, T=T):
    a1 = net.buffer("a1", torch.float32, (T + 1, N, 16, 20, 20))[:T].cpu().numpy()
    a2 = net.buffer("a2", torch.float32, (T + 1, N, 32, 9, 9))[:T].cpu().numpy()
    h = net.buffer("hfc", torch.float32, (T + 1, N, 256))[:T].cpu().numpy()
    return a1.reshape(T * N, 16, 20, 20), a2.reshape(T * N, 32, 9, 9), h.reshape(T * N, 256)


def run_case(gpu, layout, start, P, windows=None, T=T):
    R = T + 4
    windows = R + 1 if windows is None else windows
    obs, rewards, dones, planes = pools(layout)
    arch = O.ARCH_FF | (O.ARCH_RGB if layout == "rgb" else 0)
    net = make_net(layout, T)
    net.reset()
    ctl = net.buffer("ctl", torch.int64)
    ctl[CTL_STEP] = start
    dp, dr, dd = (torch.from_numpy(np.array(x[:P])).to(gpu) for x in (obs, rewards, dones))
    params = net.state_dict()
    per = {"ring": (84, 84), "rgb": (3, 84, 84), "stack": (4, 84, 84)}[layout]
    frames = net.buffer("frames", torch.uint8, (R, N) + per)
    nvalid = net.buffer("nvalid", torch.uint8, (R, N))
    k0 = start                       # Python's mirror of the counter
    nv = np.zeros(N, np.int64)       # planes since the env's last reset, as ale.py's deque has them
    state = {}                       # obs step -> (N, C, 84, 84) f32 state the oracle is fed
    prev_reset = None
    for w in range(windows):
        want_reset = np.zeros((T + 1, N), np.uint8)
        for t in range(T + 1):
            k = k0 + t
            if w == 0 or t >= 1:
                forced = w == 0 and t == 0
                net.observe(t, dp, dr, dd, P, force_reset=forced)
                rs = np.ones(N, bool) if forced else dones[k % P] != 0
                nv = np.where(rs, 1, np.minimum(nv + 1, 4))
                want_reset[t] = rs
                if layout == "ring":
                    s = np.zeros((N, 4, 84, 84), np.uint8)
                    for e in range(N):
                        for c in range(4 - nv[e], 4):
                            s[e, c] = planes[(k - 3 + c) % P, e]
                    state[k] = O.PHI_LUT[s]
                else:
                    state[k] = O.PHI_LUT[planes[k % P]]
                state[k] = (state[k], nv.copy())
            else:
                want_reset[0] = prev_reset
            net.act(t, mode=1 if t < T else 0)
        torch.cuda.synchronize()
        assert int(ctl[CTL_STEP]) == k0
        fr, nvd = frames.cpu().numpy(), nvalid.cpu().numpy()
        # ---- the ring, by Python's %: every observation of the window sits in slot k % R, with its nvalid
        for t in range(T + 1):
            k = k0 + t
            x, nvk = state[k]
            assert (fr[k % R] == planes[k % P]).all(), (w, t, "plane")
            if layout == "ring":
                assert (nvd[k % R] == nvk).all(), (w, t, "nvalid", nvd[k % R], nvk)
                got = O.state_from_ring(fr, nvd[k % R], [(k - 3 + c) % R for c in range(4)])
                assert (got == x).all(), (w, t, "stack")
            else:
                assert (nvd[k % R] == (3 if layout == "rgb" else 4)).all(), (w, t, "nvalid")
        # ---- what the ring kernel ingested: pool entry k % P
        rew = net.buffer("rewards", torch.float32, (T, N)).cpu().numpy()
        dn = net.buffer("dones", torch.uint8, (T, N)).cpu().numpy()
        rf = net.buffer("reset", torch.uint8, (T + 1, N)).cpu().numpy()
        idx = [(k0 + t + 1) % P for t in range(T)]
        assert (rew == rewards[idx]).all() and (dn == dones[idx]).all(), (w, "rewards / dones")
        assert (rf == want_reset).all(), (w, "reset flags", rf, want_reset)
        prev_reset = want_reset[T]
        # ---- the window's logits and values against the oracle on the same frames
        xs = np.stack([state[k0 + t][0] for t in range(T)])
        boot = state[k0 + T][0]
        logits = net.buffer("logits", torch.float32, (T + 1, N, A))[:T].cpu().numpy()
        v = net.buffer("v", torch.float32, (T + 1, N)).cpu().numpy()
        if w == 0:                   # and the gradient of one window per start
            net.learn()
            torch.cuda.synchronize()
            acts = net.buffer("actions", torch.int32, (T + 1, N))[:T].cpu().numpy()
            g, aux = O.ff_window_grads(params, xs, acts, rewards[idx], dones[idx], boot, arch=arch,
                                       dev_acts=dev_acts(net, T))
            want_l, want_v, want_b = aux["logits"], aux["v"], aux["vboot"]
            grads_match(net.state_dict(net.grads), g, aux["grad_mag"], rtol=RTOL, rtol_elem=RTOL)
        else:
            want_l, want_v, _ = O.pi_and_v_ff(params, xs.reshape((T * N,) + xs.shape[2:]), arch)
            want_l, want_v = want_l.reshape(T, N, A), want_v.reshape(T, N)
            _, want_b, _ = O.pi_and_v_ff(params, boot, arch)
        for what, a, b in (("logits", logits, want_l), ("v", v[:T], want_v), ("vboot", v[T], want_b)):
            ok, err = close_normscaled(a, b, RTOL)
            assert ok, (w, what, err)
        net.advance()
        k0 += T
        for k in [k for k in state if k < k0]:
            del state[k]
    torch.cuda.synchronize()
    assert int(ctl[CTL_STEP]) == start + windows * T


@pytest.mark.parametrize("P", [3, 7])
@pytest.mark.parametrize("start", STARTS)
def test_ring_slots_follow_the_counter(gpu, start, P):
    run_case(gpu, "ring", start, P)


@pytest.mark.parametrize("start", ring_starts(33))
def test_ring_slots_follow_the_counter_in_a_long_ring(gpu, start):
    """t_max 33: a ring of R = 37 slots, its fd_make(37) residues with the counter at R - 1, 2^32 - 3 and a
    multiple of T above 2^40 (stage_ref.ring_starts), pool length 7 (no divisor of 37; 33 steps wrap it four
    times), two windows, the second across the ring's end."""
    assert start % 37 and 37 % PMAX and 33 % PMAX
    run_case(gpu, "ring", start, PMAX, windows=2, T=33)


@pytest.mark.parametrize("layout", ["rgb", "stack"])
def test_ring_slots_rgb_and_stack_layouts(gpu, layout):
    run_case(gpu, layout, 2 ** 32 - 3, PMAX)
