"""GPU: single window stages (arl_run_stage) on synthetic operands written into
the workspace, against the float64 references of tests/stage_ref.py -- at the
window sizes where the backward kernels change shape: more than one job A
sample range (the in-launch ticket reduce of fc_bwd.hip, for the FC layer and
the LSTM gate weights) and more than one sample per conv_bwd.hip workgroup;
and the three hot-path stages whose outputs are intermediate in a window:
conv_fwd (both LDS layouts, an idle env slot, three frame layouts, the a2
mask), one lstm_bptt step and the learner's whole BPTT chain, and the returns
launch in every instantiation the host picks, one and two row passes.

Tolerances are the suite's own (conftest): reduced tensors grads_match(rtol =
1e-5, rtol_elem = 1e-5) against the reference and its per-element scales,
non-reduced ones close_normscaled(1e-5) and exactly 0.0 under a zero ReLU mask.
tests/test_stage_ref.py shows on the CPU that every mistake these cases exist
for misses those bounds by more than 10x on the same data."""
import numpy as np
import pytest
import torch

import oracle as O
import stage_ref as R
from conftest import close_normscaled, grads_match

pytestmark = pytest.mark.gpu

RTOL = 1e-5
f32 = torch.float32


def put(net, name, arr, dtype=f32):
    arr = np.ascontiguousarray(arr)
    if arr.dtype == np.uint32:
        arr, dtype = arr.view(np.int32), torch.int32
    net.buffer(name, dtype).copy_(torch.from_numpy(arr.reshape(-1)))


def put_param(net, name, arr):
    net.param(name).copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    net.params_changed()


def get(net, name, shape):
    return net.buffer(name, f32, shape).cpu().numpy()


def check_grads(net, names, ref, mag):
    """The stage's tensors of the flat gradient against the reference; every other
    tensor still holds the prefill."""
    got = {k: net.grad(name).cpu().numpy() for k, name in names.items()}
    for k, v in got.items():
        assert np.isfinite(v).all() and not (v == R.PREFILL).any(), k
    grads_match(got, {k: ref[k].reshape(got[k].shape) for k in names},
                {k: mag[k].reshape(got[k].shape) for k in names}, rtol=RTOL, rtol_elem=RTOL)
    for name in net.layout:
        if name not in names.values():
            assert bool((net.grad(name) == R.PREFILL).all()), name


def check_masked(got, want, mask, what):
    ok, err = close_normscaled(got, want, RTOL)
    assert ok, (what, err)
    assert (got[~mask] == 0).all(), what


# ------------------------------------------------------------------ fc_bwd
def _fc_bwd(n_envs, t_max, Z, lstm=False):
    from asyncrl_amd import A3CFF, A3CLSTM
    d = R.fc_data(n_envs, t_max, lstm=lstm)
    S, T = d["S"], t_max
    net = (A3CLSTM if lstm else A3CFF)(d["A"], n_envs=n_envs, t_max=t_max, init_seed=0, frames="pairs").net
    net.reset()
    assert R.ranges(S)[0] == Z
    assert net.buffer("fc_bwd_partials", f32).numel() == R.part_floats(S)
    a2 = d["a2"][:T].reshape(S, R.A2)
    put(net, "a2", d["a2"])
    words = R.pack_a2_mask(d["a2"])
    words[T] = 0xFFFFFFFF
    put(net, "a2_mask", words)
    if lstm:   # the heads read hbuf slot t + 1; nothing of this stage reads hfc
        put(net, "hbuf", d["hbuf"])
        net.buffer("hfc", f32).fill_(float(R.SENTINEL))
        names = {"fcW": "0/2/W", "fcb": "0/2/b", "piW": "2/0/W", "pib": "2/0/b", "vW": "3/0/W", "vb": "3/0/b"}
    else:
        put(net, "hfc", d["hfc"])
        names = {"fcW": "0/2/W", "fcb": "0/2/b", "piW": "1/0/W", "pib": "1/0/b", "vW": "2/0/W", "vb": "2/0/b"}
    put(net, "dlogits", d["dlogits"])
    put(net, "dv", d["dv"])
    put_param(net, "0/2/W", d["W"])
    for k in range(R.LAUNCHES if Z > 1 else 1):   # in a row: a stale slot or an un-re-armed ticket shows
        dfc = d["fresh_dfc"](k)
        put(net, "dfc", dfc)
        net.grads.fill_(R.PREFILL)
        net.buffer("da2", f32).fill_(R.PREFILL)
        net.run_stage("fc_bwd")
        torch.cuda.synchronize()
        ref, mag = R.fc_bwd_ref(dfc, a2, d["W"], d["dlogits"], d["dv"], d["hh"])
        check_grads(net, names, ref, mag)
        check_masked(get(net, "da2", (S, R.A2)), ref["da2"], a2 > 0, ("da2", k))


@pytest.mark.parametrize("n_envs,t_max,Z", [c + (z,) for c, z in zip(R.FC_CASES, (1, 1, 1, 2, 2, 3))])
def test_fc_bwd_stage(gpu, n_envs, t_max, Z):
    """FF net, S = 1, 129 (one past the 128-sample f64 flush; the last job B tile
    has one row), 1199 (the largest Z = 1), 1200 (the first Z = 2), 1205 (ranges
    of 608 / 597 samples, the second ending mid-chunk), 2000 (Z = 3: the pairwise
    slot loop clamps its second slot).  Z > 1: four launches in a row."""
    _fc_bwd(n_envs, t_max, Z)


def test_fc_bwd_stage_lstm_arch(gpu):
    """The same stage on an LSTM net: the heads' weight gradients read hbuf slot t + 1."""
    _fc_bwd(*R.FC_LSTM_ARCH_CASE, Z=1, lstm=True)


# ------------------------------------------------------------------ lstm_wgrad
@pytest.mark.parametrize("n_envs,t_max,Z", [c + (z,) for c, z in zip(R.LSTM_CASES, (1, 1, 1, 2, 3))])
def test_lstm_wgrad_stage(gpu, n_envs, t_max, Z):
    """S = 1, 129, 1024 (Z = 1 with a full LDS reset table), 1025 (Z = 2 from the
    reset table alone), 2000 (Z = 3).  The first and last sample of every range are
    reset rows (their h_prev DMA'd from the zero row).  Z > 1: four launches in a row."""
    from asyncrl_amd import A3CLSTM
    d = R.lstm_data(n_envs, t_max)
    S, T = d["S"], t_max
    net = A3CLSTM(4, n_envs=n_envs, t_max=t_max, init_seed=0, frames="pairs").net
    net.reset()
    assert R.ranges(S, lstm=True)[0] == Z
    assert net.buffer("fc_bwd_partials", f32).numel() == R.part_floats(S)
    hfc, hprev, reset = d["hfc"][:T].reshape(S, -1), d["hbuf"][:T].reshape(S, -1), d["reset"].reshape(-1)[:S]
    put(net, "hfc", d["hfc"])
    put(net, "hbuf", d["hbuf"])
    put(net, "reset", d["reset"], torch.uint8)
    put_param(net, "1/upward/W", d["Wu"])
    names = {"gWu": "1/upward/W", "gWl": "1/lateral/W", "gbu": "1/upward/b"}
    for k in range(R.LAUNCHES if Z > 1 else 1):
        dG = d["fresh_dG"](k)
        put(net, "dG", dG)
        net.grads.fill_(R.PREFILL)
        net.buffer("dfc", f32).fill_(R.PREFILL)
        net.run_stage("lstm_wgrad")
        torch.cuda.synchronize()
        ref, mag = R.lstm_wgrad_ref(dG, hfc, hprev, reset, d["Wu"])
        check_grads(net, names, ref, mag)
        check_masked(get(net, "dfc", (S, R.HID)), ref["dfc"], hfc > 0, ("dfc", k))


# ------------------------------------------------------------------ conv_bwd + conv_reduce
def _conv_bwd(n_envs, t_max, layout):
    from asyncrl_amd import A3CFF, DoomA3CFF
    d = R.conv_data(n_envs, t_max, layout)
    S = d["S"]
    if layout == "rgb":
        net = DoomA3CFF(3, n_envs=n_envs, t_max=t_max, init_seed=0).net
    else:
        net = A3CFF(4, n_envs=n_envs, t_max=t_max, init_seed=0, frames="stacks" if layout == "stack" else "pairs").net
    net.reset()
    assert net.buffer("slab", f32).numel() >= R.blocks(S) * 12336
    put(net, "frames", d["frames"], torch.uint8)
    put(net, "nvalid", d["nvalid"], torch.uint8)
    put(net, "a1", d["a1"])
    put(net, "da2", d["da2"])
    put_param(net, "0/1/W", d["W2"])
    net.grads.fill_(R.PREFILL)
    net.buffer("slab", f32).fill_(R.PREFILL)
    net.run_stage("conv_bwd")
    net.run_stage("conv_reduce")
    torch.cuda.synchronize()
    ref, mag = R.conv_bwd_ref(d["x"], d["a1"][:t_max].reshape(S, 16, 20, 20), d["da2"], d["W2"])
    check_grads(net, {"c2W": "0/1/W", "c2b": "0/1/b", "c1W": "0/0/W", "c1b": "0/0/b"}, ref, mag)


@pytest.mark.parametrize("n_envs,t_max", R.CONV_CASES)
def test_conv_bwd_stage(gpu, n_envs, t_max):
    """Ring layout, S = 1, 255 (below the 256-workgroup cap), 257 (only workgroup 0
    loops), 260 (workgroups 0..3 loop), 603 (3 / 2 samples a workgroup; the ring of
    13 slots wraps), 2565 (11 / 10 samples a workgroup, the bench's accumulation
    depth), and (3, 64): S = 192 samples of 64 steps in a ring of 68 slots (slot
    addressing at t up to 63, step 0's planes in slots 65 .. 67).  nvalid is drawn
    from 1..4 per (slot, env)."""
    _conv_bwd(n_envs, t_max, "ring")


@pytest.mark.parametrize("layout", ["rgb", "stack"])
def test_conv_bwd_stage_layouts(gpu, layout):
    """DoomA3CFF (planes [0, R, G, B], conv1 W (16, 3, 8, 8)) and a frames="stacks"
    net at S = 260."""
    _conv_bwd(*R.CONV_LAYOUT_CASE, layout)


# ------------------------------------------------------------------ forward stages, large-launch forms
def _fc_ref(p, a2):
    return np.maximum(R.mm64(a2, p["0/2/W"].T) + p["0/2/b"], 0.0)


def _close(got, want, what):
    ok, err = close_normscaled(got, want, RTOL)
    assert ok, (what, err)


@pytest.mark.parametrize("n_envs", [33, 512, 577])
def test_fc_fwd_policy_stages(gpu, n_envs):
    """fc_fwd + policy on an FF net at slots 0 and t_max against relu(a2 W^T + b) and
    the heads in float64: 32-row tiles (33 envs), and from 512 envs the 64-row
    tiles, whole (512) and with a one-row last tile (577)."""
    from asyncrl_amd import A3CFF
    N, T, A = n_envs, 2, 6
    net = A3CFF(A, n_envs=N, t_max=T, init_seed=0, frames="pairs").net
    net.reset()
    p = net.state_dict()
    for t in (0, T):
        a2 = np.full((T + 1, N, R.A2), R.SENTINEL, np.float32)
        a2[t] = R.act_like(np.random.default_rng([7, N, t]), (N, R.A2))
        put(net, "a2", a2)
        for name in ("hfc", "logits", "v"):
            net.buffer(name, f32).fill_(R.PREFILL)
        net.run_stage("fc_fwd", t)
        net.run_stage("policy", t)
        torch.cuda.synchronize()
        h = _fc_ref(p, a2[t])
        hfc = get(net, "hfc", (T + 1, N, R.HID))
        _close(hfc[t], h, ("hfc", t))
        _close(get(net, "logits", (T + 1, N, A))[t], h @ p["1/0/W"].T.astype(np.float64) + p["1/0/b"], ("logits", t))
        _close(get(net, "v", (T + 1, N))[t], (h @ p["2/0/W"].T.astype(np.float64))[:, 0] + p["2/0/b"], ("v", t))
        assert (np.delete(hfc, t, 0) == R.PREFILL).all()


@pytest.mark.parametrize("n_envs", [37, 577])
def test_fc_fwd_lstm_gates_stages(gpu, n_envs):
    """fc_fwd + lstm_gates of slot 1 on an LSTM net with ~20 % reset rows (their
    h / c carry a sentinel) against oracle.lstm_cell on the float64 FC: the
    split-K partials reduced in the gate kernel (37 envs) and by the FC's
    last-arriver ticket on 64-row tiles (577)."""
    from asyncrl_amd import A3CLSTM
    N, T, t = n_envs, 2, 1
    net = A3CLSTM(4, n_envs=N, t_max=T, init_seed=0, frames="pairs").net
    net.reset()
    p = net.state_dict()
    rng = np.random.default_rng([8, N])
    a2 = np.full((T + 1, N, R.A2), R.SENTINEL, np.float32)
    a2[t] = R.act_like(rng, (N, R.A2))
    reset = np.ones((T + 1, N), np.uint8)
    reset[t] = rng.random(N) < 0.2
    reset[t, 0], reset[t, N - 1] = 1, 0
    hbuf = np.full((T + 2, N, R.HID), R.SENTINEL, np.float32)
    cbuf = hbuf.copy()
    live = reset[t] == 0
    hbuf[t, live] = rng.normal(size=(int(live.sum()), R.HID)) * 0.5
    cbuf[t, live] = rng.normal(size=(int(live.sum()), R.HID))
    put(net, "a2", a2)
    put(net, "reset", reset, torch.uint8)
    put(net, "hbuf", hbuf)
    put(net, "cbuf", cbuf)
    for name in ("hfc", "gates"):
        net.buffer(name, f32).fill_(R.PREFILL)
    net.run_stage("fc_fwd", t)
    net.run_stage("lstm_gates", t)
    torch.cuda.synchronize()
    h = _fc_ref(p, a2[t])
    g, c, hn = O.lstm_cell(p, O.ARCH_LSTM, h.astype(np.float32), hbuf[t], cbuf[t], live)
    _close(get(net, "hfc", (T + 1, N, R.HID))[t], h, "hfc")
    _close(get(net, "gates", (T + 1, N, R.GATES))[t], g, "gates")
    _close(get(net, "cbuf", (T + 2, N, R.HID))[t + 1], c, "cbuf")
    _close(get(net, "hbuf", (T + 2, N, R.HID))[t + 1], hn, "hbuf")


# ------------------------------------------------------------------ conv_fwd
MASK_PREFILL = 0x5A5A5A5A


def _conv_fwd(n_envs, layout, t_max=1, slots=(0, 1)):
    from asyncrl_amd import A3CFF, DoomA3CFF
    d = R.conv_fwd_data(n_envs, layout, t_max=t_max)
    N, T = n_envs, t_max
    if layout == "rgb":
        net = DoomA3CFF(3, n_envs=N, t_max=T, init_seed=0).net
    else:
        net = A3CFF(4, n_envs=N, t_max=T, init_seed=0, frames="stacks" if layout == "stack" else "pairs").net
    net.reset()
    put(net, "frames", d["frames"], torch.uint8)
    put(net, "nvalid", d["nvalid"], torch.uint8)
    for name, key in (("0/0/W", "W1"), ("0/0/b", "b1"), ("0/1/W", "W2"), ("0/1/b", "b2")):
        put_param(net, name, d[key])
    for t in slots:
        sl = slice(t * N, (t + 1) * N)
        a1r, a2r, z1, z2 = R.conv_fwd_ref(d["x"][sl], d["W1"], d["b1"], d["W2"], d["b2"])
        net.buffer("a1", f32).fill_(R.PREFILL)
        net.buffer("a2", f32).fill_(R.PREFILL)
        net.buffer("a2_mask", torch.int32).fill_(MASK_PREFILL)
        net.run_stage("conv_fwd", t)
        torch.cuda.synchronize()
        a1 = get(net, "a1", (T + 1, N, 16, 20, 20))
        a2 = get(net, "a2", (T + 1, N, 32, 9, 9))
        words = net.buffer("a2_mask", torch.int32, (T + 1, N, R.A2W)).cpu().numpy().view(np.uint32)
        e2 = close_normscaled(R.conv1_split_model(d["xint"][sl], d["W1"], d["b1"], 2), a1r, RTOL)[1]
        e1d, e2d = close_normscaled(a1[t], a1r, RTOL)[1], close_normscaled(a2[t], a2r, RTOL)[1]
        print(f"conv_fwd {layout} N={N} T={T} t={t}: a1 {e1d:.3g} a2 {e2d:.3g} of the scale; a1 against the two-plane "
              f"model's {e2:.3g}: {e1d / e2:.3g}")
        for got, want, z, what in ((a1[t], a1r, z1, "a1"), (a2[t], a2r, z2, "a2")):
            assert not (got == R.PREFILL).any(), (what, t)
            _close(got, want, (what, t))
            sure = ~R.tie_band(z)
            assert (got[sure & (z < 0)] == 0).all() and (got[sure & (z > 0)] > 0).all(), (what, t)
        assert e1d <= e2 / 3, (t, e1d, e2)
        assert np.array_equal(words[t], R.pack_a2_mask(a2[t].reshape(N, R.A2))), t
        sure = ~R.tie_band(z2).reshape(N, R.A2)
        assert np.array_equal(R.unpack_a2_mask(words[t])[sure], (z2 > 0).reshape(N, R.A2)[sure]), t
        assert (np.delete(a1, t, 0) == R.PREFILL).all() and (np.delete(a2, t, 0) == R.PREFILL).all(), t
        assert (np.delete(words, t, 0) == MASK_PREFILL).all(), t


@pytest.mark.parametrize("n_envs,layout", R.CONV_FWD_CASES)
def test_conv_fwd_stage(gpu, n_envs, layout):
    """conv_fwd at slots 0 and 1 (the bootstrap slot) of a t_max = 1 net against
    conv_fwd_ref: 1, 5 envs (one env a workgroup), 512 and 513 (two a workgroup; 513:
    the last workgroup's second slot idle), the ring, RGB and stack frame layouts.
    a1 / a2 at 1e-5 of the scale and a1 within a third of the error a dropped low
    split plane of W1 makes (stage_ref.conv1_split_model); outside the tie band
    the ReLU decisions and the a2_mask bits are the reference's; a2_mask is the
    packed device a2 exactly; the other slot keeps its prefill."""
    _conv_fwd(n_envs, layout)


def test_conv_fwd_stage_long_ring(gpu):
    """The same checks on a t_max = 64 net, 3 envs, at slots 0, 63 and 64 (the bootstrap
    slot): the output rows of slots past 9 and a ring of R = 68 slots, where slot 0's
    three older planes sit in slots 65 .. 67.  Every other slot of a1 / a2 / a2_mask
    keeps its prefill."""
    n_envs, t_max, slots = R.CONV_FWD_LONG_CASE
    _conv_fwd(n_envs, "ring", t_max, slots)


# ------------------------------------------------------------------ lstm_bptt
@pytest.mark.parametrize("n_envs,t", R.BPTT_CASES)
def test_lstm_bptt_stage(gpu, n_envs, t):
    """One BPTT step t -> t - 1 of a t_max = 3 LSTM net against lstm_bptt_ref: 1 env,
    33 (the second 32-row tile holds one row, the rest clamped) and 64; ~20 % reset
    rows at both steps, row 0 at step t and the last row at step t - 1 among them.
    Every dG / gates / cbuf / dh slot the step must not read holds the sentinel, as
    does c_prev of the rows reset at t - 1."""
    from asyncrl_amd import A3CLSTM
    d = R.bptt_data(n_envs, R.BPTT_T, t)
    N, T = n_envs, R.BPTT_T
    net = A3CLSTM(4, n_envs=N, t_max=T, init_seed=0, frames="pairs").net
    net.reset()
    dG0 = d["dG"].copy()
    dG0[t - 1] = R.PREFILL
    put(net, "dG", dG0)
    for name in ("gates", "cbuf", "dh", "dcn"):
        put(net, name, d[name])
    put(net, "reset", d["reset"], torch.uint8)
    put_param(net, "1/lateral/W", d["Wl"])
    net.buffer("dhn", f32).fill_(R.PREFILL)
    net.run_stage("lstm_bptt", t)
    torch.cuda.synchronize()
    dGr, dcr = R.lstm_bptt_ref(d["dG"][t], d["Wl"], d["reset"][t], d["gates"][t - 1], d["cbuf"][t], d["cbuf"][t - 1],
                               d["reset"][t - 1], d["dh"][t - 1], d["dcn"])
    dG, dcn = get(net, "dG", (T, N, R.GATES)), get(net, "dcn", (N, R.HID))
    print(f"lstm_bptt N={N} t={t}: dG {close_normscaled(dG[t - 1], dGr, RTOL)[1]:.3g} dcn "
          f"{close_normscaled(dcn, dcr, RTOL)[1]:.3g} of the scale")
    assert not (dG[t - 1] == R.PREFILL).any()
    _close(dG[t - 1], dGr, "dG")
    _close(dcn, dcr, "dcn")
    assert (dcn[d["reset"][t - 1] != 0] == 0).all()
    assert np.array_equal(np.delete(dG, t - 1, 0), np.delete(d["dG"], t - 1, 0))
    assert bool((net.buffer("dhn", f32) == R.PREFILL).all())


@pytest.mark.parametrize("n_envs,t_max", R.BPTT_CHAIN_CASES)
def test_lstm_bptt_chain(gpu, n_envs, t_max):
    """The learner's trunk part on an LSTM net, T = 5, 37 envs and 1: the first cell
    launch (dhn / dcn hold the sentinel: it must ignore them) and the T - 1 BPTT
    launches against lstm_bptt_chain_ref over the whole dG, then the LSTM weight
    gradients of the same run against lstm_wgrad_ref fed the reference dG.
    (3, 64) and (33, 33): 63 and 32 BPTT launches on crafted reset flags (env 0's
    chain runs over the whole window; resets at step 0, at step T - 1 and past step
    32), 33 envs a second 32-row tile and two sample ranges of the weight gradient.
    The float32 restatement of the chain differs from the float64 reference by at
    most 2.9e-7 of the scale on these cases (tests/test_long_windows_ref.py), so the
    suite's 1e-5 holds here as it stands."""
    from asyncrl_amd import A3CLSTM
    from asyncrl_amd._lib import LEARN_TRUNK
    d = R.bptt_chain_data(n_envs, t_max)
    if (n_envs, t_max) in R.BPTT_LONG_CASES:
        assert R.crafted_flags_hold(d["reset"][:t_max]) and not d["reset"][:t_max, 0].any()
    fc = d["fc"]
    N, T, S = n_envs, t_max, d["S"]
    net = A3CLSTM(fc["A"], n_envs=N, t_max=T, init_seed=0, frames="pairs").net
    net.reset()
    for name in ("hfc", "hbuf", "gates", "cbuf", "dh"):
        put(net, name, d[name])
    put(net, "reset", d["reset"], torch.uint8)
    put(net, "a2", fc["a2"])
    words = R.pack_a2_mask(fc["a2"])
    words[T] = 0xFFFFFFFF
    put(net, "a2_mask", words)
    put(net, "dlogits", fc["dlogits"])
    put(net, "dv", fc["dv"])
    for name, arr in (("1/upward/W", d["Wu"]), ("1/lateral/W", d["Wl"]), ("0/2/W", fc["W"])):
        put_param(net, name, arr)
    for name in ("dhn", "dcn"):
        net.buffer(name, f32).fill_(float(R.SENTINEL))
    for name in ("dG", "dfc"):
        net.buffer(name, f32).fill_(R.PREFILL)
    net.grads.fill_(R.PREFILL)
    net.learn_parts([LEARN_TRUNK])
    torch.cuda.synchronize()
    dGr = R.lstm_bptt_chain_ref(d["Wl"], d["reset"], d["gates"], d["cbuf"], d["dh"])
    dG = get(net, "dG", (T, N, R.GATES))
    print(f"lstm_bptt chain N={N} T={T}: dG {close_normscaled(dG, dGr, RTOL)[1]:.3g} of the scale")
    assert not (dG == R.PREFILL).any()
    _close(dG, dGr, "dG")
    hfc, hprev, reset = d["hfc"][:T].reshape(S, -1), d["hbuf"][:T].reshape(S, -1), d["reset"].reshape(-1)[:S]
    ref, mag = R.lstm_wgrad_ref(dGr.reshape(S, R.GATES).astype(np.float32), hfc, hprev, reset, d["Wu"])
    names = {"gWu": "1/upward/W", "gWl": "1/lateral/W", "gbu": "1/upward/b"}
    got = {k: net.grad(name).cpu().numpy() for k, name in names.items()}
    grads_match(got, {k: ref[k].reshape(got[k].shape) for k in names}, {k: mag[k].reshape(got[k].shape) for k in names},
                rtol=RTOL, rtol_elem=RTOL)


# ------------------------------------------------------------------ returns
def _returns(t_max, n_actions, n_envs, lstm=False):
    from asyncrl_amd import A3CFF, A3CLSTM
    d = R.returns_data(t_max, n_actions, n_envs, lstm)
    T, A, N = t_max, n_actions, n_envs
    net = (A3CLSTM if lstm else A3CFF)(A, n_envs=N, t_max=T, init_seed=0, frames="pairs").net
    net.reset()

    def slot_T(arr, fill):   # the window's rows, then a slot T the stage must not read
        return np.concatenate([arr, np.full((1,) + arr.shape[1:], fill, arr.dtype)])

    put(net, "rewards", d["rewards"])
    put(net, "dones", d["dones"], torch.uint8)
    put(net, "v", d["v"])
    put(net, "probs", slot_T(d["probs"], R.SENTINEL))
    put(net, "logp", slot_T(d["logp"], R.SENTINEL))
    put(net, "actions", slot_T(d["actions"], 10 ** 6), torch.int32)
    put(net, "hfc", d["hfc"])
    pi, vf = ("2/0/W", "3/0/W") if lstm else ("1/0/W", "2/0/W")
    put_param(net, pi, d["Wpi"])
    put_param(net, vf, d["Wv"])
    out = "dh" if lstm else "dfc"
    for name in ("dlogits", "dv", "loss", "dfc") + (("dh",) if lstm else ()):
        net.buffer(name, f32).fill_(R.PREFILL)
    net.run_stage("returns")
    torch.cuda.synchronize()
    ref = R.returns_heads_ref(d["rewards"], d["dones"], d["v"], d["probs"], d["logp"], d["actions"], d["Wpi"], d["Wv"],
                              None if lstm else d["hfc"][:T])
    got = (get(net, "dlogits", (T, N, A)), get(net, "dv", (T, N)), get(net, "loss", (N, 2)), get(net, out, (T, N, R.HID)))
    errs = [close_normscaled(g, r, RTOL)[1] for g, r in zip(got, ref)]
    print(f"returns T={T} A={A} N={N}{' lstm' if lstm else ''}: dlogits / dv / loss / {out} "
          + " / ".join(f"{e:.3g}" for e in errs) + " of the scale")
    for g, r, what in zip(got, ref, ("dlogits", "dv", "loss", out)):
        assert not (g == R.PREFILL).any(), what
        _close(g, r, what)
    if lstm:   # unmasked, and nothing of the FF form written
        assert bool((net.buffer("dfc", f32) == R.PREFILL).all())
    else:
        assert (got[3][d["hfc"][:T] <= 0] == 0).all()


@pytest.mark.parametrize("t_max,n_actions,n_envs", R.RETURNS_CASES)
def test_returns_stage(gpu, t_max, n_actions, n_envs):
    """The learner's first launch on FF nets against returns_heads_ref, one case for
    each returns_heads_kernel<AM, RB> the host picks and each row-pass count: t_max
    <= 8 with A <= 4 / <= 8 / above (AM = 4, 8, 32; A = 4, 8 the largest of their
    form), t_max = 9 (32 rows a pass, the returns' window loop from memory), 32 x 32
    (every row and action register in use), 33 and 64 (a second pass over rows)."""
    _returns(t_max, n_actions, n_envs)


def test_returns_stage_lstm_arch(gpu):
    """The same launch on an LSTM net: the output is dh, unmasked, and hfc (all
    sentinel) is not read."""
    _returns(*R.RETURNS_LSTM_CASE, lstm=True)
