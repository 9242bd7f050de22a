"""GPU: single window stages (arl_run_stage) on synthetic operands written into
the workspace, against the float64 references of tests/stage_ref.py -- at the
window sizes where the backward kernels change shape: more than one job A
sample range (the in-launch ticket reduce of fc_bwd.hip, for the FC layer and
the LSTM gate weights) and more than one sample per conv_bwd.hip workgroup.

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
    depth).  nvalid is drawn from 1..4 per (slot, env)."""
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
