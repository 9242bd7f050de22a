"""GPU: the two model paths that run on the generic implicit-GEMM template
(csrc/gemm.hpp with the accessors and epilogues of csrc/layers.hpp) -- the
Nature head (csrc/nature.hip) and the f32-state convs of an ARCH_STATES net
(csrc/states.hip) -- one stage at a time (arl_run_stage, and net.learn() for
the launches it refuses there) on synthetic operands written into the
workspace, against the float64 references of tests/stage_ref.py.  The shapes
are the smallest at which the launches change form: more than one K slice
with a shorter last one, slice counts that are no multiple of the reduce's 4
slice groups, K no multiple of BK = 32 (nor of 4), ragged last M / N tiles,
a second M tile of the FC forward and of the heads GEMM, two returns_kernel
workgroups, and device step counters past 2^32 and 2^40 in the two ring
accessors (RingIm2col, StatesIm2col).

Conventions and tolerances are those of tests/test_gpu_stages.py: reduced
tensors grads_match(rtol = 1e-5, rtol_elem = 1e-5) against the reference and
its per-element scales, non-reduced ones close_normscaled(1e-5) and exactly
0.0 under a zero ReLU mask.  tests/test_stage_ref.py pins each case's launch
geometry and shows on the CPU that the mistakes these cases exist for miss
those bounds by more than 10x on the same data."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
import stage_ref as R
from conftest import close_grad, close_normscaled, grads_match

pytestmark = pytest.mark.gpu

RTOL = 1e-5
f32 = torch.float32
CTL_STEP = 0
NAT = R.NATURE_NAMES


def put(net, name, arr, dtype=f32):
    net.buffer(name, dtype).copy_(torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)))


def put_param(net, name, arr):
    net.param(name).copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    net.params_changed()


def get(net, name, shape):
    return net.buffer(name, f32, shape).cpu().numpy()


def prefill(net, *names):
    for name in names:
        net.buffer(name, f32).fill_(R.PREFILL)


def set_step(net, start):
    net.buffer("ctl", torch.int64)[CTL_STEP] = start
    torch.cuda.synchronize()
    assert int(net.buffer("ctl", torch.int64)[CTL_STEP]) == start


def errs(tag, pairs):
    """Print each tensor's error as a fraction of its scale, then assert close_normscaled(1e-5)."""
    es = [(what, close_normscaled(got, want, RTOL)) for what, got, want in pairs]
    print(f"{tag}: " + " ".join(f"{what} {e:.3g}" for what, (_, e) in es) + " of the scale")
    for (what, got, _), (_, (ok, e)) in zip(pairs, es):
        assert np.isfinite(got).all() and not (got == R.PREFILL).any(), (tag, what)
        assert ok, (tag, what, e)


def masked(tag, what, got, want, mask):
    errs(tag, [(what, got, want)])
    assert (got[~mask] == 0).all(), (tag, what)


def check_grads(tag, net, names, ref, mag):
    """The named tensors of the flat gradient against the reference (errors printed as
    fractions of the tensor's scale / of the element's own scale); every other tensor
    still holds the prefill."""
    got = {k: net.grad(name).cpu().numpy() for k, name in names.items()}
    want = {k: ref[k].reshape(got[k].shape) for k in names}
    scale = {k: mag[k].reshape(got[k].shape) for k in names}
    print(f"{tag}: " + " ".join(f"{k} {close_normscaled(got[k], want[k], RTOL)[1]:.3g}/"
                                f"{close_grad(got[k], want[k], scale[k], RTOL)[1]:.3g}" for k in names)
          + " of the tensor's / the element's scale")
    for k, v in got.items():
        assert np.isfinite(v).all() and not (v == R.PREFILL).any(), (tag, k)
    grads_match(got, want, scale, rtol=RTOL, rtol_elem=RTOL)
    for name in net.layout:
        if name not in names.values():
            assert bool((net.grad(name) == R.PREFILL).all()), (tag, name)


def relu_checks(tag, what, got, want, z):
    """got = max(z, 0) at 1e-5 of the scale; outside the tie band the ReLU decisions are the
    reference's; the band exempts at most TIE_SHARE_MAX of the tensor."""
    sure = ~R.tie_band(z)
    assert 1.0 - sure.mean() <= R.TIE_SHARE_MAX, (tag, what, 1.0 - sure.mean())
    assert (got[sure & (z < 0)] == 0).all() and (got[sure & (z > 0)] > 0).all(), (tag, what)


# ------------------------------------------------------------------ shared operands and references (never written)
@functools.lru_cache(maxsize=None)
def nature_case(n_envs, t_max, n_actions):
    return R.nature_data(n_envs, t_max, n_actions)


@functools.lru_cache(maxsize=None)
def nature_fwd_slots(n_envs, t_max, n_actions):
    """nature_fwd_ref of slot 0's and the bootstrap slot's samples, in that order."""
    d, N, T = nature_case(n_envs, t_max, n_actions), n_envs, t_max
    x = np.concatenate([d["x_fwd"][:N], d["x_fwd"][T * N:(T + 1) * N]])
    return R.nature_fwd_ref(x, d["p"])


@functools.lru_cache(maxsize=None)
def nature_conv_bwd_case(n_envs, t_max, n_actions):
    d, T, S = nature_case(n_envs, t_max, n_actions), t_max, n_envs * t_max
    return R.nature_conv_bwd_ref(d["x"], d["a1"][:T].reshape(S, R.NC1, 20, 20), d["a2"][:T].reshape(S, R.NC2, 9, 9),
                                 d["da3"], d["p"]["0/2/W"], d["p"]["0/1/W"])


@functools.lru_cache(maxsize=None)
def states_case(n_envs, t_max):
    return R.states_data(n_envs, t_max)


@functools.lru_cache(maxsize=None)
def states_fwd_slots(n_envs, t_max):
    d, N, T = states_case(n_envs, t_max), n_envs, t_max
    x = np.concatenate([d["x_fwd"][:N], d["x_fwd"][T * N:(T + 1) * N]])
    return R.conv_fwd_ref(x, d["W1"], d["b1"], d["W2"], d["b2"])


@functools.lru_cache(maxsize=None)
def states_conv_bwd_case(n_envs, t_max):
    d, T, S = states_case(n_envs, t_max), t_max, n_envs * t_max
    a1 = d["a1"][:T].reshape(S, 16, 20, 20)
    g, mag = R.conv_bwd_ref(d["x"], a1, d["da2"], d["W2"])
    return g, mag, R.conv_transpose_ref(d["da2"], d["W2"], 2) * (a1 > 0)


def nature_net(d, start=0):
    """A Nature net with the case's parameters, its frame ring as it stands under a step
    counter of `start`, and the counter written."""
    from asyncrl_amd import A3CFFNature
    net = A3CFFNature(d["A"], n_envs=d["N"], t_max=d["T"], init_seed=0).net
    net.reset()
    for name, arr in d["p"].items():
        put_param(net, name, arr)
    put(net, "frames", R.rolled(d["frames"], start, d["R"]), torch.uint8)
    put(net, "nvalid", R.rolled(d["nvalid"], start, d["R"]), torch.uint8)
    set_step(net, start)
    pl, mn = R.nature_plans(d["S"], d["A"]), {"heads": (d["A"] + 1) * 513, "fc": 512 * 3137, "c3": 64 * 577, "c2": 64 * 513,
                                              "c1": 32 * 257}   # nature_slab_floats: slices x (M x N) of every split GEMM
    assert net.buffer("slab", f32).numel() == max([R.NFC_SPLIT * d["N"] * R.NHID] + [pl[k] * mn[k] for k in pl])
    return net


# ------------------------------------------------------------------ Nature: conv_fwd
def _nature_conv_fwd(case, start=0):
    d, ref = nature_case(*case), nature_fwd_slots(*case)
    N, T = d["N"], d["T"]
    net = nature_net(d, start)
    shapes = {"a1": (T + 1, N, R.NC1, 20, 20), "a2": (T + 1, N, R.NC2, 9, 9), "a3": (T + 1, N, R.NC3, 7, 7)}
    for i, t in enumerate((0, T)):
        sl = slice(i * N, (i + 1) * N)
        prefill(net, *shapes)
        net.run_stage("conv_fwd", t)
        torch.cuda.synchronize()
        got = {k: get(net, k, s) for k, s in shapes.items()}
        tag = f"nature conv_fwd {case} start={start} t={t}"
        errs(tag, [(k, got[k][t], ref[k][sl]) for k in shapes])
        for k in shapes:
            relu_checks(tag, k, got[k][t], ref[k][sl], ref["z" + k[1:]][sl])
            assert (np.delete(got[k], t, 0) == R.PREFILL).all(), (tag, k)


@pytest.mark.parametrize("case", R.NATURE_CASES)
def test_nature_conv_fwd_stage(gpu, case):
    """conv_fwd of a Nature net at slot 0 and the bootstrap slot against nature_fwd_ref:
    conv1 launch_gemm<64, 32, GK, GK> on RingIm2col (nvalid from 1..4, env 0 masked at both
    slots), conv2 / conv3 launch_gemm<64, 64, GS, GK> on Im2col.  (1, 1, 4): one workgroup
    of conv3 with a 49-row tile; (33, 5, 18): M = 13200 / 2673 / 1617 rows, conv2 and
    conv3 end in a ragged tile (53 and 21 rows), conv3's K = 576 is 18 whole chunks; (67,
    2, 6): 26800 / 5427 / 3283 rows.  Outside the tie band the ReLU decisions are the
    reference's; the band's share of a1 / a2 / a3, measured on the reference alone: at
    most 1.6e-4 / 4.0e-5 / 6.8e-5 over these cases (bound 1e-3).  The other slots keep
    their prefill."""
    _nature_conv_fwd(case)


@pytest.mark.parametrize("start", R.ring_starts(R.NATURE_RING_CASE[1]))
def test_nature_conv_fwd_ring_residues(gpu, start):
    """The (33, 5, 18) case once more with the device step counter at R - 1, 2^32 - 3 and a
    multiple of T above 2^40: RingIm2col's own copy of the residue arithmetic (fd_mod64 of
    the counter, fd_wrap of the window-local offsets).  The ring holds the same window
    rolled to where (start + t) % R says, so the reference is the case's own."""
    assert start % (R.NATURE_RING_CASE[1] + 4) != 0
    _nature_conv_fwd(R.NATURE_RING_CASE, start)


# ------------------------------------------------------------------ Nature: fc_fwd + policy
@pytest.mark.parametrize("case", R.NATURE_CASES)
def test_nature_fc_fwd_policy_stages(gpu, case):
    """fc_fwd + policy of a Nature net at slot 0 and the bootstrap slot on a synthetic a3
    (every other slot a sentinel): the split-K FC launch_gemm<64, 64, GK, GK> (K = 3136 in
    8 slices of 416, the last 224) into the slab, the MapBiasRelu reduce of 8 slices, and
    the 512-wide policy launch; h, logits, v, probs, logp and the entropy in float64.
    (1, 1, 4): one row; (33, 5, 18): a 33-row tile, 18 actions; (67, 2, 6): a second M
    tile with 3 rows."""
    d = nature_case(*case)
    N, T, A, p = d["N"], d["T"], d["A"], d["p"]
    net = nature_net(d)
    names = ("hfc", "logits", "v", "probs", "logp", "entropy")
    shapes = {"hfc": (T + 1, N, R.NHID), "logits": (T + 1, N, A), "v": (T + 1, N), "probs": (T + 1, N, A),
              "logp": (T + 1, N, A), "entropy": (T + 1, N)}
    for t in (0, T):
        a3 = np.full((T + 1, N, R.NA3), R.SENTINEL, np.float32)
        a3[t] = R.act_like(np.random.default_rng([7, N, t]), (N, R.NA3))
        put(net, "a3", a3)
        prefill(net, *names)
        net.run_stage("fc_fwd", t)
        net.run_stage("policy", t)
        torch.cuda.synchronize()
        h = np.maximum(R.mm64(a3[t], p["0/3/W"].T) + p["0/3/b"], 0.0)
        want = dict(R.policy_ref(h, p["1/0/W"], p["1/0/b"], p["2/0/W"], p["2/0/b"]), hfc=h)
        got = {k: get(net, k, shapes[k]) for k in names}
        errs(f"nature fc_fwd + policy {case} t={t}", [(k, got[k][t], want[k]) for k in names])
        for k in names:
            assert (np.delete(got[k], t, 0) == R.PREFILL).all(), (k, t)


# ------------------------------------------------------------------ Nature: fc_bwd
@pytest.mark.parametrize("case", R.NATURE_CASES + [R.NATURE_HEADS_CASE] + R.NATURE_HEADS_EDGE_CASES)
def test_nature_fc_bwd_stage(gpu, case):
    """fc_bwd of a Nature net against nature_fc_bwd_ref: the weight gradient launch_gemm<64,
    64, GM, GM>(ColMajor dfc, OnesColB a3) with N = 3137 (the bias column alone in the
    last 4-vector and in the 50th N tile), its MapDense reduce, and da3 = (dfc W) * (a3 >
    0) launch_gemm<64, 64, GK, GM> with EpiMask.  (1, 1, 4): K = 1, one slice; (33, 5, 18):
    S = 165 in slices of 96 + 69, da3 with a 37-row last tile; (67, 2, 6): 96 + 38; (41,
    9, 4): S = 369 in 192 + 177.  Two slices: four launches in a row with fresh dfc (a
    stale slab row shows).  Every other gradient tensor keeps its prefill.  (5, 3, 15) and
    (5, 3, 16): the slab sized by heads GEMMs of one exact 16-row tile and of a second tile
    that holds the value row alone (nature_net asserts the size; the heads GEMM itself runs
    in test_nature_learn_synthetic_window)."""
    d = nature_case(*case)
    T, S = d["T"], d["S"]
    net = nature_net(d)
    Z = R.nature_plans(S, d["A"])["fc"]
    put(net, "a3", d["a3"])
    a3 = d["a3"][:T].reshape(S, R.NA3)
    for k in range(R.LAUNCHES if Z > 1 else 1):
        dfc = d["fresh_dfc"](k)
        put(net, "dfc", dfc)
        net.grads.fill_(R.PREFILL)
        prefill(net, "da3")
        net.run_stage("fc_bwd")
        torch.cuda.synchronize()
        ref, mag = R.nature_fc_bwd_ref(dfc, a3, d["p"]["0/3/W"])
        tag = f"nature fc_bwd {case} launch {k}"
        check_grads(tag, net, {"fcW": NAT["fcW"], "fcb": NAT["fcb"]}, ref, mag)
        masked(tag, "da3", get(net, "da3", (S, R.NA3)), ref["da3"], a3 > 0)


# ------------------------------------------------------------------ Nature: conv_bwd
def _nature_conv_bwd(case, start=0):
    d = nature_case(*case)
    T, S = d["T"], d["S"]
    ref, mag, da2r, da1r = nature_conv_bwd_case(*case)
    net = nature_net(d, start)
    for name in ("a1", "a2", "da3"):
        put(net, name, d[name])
    net.grads.fill_(R.PREFILL)
    prefill(net, "da2", "da1", "slab")
    net.run_stage("conv_bwd")
    torch.cuda.synchronize()
    tag = f"nature conv_bwd {case} start={start}"
    check_grads(tag, net, {k: NAT[k] for k in ("c3W", "c3b", "c2W", "c2b", "c1W", "c1b")}, ref, mag)
    masked(tag, "da2", get(net, "da2", da2r.shape), da2r, d["a2"][:T].reshape(da2r.shape) > 0)
    masked(tag, "da1", get(net, "da1", da1r.shape), da1r, d["a1"][:T].reshape(da1r.shape) > 0)


@pytest.mark.parametrize("case", R.NATURE_CASES)
def test_nature_conv_bwd_stage(gpu, case):
    """conv_bwd of a Nature net on synthetic a1 / a2 / da3 / W3 / W2 against
    nature_conv_bwd_ref: the three weight-gradient GEMMs (ConvDyT x OnesCol<Im2col>, and
    OnesCol<RingIm2col> from the frame ring) with their MapDense reduces, the stride-1
    transposed conv of conv3 (ConvT1A, ConvTW, EpiConvMask) and the four parity classes of
    conv2's (ConvT2ClassA / W, EpiT2Class).  (1, 1, 4): K = 49 / 81 / 400 in 1 / 1 / 4
    slices; (33, 5, 18): 64 / 105 / 188 slices with last ones of 21 / 53 / 176, K = 8085
    and 13365 odd, 105 no multiple of the reduce's 4 slice groups, the transposed convs'
    last M tiles of 53 and 52 rows; (67, 2, 6): 52 / 85 / 187 slices.  da2 and da1 are
    exactly 0 under their masks; the bootstrap slot of a1 / a2 is a sentinel."""
    _nature_conv_bwd(case)


@pytest.mark.parametrize("start", R.ring_starts(R.NATURE_RING_CASE[1]))
def test_nature_conv_bwd_ring_residues(gpu, start):
    """The (33, 5, 18) case with the step counter at R - 1, 2^32 - 3 and above 2^40: conv1's
    weight gradient reads the ring through RingIm2col at t0 = 0 over the window's T steps."""
    _nature_conv_bwd(R.NATURE_RING_CASE, start)


# ------------------------------------------------------------------ Nature: net.learn()
@pytest.mark.parametrize("lam", R.GAE_LAMBDAS)
@pytest.mark.parametrize("case", R.NATURE_LEARN_CASES + R.NATURE_HEADS_EDGE_CASES)
def test_nature_learn_synthetic_window(gpu, case, lam):
    """net.learn() of a Nature net on a synthetic workspace (rewards, dones, v, probs, logp,
    actions, hfc, a3, a2, a1, frames) against the chained reference nature_learn_ref: the
    only way to the launches arl_run_stage refuses on this architecture -- the returns_kernel
    form launch_returns picks (n-step, and GAE at lambda = 0.95), the heads GEMM
    launch_gemm<16, 64, GS, GM>(HeadsGA, OnesColB) with its MapHeads reduce, and
    heads_bwd_kernel.  (33, 5, 18): 19 rows = two M tiles of the heads GEMM, two K slices,
    one returns workgroup from registers (T <= 8); (41, 9, 4): three K slices (128 + 128 +
    113), T > 8 (the returns scan from memory), two returns workgroups (28 envs each); (5, 3,
    15): M = 16, one exact tile of the heads GEMM; (5, 3, 16): M = 17, the value row alone
    in the second tile.  All 12 gradient tensors, dlogits, dv, the per-env losses and dfc."""
    d = nature_case(*case)
    N, T, A, S = d["N"], d["T"], d["A"], d["S"]
    outs, g, mag = nature_learn_case(case, lam)
    net = nature_net(d)

    def slot_T(arr, fill):
        return np.concatenate([arr, np.full((1,) + arr.shape[1:], fill, arr.dtype)])

    put(net, "rewards", d["rewards"])
    put(net, "dones", d["dones"], torch.uint8)
    put(net, "v", d["v"])
    put(net, "probs", slot_T(d["probs"], R.SENTINEL))
    put(net, "logp", slot_T(d["logp"], R.SENTINEL))
    put(net, "actions", slot_T(d["actions"], 10 ** 6), torch.int32)
    for name in ("hfc", "a3", "a2", "a1"):
        put(net, name, d[name])
    if lam != 1.0:
        net.set_gae(lam)
    net.grads.fill_(R.PREFILL)
    prefill(net, "dlogits", "dv", "loss", "dfc", "da3", "da2", "da1", "slab")
    net.learn()
    torch.cuda.synchronize()
    tag = f"nature learn {case} lambda={lam}"
    errs(tag, [("dlogits", get(net, "dlogits", (T, N, A)), outs["dlogits"]), ("dv", get(net, "dv", (T, N)), outs["dv"]),
               ("loss", get(net, "loss", (N, 2)), outs["loss"])])
    masked(tag, "dfc", get(net, "dfc", (T, N, R.NHID)), outs["dfc"], d["hfc"][:T] > 0)
    check_grads(tag, net, NAT, g, mag)


@functools.lru_cache(maxsize=None)
def nature_learn_case(case, lam):
    return R.nature_learn_ref(nature_case(*case), lam)


# ------------------------------------------------------------------ ARCH_STATES: conv_fwd, conv_bwd
def states_net(d, start=0, bwd=False):
    """An A3CFF(frames="states") net with the case's conv parameters and its f32 ring as it
    stands under a step counter of `start`; every slot the stage must not read is a
    sentinel (bwd: the bootstrap slot too)."""
    from asyncrl_amd import A3CFF
    net = A3CFF(4, n_envs=d["N"], t_max=d["T"], init_seed=0, frames="states").net
    net.reset()
    for name, key in (("0/0/W", "W1"), ("0/0/b", "b1"), ("0/1/W", "W2"), ("0/1/b", "b2")):
        put_param(net, name, d[key])
    frames = d["frames"].copy()
    if bwd:
        frames[d["T"]] = R.SENTINEL
    put(net, "frames", R.rolled(frames, start, d["R"]))
    set_step(net, start)
    return net


def _states_conv_fwd(case, start=0):
    d = states_case(*case)
    N, T = d["N"], d["T"]
    a1r, a2r, z1, z2 = states_fwd_slots(*case)
    net = states_net(d, start)
    for i, t in enumerate((0, T)):
        sl = slice(i * N, (i + 1) * N)
        prefill(net, "a1", "a2")
        net.run_stage("conv_fwd", t)
        torch.cuda.synchronize()
        a1, a2 = get(net, "a1", (T + 1, N, 16, 20, 20)), get(net, "a2", (T + 1, N, 32, 9, 9))
        tag = f"states conv_fwd {case} start={start} t={t}"
        errs(tag, [("a1", a1[t], a1r[sl]), ("a2", a2[t], a2r[sl])])
        relu_checks(tag, "a1", a1[t], a1r[sl], z1[sl])
        relu_checks(tag, "a2", a2[t], a2r[sl], z2[sl])
        assert (np.delete(a1, t, 0) == R.PREFILL).all() and (np.delete(a2, t, 0) == R.PREFILL).all(), tag


@pytest.mark.parametrize("case", R.STATES_CASES)
def test_states_conv_fwd_stage(gpu, case):
    """conv_fwd of an A3CFF(frames="states") net at slot 0 and the bootstrap slot against
    conv_fwd_ref on the f32 ring (signed normal states, no image of uint8 frames): conv1
    launch_gemm<64, 16, 4 x 1 waves, GK, GS> on StatesIm2col, conv2 launch_gemm<32, 32, GS,
    GK>.  (1, 1): 400 / 81 rows (a 16-row and a 17-row last tile); (33, 5): 13200 / 2673
    rows.  The three ring slots outside the window hold a sentinel.  The tie band's share
    of a1 / a2 on the reference alone: at most 3.3e-5 / 3.5e-5 (bound 1e-3)."""
    _states_conv_fwd(case)


@pytest.mark.parametrize("start", R.ring_starts(R.STATES_RING_CASE[1]))
def test_states_conv_fwd_ring_residues(gpu, start):
    """The (33, 5) case with the step counter at R - 1, 2^32 - 3 and above 2^40:
    StatesIm2col's own copy of the residue arithmetic; a wrong slot reads a sentinel."""
    assert start % (R.STATES_RING_CASE[1] + 4) != 0
    _states_conv_fwd(R.STATES_RING_CASE, start)


def _states_conv_bwd(case, start=0):
    d = states_case(*case)
    S = d["S"]
    ref, mag, da1r = states_conv_bwd_case(*case)
    net = states_net(d, start, bwd=True)
    put(net, "a1", d["a1"])
    put(net, "da2", d["da2"])
    net.grads.fill_(R.PREFILL)
    prefill(net, "da1", "slab")
    net.run_stage("conv_bwd")
    torch.cuda.synchronize()
    tag = f"states conv_bwd {case} start={start}"
    check_grads(tag, net, {"c2W": "0/1/W", "c2b": "0/1/b", "c1W": "0/0/W", "c1b": "0/0/b"}, ref, mag)
    masked(tag, "da1", get(net, "da1", da1r.shape), da1r, d["a1"][:d["T"]].reshape(da1r.shape) > 0)


@pytest.mark.parametrize("case", R.STATES_CASES)
def test_states_conv_bwd_stage(gpu, case):
    """conv_bwd of an A3CFF(frames="states") net against conv_bwd_ref: conv2's weight
    gradient launch_gemm<32, 64, GS, GS> (N = 257), the four parity classes of the
    transposed conv launch_gemm<64, 16, 4 x 1 waves>, conv1's launch_gemm<32, 64, GK, GM>
    with OnesCol<StatesIm2col>.  (1, 1): 1 / 4 slices; (33, 5): 105 / 188 slices, last
    ones of 53 / 176.  da1 is exactly 0 under its mask; the bootstrap ring slot and the
    three slots outside the window hold a sentinel."""
    _states_conv_bwd(case)


@pytest.mark.parametrize("start", R.ring_starts(R.STATES_RING_CASE[1]))
def test_states_conv_bwd_ring_residues(gpu, start):
    """The (33, 5) case with the step counter at R - 1, 2^32 - 3 and above 2^40."""
    _states_conv_bwd(R.STATES_RING_CASE, start)


# ------------------------------------------------------------------ explicit-state forward on fewer states than envs
@pytest.mark.parametrize("n", [37, 1])
@pytest.mark.parametrize("nature", [True, False])
def test_pi_and_v_on_fewer_states_than_envs(gpu, nature, n):
    """A3CFFNature.pi_and_v and A3CFF.pi_and_v on 37 states and on 1 of a 40-env model
    against oracle.pi_and_v_ff: the split-K slab is indexed by the call's n, the output
    slot by the net's N."""
    from asyncrl_amd import A3CFF, A3CFFNature, dqn_phi
    A, N = 5, 40
    model = (A3CFFNature if nature else A3CFF)(A, n_envs=N, t_max=3, init_seed=3)
    params = model.net.state_dict()
    stacks = np.random.default_rng([14, n]).integers(0, 256, (n, 4, 84, 84), dtype=np.uint8)
    stacks[0, :3] = 0
    pout, v = model.pi_and_v(dqn_phi(torch.from_numpy(stacks).to(gpu)))
    lo, vo, _ = O.pi_and_v_ff(params, O.PHI_LUT[stacks], O.ARCH_FF_NATURE if nature else O.ARCH_FF)
    assert pout.logits.shape == (n, A) and v.shape == (n,)
    errs(f"pi_and_v nature={nature} n={n} of {N}",
         [("logits", pout.logits.cpu().numpy(), lo), ("v", v.cpu().numpy(), vo),
          ("probs", pout.probs.cpu().numpy(), O.softmax(lo))])
