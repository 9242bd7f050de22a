"""CPU tests of tests/stage_ref.py: the stage references against the oracle,
the launch geometry restated from the .hip sources, and the sensitivity of
the GPU stage tests' tolerance to the mistakes they exist to catch."""
import functools

import numpy as np
import pytest

import oracle as O
import stage_ref as R
from conftest import close_grad, close_normscaled

RTOL = 1e-5


def _equal(got, want, names):
    for k, name in names.items():
        assert got[k].dtype == np.float32 and got[k].shape == want[name].shape, k
        assert np.array_equal(got[k], want[name]), k


# ------------------------------------------------------------------ references against the oracle
def test_ff_stage_refs_equal_oracle_backward():
    """S = 7: fc_bwd_ref and conv_bwd_ref, fed the oracle's own dfc / da2, give
    oracle.ff_backward's gradients bit for bit (both round one float64 sum), and
    its error scales."""
    d = R.conv_data(7, 1, seed=3)
    x = d["x"][:]
    rng = np.random.default_rng(3)
    p = O.init_like_torch(O.ARCH_FF, 5, rng)
    acts = O.nips_head(p, O.ARCH_FF, x)
    a1, a2, h = acts
    dl, dv = R.grad_like(rng, (7, 5)), R.grad_like(rng, (7,))
    mag_o = {}
    g_o = O.ff_backward(p, x, acts, dl, dv, mag=mag_o)
    dh = (dl @ p["1/0/W"] + dv[:, None] * p["2/0/W"]).astype(np.float32)
    dfc = dh * (h > 0)
    a2f = a2.reshape(7, -1)
    g, mag = R.fc_bwd_ref(dfc, a2f, p["0/2/W"], dl, dv, h)
    names = {"fcW": "0/2/W", "fcb": "0/2/b", "piW": "1/0/W", "pib": "1/0/b", "vW": "2/0/W", "vb": "2/0/b"}
    _equal(g, g_o, names)
    da2_o = ((dfc @ p["0/2/W"]).reshape(a2.shape) * (a2 > 0)).astype(np.float32)   # oracle._head_backward
    ok, err = close_normscaled(g["da2"], da2_o.reshape(7, -1), 1e-6)
    assert ok, err
    assert (g["da2"][a2f <= 0] == 0).all()
    gc, magc = R.conv_bwd_ref(x, a1, da2_o, p["0/1/W"])
    namesc = {"c2W": "0/1/W", "c2b": "0/1/b", "c1W": "0/0/W", "c1b": "0/0/b"}
    _equal(gc, g_o, namesc)
    for m, nm in ((mag, names), (magc, namesc)):
        for k, name in nm.items():
            assert np.allclose(m[k], mag_o[name], rtol=1e-12, atol=0), k
    # chunks of 3, 3, 1 samples: the same sums to float64 rounding
    g3, mag3 = R.conv_bwd_ref(x, a1, da2_o, p["0/1/W"], chunk=3)
    for k in gc:
        assert np.allclose(g3[k], gc[k], rtol=1e-6, atol=0) and np.allclose(mag3[k], magc[k], rtol=1e-12), k


def test_lstm_wgrad_ref_equals_oracle_window(monkeypatch):
    """S = 7: lstm_wgrad_ref on the dG / hfc / h_prev of oracle.lstm_window (taken
    from its own weight-gradient products) gives its upward / lateral gradients bit
    for bit; the rows of reset samples carry a sentinel the reference must drop."""
    rng = np.random.default_rng(4)
    N, T, A = 7, 1, 4
    p = O.init_like_torch(O.ARCH_LSTM, A, rng)
    states = O.PHI_LUT[rng.integers(0, 256, (T + 1, N, 4, 84, 84), dtype=np.uint8)]
    st0 = O.LSTMState(h=rng.normal(size=(N, 256)).astype(np.float32), c=rng.normal(size=(N, 256)).astype(np.float32),
                      has=np.array([1, 1, 0, 1, 1, 0, 1], bool))
    dprev = np.array([[0, 1, 0, 0, 1, 1, 0]], np.uint8)
    calls = []
    gmm = O.gmm
    monkeypatch.setattr(O, "gmm", lambda a, b: (calls.append((a, b)), gmm(a, b))[1])
    g_o, aux = O.lstm_window(p, states[:T], rng.integers(0, A, (T, N)), rng.normal(size=(T, N)).astype(np.float32),
                             dprev, np.zeros((T, N), np.uint8), states[T], st0)
    (dGt, hfc), (dGt2, hp) = calls[2], calls[3]        # gmm(dGf.T, hh), gmm(dGf.T, hprev * has)
    assert dGt.shape == (1024, 7) and np.array_equal(dGt2, dGt) and hfc.shape == hp.shape == (7, 256)
    reset = ~(st0.has & (dprev[0] == 0))
    assert reset.sum() == 4 and (hp[reset] == 0).all() and np.array_equal(hp[~reset], st0.h[~reset])
    hprev = np.where(reset[:, None], R.SENTINEL, st0.h)
    g, mag = R.lstm_wgrad_ref(np.ascontiguousarray(dGt.T), hfc, hprev, reset.astype(np.uint8), p["1/upward/W"])
    names = {"gWu": "1/upward/W", "gWl": "1/lateral/W", "gbu": "1/upward/b"}
    _equal(g, g_o, names)
    for k, name in names.items():
        assert np.allclose(mag[k], aux["grad_mag"][name], rtol=1e-12, atol=0), k
    dfc_o = (dGt.T @ p["1/upward/W"]).astype(np.float32) * (hfc > 0)   # lstm_window's dx, _head_backward's mask
    ok, err = close_normscaled(g["dfc"], dfc_o, 1e-6)
    assert ok, err
    assert (g["dfc"][hfc <= 0] == 0).all()


def test_conv_fwd_ref_equals_oracle_head():
    """N = 8 ring states with masked planes and N = 8 RGB states: conv_fwd_ref's a1 /
    a2 against oracle.nips_head's f32 ones within 1e-6 of the scale (measured 6.4e-7
    and 6.2e-7 on uniform frames), and a1 / a2 = max(z, 0)."""
    for layout, arch in (("ring", O.ARCH_FF), ("rgb", O.ARCH_FF | O.ARCH_RGB)):
        d = R.conv_fwd_data(8, layout, seed=2)
        x = d["x"][:8]
        p = {"0/0/W": d["W1"], "0/0/b": d["b1"], "0/1/W": d["W2"], "0/1/b": d["b2"],
             "0/2/W": np.zeros((256, R.A2), np.float32), "0/2/b": np.zeros(256, np.float32)}
        a1_o, a2_o, _ = O.nips_head(p, arch, x)
        a1, a2, z1, z2 = R.conv_fwd_ref(d["x"], d["W1"], d["b1"], d["W2"], d["b2"], chunk=3)
        assert a1.shape == (16, 16, 20, 20) and a2.shape == (16, 32, 9, 9) and a1.dtype == np.float64
        for got, want, what in ((a1[:8], a1_o, "a1"), (a2[:8], a2_o, "a2")):
            ok, err = close_normscaled(got, want, 1e-6)
            print(f"conv_fwd_ref {layout} {what}: {err:.3g} of the scale from oracle.nips_head")
            assert ok, (layout, what, err)
        assert np.array_equal(a1, np.maximum(z1, 0)) and np.array_equal(a2, np.maximum(z2, 0))
        assert (z1 < 0).any() and (z2 < 0).any()


def test_lstm_bptt_chain_ref_equals_oracle_window(monkeypatch):
    """T = 4, N = 6 with resets inside the window: lstm_bptt_chain_ref on the gates,
    cells and reset flags of oracle.lstm_window's forward (restated here with
    oracle.lstm_cell) and its heads' dh gives the dG of the oracle's own
    weight-gradient products within 1e-6 of the scale; the cell before step 0
    carries a sentinel on the rows that start without a state."""
    rng = np.random.default_rng(6)
    N, T, A = 6, 4, 4
    p = O.init_like_torch(O.ARCH_LSTM, A, rng)
    states = O.PHI_LUT[rng.integers(0, 256, (T + 1, N, 4, 84, 84), dtype=np.uint8)]
    st0 = O.LSTMState(h=rng.normal(size=(N, 256)).astype(np.float32), c=rng.normal(size=(N, 256)).astype(np.float32),
                      has=np.array([1, 0, 1, 1, 0, 1], bool))
    dprev = np.array([[0, 0, 1, 0, 0, 0], [0, 1, 0, 0, 0, 1], [0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1]], np.uint8)
    dones = np.concatenate([dprev[1:], np.zeros((1, N), np.uint8)])
    calls = []
    gmm = O.gmm
    monkeypatch.setattr(O, "gmm", lambda a, b: (calls.append((a, b)), gmm(a, b))[1])
    _, aux = O.lstm_window(p, states[:T], rng.integers(0, A, (T, N)), rng.normal(size=(T, N)).astype(np.float32),
                           dprev, dones, states[T], st0)
    dG_o = calls[2][0].T.reshape(T, N, 1024)   # gmm(dGf.T, hh)
    # the forward, as lstm_window runs it
    hh = O.nips_head(p, O.ARCH_LSTM, states[:T].reshape(T * N, 4, 84, 84))[2].reshape(T, N, 256)
    gates, cbuf = np.zeros((T, N, 1024), np.float32), np.zeros((T + 1, N, 256), np.float32)
    reset = np.zeros((T, N), np.uint8)
    h, cbuf[0], has = st0.h, st0.c, st0.has.copy()
    for t in range(T):
        has = has & (dprev[t] == 0)
        reset[t] = ~has
        gates[t], cbuf[t + 1], h = O.lstm_cell(p, O.ARCH_LSTM, hh[t], h, cbuf[t], has)
        has = np.ones(N, bool)
    assert reset.sum() == 8 and reset[0].sum() == 3
    cbuf[0][reset[0] != 0] = R.SENTINEL
    dH = aux["dlogits"].astype(np.float64) @ p["2/0/W"] + aux["dv"][..., None].astype(np.float64) * p["3/0/W"][0]
    dG = R.lstm_bptt_chain_ref(p["1/lateral/W"], reset, gates, cbuf, dH)
    ok, err = close_normscaled(dG, dG_o, 1e-6)
    print(f"lstm_bptt_chain_ref: {err:.3g} of the scale from oracle.lstm_window's dG")
    assert ok, err
    assert np.abs(dG_o[0]).max() > 0


def test_returns_heads_ref_equals_oracle():
    """returns_heads_ref against oracle.returns_and_lossgrad (f32 R and advantage)
    and ff_backward's dh, within 1e-6 of the scale; the losses summed over envs."""
    for case in ((8, 5, 3), (33, 6, 2)):
        d = R.returns_data(*case)
        T = d["T"]
        dl, dv, loss, dfc = R.returns_heads_ref(d["rewards"], d["dones"], d["v"], d["probs"], d["logp"], d["actions"],
                                                d["Wpi"], d["Wv"], d["hfc"][:T])
        _, _, dl_o, dv_o, pil, vl = O.returns_and_lossgrad(d["rewards"], d["dones"], d["v"][:T], d["v"][T], d["probs"],
                                                           d["logp"], d["actions"])
        dfc_o = (dl_o @ d["Wpi"] + dv_o[..., None] * d["Wv"][0]) * (d["hfc"][:T] > 0)
        for got, want, what in ((dl, dl_o, "dlogits"), (dv, dv_o, "dv"), (dfc, dfc_o, "dfc")):
            ok, err = close_normscaled(got, want, 1e-6)
            print(f"returns_heads_ref {case} {what}: {err:.3g} of the scale from the oracle")
            assert ok, (case, what, err)
        assert np.allclose(loss.sum(0), [pil, vl], rtol=1e-6, atol=0)
        assert (dfc[d["hfc"][:T] <= 0] == 0).all() and d["dones"].sum() > 2 and (np.abs(d["rewards"]) > 1).any()


def test_ring_x_equals_state_from_ring():
    d = R.conv_data(3, 9, seed=1)
    x, Rr = d["x"], d["R"]
    assert x.shape == (27, 4, 84, 84) and (d["nvalid"] < 4).any()
    for t in range(9):
        want = O.state_from_ring(d["frames"], d["nvalid"][t % Rr], [(t - 3 + c) % Rr for c in range(4)])
        assert np.array_equal(x[3 * t:3 * t + 3], want), t
    assert np.array_equal(x[5:17], x[:][5:17])
    for layout, C in (("stack", 4), ("rgb", 3)):
        d = R.conv_data(2, 3, layout, seed=1)
        assert np.array_equal(d["x"][:], O.PHI_LUT[d["frames"][:3].reshape(6, C, 84, 84)])


def test_pack_a2_mask_round_trips():
    a2 = R.act_like(np.random.default_rng(5), (3, 4, R.A2))
    w = R.pack_a2_mask(a2)
    assert w.shape == (3, 4, 81) and w.dtype == np.uint32
    assert np.array_equal(R.unpack_a2_mask(w), a2 > 0)
    one = np.zeros((1, R.A2), np.float32)
    one[0, 32 * 7 + 5] = 1.0
    assert R.pack_a2_mask(one)[0, 7] == 1 << 5 and R.pack_a2_mask(one).sum() == 1 << 5


def test_launch_geometry():
    assert [R.fc_bwd_ranges(S) for S in (1199, 1200, 1205, 2000)] == [1, 2, 2, 3]
    assert [R.lstm_wgrad_ranges(S) for S in (1024, 1025, 2000)] == [1, 2, 3]
    assert R.range_len(1205, 2) == 608 and R.range_len(1025, 2) == 544
    assert R.ranges(1205) == (2, 608) and R.range_bounds(1205) == [(0, 608), (608, 1205)]
    assert R.ranges(1025, lstm=True) == (2, 544) and R.ranges(1025) == (1, 1056)
    assert [R.blocks(S) for S in (255, 256, 257, 603)] == [255, 256, 256, 256]
    assert R.part_floats(2000) == 82 * 3 * 8320 and R.part_floats(1025) == 64 * 2 * 8320


# ------------------------------------------------------------------ sensitivity of the GPU tests' tolerance
def _excess(pert, ref, mag):
    """How far `pert` is outside what grads_match(rtol=1e-5, rtol_elem=1e-5) accepts,
    in units of the bound (> 1: the check fails)."""
    worst = 0.0
    for k, want in pert.items():
        worst = max(worst, close_normscaled(want, ref[k], RTOL)[1] / RTOL)
        if k in mag:
            worst = max(worst, close_grad(want, ref[k], mag[k], RTOL)[1] / RTOL)
    return worst


def _job_a_mistakes(S, lstm, dY, X, ref, keys):
    """Perturbed results of job A's reductions (dW = dY^T X per block of X columns, db):
    the last sample of a range dropped; with Z > 1 one range's partial dropped, range
    0's added twice.  Yields (what, perturbed tensors)."""
    def part(r0, r1):
        out = {"b": dY[r0:r1].sum(0, dtype=np.float64)}
        out.update({k: R.mm64(dY[r0:r1].T, Xk[r0:r1]) for k, Xk in X.items()})
        return {keys[k]: v for k, v in out.items()}
    bounds = R.range_bounds(S, lstm)
    for z, (r0, r1) in enumerate(bounds):
        last = part(r1 - 1, r1)
        yield f"last sample of range {z} dropped", {k: ref[k] - v for k, v in last.items()}
        if len(bounds) > 1:
            whole = part(r0, r1)
            yield f"partial of range {z} dropped", {k: ref[k] - v for k, v in whole.items()}
            if z == 0:
                yield "partial of range 0 added twice", {k: ref[k] + v for k, v in whole.items()}


@pytest.mark.parametrize("n_envs,t_max", R.FC_CASES + [R.FC_LSTM_ARCH_CASE])
def test_fc_tolerance_catches_range_mistakes(n_envs, t_max):
    d = R.fc_data(n_envs, t_max, lstm=(n_envs, t_max) == R.FC_LSTM_ARCH_CASE)
    S, dfc, a2 = d["S"], d["fresh_dfc"](0), d["a2"][:t_max].reshape(-1, R.A2)
    ref, mag = R.fc_bwd_ref(dfc, a2, d["W"], d["dlogits"], d["dv"], d["hh"])
    for what, pert in _job_a_mistakes(S, False, dfc, {"W": a2}, ref, {"W": "fcW", "b": "fcb"}):
        f = _excess(pert, ref, mag)
        print(f"fc S={S} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)


@pytest.mark.parametrize("n_envs,t_max", R.LSTM_CASES)
def test_lstm_tolerance_catches_range_and_reset_mistakes(n_envs, t_max):
    d = R.lstm_data(n_envs, t_max)
    S, dG = d["S"], d["fresh_dG"](0)
    hfc, hprev, reset = d["hfc"][:t_max].reshape(S, -1), d["hbuf"][:t_max].reshape(S, -1), d["reset"].reshape(-1)[:S]
    ref, mag = R.lstm_wgrad_ref(dG, hfc, hprev, reset, d["Wu"])
    hp = hprev * (reset == 0)[:, None]
    mistakes = list(_job_a_mistakes(S, True, dG, {"u": hfc, "l": hp}, ref, {"u": "gWu", "l": "gWl", "b": "gbu"}))
    mistakes.append(("reset ignored", {"gWl": R.mm64(dG.T, hprev)}))
    for what, pert in mistakes:
        f = _excess(pert, ref, mag)
        print(f"lstm S={S} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)


@pytest.mark.parametrize("n_envs,t_max,layout", [c + ("ring",) for c in R.CONV_CASES]
                         + [R.CONV_LAYOUT_CASE + ("rgb",), R.CONV_LAYOUT_CASE + ("stack",)])
def test_conv_tolerance_catches_sample_loop_mistakes(n_envs, t_max, layout):
    d = R.conv_data(n_envs, t_max, layout)
    S, G, x, W2 = d["S"], R.blocks(d["S"]), d["x"], d["W2"]
    a1, da2 = d["a1"][:t_max].reshape(S, 16, 20, 20), d["da2"]
    ref, mag = R.conv_bwd_ref(x, a1, da2, W2)

    def one(s, xs=None, a1s=None):   # sample s's contribution, optionally with another sample's x / a1
        xs, a1s = s if xs is None else xs, s if a1s is None else a1s
        return R.conv_bwd_ref(x[xs:xs + 1], a1[a1s:a1s + 1], da2[s:s + 1], W2)[0]

    def swap(new, old):
        return {k: ref[k].astype(np.float64) + new[k] - old[k] for k in ref}

    zero = {k: np.zeros_like(v) for k, v in ref.items()}
    mistakes = [("last sample dropped", swap(zero, one(S - 1)))]
    if S > G:      # workgroup 0's second sample is G
        mistakes.append(("sample G given the screens of sample 0", swap(one(G, xs=0), one(G))))
        mistakes.append(("sample G given the a1 of sample 0", swap(one(G, a1s=0), one(G))))
    if layout == "ring":   # workgroup 0's samples, nvalid ignored (every plane kept)
        all4 = R.RingX(d["frames"], np.full_like(d["nvalid"], 4), n_envs, t_max)
        delta = {k: np.zeros(v.shape) for k, v in ref.items()}
        for s in range(0, S, G):
            new, old = R.conv_bwd_ref(all4[s:s + 1], a1[s:s + 1], da2[s:s + 1], W2)[0], one(s)
            for k in delta:
                delta[k] += new[k].astype(np.float64) - old[k]
        mistakes.append(("nvalid ignored", {k: ref[k] + delta[k] for k in ref}))
    for what, pert in mistakes:
        f = _excess(pert, ref, mag)
        print(f"conv {layout} S={S} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)


# ------------------------------------------------------------------ conv_fwd: tie share, split planes, sensitivity
def _worst(pert, ref):
    """The largest close_normscaled(1e-5) error of the perturbed tensors, in units of the bound."""
    return max(close_normscaled(p, r, RTOL)[1] / RTOL for p, r in zip(pert, ref))


@pytest.mark.parametrize("n_envs,layout", R.CONV_FWD_CASES)
def test_conv_fwd_ties_split_planes_and_sensitivity(n_envs, layout):
    """On the data of every conv_fwd case: the tie band exempts at most 0.1 % of a1 and
    of a2 from the sign checks (each slot); the model of conv1 with the low split
    plane dropped is >= 5x further from the reference than with all three (the GPU
    test holds a1 to a third of the two-plane error); and each mistake the case exists
    for misses the 1e-5 bound by >= 10x (slot 0's samples)."""
    d = R.conv_fwd_data(n_envs, layout)
    N, W = n_envs, (d["W1"], d["b1"], d["W2"], d["b2"])
    a1, a2, z1, z2 = R.conv_fwd_ref(d["x"], *W)
    for t in (0, 1):
        sl = slice(t * N, (t + 1) * N)
        s1, s2 = R.tie_band(z1[sl]).mean(), R.tie_band(z2[sl]).mean()
        e3, e2, e1 = (close_normscaled(R.conv1_split_model(d["xint"][sl], d["W1"], d["b1"], k), a1[sl], RTOL)[1]
                      for k in (3, 2, 1))
        print(f"conv_fwd {layout} N={N} t={t}: tie share a1 {s1:.2g} a2 {s2:.2g}; conv1 model error of the scale, "
              f"3 / 2 / 1 planes: {e3:.3g} / {e2:.3g} / {e1:.3g}")
        assert s1 <= 1e-3 and s2 <= 1e-3, (t, s1, s2)
        assert e3 <= RTOL and e2 >= 5 * e3 and e1 >= 5 * e2, (t, e3, e2, e1)
    x = d["x"][:N]
    ref = (a1[:N], a2[:N])
    W1, b1, W2, b2 = W

    def run(xs=x, W1=W1, b1=b1, W2=W2, b2=b2):
        return R.conv_fwd_ref(xs, W1, b1, W2, b2)[:2]

    W1k, W2k = W1.copy(), W2.copy()
    W1k[:, -1, 7, :] = 0
    W2k[:, :, 3, 3] = 0
    mistakes = [("conv1 bias omitted", run(b1=np.zeros_like(b1))), ("conv2 bias omitted", run(b2=np.zeros_like(b2))),
                ("planes in reverse order", run(np.ascontiguousarray(x[:, ::-1]))),
                ("the last 8 of conv1's 256 terms dropped", run(W1=W1k)), ("one conv2 tap dropped", run(W2=W2k)),
                ("1/256 for 1/255", run(x * np.float32(255 / 256)))]
    if layout == "ring":
        all4 = R.RingX(d["frames"], np.full_like(d["nvalid"], 4), N, 1)
        mistakes.append(("nvalid ignored", run(all4[:N])))
    if layout == "rgb":   # conv planes [0, R, G, B]: the weights meet [0, R, G]
        mistakes.append(("rgb weights on planes 0..2", run(np.concatenate([np.zeros_like(x[:, :1]), x[:, :2]], 1))))
    if N > 1:
        mistakes.append(("env e given env e - 1's screens", run(np.roll(x, 1, 0))))
    for what, pert in mistakes:
        f = _worst(pert, ref)
        print(f"conv_fwd {layout} N={N} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)


# ------------------------------------------------------------------ lstm_bptt
@pytest.mark.parametrize("n_envs,t", R.BPTT_CASES)
def test_bptt_tolerance_catches_step_mistakes(n_envs, t):
    """One env: both forced resets fall on the one row, so dh is masked and only the
    mistakes on the reset flags and the cell's own operands can show."""
    d = R.bptt_data(n_envs, R.BPTT_T, t)
    N = n_envs
    args = dict(dG_t=d["dG"][t], Wl=d["Wl"], reset_t=d["reset"][t], gates=d["gates"][t - 1], c_t=d["cbuf"][t],
                c_prev=d["cbuf"][t - 1], reset_prev=d["reset"][t - 1], dH=d["dh"][t - 1], dcn_in=d["dcn"])
    ref = R.lstm_bptt_ref(**args)
    assert args["reset_t"][0] and args["reset_prev"][N - 1] and (args["c_prev"][N - 1] == R.SENTINEL).all()

    def run(**kw):
        return R.lstm_bptt_ref(**{**args, **kw})

    norst = run(reset_prev=np.zeros(N, np.uint8))
    swapped = args["gates"].copy()
    swapped[:, 1::4], swapped[:, 2::4] = args["gates"][:, 2::4], args["gates"][:, 1::4]
    mistakes = [("reset_t ignored", run(reset_t=np.zeros(N, np.uint8))),
                ("reset_{t-1} ignored in c_prev", (norst[0], ref[1])), ("reset_{t-1} ignored in dcn", (ref[0], norst[1])),
                ("carried dc dropped", run(dcn_in=np.zeros_like(d["dcn"]))),
                ("dH dropped", run(dH=np.zeros_like(args["dH"]))), ("gates i and f swapped", run(gates=swapped))]
    if N > 1:
        half = args["dG_t"].copy()
        half[:, 512:] = 0
        mistakes.append(("one K half dropped from dh", run(dG_t=half)))
        dGc, rsc = args["dG_t"].copy(), args["reset_t"].copy()
        dGc[N - 2], rsc[N - 2] = dGc[N - 1], rsc[N - 1]
        mistakes.append(("row n - 2 given row n - 1's dh", run(dG_t=dGc, reset_t=rsc)))
    for what, pert in mistakes:
        f = _worst(pert, ref)
        print(f"lstm_bptt N={N} t={t} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)


# ------------------------------------------------------------------ returns
@pytest.mark.parametrize("t_max,n_actions,n_envs,lstm",
                         [c + (False,) for c in R.RETURNS_CASES] + [R.RETURNS_LSTM_CASE + (True,)])
def test_returns_tolerance_catches_mistakes(t_max, n_actions, n_envs, lstm):
    """The (1, 1, 1) case is one terminal sample with one action (dlogits = 0, no
    bootstrap, one step): there only the terminal and the clip can show."""
    d = R.returns_data(t_max, n_actions, n_envs, lstm)
    T, A = t_max, n_actions
    args = dict(rewards=d["rewards"], dones=d["dones"], v=d["v"], probs=d["probs"], logp=d["logp"], actions=d["actions"],
                Wpi=d["Wpi"], Wv=d["Wv"], hfc=None if lstm else d["hfc"][:T])
    ref = R.returns_heads_ref(**args)

    def run(**kw):
        return R.returns_heads_ref(**{**args, **kw})

    vb = d["v"].copy()
    vb[T] = vb[T - 1]
    mistakes = [("a terminal not restarting R", run(dones=np.zeros_like(d["dones"]))),
                ("reward clip omitted", run(clip_reward=False))]
    if (T, A, n_envs) != (1, 1, 1):
        Wc = d["Wpi"].copy()
        Wc[A - 1] = d["Wv"][0]
        mistakes += [("bootstrap taken from slot T - 1", run(v=vb)), ("the Wv column used for action A - 1", run(Wpi=Wc))]
    if not lstm and T > 1:
        mistakes.append(("mask taken from the wrong step", run(hfc=np.roll(d["hfc"][:T], 1, 0))))
    if T > 32:
        left = ref[3].copy()
        left[32:] = R.PREFILL
        again = ref[3].copy()
        again[32:] = ref[3][:T - 32]
        mistakes += [("rows >= 32 left unwritten", ref[:3] + (left,)),
                     ("rows >= 32 given rows 0..'s values", ref[:3] + (again,))]
    for what, pert in mistakes:
        f = _worst(pert, ref)
        print(f"returns T={T} A={A} N={n_envs} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)


# ================================================================ the generic implicit-GEMM paths (Nature head, f32 states)
NAT = R.NATURE_NAMES


@functools.lru_cache(maxsize=None)
def _nature_case(case):
    return R.nature_data(*case)


@functools.lru_cache(maxsize=None)
def _nature_conv_bwd_case(case):
    d = _nature_case(case)
    T, S = d["T"], d["S"]
    return R.nature_conv_bwd_ref(d["x"], d["a1"][:T].reshape(S, R.NC1, 20, 20), d["a2"][:T].reshape(S, R.NC2, 9, 9),
                                 d["da3"], d["p"]["0/2/W"], d["p"]["0/1/W"])


@functools.lru_cache(maxsize=None)
def _states_case(case):
    return R.states_data(*case)


def test_nature_refs_equal_oracle_backward():
    """S = 7: the Nature references, fed the oracle's own intermediates, against
    oracle.ff_backward(arch=ARCH_FF_NATURE): the heads', the FC's and conv3's
    gradients bit for bit (both round one float64 sum of the same f32 operands);
    conv2's and conv1's within 1e-6 of the scale (the oracle forms da2 / da1 in
    float32, the reference in float64), as da3 / da2 / da1 / dfc themselves."""
    d = R.conv_data(7, 1, seed=3)
    x = d["x"][:]
    rng = np.random.default_rng(3)
    A = 5
    p = O.init_like_torch(O.ARCH_FF_NATURE, A, rng)
    acts = O.nature_head(p, x)
    a1, a2, a3, h = acts
    r = R.returns_data(1, A, 7, seed=3)
    outs, gh, mh = R.nature_heads_ref(r["rewards"], r["dones"], r["v"], r["probs"], r["logp"], r["actions"], p["1/0/W"],
                                      p["2/0/W"], h[None])
    dl, dv = outs["dlogits"].reshape(7, A).astype(np.float32), outs["dv"].reshape(7).astype(np.float32)
    mag_o = {}
    g_o = O.ff_backward(p, x, acts, dl, dv, arch=O.ARCH_FF_NATURE, mag=mag_o)
    heads = {k: NAT[k] for k in ("piW", "pib", "vW", "vb")}
    _equal(gh, g_o, heads)
    for k, name in heads.items():
        assert np.allclose(mh[k], mag_o[name], rtol=1e-12, atol=0), k
    dfc_o = (dl @ p["1/0/W"] + dv[:, None] * p["2/0/W"]).astype(np.float32) * (h > 0)
    ok, err = close_normscaled(outs["dfc"].reshape(7, -1), dfc_o, 1e-6)
    assert ok, err
    a3f = a3.reshape(7, -1)
    gf, mf = R.nature_fc_bwd_ref(dfc_o, a3f, p["0/3/W"])
    _equal(gf, g_o, {"fcW": NAT["fcW"], "fcb": NAT["fcb"]})
    assert np.allclose(mf["fcW"], O._mag_mm(dfc_o.T, a3f), rtol=1e-12) and np.allclose(mf["fcb"], O._mag_sum(dfc_o))
    da3_o = ((dfc_o @ p["0/3/W"]).reshape(a3.shape) * (a3 > 0)).astype(np.float32)   # oracle._nature_backward
    ok, err = close_normscaled(gf["da3"], da3_o.reshape(7, -1), 1e-6)
    assert ok, err
    assert (gf["da3"][a3f <= 0] == 0).all()
    gc, mc, da2, da1 = R.nature_conv_bwd_ref(x, a1, a2, da3_o, p["0/2/W"], p["0/1/W"])
    _equal(gc, g_o, {"c3W": NAT["c3W"], "c3b": NAT["c3b"]})
    _, _, da2_o = O.conv2d_backward(a2, p["0/2/W"], da3_o, 1)
    da2_o = (da2_o * (a2 > 0)).astype(np.float32)
    _, _, da1_o = O.conv2d_backward(a1, p["0/1/W"], da2_o, 2)
    da1_o = (da1_o * (a1 > 0)).astype(np.float32)
    for got, want, what in ((da2, da2_o, "da2"), (da1, da1_o, "da1")) + tuple(
            (gc[k], g_o[NAT[k]], k) for k in ("c2W", "c2b", "c1W", "c1b")):
        ok, err = close_normscaled(got, want, 1e-6)
        print(f"nature_conv_bwd_ref {what}: {err:.3g} of the scale from the oracle")
        assert ok and got.shape == want.shape, (what, err)
    assert (da2[a2 <= 0] == 0).all() and (da1[a1 <= 0] == 0).all()
    # the error scales: oracle._mag_mm / _mag_sum of the same operands
    gy3 = da3_o.transpose(0, 2, 3, 1).reshape(-1, 64)
    cols3 = O._im2col(a2, 3, 1)[0].reshape(-1, 576)
    assert np.allclose(mc["c3W"].reshape(64, 576), O._mag_mm(gy3.T, cols3), rtol=1e-12)
    assert np.allclose(mc["c3b"], O._mag_sum(gy3), rtol=1e-12)
    # chunks of 3, 3, 1 samples: the same sums to float64 rounding
    g3, m3, _, _ = R.nature_conv_bwd_ref(x, a1, a2, da3_o, p["0/2/W"], p["0/1/W"], chunk=3)
    for k in gc:
        assert np.allclose(g3[k], gc[k], rtol=1e-6, atol=1e-12) and np.allclose(m3[k], mc[k], rtol=1e-12), k


def test_nature_fwd_ref_equals_oracle_head():
    """N = 7 ring states with masked planes: nature_fwd_ref against oracle.nature_head's
    f32 activations within 1e-6 of the scale; a = max(z, 0); policy_ref against the
    oracle's heads and softmax."""
    d = R.conv_data(7, 1, seed=2)
    p = O.init_like_torch(O.ARCH_FF_NATURE, 6, np.random.default_rng(2))
    want = dict(zip(("a1", "a2", "a3", "h"), O.nature_head(p, d["x"][:])))
    got = R.nature_fwd_ref(d["x"], p, chunk=3)
    for k, w in want.items():
        ok, err = close_normscaled(got[k].reshape(w.shape), w, 1e-6)
        print(f"nature_fwd_ref {k}: {err:.3g} of the scale from oracle.nature_head")
        assert ok and got[k].dtype == np.float64, (k, err)
        z = got["z" + k[1:]] if k != "h" else got["zh"]
        assert np.array_equal(got[k], np.maximum(z, 0)) and (z < 0).any()
    lo, vo, _ = O.pi_and_v_ff(p, d["x"][:], O.ARCH_FF_NATURE)
    pol = R.policy_ref(want["h"], p["1/0/W"], p["1/0/b"], p["2/0/W"], p["2/0/b"])
    lp = O.log_softmax(lo)
    for k, w in (("logits", lo), ("v", vo), ("probs", O.softmax(lo)), ("logp", lp),
                 ("entropy", O.entropy(O.softmax(lo), lp))):
        ok, err = close_normscaled(pol[k], w, 1e-6)
        assert ok, (k, err)


def test_returns_heads_ref_gae_equals_the_replay():
    """returns_heads_ref(lam=0.95) against tests/gae_replay.py (the device's own order of
    operations) within 1e-6 of the scale; lam = 1 is the n-step form unchanged."""
    from gae_replay import returns_and_lossgrad_gae
    d = R.returns_data(9, 4, 5)
    T = d["T"]
    args = (d["rewards"], d["dones"], d["v"], d["probs"], d["logp"], d["actions"], d["Wpi"], d["Wv"], d["hfc"][:T])
    dl, dv, loss, _ = R.returns_heads_ref(*args, lam=0.95)
    _, _, dl_o, dv_o, pil, vl = returns_and_lossgrad_gae(d["rewards"], d["dones"], d["v"][:T], d["v"][T], d["probs"],
                                                         d["logp"], d["actions"], lam=0.95, per_env=True)
    for got, want in ((dl, dl_o), (dv, dv_o), (loss[:, 0], pil), (loss[:, 1], vl)):
        ok, err = close_normscaled(got, want, 1e-6)
        assert ok, err
    assert not close_normscaled(dl, R.returns_heads_ref(*args)[0], 1e-3)[0]


def test_ring_x_start_and_states_layout():
    """RingX(start=k0) is oracle.state_from_ring at the slots (k0 + t - 3 + c) % R; rolled()
    moves a window to where another counter finds it; the states layout returns the f32
    ring slot (k0 + t) % R as it is."""
    d = R.conv_data(3, 5, seed=1)
    Rr, base = d["R"], d["x"][:]
    for k0 in [4] + R.ring_starts(5):
        fr, nv = R.rolled(d["frames"], k0, Rr), R.rolled(d["nvalid"], k0, Rr)
        x = R.RingX(fr, nv, 3, 5, start=k0)
        for t in range(5):
            want = O.state_from_ring(fr, nv[(k0 + t) % Rr], [(k0 + t - 3 + c) % Rr for c in range(4)])
            assert np.array_equal(x[3 * t:3 * t + 3], want), (k0, t)
        assert np.array_equal(x[:], base)
        assert k0 % Rr == 0 or not np.array_equal(R.RingX(fr, nv, 3, 5)[:], base)
    s = _states_case((1, 1))
    k0 = 2 ** 32 - 3
    x = R.RingX(R.rolled(s["frames"], k0, 5), None, 1, 1, "states", steps=2, start=k0)
    assert x.shape == (2, 4, 84, 84) and np.array_equal(x[:], s["frames"][:2, 0]) and (s["frames"][2:] == R.SENTINEL).all()
    assert np.array_equal(R.RingX(s["frames"], None, 1, 1, "states", steps=2)[1:2], s["frames"][1])


# ------------------------------------------------------------------ launch geometry of the GPU cases
def test_gemm_launch_geometry():
    """plan_splits / effective_splits / nature_plans / states_plans restated from
    layers.hpp, gemm.hpp, nature.hip and states.hip: the slice and tile counts each case of
    tests/test_gpu_gemm_stages.py exists for."""
    plans = {c: R.nature_plans(c[0] * c[1], c[2]) for c in R.NATURE_CASES + [R.NATURE_HEADS_CASE]}
    assert plans[(33, 5, 18)] == {"heads": 2, "fc": 2, "c3": 64, "c2": 105, "c1": 188}
    assert plans[(1, 1, 4)] == {"heads": 1, "fc": 1, "c3": 1, "c2": 1, "c1": 4}
    assert plans[(67, 2, 6)] == {"heads": 2, "fc": 2, "c3": 52, "c2": 85, "c1": 187}
    assert plans[(41, 9, 4)]["heads"] == 3 and plans[(41, 9, 4)]["fc"] == 2
    assert R.states_plans(165) == {"c2": 105, "c1": 188} and R.states_plans(1) == {"c2": 1, "c1": 4}
    # the first S with two and three slices of the heads / FC weight gradients
    assert [R.nature_plans(S, 6)["heads"] for S in (12, 128, 129, 256, 257)] == [1, 1, 2, 2, 3]
    assert [R.nature_plans(S, 6)["fc"] for S in (12, 128, 129, 257)] == [1, 1, 2, 2]
    # (33, 5, 18), S = 165: shorter last slices, none a whole number of chunks, conv3's and conv2's no multiple of 4
    assert R.slice_bounds(165, 2) == [(0, 96), (96, 165)]
    assert R.slice_bounds(165 * 49, 64)[-1] == (8064, 8085) and R.slice_bounds(165 * 81, 105)[-1] == (13312, 13365)
    assert R.slice_bounds(165 * 400, 188)[-1] == (65824, 66000)
    assert 165 % 4 and (165 * 49) % 4 and (165 * 81) % 4 and 21 % 4 and 53 % 4 and 69 % 32 and 176 % 32
    # slice counts the reduce's 4 slice groups do not divide: 2 (heads, FC), 105 (conv2), 85 and 187 at (67, 2, 6)
    assert 2 % 4 and 105 % 4 and 85 % 4 and 187 % 4 and 3 % 4
    assert R.slice_bounds(369, 3) == [(0, 128), (128, 256), (256, 369)] and R.slice_bounds(369, 2)[-1] == (192, 369)
    # tiles: the heads GEMM's M (A + 1 rows in tiles of 16), the FC forward's M (envs in tiles of 64), ragged edges
    assert R.ceil_div(18 + 1, 16) == 2 and R.ceil_div(4 + 1, 16) == 1 and R.ceil_div(R.NHID + 1, 64) == 9
    # the heads GEMM at the tile edge: A = 15 is one exact 16-row tile, at A = 16 the second tile holds the value row alone
    edge = {c: R.nature_plans(c[0] * c[1], c[2]) for c in R.NATURE_HEADS_EDGE_CASES}
    assert [c[2] for c in edge] == [15, 16] and all(p == {"heads": 1, "fc": 1, "c3": 6, "c2": 10, "c1": 47} for p in edge.values())
    assert (15 + 1) % 16 == 0 and R.ceil_div(15 + 1, 16) == 1 and R.ceil_div(16 + 1, 16) == 2 and (16 + 1) % 16 == 1
    assert R.ceil_div(67, 64) == 2 and 67 % 64 == 3 and R.ceil_div(33, 64) == 1
    assert 165 % 64 == 37 and (165 * 81) % 64 == 53 and (165 * 49) % 64 == 21 and (165 * 100) % 64 == 52
    assert (R.NA3 + 1) % 4 == 1 and (R.NHID + 1) % 4 == 1 and 257 % 4 == 1 and 577 % 64 == 1 and 513 % 64 == 1
    # the FC forward: K = 3136 in 8 slices of 416, the last 224
    assert R.slice_bounds(R.NA3, R.NFC_SPLIT)[-1] == (2912, 3136) and R.effective_splits(R.NA3, R.NFC_SPLIT) == 8
    # returns_kernel: 256 / T envs a workgroup; T <= 8 scans registers
    assert R.returns_blocks(5, 33) == 1 and R.returns_blocks(9, 41) == 2 and 256 // 9 == 28
    for T in (5,):
        assert all(s % (T + 4) for s in R.ring_starts(T)) and R.ring_starts(T)[0] == T + 3
        assert R.ring_starts(T)[2] > 2 ** 40 and R.ring_starts(T)[2] % T == 0


# ------------------------------------------------------------------ tie-band shares of the conv_fwd cases
@pytest.mark.parametrize("case", R.NATURE_CASES)
def test_nature_conv_fwd_tie_share_and_sensitivity(case):
    """On the data of every Nature conv_fwd case (slot 0 and the bootstrap slot): the tie
    band exempts at most 0.1 % of a1, a2 and a3; mistakes (g) nvalid ignored and (h) the
    ring slot taken from t % R under another step counter miss the 1e-5 bound by >= 10x."""
    d = _nature_case(case)
    N, T = d["N"], d["T"]
    x = np.concatenate([d["x_fwd"][:N], d["x_fwd"][T * N:(T + 1) * N]])
    ref = R.nature_fwd_ref(x, d["p"])
    for k in ("1", "2", "3"):
        share = max(R.tie_band(ref["z" + k][sl]).mean() for sl in (slice(0, N), slice(N, 2 * N)))
        print(f"nature conv_fwd {case}: tie share of a{k} {share:.2g}")
        assert share <= R.TIE_SHARE_MAX, (k, share)
    want = [ref[k] for k in ("a1", "a2", "a3")]

    def run(xs):
        out = R.nature_fwd_ref(xs, d["p"])
        return [out[k] for k in ("a1", "a2", "a3")]

    all4 = R.RingX(d["frames"], np.full_like(d["nvalid"], 4), N, T, steps=T + 1)
    mistakes = [("(g) nvalid ignored", run(np.concatenate([all4[:N], all4[T * N:(T + 1) * N]])))]
    if case == R.NATURE_RING_CASE:
        for start in R.ring_starts(T):
            xw = R.RingX(R.rolled(d["frames"], start, d["R"]), R.rolled(d["nvalid"], start, d["R"]), N, T, steps=T + 1)
            mistakes.append((f"(h) slot t % R at step {start}", run(np.concatenate([xw[:N], xw[T * N:(T + 1) * N]]))))
    for what, pert in mistakes:
        f = _worst(pert, want)
        print(f"nature conv_fwd {case} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)


@pytest.mark.parametrize("case", R.STATES_CASES)
def test_states_conv_fwd_tie_share_and_sensitivity(case):
    d = _states_case(case)
    N, T = d["N"], d["T"]
    W = (d["W1"], d["b1"], d["W2"], d["b2"])
    x = np.concatenate([d["x_fwd"][:N], d["x_fwd"][T * N:(T + 1) * N]])
    a1, a2, z1, z2 = R.conv_fwd_ref(x, *W)
    for z, k in ((z1, "a1"), (z2, "a2")):
        share = max(R.tie_band(z[sl]).mean() for sl in (slice(0, N), slice(N, 2 * N)))
        print(f"states conv_fwd {case}: tie share of {k} {share:.2g}")
        assert share <= R.TIE_SHARE_MAX, (k, share)
    assert (x < 0).any() and not np.isin(x[0, 0, 0, :8], O.PHI_LUT).any()
    if case == R.STATES_RING_CASE:
        for start in R.ring_starts(T):
            xw = R.RingX(R.rolled(d["frames"], start, d["R"]), None, N, T, "states", steps=T + 1)
            f = _worst(R.conv_fwd_ref(np.concatenate([xw[:N], xw[T * N:(T + 1) * N]]), *W)[:2], (a1, a2))
            print(f"states conv_fwd {case} (h) slot t % R at step {start}: {f:.3g} x the bound")
            assert f >= 10, (start, f)


# ------------------------------------------------------------------ sensitivity of the backward cases
def _tail(dy, xin, k, s, k0=0):
    """The contribution of the flattened (sample, position) rows [k0, K) to a conv's weight
    and bias gradient (float64): dy (S, OC, OH, OH) f32, xin the conv's input."""
    P = dy.shape[2] * dy.shape[3]
    s0 = k0 // P
    cols = O._im2col(np.ascontiguousarray(xin[s0:]), k, s)[0]
    cols = cols.reshape(-1, cols.shape[-1])
    gy = dy[s0:].transpose(0, 2, 3, 1).reshape(-1, dy.shape[1])
    off = k0 - s0 * P
    return R.mm64(gy[off:].T, cols[off:]), gy[off:].sum(0, dtype=np.float64)


def _k_mistakes(K, Z, part, ref, keys):
    """(a) the last of Z K slices dropped, (e) the last K % 4 elements of K dropped; part(k0)
    -> (dW, db) of the rows [k0, K)."""
    out = []
    if Z > 1:
        out.append(("(a) last K slice dropped", R.slice_bounds(K, Z)[-1][0]))
    if K % 4:
        out.append(("(e) last K % 4 elements dropped", K - K % 4))
    for what, k0 in out:
        dW, db = part(k0)
        yield f"{what} ({keys[0]})", {keys[0]: ref[keys[0]] - dW.reshape(ref[keys[0]].shape), keys[1]: ref[keys[1]] - db}


def _convt1_gather(dy, W, wrap=False):
    """convT(dy, W) of conv3 (k3 s1, 7 x 7 -> 9 x 9) as ConvT1A gathers it: out[y, x] = sum
    dy[y - ky, x - kx] W[ky, kx] with the taps outside the 7 x 7 grid zero.  wrap: mistake (d),
    the tap at ox = -1 not zeroed -- it reads the flat neighbour, the last column of the row
    above."""
    S, OC = dy.shape[:2]
    pad = np.zeros((S, OC, 11, 11))
    pad[:, :, 2:9, 2:9] = dy
    if wrap:
        pad[:, :, 3:9, 1] = dy[:, :, 0:6, 6]
    out = np.zeros((S, W.shape[1], 9, 9))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("sohw,oi->sihw", pad[:, :, 2 - ky:11 - ky, 2 - kx:11 - kx],
                             np.asarray(W[:, :, ky, kx], np.float64))
    return out


def _convt2_wrong_class(dy, W2):
    """Mistake (c): the output parity class (1, 1) of the stride-2 transposed conv computed
    with the taps of class (0, 0) (ky, kx in {0, 2} for {1, 3})."""
    good = R.conv_transpose_ref(dy, W2, 2)
    good[:, :, 1::2, 1::2] = R.conv_transpose_ref(dy, np.roll(W2, (1, 1), (2, 3)), 2)[:, :, 1::2, 1::2]
    return good


@pytest.mark.parametrize("case", R.NATURE_CASES)
def test_nature_conv_bwd_tolerance_catches_gemm_mistakes(case):
    d = _nature_case(case)
    N, T, S, p = d["N"], d["T"], d["S"], d["p"]
    ref, mag, da2, da1 = _nature_conv_bwd_case(case)
    plans = R.nature_plans(S, d["A"])
    a1, a2 = d["a1"][:T].reshape(S, R.NC1, 20, 20), d["a2"][:T].reshape(S, R.NC2, 9, 9)
    da3, d2, d1 = d["da3"], da2.astype(np.float32), da1.astype(np.float32)
    ops = {"c3": (da3, a2, 3, 1, R.NP3), "c2": (d2, a1, 4, 2, R.NP2), "c1": (d1, d["x"], 8, 4, R.NP1)}
    mistakes = []
    for key, (dy, xin, k, s, P) in ops.items():
        mistakes += list(_k_mistakes(S * P, plans[key], lambda k0: _tail(dy, xin, k, s, k0), ref, (key + "W", key + "b")))
    if S > 1:   # (b) the ones column of conv3's OnesCol<Im2col> reads k = 576: channel 0 of the next sample
        nxt = d["a2"].reshape(-1, R.NC2, 9, 9)[1:S + 1, 0, :7, :7]
        mistakes.append(("(b) ones column reads the operand (c3b)",
                         {"c3b": np.einsum("sohw,shw->o", da3.astype(np.float64), nxt)}))
    all4 = R.RingX(d["frames"], np.full_like(d["nvalid"], 4), N, T)
    gW, gb = _tail(d1, all4, 8, 4)
    mistakes.append(("(g) nvalid ignored", {"c1W": gW.reshape(ref["c1W"].shape), "c1b": gb}))
    if case == R.NATURE_RING_CASE:
        for start in R.ring_starts(T):
            xw = R.RingX(R.rolled(d["frames"], start, d["R"]), R.rolled(d["nvalid"], start, d["R"]), N, T)
            mistakes.append((f"(h) slot t % R at step {start}", {"c1W": _tail(d1, xw, 8, 4)[0].reshape(ref["c1W"].shape)}))
    for what, pert in mistakes:
        f = _excess(pert, ref, mag)
        print(f"nature conv_bwd {case} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)
    # the non-reduced outputs
    m2, m1 = a2 > 0, a1 > 0
    good = _convt1_gather(da3, p["0/2/W"]) * m2
    assert close_normscaled(good, da2, 1e-12)[0]
    plain = [("(c) class (1, 1) with class (0, 0)'s taps", _convt2_wrong_class(d2, p["0/1/W"]) * m1, da1),
             ("(d) boundary tap not zeroed", _convt1_gather(da3, p["0/2/W"], wrap=True) * m2, da2)]
    if (S * R.NP2) % 64:   # (f): da2 is (s, ic, p), the GEMM's rows are (s, p)
        t = da2.transpose(0, 2, 3, 1).reshape(S * R.NP2, R.NC2).copy()
        t[(S * R.NP2) // 64 * 64:] = 0
        plain.append(("(f) last partial M tile dropped (da2)", t.reshape(S, 9, 9, R.NC2).transpose(0, 3, 1, 2), da2))
    for what, pert, want in plain:
        f = _worst([pert], [want])
        print(f"nature conv_bwd {case} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)


@pytest.mark.parametrize("case", R.NATURE_CASES + [R.NATURE_HEADS_CASE])
def test_nature_fc_bwd_tolerance_catches_gemm_mistakes(case):
    d = _nature_case(case)
    T, S = d["T"], d["S"]
    dfc, a3 = d["fresh_dfc"](0), d["a3"][:T].reshape(S, R.NA3)
    ref, mag = R.nature_fc_bwd_ref(dfc, a3, d["p"]["0/3/W"])
    mistakes = list(_k_mistakes(S, R.nature_plans(S, d["A"])["fc"],
                                lambda k0: (R.mm64(dfc[k0:].T, a3[k0:]), dfc[k0:].sum(0, dtype=np.float64)), ref,
                                ("fcW", "fcb")))
    nxt = d["a3"].reshape(-1, R.NA3)[1:S + 1, 0]   # OnesColB at j = K: the next sample's first element
    mistakes.append(("(b) ones column reads the operand", {"fcb": R.mm64(dfc.T, nxt)}))
    mistakes.append(("(e) the last N % 4 columns (the bias column) dropped", {"fcb": np.zeros(R.NHID)}))
    for what, pert in mistakes:
        f = _excess(pert, ref, mag)
        print(f"nature fc_bwd {case} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)
    if S % 64:
        pert = ref["da3"].copy()
        pert[S // 64 * 64:] = 0
        f = _worst([pert], [ref["da3"]])
        print(f"nature fc_bwd {case} (f) last partial M tile dropped (da3): {f:.3g} x the bound")
        assert f >= 10, f


@pytest.mark.parametrize("lam", R.GAE_LAMBDAS)
@pytest.mark.parametrize("case", R.NATURE_LEARN_CASES)
def test_nature_heads_tolerance_catches_gemm_mistakes(case, lam):
    d = _nature_case(case)
    T, S, A, p = d["T"], d["S"], d["A"], d["p"]
    args = (d["rewards"], d["dones"], d["v"], d["probs"], d["logp"], d["actions"], p["1/0/W"], p["2/0/W"], d["hfc"][:T])
    outs, ref, mag = R.nature_heads_ref(*args, lam=lam)
    dl, dv = outs["dlogits"].reshape(S, A).astype(np.float32), outs["dv"].reshape(S, 1).astype(np.float32)
    hh = d["hfc"][:T].reshape(S, R.NHID)

    def part(k0):
        return {"piW": R.mm64(dl[k0:].T, hh[k0:]), "pib": dl[k0:].sum(0, dtype=np.float64),
                "vW": R.mm64(dv[k0:].T, hh[k0:]), "vb": dv[k0:].sum(0, dtype=np.float64)}

    mistakes = []
    Z = R.nature_plans(S, A)["heads"]
    assert Z > 1 and S % 4
    for what, k0 in (("(a) last K slice dropped", R.slice_bounds(S, Z)[-1][0]),
                     ("(e) last K % 4 samples dropped", S - S % 4)):
        mistakes.append((what, {k: ref[k] - v for k, v in part(k0).items()}))
    nxt = d["hfc"].reshape(-1, R.NHID)[1:S + 1, 0]
    mistakes.append(("(b) ones column reads the operand", {"pib": R.mm64(dl.T, nxt), "vb": R.mm64(dv.T, nxt)}))
    if (A + 1) % 16 and A + 1 > 16:   # rows 16 .. A of the (A + 1)-row GEMM: the last policy rows and the value row
        w = ref["piW"].copy()
        w[16:] = 0
        mistakes.append(("(f) last partial M tile dropped", {"piW": w, "vW": np.zeros_like(ref["vW"])}))
    w, b = ref["piW"].copy(), ref["pib"].copy()
    w[A - 1], b[A - 1] = ref["vW"][0], ref["vb"][0]
    mistakes.append(("(i) the value row written into the policy rows", {"piW": w, "pib": b}))
    for what, pert in mistakes:
        f = _excess(pert, ref, mag)
        print(f"nature heads {case} lambda={lam} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)
    other = R.returns_heads_ref(*args, lam=1.0 if lam != 1.0 else 0.95)
    f = _worst([other[0], other[3]], [outs["dlogits"], outs["dfc"]])
    print(f"nature heads {case} lambda={lam} the other lambda's advantage: {f:.3g} x the bound")
    assert f >= 10, f


@pytest.mark.parametrize("case", R.STATES_CASES)
def test_states_conv_bwd_tolerance_catches_gemm_mistakes(case):
    d = _states_case(case)
    N, T, S = d["N"], d["T"], d["S"]
    a1, da2, W2 = d["a1"][:T].reshape(S, 16, 20, 20), d["da2"], d["W2"]
    ref, mag = R.conv_bwd_ref(d["x"], a1, da2, W2)
    da1 = R.conv_transpose_ref(da2, W2, 2) * (a1 > 0)
    d1 = da1.astype(np.float32)
    plans = R.states_plans(S)
    mistakes = list(_k_mistakes(S * 81, plans["c2"], lambda k0: _tail(da2, a1, 4, 2, k0), ref, ("c2W", "c2b")))
    mistakes += list(_k_mistakes(S * 400, plans["c1"], lambda k0: _tail(d1, d["x"], 8, 4, k0), ref, ("c1W", "c1b")))
    if case == R.STATES_RING_CASE:
        fr = d["frames"].copy()
        fr[T] = R.SENTINEL
        for start in R.ring_starts(T):
            xw = R.RingX(R.rolled(fr, start, d["R"]), None, N, T, "states")
            mistakes.append((f"(h) slot t % R at step {start}", {"c1W": _tail(d1, xw, 8, 4)[0].reshape(ref["c1W"].shape)}))
    for what, pert in mistakes:
        f = _excess(pert, ref, mag)
        print(f"states conv_bwd {case} {what}: {f:.3g} x the bound")
        assert f >= 10, (what, f)
    f = _worst([_convt2_wrong_class(da2, W2) * (a1 > 0)], [da1])
    print(f"states conv_bwd {case} (c) class (1, 1) with class (0, 0)'s taps: {f:.3g} x the bound")
    assert f >= 10, f


def test_fc_fwd_second_m_tile_sensitivity():
    """(f) on the FC forward at 67 envs: the 3 rows of the second 64-row tile dropped."""
    N = 67
    p = _nature_case((67, 2, 6))["p"]
    a3 = R.act_like(np.random.default_rng([7, N, 0]), (N, R.NA3))
    h = np.maximum(R.mm64(a3, p["0/3/W"].T) + p["0/3/b"], 0.0)
    pert = h.copy()
    pert[64:] = 0
    assert (h[64:] > 0).any() and _worst([pert], [h]) >= 10


# ================================================================ the loss-gradient forms (GAE, PPO, the fused bootstrap)
def _pinned(got, want, what):
    ok, err = close_normscaled(got, want, 1e-6)
    print(f"{what}: {err:.3g} of the scale from the restatement")
    assert ok, (what, err)


def test_lossgrad_refs_equal_the_restatements():
    """returns_heads_ref with pi_loss_coef, keep_loss_scale_same and a truncated tail, and ppo_heads_ref, on a
    T = 8 window closed at t_len = 6 with terminals inside it, against oracle.returns_and_lossgrad,
    gae_replay, ppo_ref.lossgrad and ppo_options_ref.lossgrad_vclip (each the device's own f32 order of
    operations), within 1e-6 of the scale; the heads' dh against the same product of the restatements'
    dlogits / dv."""
    import ppo_options_ref
    import ppo_ref
    from gae_replay import returns_and_lossgrad_gae
    d = R.lossgrad_data(8, 5, 3, t_len=6)
    T, c = d["T"], R.COEF
    dn = d["dones_t"].astype(np.int64)
    term, valid = (dn & 1).astype(np.uint8), (dn & 2) == 0
    assert term[:5].sum() >= 2 and (~valid).sum() == 6 and d["redrawn"] == 0
    hfc = d["hfc"][:T]

    def dh_of(dl, dv):
        return (dl @ d["Wpi"] + dv[..., None] * d["Wv"][0]) * (hfc > 0)

    okw = dict(gamma=c["gamma"], beta=c["beta"], v_loss_coef=c["vcoef"], clip_reward=True, pi_loss_coef=c["pi_loss_coef"],
               keep_loss_scale_same=True, valid=valid)
    oargs = (d["rewards_t"], term, d["v"][:T], d["v"][T], d["probs"], d["logp"], d["actions"])
    for form, lam, want in (("nstep", 1.0, O.returns_and_lossgrad(*oargs, **okw)),
                            ("gae", 0.95, returns_and_lossgrad_gae(*oargs, lam=0.95, **okw))):
        ref = R.lossgrad_ref(d, form, True, lam)
        _, _, dl_o, dv_o, pil, vl = want
        _pinned(ref["dlogits"], dl_o, form + " dlogits")
        _pinned(ref["dv"], dv_o, form + " dv")
        _pinned(ref["dh"], dh_of(dl_o, dv_o), form + " dfc")
        assert np.allclose(ref["loss"].sum(0), [pil, vl], rtol=1e-6, atol=0)
        assert (ref["dh"][~valid] == 0).all() and (ref["dlogits"][~valid] == 0).all()
    assert not close_normscaled(R.lossgrad_ref(d, "nstep", False)["dlogits"], R.lossgrad_ref(d, "nstep", True)["dlogits"],
                                1e-3)[0]   # (the scale does something on this window)
    pargs = (dn, d["v"], d["probs"], d["logp"], d["actions"], d["logp_old"], d["adv"], d["ret"])
    for form, o in (("ppo", ppo_ref.lossgrad(*pargs, R.PPO_CLIP, c["beta"], c["pi_loss_coef"], c["vcoef"], True)),
                    ("ppo_vc", ppo_options_ref.lossgrad_vclip(*pargs, d["v_old"], R.PPO_CLIP, R.PPO_VCLIP, c["beta"],
                                                              c["pi_loss_coef"], c["vcoef"], True))):
        ref = R.lossgrad_ref(d, form, True)
        for k in ("dlogits", "dv", "loss", "ratio"):
            _pinned(ref[k], o[k], f"{form} {k}")
        _pinned(ref["dh"], dh_of(o["dlogits"], o["dv"]), form + " dfc")
        assert 0 < o["active"].sum() < valid.sum() and (ref["ratio"][~valid] == 0).all()
        if form == "ppo_vc":
            assert o["taken"].any() and o["inside"].any() and o["outside_kept"].any() and (ref["dv"][o["taken"]] == 0).all()


def test_fused_bootstrap_ref_equals_oracle():
    """fused_bootstrap_ref against the oracle's f32 FC, heads and softmax of slot T and its
    returns_and_lossgrad with that value as the bootstrap, within 1e-6 of the scale."""
    d = R.fused_data(8, 5, 3)
    T, c = d["T"], R.COEF
    hT, pol, (dl, dv, loss, dfc) = R.fused_bootstrap_ref(
        d["a2T"], d["Wfc"], d["bfc"], d["Wpi"], d["bpi"], d["Wv"], d["bv"], d["rewards"], d["dones"], d["v"], d["probs"],
        d["logp"], d["actions"], d["hfc"][:T], gamma=c["gamma"], beta=c["beta"], vcoef=c["vcoef"],
        pi_loss_coef=c["pi_loss_coef"], keep_loss_scale_same=True)
    h_o = np.maximum(O.linear(d["a2T"], d["Wfc"], d["bfc"]), 0)
    lo, v_o = O.linear(h_o, d["Wpi"], d["bpi"]), O.linear(h_o, d["Wv"], d["bv"])[:, 0]
    for got, want, what in ((hT, h_o, "hfc[T]"), (pol["logits"], lo, "logits"), (pol["v"], v_o, "v[T]"),
                            (pol["probs"], O.softmax(lo), "probs"), (pol["logp"], O.log_softmax(lo), "logp")):
        _pinned(got, want, what)
    _, _, dl_o, dv_o, pil, vl = O.returns_and_lossgrad(
        d["rewards"], d["dones"], d["v"][:T], v_o, d["probs"], d["logp"], d["actions"], gamma=c["gamma"], beta=c["beta"],
        v_loss_coef=c["vcoef"], pi_loss_coef=c["pi_loss_coef"], keep_loss_scale_same=True)
    _pinned(dl, dl_o, "dlogits")
    _pinned(dv, dv_o, "dv")
    _pinned(dfc, (dl_o @ d["Wpi"] + dv_o[..., None] * d["Wv"][0]) * (d["hfc"][:T] > 0), "dfc")
    assert np.allclose(loss.sum(0), [pil, vl], rtol=1e-6, atol=0)
    assert (np.abs(d["zT"]) >= R.MARGIN * np.abs(d["zT"]).max()).all() and (d["zT"] < 0).any()
    assert not np.array_equal(d["v"][T], pol["v"].astype(np.float32))


def test_lossgrad_data_keeps_every_decision_off_its_threshold():
    """Every sample of every GPU case, truncated ones included: near_threshold is empty (lossgrad_data redraws,
    nothing is exempted), both signs of adv, exact zeros in it, and on both sides of every PPO threshold."""
    cases = [(c, None) for c in R.RETURNS_CASES] + R.TRUNC_CASES
    n = {k: 0 for k in ("pos", "neg", "zero", "below", "between", "above", "inside", "outside")}
    lo, hi = R.clip_range(R.PPO_CLIP)
    for case, t_len in cases:
        d = R.lossgrad_data(*case, t_len=t_len)
        assert not R.near_threshold(d).any()
        T = d["T"]
        lpa = np.take_along_axis(d["logp"], d["actions"][..., None].astype(np.int64), 2)[..., 0]
        rho = np.exp(np.asarray(lpa, np.float64) - d["logp_old"])
        dvo = np.abs(np.asarray(d["v"][:T], np.float64) - d["v_old"])
        for k, m in (("pos", d["adv"] > 0), ("neg", d["adv"] < 0), ("zero", d["adv"] == 0), ("below", rho < lo),
                     ("between", (rho > lo) & (rho < hi)), ("above", rho > hi), ("inside", dvo < R.PPO_VCLIP),
                     ("outside", dvo > R.PPO_VCLIP)):
            n[k] += int(m.sum())
        if d["adv"].size >= 24:
            assert (d["adv"] > 0).any() and (d["adv"] < 0).any() and (d["adv"] == 0).any()
    total = n["pos"] + n["neg"] + n["zero"]
    print(n)
    assert all(v > 0 for v in n.values()) and n["zero"] < 0.2 * total
    for case in R.FUSED_CASES:
        z = R.fused_data(*case)["zT"]
        assert (np.abs(z) >= R.MARGIN * np.abs(z).max()).all()


def _run_mistakes(d, form, keep, lam, lstm):
    """{mistake: perturbed reference} of one heads-kernel run: every mistake of the issue's list that can show on
    the run's data; the comments say when one cannot."""
    T = d["T"]
    dn = d["dones_t"].astype(np.int64)
    term, live = (dn & 1) != 0, (dn & 2) == 0
    ref = R.lossgrad_ref(d, form, keep, lam, lstm)
    out = {}

    def run(m):
        return R.lossgrad_ref(d, form, keep, lam, lstm, mistake=m)

    if form == "gae":
        # step RW - 1 must exist, be live and not a terminal (else v[k + 1] is not read there): not at T < RW,
        # not in the T = 8 window truncated to 5 steps
        if T >= R.RW and (live & ~term)[R.RW - 1].any():
            out["v[k + 1] from v[k] at k = RW - 1"] = run("vnext_rw")
        # step T - 1 must be live and not a terminal: not in a truncated window, not in the one-sample case
        if (live & ~term)[T - 1].any():
            out["bootstrap value dropped from the last delta"] = run("no_boot")
        # G is carried only at lambda > 0, and across a terminal only where one has a live step before it
        if lam > 0 and term[1:].any():
            out["a terminal not cutting G"] = run("keep_G")
        # gl multiplies a carried G: a live step that is not a terminal below another live one (not at T = 1)
        if (live[:-1] & ~term[:-1]).any():
            out["gamma where gl belongs"] = R.lossgrad_ref(d, form, keep, 1.0, lstm)
    if form in ("ppo", "ppo_vc"):
        rho, adv = ref["ratio"], np.asarray(d["adv"], np.float64)
        lo, hi = R.clip_range(R.PPO_CLIP)
        # a live sample with adv < 0 whose ratio is outside [lo, hi]: there the two sides decide differently
        if (live & (adv < 0) & ((rho > hi) | (rho < lo))).any():
            out["the clip on the wrong side for adv < 0"] = run("neg_side")
        # only the gradient changes, which is identically 0 with one action (the one-sample case)
        if d["A"] > 1 and (live & (adv != 0)).any():
            out["the ratio not applied to the gradient"] = run("no_ratio")
        if (live & (adv != 0)).any():
            out["lo / hi swapped"] = run("swap")
    if form == "ppo_vc":
        v, vo, Rf = (np.asarray(x, np.float64) for x in (d["v"][:T], d["v_old"], d["ret"]))
        ev = np.float64(np.float32(R.PPO_VCLIP))
        lu, lc, lw = (v - Rf) ** 2, (vo - ev - Rf) ** 2, (vo + ev - Rf) ** 2
        taken = live & (ref["dv"] == 0) & (v != Rf)
        # a live sample whose clipped square is the larger one
        if taken.any():
            out["a clipped-away value sample keeping its gradient"] = run("vc_grad")
        # a live sample below v_old - ev on which the larger square changes: where the unclipped square is the
        # largest of the three (ret above v_old + ev), the loss and the gradient are the unclipped ones either way
        if (live & (v - vo < -ev) & (np.maximum(lu, lc) != np.maximum(lu, lw))).any():
            out["v_old + ev where v_old - ev belongs"] = run("vc_plus")
    if T > 32:
        again = dict(ref)
        again["dh"] = ref["dh"].copy()
        again["dh"][32:] = ref["dh"][:T - 32]
        out["rows >= 32 given rows 0..'s dh"] = again
    if not live.all():   # the dead rows' dh as if they were live steps
        asif = R.lossgrad_ref({**d, "dones_t": (dn & 1).astype(np.uint8)}, form, keep, lam, lstm)
        kept = dict(ref)
        kept["dh"] = np.where(live[..., None], ref["dh"], asif["dh"])
        out["a truncated row's dh not zeroed"] = kept
    # an env with two live terminals: the second one's segment starts after the first
    if keep and ((term & live).sum(0) >= 2).any():
        out["seg_start ignoring the terminal before t"] = run("seg_start")
    return ref, out


LOSSGRAD_MISTAKES = 12   # of the issue's 13; the 13th is the fused form's, below


def test_lossgrad_tolerance_catches_mistakes():
    """Every mistake of _run_mistakes on every heads-kernel run's own data, keep_loss_scale_same off and on, misses
    close_normscaled(1e-5) by more than 10x; each of the mistakes is shown by at least one run.  Prints the
    smallest ratio of each."""
    worst = {}
    for case, form, lam, t_len, lstm in R.lossgrad_runs():
        d = R.lossgrad_data(*case, lstm=lstm, t_len=t_len)
        for keep in (False, True):
            ref, perts = _run_mistakes(d, form, keep, lam, lstm)
            for what, pert in perts.items():
                f = _worst([pert[k] for k in ref], [ref[k] for k in ref])
                assert f >= 10, (what, case, form, lam, t_len, keep, f)
                worst[what] = min(worst.get(what, np.inf), f)
    for what, f in worst.items():
        print(f"lossgrad {what}: at least {f:.3g} x the bound")
    assert len(worst) == LOSSGRAD_MISTAKES, sorted(worst)


def test_fused_tolerance_catches_the_wrong_bootstrap_slot():
    """The fused form bootstrapping from slot T - 1's value (the last the policy stored before it) instead of its
    own row's: more than 10x the bound on every fused case (each has an env whose last step is no terminal)."""
    worst = np.inf
    for case in R.FUSED_CASES:
        d = R.fused_data(*case)
        T, c = d["T"], R.COEF
        assert (d["dones"][T - 1] == 0).any()
        for lam in (1.0, R.GAE_LAMBDA):
            for keep in (False, True):
                kw = dict(gamma=c["gamma"], beta=c["beta"], vcoef=c["vcoef"], pi_loss_coef=c["pi_loss_coef"],
                          keep_loss_scale_same=keep, lam=lam)
                args = (d["probs"], d["logp"], d["actions"], d["Wpi"], d["Wv"], d["hfc"][:T])
                ref = R.fused_bootstrap_ref(d["a2T"], d["Wfc"], d["bfc"], d["Wpi"], d["bpi"], d["Wv"], d["bv"], d["rewards"],
                                            d["dones"], d["v"], d["probs"], d["logp"], d["actions"], d["hfc"][:T], **kw)[2]
                vb = np.concatenate([d["v"][:T], d["v"][T - 1:T]])
                f = _worst(R.returns_heads_ref(d["rewards"], d["dones"], vb, *args, **kw), ref)
                assert f >= 10, (case, lam, keep, f)
                worst = min(worst, f)
    print(f"fused bootstrapping from slot T - 1: at least {worst:.3g} x the bound")
