"""CPU tests of tests/stage_ref.py: the stage references against the oracle,
the launch geometry restated from the .hip sources, and the sensitivity of
the GPU stage tests' tolerance to the mistakes they exist to catch."""
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
