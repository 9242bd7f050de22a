"""CPU: NonbiasWeightDecay (nonbias_weight_decay.py, a3c_ale.py:227-228) -- the
NumPy restatement of one reference update against the fixture recorded from
the reference's own hook and optimizer (tests/golden/gen_weight_decay_golden.py),
the host side of arl_net_set_weight_decay, and RMSpropAsync.add_hook's rules.

One update of the reference, hooks in insertion order (clip, then decay):
  1. norm = sqrt(sum g^2) of the gradient before the decay; if clip / norm < 1:
     g *= f32(clip / norm);
  2. every parameter whose name is not 'b' and does not end in '/b':
     t = f32(f32(rate) * p); g = f32(g + t)   (two roundings, not an FMA);
  3. update_one_cpu on that g.
Without a triggering clip every op is an elementwise f32 op, so the
restatement is bit-exact; a triggering clip goes through the norm, whose f32
rounding differs by summation order, hence the tolerance of
test_rmsprop_tiny_arrays_match_oracle's clipped case (rtol 1e-6, atol 1e-7
for p, 1e-9 for ms)."""
import ctypes

import numpy as np
import pytest

import oracle as O
from conftest import golden

F32 = np.float32
CLIP_TOL = dict(p=dict(rtol=1e-6, atol=1e-7), ms=dict(rtol=1e-6, atol=1e-9))


def is_bias(name: str) -> bool:
    """nonbias_weight_decay.py:22."""
    return name == "b" or name.endswith("/b")


def reference_update(p, ms, g, rate, clip, lr=7e-4, alpha=0.99, eps=0.1, exact_norm=False, decay_first=False):
    """Steps 1-3 on dicts name -> f32 array; returns (p', ms').  rate 0: no
    decay hook.  decay_first: the WRONG hook order (decay, then clip by the
    decayed gradient's norm), for the tests that show the order matters."""
    names = list(p)
    g = {n: np.asarray(g[n], F32).copy() for n in names}

    def clip_():
        if clip > 0:
            gs, _ = O.clip_grads([g[n] for n in names], clip, exact_norm=exact_norm)
            g.update(zip(names, gs))

    def decay_():
        for n in names:
            if rate > 0 and not is_bias(n):
                t = (F32(rate) * np.asarray(p[n], F32)).astype(F32)
                g[n] = (g[n] + t).astype(F32)

    for hook in ((decay_, clip_) if decay_first else (clip_, decay_)):
        hook()
    out = {n: O.rmsprop_update(np.asarray(p[n], F32), np.asarray(ms[n], F32), g[n], lr, alpha, eps) for n in names}
    return {n: out[n][0] for n in names}, {n: out[n][1] for n in names}


def close(kind, got, want):
    return np.allclose(got, want, **CLIP_TOL[kind])


def _split(flat, names, sizes):
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return {n: flat[offs[i]:offs[i + 1]] for i, n in enumerate(names)}


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_restatement_reproduces_reference_fixture(case):
    """Three consecutive opt.update() calls of the reference (decay alone; clip
    not triggering + decay; clip triggering + decay): a and b bit-exact, c
    within the clipped-update tolerance -- and for c the wrong hook order is
    far outside it."""
    z = golden("weight_decay_golden.npz")
    names = [str(n).lstrip("/") for n in z["names"]]
    sizes = z["sizes"]
    assert any(is_bias(n) for n in names) and "rnn/lateral/W" in names and "rnn/upward/b" in names
    rate, clip = float(z["rate"]), float(z["clip"]) if case != "a" else 0.0
    hyper = dict(lr=float(z["lr"]), alpha=float(z["alpha"]), eps=float(z["eps"]))
    p = _split(z[f"{case}_p0"], names, sizes)
    ms = {n: np.zeros_like(v) for n, v in p.items()}
    for step in range(z[f"{case}_g"].shape[0]):
        g = _split(z[f"{case}_g"][step], names, sizes)
        want_p = _split(z[f"{case}_p"][step], names, sizes)
        want_ms = _split(z[f"{case}_ms"][step], names, sizes)
        triggered = clip > 0 and z[f"{case}_norm"][step] > clip
        assert triggered == (case == "c")
        p1, ms1 = reference_update(p, ms, g, rate, clip, **hyper)
        for n in names:
            if triggered:
                assert close("p", p1[n], want_p[n]) and close("ms", ms1[n], want_ms[n]), (step, n)
            else:
                assert (p1[n] == want_p[n]).all() and (ms1[n] == want_ms[n]).all(), (step, n)
        # the decay is in the fixture: the same update without it misses every non-bias tensor
        p0, _ = reference_update(p, ms, g, 0.0, clip, **hyper)
        for n in names:
            same = close("p", p0[n], want_p[n]) if triggered else bool((p0[n] == want_p[n]).all())
            assert is_bias(n) == same, (step, n)
        if triggered:   # decay before clip: the decay enters the norm
            pw, msw = reference_update(p, ms, g, rate, clip, decay_first=True, **hyper)
            assert not all(close("p", pw[n], want_p[n]) and close("ms", msw[n], want_ms[n]) for n in names)
        p, ms = want_p, want_ms   # continue from the reference's own state


def test_single_rounding_form_misses_the_fixture():
    """The fixture pins the two roundings of g += rate * p: an FMA-style single
    rounding differs on recorded non-bias elements (case a, first update)."""
    z = golden("weight_decay_golden.npz")
    names = [str(n).lstrip("/") for n in z["names"]]
    nb = np.concatenate([np.full(s, not is_bias(n)) for n, s in zip(names, z["sizes"])])
    p, g = z["a_p0"][nb], z["a_g"][0][nb]
    r = F32(float(z["rate"]))
    two = (g + (r * p).astype(F32)).astype(F32)
    one = (g.astype(np.float64) + np.float64(r) * p.astype(np.float64)).astype(F32)
    assert (two != one).any()


@pytest.mark.parametrize("arch", [0, 1, 2, 17, 33])
def test_set_weight_decay_host_state(arch):
    """arl_net_set_weight_decay: host state of an unbound handle; rejects a
    negative, NaN or infinite rate with ARL_EINVAL and a message."""
    from asyncrl_amd._lib import lib
    h = ctypes.c_void_p()
    assert lib.arl_net_create(ctypes.byref(h), arch, 4, 8, 2, 0, 0) == 0
    try:
        assert lib.arl_net_set_weight_decay(h, 0.0) == 0
        assert lib.arl_net_set_weight_decay(h, 1e-4) == 0
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert lib.arl_net_set_weight_decay(h, bad) == 1, bad
            assert b"weight_decay" in lib.arl_last_error()
        assert lib.arl_net_set_weight_decay(h, 0.3) == 0
    finally:
        lib.arl_net_destroy(h)
    assert lib.arl_net_set_weight_decay(None, 0.1) == 1


def test_rmsprop_wd_validates_before_launching():
    from asyncrl_amd._lib import lib
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.arl_rmsprop_wd(None, None, None, 0, 7e-4, 0.99, 0.1, 0.0, None, bad, None) == 1
    assert lib.arl_rmsprop_wd(None, None, None, -1, 7e-4, 0.99, 0.1, 0.0, None, 0.1, None) == 1
    assert lib.arl_rmsprop_wd(None, None, None, 0, 7e-4, 0.99, 0.1, 0.0, None, 0.1, None) == 0   # n == 0: no launch


def test_hook_rules():
    from asyncrl_amd import GradientClipping, NonbiasWeightDecay, RMSpropAsync
    assert NonbiasWeightDecay.name == "NonbiasWeightDecay" and NonbiasWeightDecay(0.25).rate == 0.25

    def opt(*hooks):
        o = RMSpropAsync(lr=7e-4, eps=0.1, alpha=0.99)
        for h in hooks:
            o.add_hook(h)
        return o

    o = opt(GradientClipping(40), NonbiasWeightDecay(1e-4))          # the reference's order
    assert (o.clip_threshold, o.weight_decay) == (40.0, 1e-4)
    o = opt(NonbiasWeightDecay(0.5))                                  # decay alone
    assert (o.clip_threshold, o.weight_decay) == (0.0, 0.5)
    o = opt(GradientClipping(40))
    assert (o.clip_threshold, o.weight_decay) == (40.0, 0.0)
    with pytest.raises(ValueError):                                   # would clip the decayed gradient
        opt(NonbiasWeightDecay(0.5), GradientClipping(40))
    with pytest.raises(ValueError):
        opt(GradientClipping(40), GradientClipping(10))
    with pytest.raises(ValueError):
        opt(GradientClipping(40), NonbiasWeightDecay(0.1), NonbiasWeightDecay(0.1))

    class Lasso:
        name = "Lasso"

    with pytest.raises(TypeError):                                    # not dropped silently
        opt(Lasso())
