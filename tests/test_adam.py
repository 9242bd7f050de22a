"""CPU: the host side of Adam (arl_net_set_adam, arl_net_set_adam_t, arl_adam,
asyncrl_amd.Adam) and the oracle of the GPU tests (adam_ref.py) -- no kernel
launches."""
import ctypes
import math

import numpy as np
import pytest

from adam_ref import F32, adam_arrays, adam_elementwise, bits_equal, hooked_grad, lr_t

EINVAL, ESTATE = 1, 3


def test_library_exports_the_adam_symbols():
    from asyncrl_amd import _lib
    for s in ("arl_net_set_adam", "arl_net_set_adam_t", "arl_adam"):
        assert hasattr(_lib.lib, s) and s in _lib.SIGNATURES, s
    assert _lib.CTL_ADAM_T == 3


def test_set_adam_validates_on_the_host():
    """On a handle bound to fake, never-dereferenced pointers: a good call and
    NULL pass; a misaligned m, beta = 1, a negative, infinite or NaN beta fail."""
    from asyncrl_amd._lib import lib
    h = ctypes.c_void_p()
    assert lib.arl_net_create(ctypes.byref(h), 0, 4, 8, 2, 0, 0) == 0
    try:
        fake = 1 << 40
        assert lib.arl_net_set_adam_t(h, 3, None) == ESTATE          # the counter lives in the bound workspace
        assert lib.arl_net_bind(h, fake, fake, fake, fake) == 0
        m = fake + (1 << 30)
        assert lib.arl_net_set_adam(h, m, 0.9, 0.999) == 0
        assert lib.arl_net_set_adam(h, m, 0.0, 0.0) == 0
        assert lib.arl_net_set_adam(h, None, 0.9, 0.999) == 0        # back to RMSpropAsync
        assert lib.arl_net_set_adam(h, None, float("nan"), 2.0) == 0  # (betas are not read then)
        assert lib.arl_net_set_adam(h, m + 4, 0.9, 0.999) == EINVAL
        assert b"aligned" in lib.arl_last_error()
        for b1, b2 in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (float("nan"), 0.999), (0.9, float("nan")),
                       (float("inf"), 0.999), (0.9, -float("inf"))):
            assert lib.arl_net_set_adam(h, m, b1, b2) == EINVAL, (b1, b2)
            assert b"beta" in lib.arl_last_error()
        assert lib.arl_net_set_adam_t(h, -1, None) == EINVAL
    finally:
        lib.arl_net_destroy(h)
    assert lib.arl_net_set_adam(None, None, 0.9, 0.999) == EINVAL


def test_arl_adam_validates_before_launching():
    from asyncrl_amd._lib import lib
    a = (1e-3, 0.9, 0.999, 1e-8)
    assert lib.arl_adam(None, None, None, None, 0, *a, 0, 0.0, None, 0.0, None) == EINVAL      # t = 0
    assert b"t must be" in lib.arl_last_error()
    fake = 1 << 40
    assert lib.arl_adam(fake, fake, fake, fake, 8, *a, 0, 0.0, None, 0.0, None) == EINVAL      # before any launch
    assert lib.arl_adam(fake, fake, fake, fake, 8, *a, -3, 0.0, None, 0.0, None) == EINVAL
    assert lib.arl_adam(fake, fake, fake, fake, 8, 1e-3, 1.0, 0.999, 1e-8, 1, 0.0, None, 0.0, None) == EINVAL
    assert lib.arl_adam(fake, fake, fake, fake, 8, *a, 1, 0.0, None, -1.0, None) == EINVAL     # weight decay
    assert lib.arl_adam(fake, fake, fake, fake, 8, *a, 1, 40.0, None, 0.0, None) == EINVAL     # clip without scratch
    assert lib.arl_adam(fake, fake + 4, fake, fake, 8, *a, 1, 0.0, None, 0.0, None) == EINVAL  # misaligned m
    assert lib.arl_adam(None, None, None, None, -1, *a, 1, 0.0, None, 0.0, None) == EINVAL
    assert lib.arl_adam(None, None, None, None, 0, *a, 1, 0.0, None, 0.0, None) == 0           # n == 0: no launch


def test_lr_property_is_chainers():
    from asyncrl_amd import Adam
    for hyper in (dict(), dict(alpha=7e-4, beta1=0.5, beta2=0.99)):
        o = Adam(**hyper)
        for t in (1, 2, 1000):
            o.t = t
            want = o.alpha * math.sqrt(1.0 - o.beta2 ** t) / (1.0 - o.beta1 ** t)
            assert o.lr == want == lr_t(o.alpha, o.beta1, o.beta2, t)
    o = Adam()
    assert (o.alpha, o.beta1, o.beta2, o.eps) == (0.001, 0.9, 0.999, 1e-8)
    o.t = 1
    assert abs(o.lr - 0.001 * math.sqrt(0.001) / 0.1) < 1e-15
    with pytest.raises(AttributeError):
        o.lr = 0.1                                                   # read-only


def test_hook_rules():
    from asyncrl_amd import Adam, GradientClipping, NonbiasWeightDecay

    def opt(*hooks):
        o = Adam()
        for h in hooks:
            o.add_hook(h)
        return o

    o = opt(GradientClipping(40), NonbiasWeightDecay(1e-4))
    assert (o.clip_threshold, o.weight_decay) == (40.0, 1e-4)
    assert (opt().clip_threshold, opt().weight_decay) == (0.0, 0.0)
    with pytest.raises(ValueError):                                   # would clip the decayed gradient
        opt(NonbiasWeightDecay(0.5), GradientClipping(40))
    with pytest.raises(ValueError):
        opt(GradientClipping(40), GradientClipping(10))
    with pytest.raises(ValueError):
        opt(NonbiasWeightDecay(0.1), NonbiasWeightDecay(0.1))

    class Lasso:
        name = "Lasso"

    with pytest.raises(TypeError):
        opt(Lasso())


def test_update_args():
    from asyncrl_amd import Adam, GradientClipping
    o = Adam(alpha=3e-4, eps=1e-5)
    o.add_hook(GradientClipping(40))
    a = o.update_args()
    assert a["lr0"] == 3e-4 and a["eps"] == 1e-5 and a["clip"] == 40.0 and a["total_steps"] == 0 and o.t == 1
    assert sorted(a) == ["alpha", "clip", "eps", "lr0", "n_total", "total_steps"]      # RMSpropAsync's keys
    o.anneal_total_steps = 1000
    with pytest.raises(ValueError):
        o.update_args()
    assert o.t == 1
    o.n_total_envs = 8
    assert o.update_args()["n_total"] == 8 and o.t == 2


def test_array_form_equals_the_operation_list():
    """The oracle's NumPy array evaluation of Chainer's three lines against the
    header's operation list, one rounding at a time: 4 updates on carried
    state, with +-0 gradients, a clip scale and a decay."""
    rng = np.random.default_rng(7)
    n = 1500
    p = rng.standard_normal(n).astype(F32)
    m1 = v1 = m2 = v2 = np.zeros(n, F32)
    p1 = p2 = p
    for t in range(1, 5):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(F32)
        g[:4] = [0.0, -0.0, 0.0, -0.0]
        g1 = hooked_grad(p1, g, scale=0.37 if t == 2 else None, rate=0.3 if t > 2 else 0.0)
        lr = lr_t(1e-3, 0.9, 0.999, t)
        p1, m1, v1 = adam_arrays(p1, m1, v1, g1, lr, 0.9, 0.999, 1e-8)
        p2, m2, v2 = adam_elementwise(p2, m2, v2, hooked_grad(p2, g, scale=0.37 if t == 2 else None,
                                                              rate=0.3 if t > 2 else 0.0), lr, 0.9, 0.999, 1e-8)
        assert bits_equal(p1, p2) and bits_equal(m1, m2) and bits_equal(v1, v2), t
    assert not bits_equal(p1, p) and np.isfinite(p1).all()
