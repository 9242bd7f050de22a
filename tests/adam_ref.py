"""The oracle of the Adam tests: a NumPy float32 restatement of the arithmetic
in include/asyncrl_hip.h ("Adam"), which is Chainer 1.8.1's optimizers.Adam

    m += (1 - beta1) * (grad - m)
    v += (1 - beta2) * (grad * grad - v)
    param -= lr * m / (numpy.sqrt(v) + eps),   lr = alpha * sqrt(1 - beta2**t) / (1 - beta1**t)

on float32 arrays, preceded by the two hooks in the reference's order: the
GradientClipping scale (one f32 factor), then NonbiasWeightDecay
(g = f32(g + f32(f32(rate) * p)) outside the biases).  The reference has no
Adam; adam_elementwise is the same list of operations one element and one
rounding at a time, and test_adam.py holds the two forms equal bit for bit."""
import math

import numpy as np

F32 = np.float32


def lr_t(alpha, beta1, beta2, t):
    """Python floats, left to right: Chainer's Adam.lr for update t >= 1."""
    fix1 = 1.0 - beta1 ** t
    fix2 = 1.0 - beta2 ** t
    return alpha * math.sqrt(fix2) / fix1


def annealed_alpha(alpha, total_steps, global_t):
    """The on-device anneal of the update's step size (a3c_ale.py:111-112),
    clamped at 0 past the budget."""
    return max(total_steps - global_t - 1, 0) / total_steps * alpha


def hooked_grad(p, g, scale=None, rate=0.0, decay=None):
    """g after the hooks: * f32(scale) when the clip triggered (scale < 1),
    then + f32(f32(rate) * p) where decay (a bool mask; None = everywhere)."""
    g = np.asarray(g, F32).copy()
    if scale is not None and scale < 1:
        g = (g * F32(scale)).astype(F32)
    if rate > 0:
        d = (g + (F32(rate) * np.asarray(p, F32)).astype(F32)).astype(F32)
        g = d if decay is None else np.where(decay, d, g)
    return g


def adam_arrays(p, m, v, g, lr, beta1, beta2, eps):
    """Chainer's three lines on f32 arrays; lr: the step size (rounded to f32
    here, as a Python float meets an f32 array).  Returns (p', m', v')."""
    p, m, v = (np.asarray(x, F32).copy() for x in (p, m, v))
    g = np.asarray(g, F32)
    m += F32(1.0 - beta1) * (g - m)
    v += F32(1.0 - beta2) * (g * g - v)
    p -= F32(lr) * m / (np.sqrt(v) + F32(eps))
    return p, m, v


def adam_elementwise(p, m, v, g, lr, beta1, beta2, eps):
    """The operation list of the header, one f32 rounding per operation."""
    c1, c2, l, e = F32(1.0 - beta1), F32(1.0 - beta2), F32(lr), F32(eps)
    p, m, v = (np.asarray(x, F32).copy() for x in (p, m, v))
    g = np.asarray(g, F32)
    for i in range(p.size):
        gi = F32(g[i])
        m[i] = F32(m[i] + F32(c1 * F32(gi - m[i])))
        v[i] = F32(v[i] + F32(c2 * F32(F32(gi * gi) - v[i])))
        p[i] = F32(p[i] - F32(F32(l * m[i]) / F32(F32(np.sqrt(v[i])) + e)))
    return p, m, v


def bits_equal(a, b) -> bool:
    """Bitwise on f32 (== would take -0.0 for +0.0)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def ulp_apart(a, b) -> int:
    """Distance of two positive (or zero) f32 values in units in the last place."""
    return abs(int(F32(a).view(np.uint32)) - int(F32(b).view(np.uint32)))
