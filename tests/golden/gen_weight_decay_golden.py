"""Generate tests/golden/weight_decay_golden.npz from the reference's OWN
NonbiasWeightDecay hook and RMSpropAsync.

Run where a checkout of the reference is at hand (nothing is copied; its
modules are imported at generation time only):
    python tests/golden/gen_weight_decay_golden.py <reference checkout>

What runs from the reference, verbatim:
  * nonbias_weight_decay.NonbiasWeightDecay.__call__ (the CPU branch),
  * rmsprop_async.RMSpropAsync (init_state, update_one_cpu),
driven by `opt.update()` of the Chainer stand-in tests/golden/chainer_stub.py
(hooks in insertion order, then update_one per parameter), which is installed
as gen_golden.py installs it and not edited.  The three `chainer.cuda` names
the hook touches and the stub lacks are added here: `available = False`,
`get_device` (a context manager whose int() is -1, Chainer's DummyDevice) and
`elementwise` (never reached).

The model is a small stub Chain with W and b parameters at two nesting depths
and one bias-free link (shaped like L.LSTM's upward / lateral), tensors of 1
to 300 elements.  Three consecutive updates per case, fresh gradients each:
  a  NonbiasWeightDecay(0.3) alone;
  b  GradientClipping(40) that does not trigger, then NonbiasWeightDecay(0.3);
  c  GradientClipping(40) that triggers (gradients x 10), then the decay; with
     |p| ~ 1 the decayed gradient's norm is far from the norm that clipped.
Per case the file holds, flat in namedparams order: p0 (ms starts at 0, as
Optimizer.setup leaves it), g[step] as fed in, p[step] and ms[step] after
each update; `names` / `sizes` give the layout.  Data only.
"""
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, CLIP, STEPS = 0.3, 40.0, 3
LR, ALPHA, EPS = 7e-4, 0.99, 1e-1   # a3c_ale.py:224


class _DummyDevice:
    def __int__(self):
        return -1


@contextlib.contextmanager
def _get_device(*arrays):
    yield _DummyDevice()


def _elementwise(*a, **k):
    raise AssertionError("chainer.cuda.elementwise: the GPU branch is not reached")


def build_chain(ch, rng):
    """root: fc (W, b), head (W, b: one element), rnn = Chain(upward (W, b), lateral (W only))."""
    def link(w_shape, bias=True):
        lk = ch.Link()
        lk.add_param("W", w_shape)
        if bias:
            lk.add_param("b", (w_shape[0],))
        return lk

    rnn = ch.Chain(upward=link((8, 5)), lateral=link((8, 8), bias=False))
    root = ch.Chain(fc=link((3, 100)), head=link((1, 7)), rnn=rnn)
    for _, p in root.namedparams():
        p.data[...] = rng.standard_normal(p.data.shape).astype(np.float32)
    return root


def is_bias(name):
    return name == "b" or name.endswith("/b")


def run_case(ch, NonbiasWeightDecay, RMSpropAsync, seed, clip, gscale):
    rng = np.random.default_rng(seed)
    model = build_chain(ch, rng)
    opt = RMSpropAsync(lr=LR, eps=EPS, alpha=ALPHA)
    opt.setup(model)
    if clip:                                    # a3c_ale.py:226-228: clip, then decay
        opt.add_hook(sys.modules["chainer.optimizer"].GradientClipping(CLIP))
    opt.add_hook(NonbiasWeightDecay(RATE))
    named = list(model.namedparams())
    flat = lambda arrs: np.concatenate([np.asarray(a, np.float32).ravel() for a in arrs])  # noqa: E731
    out = {"p0": flat(p.data for _, p in named), "g": [], "p": [], "ms": [], "norm": []}
    for _ in range(STEPS):
        for _, p in named:
            p.grad = (rng.standard_normal(p.data.shape) * gscale).astype(np.float32)
        out["g"].append(flat(p.grad for _, p in named))
        out["norm"].append(opt.compute_grads_norm())
        opt.update()
        out["p"].append(flat(p.data for _, p in named))
        out["ms"].append(flat(opt._states[n]["ms"] for n, _ in named))
    for k in ("g", "p", "ms"):
        out[k] = np.stack(out[k])
    out["norm"] = np.asarray(out["norm"], np.float64)
    return [n for n, _ in named], [p.data.size for _, p in named], out


def main(ref):
    sys.path.insert(0, HERE)
    import chainer_stub
    chainer_stub.install()
    cuda = sys.modules["chainer.cuda"]
    cuda.available = False
    cuda.get_device = _get_device
    cuda.elementwise = _elementwise
    sys.path.insert(0, ref)
    from nonbias_weight_decay import NonbiasWeightDecay
    from rmsprop_async import RMSpropAsync
    sys.path.remove(ref)

    save = {"rate": np.float64(RATE), "clip": np.float64(CLIP), "lr": np.float64(LR), "alpha": np.float64(ALPHA),
            "eps": np.float64(EPS)}
    for case, (seed, clip, gscale) in {"a": (11, False, 1.0), "b": (12, True, 1.0), "c": (13, True, 10.0)}.items():
        names, sizes, out = run_case(chainer_stub, NonbiasWeightDecay, RMSpropAsync, seed, clip, gscale)
        if case == "b":
            assert (out["norm"] < CLIP).all(), out["norm"]
        if case == "c":
            assert (out["norm"] > 2 * CLIP).all(), out["norm"]
        # "bit-exact" must pin the two roundings of g += rate * p: on the recorded non-bias elements of
        # the first update, f32(g + f32(f32(rate) * p)) and the single-rounding (FMA) form must differ
        nb = np.concatenate([np.full(s, not is_bias(n)) for n, s in zip(names, sizes)])
        p, g = out["p0"][nb], out["g"][0][nb]
        two = g + np.float32(RATE) * p
        one = (g.astype(np.float64) + np.float64(np.float32(RATE)) * p.astype(np.float64)).astype(np.float32)
        assert two.dtype == np.float32 and (two != one).any(), case
        print("case %s: %d params, %d non-bias, %d differ between two roundings and one; norms %s"
              % (case, nb.size, int(nb.sum()), int((two != one).sum()), np.round(out["norm"], 2)))
        for k, v in out.items():
            save[f"{case}_{k}"] = v
    # names as Chainer yields them ('/fc/W', ...); the layout is the same in every case
    save["names"] = np.array(names)
    save["sizes"] = np.array(sizes, np.int64)
    assert sorted(n for n in names if not is_bias(n)) == ["/fc/W", "/head/W", "/rnn/lateral/W", "/rnn/upward/W"]
    path = os.path.join(HERE, "weight_decay_golden.npz")
    np.savez_compressed(path, **save)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
