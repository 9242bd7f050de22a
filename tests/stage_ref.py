"""Plain float64 NumPy references of single learner / forward stages, the
synthetic operands they are tested on, and the launch geometry of the HIP
kernels that run them (tests/test_stage_ref.py pins all of it on the CPU,
tests/test_gpu_stages.py compares arl_run_stage with it).  Nothing here
touches a device.

Every reduction over the window's S = t_max * n_envs samples is accumulated
in float64 and rounded to float32 once, as oracle.gmm / oracle.gsum do, and
comes with the oracle's per-element error scale (oracle._mag_mm / _mag_sum)
for conftest.grads_match."""
import numpy as np

import oracle as O

F32, F64 = np.float32, np.float64
HID, GATES, A1, A2, A2W = 256, 1024, 6400, 2592, 81
SENTINEL = F32(1e6)     # rows / slots a stage must not use (finite: a kernel may multiply a staged row by 0)
PREFILL = 1234.5        # outputs before a launch: every element must be overwritten

# ---------------------------------------------------------------- launch geometry (fc_bwd.hip, conv_bwd.hip)
BK, RST_MAX = 32, 1024
PART = 128 * 64 + 128   # floats of one published job A partial (dW tile + db)
NTA_FC, NTA_LSTM = 82, 64


def fc_bwd_ranges(S):
    return max(1, min(16, (S + 400) // 800))


def lstm_wgrad_ranges(S):
    return max(fc_bwd_ranges(S), -(-S // RST_MAX))


def range_len(S, Z):
    return (-(-S // Z) + BK - 1) // BK * BK


def ranges(S, lstm=False):
    """(Z, samples per range) of job A: launch_fc_bwd, or launch_lstm_wgrad with lstm."""
    Z = lstm_wgrad_ranges(S) if lstm else fc_bwd_ranges(S)
    return Z, range_len(S, Z)


def range_bounds(S, lstm=False):
    """[r0, r1) of every job A range."""
    Z, kpz = ranges(S, lstm)
    return [(z * kpz, min(S, (z + 1) * kpz)) for z in range(Z)]


def blocks(S):
    """conv_bwd_blocks: workgroup b handles samples b, b + G, ..."""
    return min(S, 256)


def part_floats(S):
    """fc_bwd_part_floats: the fc_bwd_partials buffer serves both launches."""
    return max(NTA_FC * fc_bwd_ranges(S), NTA_LSTM * lstm_wgrad_ranges(S)) * PART


# ---------------------------------------------------------------- references
def mm64(a, b):
    """a @ b in float64, not rounded (the inside of oracle.gmm)."""
    return np.asarray(a, F64) @ np.asarray(b, F64)


def fc_bwd_ref(dfc, a2, W, dlogits, dv, hh):
    """The fc_bwd stage: gW = dfc^T a2, gb = sum_s dfc, da2 = (dfc W) * (a2 > 0)
    and the heads' weight gradients over hh.  Returns (g, mag), float32."""
    dvc = dv[:, None]
    g = {"fcW": mm64(dfc.T, a2), "fcb": dfc.sum(0, dtype=F64),
         "piW": mm64(dlogits.T, hh), "pib": dlogits.sum(0, dtype=F64),
         "vW": mm64(dvc.T, hh), "vb": dvc.sum(0, dtype=F64),
         "da2": mm64(dfc, W) * (a2 > 0)}
    mag = {"fcW": O._mag_mm(dfc.T, a2), "fcb": O._mag_sum(dfc), "piW": O._mag_mm(dlogits.T, hh),
           "pib": O._mag_sum(dlogits), "vW": O._mag_mm(dvc.T, hh), "vb": O._mag_sum(dvc)}
    return {k: v.astype(F32) for k, v in g.items()}, mag


def lstm_wgrad_ref(dG, hfc, hprev, reset, Wu):
    """The lstm_wgrad stage: gWu = dG^T hfc, gWl = dG^T (hprev * (reset == 0)),
    gbu = sum_s dG, dfc = (dG Wu) * (hfc > 0).  Returns (g, mag), float32."""
    hp = hprev * (np.asarray(reset) == 0)[:, None]
    g = {"gWu": mm64(dG.T, hfc), "gWl": mm64(dG.T, hp), "gbu": dG.sum(0, dtype=F64),
         "dfc": mm64(dG, Wu) * (hfc > 0)}
    mag = {"gWu": O._mag_mm(dG.T, hfc), "gWl": O._mag_mm(dG.T, hp), "gbu": O._mag_sum(dG)}
    return {k: v.astype(F32) for k, v in g.items()}, mag


class _Mag:
    """oracle._mag_mm of a reduction accumulated over chunks of its samples."""

    def __init__(self, M, N):
        self.sa, self.ab, self.sb, self.X, self.Y = np.zeros(M), np.zeros((M, N)), np.zeros(N), 0.0, 0.0

    def add(self, a, b):   # a (M, s), b (s, N): float64 copies of the caller's, overwritten here
        np.abs(a, out=a)
        np.abs(b, out=b)
        self.sa += np.einsum("ij,ij->i", a, a)
        self.ab += a @ b
        self.sb += np.einsum("ij,ij->j", b, b)
        self.X, self.Y = max(self.X, float(a.max())), max(self.Y, float(b.max()))

    def mm(self):
        X, Y = self.X, self.Y
        return np.sqrt(Y * Y * self.sa[:, None] + 2.0 * X * Y * self.ab + X * X * self.sb[None, :])


def conv_bwd_ref(x, a1, da2, W2, chunk=64):
    """The conv_bwd + conv_reduce stages: gW2, gb2 of conv2 (16 -> 32, k4 s2) from
    da2 and a1, da1 = convT(da2, W2) * (a1 > 0), gW1, gb1 of conv1 (k8 s4) from da1
    and x -- oracle.conv2d_backward's mathematics (da1 itself in float32, as
    there), the four sums accumulated in float64 over chunks of <= chunk samples.
    x: anything with .shape and [i:j] -> (n, C, 84, 84) float32 (an array, or RingX).
    Returns (g, mag), float32."""
    S, C = x.shape[0], x.shape[1]
    gW2, gb2, gW1, gb1 = np.zeros((32, 256)), np.zeros(32), np.zeros((16, C * 64)), np.zeros(16)
    m2, m1 = _Mag(32, 256), _Mag(16, C * 64)
    W2f = W2.reshape(32, -1)
    for c0 in range(0, S, chunk):
        xs, a1s, d2 = x[c0:c0 + chunk], a1[c0:c0 + chunk], da2[c0:c0 + chunk]
        n = a1s.shape[0]
        cols2, oh, ow = O._im2col(a1s, 4, 2)
        cols2 = cols2.reshape(-1, 256)
        gy2 = d2.transpose(0, 2, 3, 1).reshape(-1, 32)
        a64, b64 = np.asarray(gy2.T, F64), np.asarray(cols2, F64)
        gW2 += a64 @ b64
        gb2 += gy2.sum(0, dtype=F64)
        m2.add(a64, b64)
        gcol = (gy2 @ W2f).reshape(n, oh, ow, 16, 4, 4)
        gx = np.zeros_like(a1s)
        for ky in range(4):
            for kx in range(4):
                gx[:, :, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2] += gcol[:, :, :, :, ky, kx].transpose(0, 3, 1, 2)
        da1 = (gx * (a1s > 0)).astype(F32)
        cols1 = O._im2col(xs, 8, 4)[0].reshape(-1, C * 64)
        gy1 = da1.transpose(0, 2, 3, 1).reshape(-1, 16)
        a64, b64 = np.asarray(gy1.T, F64), np.asarray(cols1, F64)
        gW1 += a64 @ b64
        gb1 += gy1.sum(0, dtype=F64)
        m1.add(a64, b64)
    g = {"c2W": gW2.reshape(32, 16, 4, 4), "c2b": gb2, "c1W": gW1.reshape(16, C, 8, 8), "c1b": gb1}
    mag = {"c2W": m2.mm().reshape(32, 16, 4, 4), "c2b": np.full(32, m2.X * np.sqrt(S * 81.0)),
           "c1W": m1.mm().reshape(16, C, 8, 8), "c1b": np.full(16, m1.X * np.sqrt(S * 400.0))}
    return {k: v.astype(F32) for k, v in g.items()}, mag


class RingX:
    """The conv input of every window sample s = t * n_envs + e, built from the
    frame ring a chunk at a time, as oracle.state_from_ring does with the
    control block's step at 0 (R = t_max + 4 slots):
      ring   frames (R, N, 84, 84): plane c = frames[(t - 3 + c) % R, e]
      stack  frames (R, N, 4, 84, 84): plane c of frames[t % R, e]
      rgb    frames (R, N, 3, 84, 84): the three planes of frames[t % R, e]
    through O.PHI_LUT; ring / stack planes c < 4 - nvalid[t % R, e] are zero."""

    def __init__(self, frames, nvalid, n_envs, t_max, layout="ring"):
        self.frames, self.nvalid, self.N, self.R, self.layout = frames, nvalid, n_envs, t_max + 4, layout
        self.shape = (t_max * n_envs, 3 if layout == "rgb" else 4, 84, 84)

    def __getitem__(self, sl):
        s = np.arange(self.shape[0])[sl]
        t, e = s // self.N, s % self.N
        if self.layout == "rgb":
            return O.PHI_LUT[self.frames[t % self.R, e]]
        if self.layout == "stack":
            x = O.PHI_LUT[self.frames[t % self.R, e]]
        else:
            x = np.stack([O.PHI_LUT[self.frames[(t - 3 + c) % self.R, e]] for c in range(4)], 1)
        keep = np.arange(4)[None, :] >= 4 - self.nvalid[t % self.R, e].astype(np.int32)[:, None]
        return np.where(keep[:, :, None, None], x, F32(0.0))


def pack_a2_mask(a2):
    """(..., 2592) activations -> (..., 81) uint32: bit i of word w is a2[..., 32 w + i] > 0
    (conv_fwd.hip's a2_mask buffer, fc_bwd.hip job B's ReLU mask)."""
    bits = (np.asarray(a2) > 0).reshape(a2.shape[:-1] + (A2W, 32)).astype(np.uint32)
    return (bits << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)


def unpack_a2_mask(words):
    bits = (np.asarray(words, np.uint32)[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(words.shape[:-1] + (A2,)).astype(bool)


# ---------------------------------------------------------------- data recipes
def grad_like(rng, shape):
    """normal * 1e-3, about half the entries exactly 0 (as a ReLU mask leaves them)."""
    return rng.standard_normal(shape, F32) * F32(1e-3) * (rng.random(shape, F32) < 0.5)


def act_like(rng, shape):
    """max(normal, 0): post-ReLU activations with exact zeros."""
    return np.maximum(rng.standard_normal(shape, F32), F32(0))


def weight_like(rng, shape):
    """U(+-1/sqrt(fan_in)), as init_like_torch."""
    b = 1.0 / np.sqrt(int(np.prod(shape[1:])))
    return rng.uniform(-b, b, shape).astype(F32)


def fc_data(n_envs, t_max, n_actions=6, lstm=False, seed=0):
    """Operands of the fc_bwd stage.  a2 / hfc carry the bootstrap slot t_max as a
    sentinel; lstm: the heads read hbuf slot t + 1 (hbuf slots 0 and t_max + 1
    sentinels).  fresh_dfc(k): the dfc of launch k."""
    rng = np.random.default_rng([seed, n_envs, t_max, 1])
    N, T, S = n_envs, t_max, n_envs * t_max
    d = {"N": N, "T": T, "S": S, "A": n_actions}
    a2 = act_like(rng, (T + 1, N, A2))
    a2[T] = SENTINEL
    d["a2"] = a2
    h = act_like(rng, (T + 2 if lstm else T + 1, N, HID))
    if lstm:
        h[0] = h[T + 1] = SENTINEL
        d["hbuf"], d["hh"] = h, h[1:T + 1].reshape(S, HID)
    else:
        h[T] = SENTINEL
        d["hfc"], d["hh"] = h, h[:T].reshape(S, HID)
    d["W"] = weight_like(rng, (HID, A2))
    d["dlogits"], d["dv"] = grad_like(rng, (S, n_actions)), grad_like(rng, (S,))
    d["fresh_dfc"] = lambda k: grad_like(np.random.default_rng([seed, n_envs, t_max, 2, k]), (S, HID))
    return d


def lstm_data(n_envs, t_max, seed=0):
    """Operands of the lstm_wgrad stage.  reset is ~20 % ones, and 1 on row 0 and on
    the first and last sample of every job A range (the rows DMA'd from the zero
    row at a range boundary).  fresh_dG(k): the dG of launch k."""
    rng = np.random.default_rng([seed, n_envs, t_max, 3])
    N, T, S = n_envs, t_max, n_envs * t_max
    hfc = act_like(rng, (T + 1, N, HID))
    hfc[T] = SENTINEL
    hbuf = rng.normal(size=(T + 2, N, HID)).astype(F32) * F32(0.5)
    hbuf[T:] = SENTINEL
    reset = np.ones((T + 1) * N, np.uint8)
    reset[:S] = rng.random(S) < 0.2
    reset[0] = 1
    for r0, r1 in range_bounds(S, lstm=True):
        reset[r0] = reset[r1 - 1] = 1
    return {"N": N, "T": T, "S": S, "hfc": hfc, "hbuf": hbuf, "reset": reset.reshape(T + 1, N),
            "Wu": weight_like(rng, (GATES, HID)),
            "fresh_dG": lambda k: grad_like(np.random.default_rng([seed, n_envs, t_max, 4, k]), (S, GATES))}


def conv_data(n_envs, t_max, layout="ring", seed=0):
    """Operands of the conv_bwd stage.  a1 carries the bootstrap slot as a sentinel.
    ring: nvalid drawn from 1..4 (env 0 of slot 0 below 4, so a one-sample case has
    a masked plane); stack: 4, rgb: 3, as the observation kernels leave them."""
    rng = np.random.default_rng([seed, n_envs, t_max, 5])
    N, T, S, R = n_envs, t_max, n_envs * t_max, t_max + 4
    planes = {"ring": (), "stack": (4,), "rgb": (3,)}[layout]
    frames = rng.integers(0, 256, (R, N) + planes + (84, 84), dtype=np.uint8)
    if layout == "ring":
        nvalid = rng.integers(1, 5, (R, N)).astype(np.uint8)
        nvalid[0, 0] = 2
    else:
        nvalid = np.full((R, N), 4 if layout == "stack" else 3, np.uint8)
    a1 = act_like(rng, (T + 1, N, 16, 20, 20))
    a1[T] = SENTINEL
    return {"N": N, "T": T, "S": S, "R": R, "layout": layout, "frames": frames, "nvalid": nvalid, "a1": a1,
            "da2": grad_like(rng, (S, 32, 9, 9)), "W2": weight_like(rng, (32, 16, 4, 4)),
            "x": RingX(frames, nvalid, N, T, layout)}


# the cases of tests/test_gpu_stages.py, (n_envs, t_max); tests/test_stage_ref.py runs the
# sensitivity check on the same list
FC_CASES = [(1, 1), (43, 3), (109, 11), (240, 5), (241, 5), (400, 5)]
FC_LSTM_ARCH_CASE = (41, 5)
LSTM_CASES = [(1, 1), (43, 3), (256, 4), (205, 5), (400, 5)]
CONV_CASES = [(1, 1), (255, 1), (257, 1), (52, 5), (67, 9), (513, 5)]
CONV_LAYOUT_CASE = (52, 5)   # also run as rgb (DoomA3CFF) and stack
LAUNCHES = 4                 # at Z > 1: launches in a row, each with fresh gradients
