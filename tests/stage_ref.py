"""Plain float64 NumPy references of single learner / forward stages, the
synthetic operands they are tested on, and the launch geometry of the HIP
kernels that run them (tests/test_stage_ref.py pins all of it on the CPU,
tests/test_gpu_stages.py and tests/test_gpu_gemm_stages.py compare
arl_run_stage with it, tests/test_gpu_lossgrad_stages.py the loss-gradient
launches in their GAE, PPO and fused forms).  Nothing here touches a device.

Every reduction over the window's S = t_max * n_envs samples is accumulated
in float64 and rounded to float32 once, as oracle.gmm / oracle.gsum do, and
comes with the oracle's per-element error scale (oracle._mag_mm / _mag_sum)
for conftest.grads_match.  The references of stages without such a reduction
(conv_fwd, lstm_bptt, returns) return float64."""
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
    control block's step at `start` (R = t_max + 4 slots; k = start + t):
      ring   frames (R, N, 84, 84): plane c = frames[(k - 3 + c) % R, e]
      stack  frames (R, N, 4, 84, 84): plane c of frames[k % R, e]
      rgb    frames (R, N, 3, 84, 84): the three planes of frames[k % R, e]
      states frames (R, N, 4, 84, 84) float32: frames[k % R, e] as it is (no
             lut, no nvalid: the ARCH_STATES ring of phi's output)
    through `lut` (O.PHI_LUT; PIXELS: the integer pixel values); ring / stack planes
    c < 4 - nvalid[k % R, e] are zero.  steps: the window slots covered (t_max;
    t_max + 1 takes in the bootstrap slot)."""

    def __init__(self, frames, nvalid, n_envs, t_max, layout="ring", steps=None, lut=None, start=0):
        self.frames, self.nvalid, self.N, self.R, self.layout = frames, nvalid, n_envs, t_max + 4, layout
        self.lut = O.PHI_LUT if lut is None else lut
        self.start = int(start)
        self.shape = ((t_max if steps is None else steps) * n_envs, 3 if layout == "rgb" else 4, 84, 84)

    def __getitem__(self, sl):
        s = np.arange(self.shape[0])[sl]
        t, e = s // self.N, s % self.N
        k = t + self.start % self.R + self.R   # the residue, as Python's % of the whole counter (k - 3 >= 0)
        if self.layout == "states":
            return self.frames[k % self.R, e]
        if self.layout == "rgb":
            return self.lut[self.frames[k % self.R, e]]
        if self.layout == "stack":
            x = self.lut[self.frames[k % self.R, e]]
        else:
            x = np.stack([self.lut[self.frames[(k - 3 + c) % self.R, e]] for c in range(4)], 1)
        keep = np.arange(4)[None, :] >= 4 - self.nvalid[k % self.R, e].astype(np.int32)[:, None]
        return np.where(keep[:, :, None, None], x, F32(0.0))


def pack_a2_mask(a2):
    """(..., 2592) activations -> (..., 81) uint32: bit i of word w is a2[..., 32 w + i] > 0
    (conv_fwd.hip's a2_mask buffer, fc_bwd.hip job B's ReLU mask)."""
    bits = (np.asarray(a2) > 0).reshape(a2.shape[:-1] + (A2W, 32)).astype(np.uint32)
    return (bits << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)


def unpack_a2_mask(words):
    bits = (np.asarray(words, np.uint32)[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(words.shape[:-1] + (A2,)).astype(bool)


# ---------------------------------------------------------------- conv_fwd
PIXELS = np.arange(256, dtype=F32)   # RingX(lut=PIXELS): the integer pixel values conv_fwd.hip multiplies
TIE_REL = 1e-5                       # oracle.relu_mask's tie band: |z| < TIE_REL * max|z|


def conv_fwd_ref(x, W1, b1, W2, b2, chunk=64):
    """The conv_fwd stage in float64 from the f32 state x (an array, or RingX):
    z1 = conv(x, W1, s4) + b1, a1 = max(z1, 0), z2 = conv(a1, W2, s2) + b2 on the
    float64 a1, a2 = max(z2, 0); chunks of <= chunk samples.  Returns (a1, a2, z1,
    z2), float64, (S, 16, 20, 20) and (S, 32, 9, 9)."""
    S, C = x.shape[0], x.shape[1]
    W1f, W2f = np.asarray(W1, F64).reshape(16, C * 64).T, np.asarray(W2, F64).reshape(32, 256).T
    z1, z2 = np.empty((S, 16, 20, 20)), np.empty((S, 32, 9, 9))
    for c0 in range(0, S, chunk):
        xs = np.ascontiguousarray(x[c0:c0 + chunk])
        n = xs.shape[0]
        cols = O._im2col(xs, 8, 4)[0].reshape(-1, C * 64)
        z = (np.asarray(cols, F64) @ W1f + np.asarray(b1, F64)).reshape(n, 20, 20, 16).transpose(0, 3, 1, 2)
        z1[c0:c0 + n] = z
        cols = O._im2col(np.maximum(z1[c0:c0 + n], 0.0), 4, 2)[0].reshape(-1, 256)
        z2[c0:c0 + n] = (cols @ W2f + np.asarray(b2, F64)).reshape(n, 9, 9, 32).transpose(0, 3, 1, 2)
    return np.maximum(z1, 0.0), np.maximum(z2, 0.0), z1, z2


def tie_band(z, rel=TIE_REL):
    """Pre-activations within rounding of 0, where either ReLU decision is a correct
    f32 result (oracle.relu_mask's rule); the sign checks exempt them."""
    return np.abs(z) < rel * np.abs(z).max()


def split_bf16(w, planes=3):
    """bf16split.hpp's split3 of f32 w: the first `planes` of the truncated pieces
    h, m, l (w = h + m + l exactly), as f32 arrays."""
    out, r = [], np.asarray(w, F32)
    for _ in range(planes):
        piece = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
        out.append(piece)
        r = r - piece   # exact
    return out


def conv1_split_model(xint, W1, b1, planes=3, chunk=64):
    """A model of conv_fwd.hip's conv1 arithmetic: the integer pixels xint (RingX with
    lut=PIXELS) times the first `planes` bf16 pieces of W1, each product exact, the
    sums in f32 (piece h in one accumulator, m and l in a second, as mfma_x3_t),
    1/255 applied to the sum, then the bias and the ReLU.  planes < 3: the mistake of
    a dropped low split plane.  Returns a1 (S, 16, 20, 20), float32."""
    S, C = xint.shape[0], xint.shape[1]
    Wp = [p.reshape(16, C * 64).T.copy() for p in split_bf16(W1, planes)]
    out = np.empty((S, 16, 20, 20), F32)
    for c0 in range(0, S, chunk):
        xs = np.ascontiguousarray(xint[c0:c0 + chunk])
        n = xs.shape[0]
        cols = O._im2col(xs, 8, 4)[0].reshape(-1, C * 64)
        big, sml = cols @ Wp[0], np.zeros((cols.shape[0], 16), F32)
        for p in Wp[:0:-1]:
            sml = sml + cols @ p
        z = ((big + sml).astype(F64) / 255.0).astype(F32) + np.asarray(b1, F32)   # div255: the IEEE quotient
        out[c0:c0 + n] = np.maximum(z, F32(0)).reshape(n, 20, 20, 16).transpose(0, 3, 1, 2)
    return out


# ---------------------------------------------------------------- lstm_bptt
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_bptt_ref(dG_t, Wl, reset_t, gates, c_t, c_prev, reset_prev, dH, dcn_in, first=False):
    """The lstm_bptt stage, step t -> t - 1, in float64: dh = dG_t Wl, zeroed on rows
    with reset_t; then F.lstm's backward of step t - 1 (lstm_cell_bwd_elem, net.hip)
    with dh + dH and the carried dc: gates (n, 1024) interleaved four per unit (a, i,
    f, o), c_t the cell after step t - 1, c_prev before it (read as 0 on rows with
    reset_prev, whose dcn_out is 0).  first: the window's last step (no dh, no
    carried dc; dG_t, Wl, reset_t, dcn_in unused).  Returns (dG_prev, dcn_out)."""
    n = gates.shape[0]
    dh, dc_in = np.asarray(dH, F64), 0.0
    if not first:
        dh = dh + mm64(dG_t, Wl) * (np.asarray(reset_t) == 0)[:, None]
        dc_in = np.asarray(dcn_in, F64)
    g = np.asarray(gates, F64).reshape(n, HID, 4)
    a, i, f, o = np.tanh(g[..., 0]), _sig(g[..., 1]), _sig(g[..., 2]), _sig(g[..., 3])
    rp = (np.asarray(reset_prev) != 0)[:, None]
    tc = np.tanh(np.asarray(c_t, F64))
    cp = np.where(rp, 0.0, np.asarray(c_prev, F64))
    dc = dh * o * (1.0 - tc * tc) + dc_in
    dG = np.stack([dc * i * (1.0 - a * a), dc * a * i * (1.0 - i), dc * cp * f * (1.0 - f), dh * tc * o * (1.0 - o)], -1)
    return dG.reshape(n, GATES), np.where(rp, 0.0, dc * f)


def lstm_bptt_chain_ref(Wl, reset, gates, cbuf, dH):
    """The window's truncated BPTT (LEARN_TRUNK's cell launch and its T - 1 lstm_bptt
    launches), t = T - 1 ... 0, in float64 throughout: reset (>= T, N), gates (>= T,
    N, 1024), cbuf (>= T + 1, N, 256) with slot t the cell before step t, dH (T, N,
    256).  Returns dG (T, N, 1024)."""
    T = dH.shape[0]
    dG = np.empty((T,) + gates.shape[1:], F64)
    dG[T - 1], dcn = lstm_bptt_ref(None, None, None, gates[T - 1], cbuf[T], cbuf[T - 1], reset[T - 1], dH[T - 1], None,
                                   first=True)
    for t in range(T - 1, 0, -1):
        dG[t - 1], dcn = lstm_bptt_ref(dG[t], Wl, reset[t], gates[t - 1], cbuf[t], cbuf[t - 1], reset[t - 1], dH[t - 1], dcn)
    return dG


# ---------------------------------------------------------------- returns
RW = 8   # policy.hip: windows up to RW steps are scanned from registers

# mistake=: the deliberate mistakes of tests/test_stage_ref.py's sensitivity checks, None everywhere else


def segment_factor(dones, keep_scale=True, mistake=None):
    """keep_loss_scale_same (a3c.py:116-121) as returns_compute applies it: the loss terms of a live
    step whose segment -- from the step after the previous terminal to the first terminal at or after
    it -- a terminal closed after len < T steps carry T / len; every other step 1.  dones (T, N) with
    bit 0 = terminal, bit 1 = past a truncated window's end.  Returns (T, N) float64.
    mistake "seg_start": the segment's start ignores the terminal before t."""
    T, N = dones.shape
    f = np.ones((T, N))
    if not keep_scale:
        return f
    term = (np.asarray(dones).astype(np.int64) & 1) != 0
    for e in range(N):
        start = 0
        for t in range(T):
            if term[t, e]:
                if t - start + 1 < T:
                    f[start:t + 1, e] = T / (t - start + 1)
                start = t + 1 if mistake != "seg_start" else start
    return f


def _heads_dh(dlogits, dv, Wpi, Wv, hfc, live):
    """dh = dlogits Wpi + dv Wv, times (hfc > 0) with hfc, 0 on the rows that are not live."""
    dh = dlogits @ np.asarray(Wpi, F64) + dv[..., None] * np.asarray(Wv, F64).reshape(-1)
    if hfc is not None:
        dh = dh * (np.asarray(hfc) > 0)
    return dh * live[..., None]


def returns_heads_ref(rewards, dones, v, probs, logp, actions, Wpi, Wv, hfc=None, gamma=0.99, beta=0.01, vcoef=0.5,
                      clip_reward=True, lam=1.0, pi_loss_coef=1.0, keep_loss_scale_same=False, mistake=None):
    """The returns stage (returns_heads_kernel, policy.hip) in float64 from the f32
    buffers: oracle.returns_and_lossgrad's mathematics (R restarted at terminals,
    rewards clipped to +-1) on rewards / dones (T, N), v (T + 1, N) with slot T the
    bootstrap value, probs / logp (T, N, A), actions (T, N); the heads' backward
    dh = dlogits Wpi + dv Wv, and with hfc (T, N, 256) dfc = dh * (hfc > 0).
    dones: bit 0 = terminal, bit 1 = past a truncated window's end (arl_truncate_window):
    there dlogits, dv, dh and the loss terms are 0.
    lam != 1: the policy term's advantage is GAE(lambda) (arl_net_set_gae: delta_k =
    r_k + gamma v_{k+1} - v_k with v_{k+1} = 0 at a terminal, the scan cut there);
    the value target stays the n-step return.
    pi_loss_coef / vcoef scale the two loss terms, and with keep_loss_scale_same both
    carry segment_factor's T / len.
    Returns dlogits (T, N, A), dv (T, N), loss (N, 2) = per-env (pi, v) losses and
    dh (or dfc) (T, N, hidden width).
    mistake (GAE): "vnext_rw" v[k + 1] taken from v[k] at k = RW - 1, "no_boot" the bootstrap value
    dropped from the delta of step T - 1, "keep_G" a terminal that does not cut G; "seg_start"."""
    T, N = rewards.shape
    r = np.asarray(rewards, F64)
    if clip_reward:
        r = np.clip(r, -1.0, 1.0)
    dn = np.asarray(dones).astype(np.int64)
    term, live = (dn & 1) != 0, (dn & 2) == 0
    v, p, lp = np.asarray(v, F64), np.asarray(probs, F64), np.asarray(logp, F64)
    R, Rs = v[T].copy(), np.empty((T, N))
    for t in reversed(range(T)):
        R = np.where(term[t], 0.0, R) * gamma + r[t]
        Rs[t] = R
    adv = Rs - v[:T]
    if lam != 1.0:
        G, adv = np.zeros(N), np.empty((T, N))
        for t in reversed(range(T)):
            vn = v[t] if mistake == "vnext_rw" and t == RW - 1 else v[t + 1]
            vn = np.where(term[t] | (mistake == "no_boot" and t == T - 1), 0.0, vn)
            G = (r[t] + gamma * vn - v[t]) + gamma * lam * np.where(term[t] & (mistake != "keep_G"), 0.0, G)
            adv[t] = G
    scale = segment_factor(dn, keep_loss_scale_same, mistake) * live
    pf, vf = pi_loss_coef * scale, vcoef * scale
    H = -(p * lp).sum(-1)
    onehot = np.zeros_like(p)
    np.put_along_axis(onehot, np.asarray(actions, np.int64)[..., None], 1.0, axis=2)
    dlogits = pf[..., None] * (-adv[..., None] * (onehot - p) + beta * p * (lp + H[..., None]))
    dv = vf * (v[:T] - Rs)
    lp_a = np.take_along_axis(lp, np.asarray(actions, np.int64)[..., None], 2)[..., 0]
    loss = np.stack([-(pf * (lp_a * adv + beta * H)).sum(0), (vf * (v[:T] - Rs) ** 2 / 2).sum(0)], 1)
    return dlogits, dv, loss, _heads_dh(dlogits, dv, Wpi, Wv, hfc, live)


def clip_range(clip_eps):
    """lo, hi of the clipped surrogate as the host forms them: one float64 operation each, rounded to f32."""
    return F32(1.0 - float(clip_eps)), F32(1.0 + float(clip_eps))


def ppo_heads_ref(dones, v, probs, logp, actions, logp_old, adv, ret, Wpi, Wv, hfc=None, clip_eps=0.2, beta=0.01,
                  vcoef=0.5, pi_loss_coef=1.0, keep_loss_scale_same=False, v_old=None, vclip_eps=None, mistake=None):
    """One clipped-surrogate epoch's loss gradient and heads backward (the RF_PPO / RF_PPO_VC forms of
    returns_heads_kernel) in float64 from the f32 buffers: the snapshot logp_old / adv / ret (T, N), the
    current v (>= T, N), probs / logp (T, N, A), actions (T, N).  rho = exp(logp[a] - logp_old); a sample is
    active while rho <= hi (adv >= 0) or rho >= lo (adv < 0): its policy gradient is that of rho * adv and
    its loss term rho * adv, else no policy gradient and the term hi * adv or lo * adv.  With v_old and
    vclip_eps the value loss is max((v - ret)^2, (v_c - ret)^2) / 2, v_c = v_old + clamp(v - v_old, +-
    vclip_eps); dv is 0 where the clipped square is the larger one.  Rows past a truncated window's end
    (dones bit 1) are 0 throughout, the ratio included.
    Returns dlogits (T, N, A), dv (T, N), ratio (T, N), loss (N, 2) and dh (or dfc).
    mistake: "neg_side" the clip applied on the hi side for adv < 0 too, "no_ratio" the ratio not applied to
    the gradient, "swap" lo / hi swapped, "vc_grad" a clipped-away value sample keeps its gradient, "vc_plus"
    v_old + ev where v_old - ev belongs; "seg_start"."""
    dn = np.asarray(dones).astype(np.int64)
    T, N = dn.shape
    live = (dn & 2) == 0
    vi, p, lp = np.asarray(v, F64)[:T], np.asarray(probs, F64)[:T], np.asarray(logp, F64)[:T]
    ac = np.asarray(actions, np.int64)[:T, :, None]
    lpo, adv, Rf = np.asarray(logp_old, F64), np.asarray(adv, F64), np.asarray(ret, F64)
    lo, hi = (F64(x) for x in clip_range(clip_eps)[::-1 if mistake == "swap" else 1])
    scale = segment_factor(dn, keep_loss_scale_same, mistake) * live
    pf, vf = pi_loss_coef * scale, vcoef * scale
    rho = np.exp(np.take_along_axis(lp, ac, 2)[..., 0] - lpo)
    pos = adv >= 0
    active = np.where(pos | (mistake == "neg_side"), rho <= hi, rho >= lo)
    surr = np.where(active, rho * adv, np.where(pos | (mistake == "neg_side"), hi, lo) * adv)
    w = np.where(active, adv if mistake == "no_ratio" else rho * adv, 0.0)
    H = -(p * lp).sum(-1)
    onehot = np.zeros_like(p)
    np.put_along_axis(onehot, ac, 1.0, axis=2)
    dlogits = pf[..., None] * (-w[..., None] * (onehot - p) + beta * p * (lp + H[..., None]))
    dvv = vi - Rf
    lsq, taken = dvv * dvv, np.zeros((T, N), bool)
    if v_old is not None:
        ev = F64(F32(vclip_eps))
        dvo = vi - np.asarray(v_old, F64)
        lc = (np.asarray(v_old, F64) + np.clip(dvo, ev if mistake == "vc_plus" else -ev, ev) - Rf) ** 2
        taken = (np.abs(dvo) > ev) & (lc > lsq)
        lsq = np.where(taken, lc, lsq)
    dv = np.where(taken & (mistake != "vc_grad"), 0.0, vf * dvv)
    loss = np.stack([-(pf * (surr + beta * H)).sum(0), (vf * lsq * 0.5).sum(0)], 1)
    return dlogits, dv, rho * live, loss, _heads_dh(dlogits, dv, Wpi, Wv, hfc, live)


def fused_bootstrap_ref(a2T, Wfc, bfc, Wpi, bpi, Wv, bv, rewards, dones, v, probs, logp, actions, hfc=None, **kw):
    """The bootstrap step with the learner's first launch folded in (policy_fc_returns_kernel) in float64:
    hfc[T] = relu(a2[T] Wfc^T + b) from a2T (N, 2592), the heads of slot T through policy_ref, then
    returns_heads_ref with that v[T] as the bootstrap value (v: (>= T, N), rows 0 .. T - 1 are read).
    Returns (hfc[T], policy_ref's dict of slot T, returns_heads_ref's tuple)."""
    T = rewards.shape[0]
    hT = np.maximum(mm64(a2T, np.asarray(Wfc).T) + np.asarray(bfc, F64), 0.0)
    pol = policy_ref(hT, Wpi, bpi, Wv, bv)
    vv = np.concatenate([np.asarray(v, F64)[:T], pol["v"][None]])
    return hT, pol, returns_heads_ref(rewards, dones, vv, probs, logp, actions, Wpi, Wv, hfc, **kw)


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


def conv_fwd_data(n_envs, layout="ring", seed=0, t_max=1):
    """Operands of the conv_fwd stage on a t_max = 1 net (slots 0 and 1, a ring of 5):
    frames and nvalid as conv_data (ring: nvalid from 1..4, a masked plane on env 0
    of both slots), the two convs' weights and biases, and x: RingX over both
    slots, sample t * n_envs + e; xint: the same with integer pixel values.
    t_max > 1: a ring of t_max + 4 and all t_max + 1 slots, env 0 masked at slot
    t_max too."""
    rng = np.random.default_rng([seed, n_envs, t_max, 6])
    N, T, R = n_envs, t_max, t_max + 4
    planes = {"ring": (), "stack": (4,), "rgb": (3,)}[layout]
    frames = rng.integers(0, 256, (R, N) + planes + (84, 84), dtype=np.uint8)
    if layout == "ring":
        nvalid = rng.integers(1, 5, (R, N)).astype(np.uint8)
        nvalid[0, 0], nvalid[1, 0], nvalid[T, 0] = 2, 3, 3
    else:
        nvalid = np.full((R, N), 4 if layout == "stack" else 3, np.uint8)
    C = 3 if layout == "rgb" else 4
    d = {"N": N, "T": T, "R": R, "layout": layout, "frames": frames, "nvalid": nvalid,
         "W1": weight_like(rng, (16, C, 8, 8)), "W2": weight_like(rng, (32, 16, 4, 4))}
    d["b1"], d["b2"] = rng.uniform(-1 / 16, 1 / 16, 16).astype(F32), rng.uniform(-1 / 16, 1 / 16, 32).astype(F32)
    d["x"] = RingX(frames, nvalid, N, T, layout, steps=T + 1)
    d["xint"] = RingX(frames, nvalid, N, T, layout, steps=T + 1, lut=PIXELS)
    return d


def bptt_data(n_envs, t_max, t, seed=0):
    """Operands of one lstm_bptt step t -> t - 1.  reset is ~20 % ones at steps t and
    t - 1, 1 on row 0 at step t and on the last row at step t - 1, 1 elsewhere;
    every dG / gates / cbuf / dh slot the step must not read holds the sentinel,
    as does c_prev (cbuf slot t - 1) on the rows with reset_{t-1}."""
    rng = np.random.default_rng([seed, n_envs, t_max, t, 7])
    N, T = n_envs, t_max
    reset = np.ones((T + 1, N), np.uint8)
    reset[t - 1:t + 1] = rng.random((2, N)) < 0.2
    reset[t, 0] = reset[t - 1, N - 1] = 1
    dG = np.full((T, N, GATES), SENTINEL, F32)
    dG[t] = grad_like(rng, (N, GATES))
    gates = np.full((T + 1, N, GATES), SENTINEL, F32)
    gates[t - 1] = rng.standard_normal((N, GATES), F32)
    cbuf = np.full((T + 2, N, HID), SENTINEL, F32)
    cbuf[t - 1:t + 1] = rng.standard_normal((2, N, HID), F32)
    cbuf[t - 1][reset[t - 1] != 0] = SENTINEL
    dh = np.full((T, N, HID), SENTINEL, F32)
    dh[t - 1] = rng.standard_normal((N, HID), F32) * F32(1e-3)
    return {"N": N, "T": T, "t": t, "reset": reset, "dG": dG, "gates": gates, "cbuf": cbuf, "dh": dh,
            "dcn": rng.standard_normal((N, HID), F32) * F32(1e-3), "Wl": weight_like(rng, (GATES, HID))}


def crafted_flags(rng, t_max, n_envs, p=0.03):
    """(T, N) uint8 reset / terminal flags of the long-window cases (T >= 33), where a drawn 15 - 20 % would leave
    no chain longer than a few steps: env 0 never flagged, env 1 at steps 0 and T - 1 only, env 2 once past step
    32 (step 40, or T - 1 where the window ends before it), every other env at about p a step."""
    T, N = t_max, n_envs
    assert T >= 33
    f = (rng.random((T, N)) < p).astype(np.uint8)
    f[:, :3] = 0
    if N > 1:
        f[0, 1] = f[T - 1, 1] = 1
    if N > 2:
        f[40 if T > 41 else T - 1, 2] = 1
    return f


def crafted_flags_hold(f):
    """The conditions crafted_flags exists for, on any (T, N) flags: an env with an unbroken chain over the whole
    window, a flag at step 0, one at step T - 1 and one past step 32."""
    f = np.asarray(f) != 0
    return bool((~f.any(0)).any() and f[0].any() and f[-1].any() and f[32:].any())


def bptt_chain_data(n_envs, t_max, seed=0, crafted=None):
    """Operands of LEARN_TRUNK's BPTT chain on top of lstm_data / fc_data (finite
    operands for the weight-gradient and FC launches that follow): gates and cbuf
    of every step (cbuf slot 0 a sentinel on the rows reset at step 0, slots past
    the window sentinels), the heads' dh, the lateral weight; hbuf slot T finite.
    crafted (default: the cases of BPTT_LONG_CASES): the window's reset flags are
    crafted_flags, from a generator of their own, instead of lstm_data's ~20 %."""
    rng = np.random.default_rng([seed, n_envs, t_max, 8])
    N, T = n_envs, t_max
    d = lstm_data(N, T, seed)
    if (n_envs, t_max) in BPTT_LONG_CASES if crafted is None else crafted:
        d["reset"][:T] = crafted_flags(np.random.default_rng([seed, n_envs, t_max, 15]), T, N)
    d["fc"] = fc_data(N, T, lstm=True, seed=seed)
    d["hbuf"][T] = rng.standard_normal((N, HID), F32) * F32(0.5)
    gates = np.full((T + 1, N, GATES), SENTINEL, F32)
    gates[:T] = rng.standard_normal((T, N, GATES), F32)
    cbuf = np.full((T + 2, N, HID), SENTINEL, F32)
    cbuf[:T + 1] = rng.standard_normal((T + 1, N, HID), F32)
    cbuf[0][d["reset"][0] != 0] = SENTINEL
    d.update(gates=gates, cbuf=cbuf, dh=rng.standard_normal((T, N, HID), F32) * F32(1e-3),
             Wl=weight_like(rng, (GATES, HID)))
    return d


def returns_data(t_max, n_actions, n_envs, lstm=False, seed=0):
    """Operands of the returns stage: rewards a mix of 0, +-1 and values beyond +-1,
    dones ~15 % with a terminal at step 0 of env 0 and at step T - 1 of the last
    env, v with the bootstrap slot T, probs / logp of random logits (float64,
    rounded once), actions, head weights, and hfc (slot T a sentinel; lstm: all of
    it, the stage must not read it)."""
    rng = np.random.default_rng([seed, t_max, n_actions, n_envs, 9])
    T, A, N = t_max, n_actions, n_envs
    rewards = rng.choice(np.array([0, 0, 1, -1, 0.5, 2.5, -3], F32), (T, N))
    rewards[0, N - 1] = 2.5
    dones = (rng.random((T, N)) < 0.15).astype(np.uint8)
    if N > 1 and T > 1:
        dones[T - 1, 0] = 0   # env 0's last steps reach the bootstrap value
    dones[0, 0] = dones[T - 1, N - 1] = 1
    z =rng.standard_normal((T, N, A)) * 2.0
    z -= z.max(-1, keepdims=True)
    lse = np.log(np.exp(z).sum(-1, keepdims=True))
    hfc = act_like(rng, (T + 1, N, HID))
    hfc[T if not lstm else slice(None)] = SENTINEL
    return {"T": T, "A": A, "N": N, "rewards": rewards, "dones": dones, "v": rng.standard_normal((T + 1, N), F32),
            "probs": np.exp(z - lse).astype(F32), "logp": (z - lse).astype(F32),
            "actions": rng.integers(0, A, (T, N)).astype(np.int32), "hfc": hfc,
            "Wpi": weight_like(rng, (A, HID)), "Wv": weight_like(rng, (1, HID))}


# the loss-gradient stage tests' coefficients (none a default, so a hard-coded default shows) and PPO settings
COEF = {"gamma": 0.9, "beta": 0.02, "vcoef": 0.25, "pi_loss_coef": 0.5}
PPO_CLIP, PPO_VCLIP = 0.2, 0.1
PPO_GRID = np.array([-0.6, -0.35, -0.1, 0.1, 0.35, 0.6], F32)      # log ratios: exp() on both sides of lo and hi
VCLIP_GRID = np.array([-0.3, -0.15, -0.05, 0.05, 0.15, 0.3], F32)   # v - v_old: on both sides of +-PPO_VCLIP
MARGIN = 1e-3   # relative distance of every decision from its threshold


def near_threshold(d):
    """(T, N) bool: the samples of lossgrad_data's d on which a decision of the PPO forms lies within MARGIN
    (relative) of its threshold: rho against lo / hi, |v - v_old| against ev, the clipped square against the
    unclipped one (where the value is outside the clip range), and a nonzero adv against 0 (an exact zero
    takes no decision: rho * 0, hi * 0 and lo * 0 are the same 0)."""
    T = d["T"]
    lo, hi = (F64(x) for x in clip_range(PPO_CLIP))
    ev = F64(F32(PPO_VCLIP))
    lpa = np.take_along_axis(np.asarray(d["logp"], F64), np.asarray(d["actions"], np.int64)[..., None], 2)[..., 0]
    rho = np.exp(lpa - np.asarray(d["logp_old"], F64))
    v, vo, Rf, adv = (np.asarray(x, F64) for x in (d["v"][:T], d["v_old"], d["ret"], d["adv"]))
    dvo = v - vo
    lu, lc = (v - Rf) ** 2, (vo + np.clip(dvo, -ev, ev) - Rf) ** 2
    bad = (np.abs(rho - lo) < MARGIN * lo) | (np.abs(rho - hi) < MARGIN * hi)
    bad |= np.abs(np.abs(dvo) - ev) < MARGIN * ev
    bad |= (np.abs(dvo) > ev) & (np.abs(lc - lu) < MARGIN * np.maximum(lc, lu))
    bad |= (adv != 0) & (np.abs(adv) < MARGIN * np.abs(adv).max())
    return bad


def lossgrad_data(t_max, n_actions, n_envs, lstm=False, t_len=None, seed=0):
    """returns_data plus what the GAE / PPO forms and a truncated window need.
    t_len: a terminal on every env at step t_len - 1; rewards_t / dones_t are the window as
    arl_truncate_window(t_len) leaves it (rows >= t_len: dones 2, rewards 0), else the window itself.
    The PPO snapshot: logp_old = logp[a] - delta with delta from PPO_GRID, adv normal with ~10 % exact
    zeros, ret the f32 n-step return at COEF's gamma, v_old = v - d with d from VCLIP_GRID.  A sample with
    a decision within MARGIN of its threshold (near_threshold) is drawn again, none is exempted; `redrawn`
    counts the draws that took."""
    d = returns_data(t_max, n_actions, n_envs, lstm, seed)
    T, N = t_max, n_envs
    rng = np.random.default_rng([seed, t_max, n_actions, n_envs, 13])
    d["rewards_t"], d["dones_t"] = d["rewards"], d["dones"]
    if t_len is not None:
        d["dones"][t_len - 1] = 1
        d["rewards_t"], d["dones_t"] = d["rewards"].copy(), d["dones"].copy()
        d["rewards_t"][t_len:], d["dones_t"][t_len:] = 0, 2
    R, ret = np.asarray(d["v"][T], F64), np.empty((T, N), F32)
    for t in reversed(range(T)):
        R = np.where(d["dones_t"][t] & 1, 0.0, R) * COEF["gamma"] + np.clip(np.asarray(d["rewards_t"][t], F64), -1.0, 1.0)
        ret[t] = R
    lpa = np.take_along_axis(d["logp"], d["actions"][..., None].astype(np.int64), 2)[..., 0]

    def draw():
        adv = rng.standard_normal((T, N), F32) * (rng.random((T, N)) >= 0.1)
        return ((lpa - rng.choice(PPO_GRID, (T, N))).astype(F32), adv.astype(F32),
                (d["v"][:T] - rng.choice(VCLIP_GRID, (T, N))).astype(F32))

    d["ret"] = ret
    d["logp_old"], d["adv"], d["v_old"] = draw()
    if T * N >= 8:
        d["adv"][T // 2, N - 1] = 0   # (an exact zero in every case but the smallest)
    d["redrawn"] = 0
    for _ in range(100):
        bad = near_threshold(d)
        if not bad.any():
            break
        d["redrawn"] += int(bad.sum())
        for k, fresh in zip(("logp_old", "adv", "v_old"), draw()):
            d[k][bad] = fresh[bad]
    assert not near_threshold(d).any()
    return d


def fused_data(t_max, n_actions, n_envs, seed=0):
    """lossgrad_data plus the bootstrap slot's forward: the FC's and the heads' parameters and a2T (N, 2592),
    post-ReLU with exact zeros.  An env whose FC pre-activation has a unit within MARGIN of 0 (relative
    to the largest) is drawn again."""
    d = lossgrad_data(t_max, n_actions, n_envs, seed=seed)
    rng = np.random.default_rng([seed, t_max, n_actions, n_envs, 14])
    d["Wfc"], d["bfc"] = weight_like(rng, (HID, A2)), rng.uniform(-1 / 51, 1 / 51, HID).astype(F32)
    d["bpi"], d["bv"] = rng.uniform(-1 / 16, 1 / 16, n_actions).astype(F32), rng.uniform(-1 / 16, 1 / 16, 1).astype(F32)
    a2T = act_like(rng, (n_envs, A2))
    for _ in range(100):
        z = mm64(a2T, d["Wfc"].T) + d["bfc"]
        bad = (np.abs(z) < MARGIN * np.abs(z).max()).any(1)
        if not bad.any():
            break
        a2T[bad] = act_like(rng, (int(bad.sum()), A2))
    assert not bad.any()
    d["a2T"], d["zT"] = a2T, z
    return d


# the cases of tests/test_gpu_stages.py, (n_envs, t_max); tests/test_stage_ref.py runs the
# sensitivity check on the same list
FC_CASES = [(1, 1), (43, 3), (109, 11), (240, 5), (241, 5), (400, 5)]
FC_LSTM_ARCH_CASE = (41, 5)
LSTM_CASES = [(1, 1), (43, 3), (256, 4), (205, 5), (400, 5)]
CONV_CASES = [(1, 1), (255, 1), (257, 1), (52, 5), (67, 9), (513, 5), (3, 64)]
CONV_LAYOUT_CASE = (52, 5)   # also run as rgb (DoomA3CFF) and stack
LAUNCHES = 4                 # at Z > 1: launches in a row, each with fresh gradients
# conv_fwd (n_envs, layout), each at slots 0 and 1 of a t_max = 1 net: from 512 envs two envs a workgroup
CONV_FWD_CASES = [(1, "ring"), (5, "ring"), (512, "ring"), (513, "ring"), (5, "rgb"), (513, "rgb"), (5, "stack"),
                  (513, "stack")]
BPTT_CASES = [(n, t) for n in (1, 33, 64) for t in (1, 2)]   # (n_envs, t) on a t_max = 3 net
BPTT_T = 3
BPTT_LONG_CASES = [(3, 64), (33, 33)]   # crafted reset flags: a chain over the whole window (bptt_chain_data)
BPTT_CHAIN_CASES = [(37, 5), (1, 5)] + BPTT_LONG_CASES
CONV_FWD_LONG_CASE = (3, 64, (0, 63, 64))   # (n_envs, t_max, slots): conv_fwd on a ring of 68, slot T the bootstrap
CONV_FWD_RING_T = 33                          # the T of the long ring-residue case: R = 37
# returns (t_max, n_actions, n_envs): one case for each returns_heads_kernel<AM, RB> and row-pass count
RETURNS_CASES = [(1, 1, 1), (8, 4, 3), (8, 5, 3), (8, 8, 2), (8, 9, 2), (9, 4, 3), (32, 32, 2), (33, 6, 2), (64, 32, 2)]
RETURNS_LSTM_CASE = (5, 6, 3)
# tests/test_gpu_lossgrad_stages.py: every RETURNS_CASES case in each form of the loss-gradient launch
LOSSGRAD_FORMS = ("nstep", "gae", "ppo", "ppo_vc")
GAE_LAMBDA = 0.95
GAE0_CASES = [(8, 8, 2), (33, 6, 2)]                                    # also at lambda = 0
TRUNC_CASES = [((8, 4, 3), 5), ((33, 6, 2), 32), ((64, 32, 2), 33)]     # (case, t_len); 32: the second row pass all dead
FUSED_CASES = [(8, 4, 3), (8, 8, 2), (9, 4, 3), (33, 6, 2), (64, 32, 2)]
# returns_kernel / ppo_snapshot_kernel packing (t_max, n_envs) at 6 actions: T = 1; the last register-window length;
# EB = 4 with a one-env tail; EB = 3 with an idle thread and a one-env tail; EB = 2; the first EB = 1; the largest T
PACK_CASES = [(1, 257), (8, 33), (64, 5), (85, 4), (128, 3), (129, 2), (256, 2)]
PACK_A = 6


def lossgrad_runs():
    """The heads-kernel runs of tests/test_gpu_lossgrad_stages.py, (case, form, lambda, t_len, lstm); each runs with
    keep_loss_scale_same off and on."""
    runs = [(c, f, GAE_LAMBDA if f == "gae" else 1.0, None, False) for c in RETURNS_CASES for f in LOSSGRAD_FORMS]
    runs += [(c, "gae", 0.0, None, False) for c in GAE0_CASES]
    runs += [(RETURNS_LSTM_CASE, "gae", GAE_LAMBDA, None, True)]
    runs += [(c, f, GAE_LAMBDA if f == "gae" else 1.0, tl, False) for c, tl in TRUNC_CASES for f in ("gae", "ppo")]
    return runs


def lossgrad_ref(d, form, keep, lam=1.0, lstm=False, mistake=None):
    """The reference of one run on lossgrad_data's d at COEF: {dlogits, dv, loss, dh, ratio (PPO forms)}."""
    T = d["T"]
    hfc = None if lstm else d["hfc"][:T]
    kw = dict(beta=COEF["beta"], vcoef=COEF["vcoef"], pi_loss_coef=COEF["pi_loss_coef"], keep_loss_scale_same=keep,
              mistake=mistake)
    if form in ("ppo", "ppo_vc"):
        if form == "ppo_vc":
            kw.update(v_old=d["v_old"], vclip_eps=PPO_VCLIP)
        dl, dv, ratio, loss, dh = ppo_heads_ref(d["dones_t"], d["v"], d["probs"], d["logp"], d["actions"], d["logp_old"],
                                                d["adv"], d["ret"], d["Wpi"], d["Wv"], hfc, PPO_CLIP, **kw)
        return {"dlogits": dl, "dv": dv, "loss": loss, "dh": dh, "ratio": ratio}
    dl, dv, loss, dh = returns_heads_ref(d["rewards_t"], d["dones_t"], d["v"], d["probs"], d["logp"], d["actions"], d["Wpi"],
                                         d["Wv"], hfc, gamma=COEF["gamma"], lam=lam, **kw)
    return {"dlogits": dl, "dv": dv, "loss": loss, "dh": dh}


# ================================================================ the generic implicit-GEMM paths
# A3CFFNature (nature.hip) and the f32-state convs of an ARCH_STATES net (states.hip), both on gemm.hpp
NHID, NC1, NC2, NC3, NP1, NP2, NP3 = 512, 32, 64, 64, 400, 81, 49
NA1, NA2, NA3 = NC1 * NP1, NC2 * NP2, NC3 * NP3
NFC_SPLIT = 8
NATURE_NAMES = {"c1W": "0/0/W", "c1b": "0/0/b", "c2W": "0/1/W", "c2b": "0/1/b", "c3W": "0/2/W", "c3b": "0/2/b",
                "fcW": "0/3/W", "fcb": "0/3/b", "piW": "1/0/W", "pib": "1/0/b", "vW": "2/0/W", "vb": "2/0/b"}


# ---------------------------------------------------------------- launch geometry (gemm.hpp, layers.hpp)
def ceil_div(a, b):
    return -(-a // b)


def plan_splits(tiles, K, bk=BK, target=1024):
    """layers.hpp: aim at ~1024 workgroups, each slice >= 4 K chunks."""
    return min(max(1, target // max(1, tiles)), max(1, ceil_div(K, bk * 4)))


def slice_len(K, splits, bk=BK):
    """launch_gemm's k_per_split: ceil(K / splits) rounded up to whole chunks."""
    return ceil_div(ceil_div(K, max(1, splits)), bk) * bk


def effective_splits(K, splits, bk=BK):
    """gemm.hpp: the K slices launch_gemm really launches for a requested count."""
    return ceil_div(K, slice_len(K, splits, bk))


def slice_bounds(K, splits):
    """[k0, k1) of every launched K slice (the last one may be shorter)."""
    kps = slice_len(K, splits)
    return [(z * kps, min(K, (z + 1) * kps)) for z in range(ceil_div(K, kps))]


def nature_plans(S, A):
    """nature.hip nature_plans: K slices of the five weight-gradient GEMMs."""
    K3, K2, K1 = S * NP3, S * NP2, S * NP1
    return {"heads": effective_splits(S, plan_splits(ceil_div(A + 1, 16) * ceil_div(NHID + 1, 64), S)),
            "fc": effective_splits(S, plan_splits(ceil_div(NHID, 64) * ceil_div(NA3 + 1, 64), S)),
            "c3": effective_splits(K3, plan_splits(ceil_div(NC2 * 9 + 1, 64), K3)),
            "c2": effective_splits(K2, plan_splits(ceil_div(NC1 * 16 + 1, 64), K2)),
            "c1": effective_splits(K1, plan_splits(ceil_div(4 * 64 + 1, 64), K1))}


def states_plans(S):
    """states.hip states_plans."""
    K2, K1 = S * 81, S * 400
    return {"c2": effective_splits(K2, plan_splits(ceil_div(16 * 16 + 1, 64), K2)),
            "c1": effective_splits(K1, plan_splits(ceil_div(4 * 64 + 1, 64), K1))}


def returns_blocks(T, N):
    """policy.hip returns_kernel (the form launch_returns picks): 256 / T envs a workgroup."""
    return ceil_div(N, 256 // T)


# ---------------------------------------------------------------- references
def _conv64(x, W, b, s):
    """conv(x, W, stride s) + b in float64; x float64 or float32."""
    oc, ic, k, _ = W.shape
    cols, oh, ow = O._im2col(x, k, s)
    z = np.asarray(cols.reshape(-1, ic * k * k), F64) @ np.asarray(W, F64).reshape(oc, -1).T + np.asarray(b, F64)
    return z.reshape(x.shape[0], oh, ow, oc).transpose(0, 3, 1, 2)


def nature_fwd_ref(x, p, chunk=64):
    """The Nature head's forward in float64 from the f32 state x (an array, or RingX)
    and the parameters p (Chainer names): z1 = conv(x, k8 s4), z2 = conv(a1, k4 s2),
    z3 = conv(a2, k3 s1), zh = a3 W^T + b, every a = max(z, 0) and each layer from the
    float64 one before it.  Returns {z1, a1, z2, a2, z3, a3, zh, h}, float64."""
    S = x.shape[0]
    z = {"z1": np.empty((S, NC1, 20, 20)), "z2": np.empty((S, NC2, 9, 9)), "z3": np.empty((S, NC3, 7, 7)),
         "zh": np.empty((S, NHID))}
    for c0 in range(0, S, chunk):
        sl = slice(c0, min(S, c0 + chunk))
        z["z1"][sl] = _conv64(np.ascontiguousarray(x[sl]), p["0/0/W"], p["0/0/b"], 4)
        z["z2"][sl] = _conv64(np.maximum(z["z1"][sl], 0.0), p["0/1/W"], p["0/1/b"], 2)
        z["z3"][sl] = _conv64(np.maximum(z["z2"][sl], 0.0), p["0/2/W"], p["0/2/b"], 1)
        a3 = np.maximum(z["z3"][sl], 0.0).reshape(-1, NA3)
        z["zh"][sl] = a3 @ np.asarray(p["0/3/W"], F64).T + np.asarray(p["0/3/b"], F64)
    z.update({"a" + k[1:]: np.maximum(v, 0.0) for k, v in z.items() if k != "zh"})
    z["h"] = np.maximum(z["zh"], 0.0)
    return z


def policy_ref(h, Wpi, bpi, Wv, bv):
    """The heads and the softmax in float64: logits, v, probs, logp, entropy."""
    h = np.asarray(h, F64)
    logits = h @ np.asarray(Wpi, F64).T + np.asarray(bpi, F64)
    v = (h @ np.asarray(Wv, F64).T)[:, 0] + F64(np.asarray(bv).reshape(-1)[0])
    zc = logits - logits.max(-1, keepdims=True)
    logp = zc - np.log(np.exp(zc).sum(-1, keepdims=True))
    probs = np.exp(logp)
    return {"logits": logits, "v": v, "probs": probs, "logp": logp, "entropy": -(probs * logp).sum(-1)}


def conv_transpose_ref(dy, W, stride):
    """The transposed convolution (a conv's backward to its input) in float64:
    dx[s, ic, stride oy + ky, stride ox + kx] += dy[s, oc, oy, ox] W[oc, ic, ky, kx]."""
    oc, ic, k, _ = W.shape
    n, _, oh, ow = dy.shape
    gcol = (np.asarray(dy, F64).transpose(0, 2, 3, 1).reshape(-1, oc) @ np.asarray(W, F64).reshape(oc, -1))
    gcol = gcol.reshape(n, oh, ow, ic, k, k)
    gx = np.zeros((n, ic, stride * (oh - 1) + k, stride * (ow - 1) + k))
    for ky in range(k):
        for kx in range(k):
            gx[:, :, ky:ky + stride * oh:stride, kx:kx + stride * ow:stride] += gcol[..., ky, kx].transpose(0, 3, 1, 2)
    return gx


def nature_fc_bwd_ref(dfc, a3, W):
    """The Nature fc_bwd stage: gW = dfc^T a3, gb = sum_s dfc, da3 = (dfc W) * (a3 > 0);
    a3 (S, 3136).  Returns (g, mag), float32."""
    g = {"fcW": mm64(dfc.T, a3), "fcb": dfc.sum(0, dtype=F64), "da3": mm64(dfc, W) * (a3 > 0)}
    mag = {"fcW": O._mag_mm(dfc.T, a3), "fcb": O._mag_sum(dfc)}
    return {k: v.astype(F32) for k, v in g.items()}, mag


def nature_conv_bwd_ref(x, a1, a2, da3, W3, W2, chunk=64):
    """The Nature conv_bwd stage: gW3, gb3 of conv3 (64 -> 64, k3 s1) from da3 and a2,
    da2 = convT(da3, W3) * (a2 > 0); gW2, gb2 of conv2 (32 -> 64, k4 s2) from da2 and
    a1, da1 = convT(da2, W2) * (a1 > 0); gW1, gb1 of conv1 (4 -> 32, k8 s4) from da1 and
    x (an array, or RingX).  da2 and da1 are formed in float64 and rounded to float32
    once, the values the next reduction is fed (as the device feeds its own); the six
    sums are accumulated in float64 over chunks of <= chunk samples.  Returns (g,
    mag) float32 and da2, da1 float64."""
    S = x.shape[0]
    shp = {"c3": (NC3, NC2, 3, 3), "c2": (NC2, NC1, 4, 4), "c1": (NC1, 4, 8, 8)}
    gW = {k: np.zeros((s[0], s[1] * s[2] * s[3])) for k, s in shp.items()}
    gb = {k: np.zeros(s[0]) for k, s in shp.items()}
    m = {k: _Mag(*v.shape) for k, v in gW.items()}
    da2, da1 = np.empty((S, NC2, 9, 9)), np.empty((S, NC1, 20, 20))

    def wgrad(key, dy, xin, k, s):
        oc = dy.shape[1]
        cols = O._im2col(xin, k, s)[0].reshape(-1, gW[key].shape[1])
        gy = dy.transpose(0, 2, 3, 1).reshape(-1, oc)
        a64, b64 = np.asarray(gy.T, F64), np.asarray(cols, F64)
        gW[key] += a64 @ b64
        gb[key] += gy.sum(0, dtype=F64)
        m[key].add(a64, b64)

    for c0 in range(0, S, chunk):
        sl = slice(c0, min(S, c0 + chunk))
        d3, a2s, a1s = np.asarray(da3[sl], F32), np.asarray(a2[sl], F32), np.asarray(a1[sl], F32)
        wgrad("c3", d3, a2s, 3, 1)
        da2[sl] = conv_transpose_ref(d3, W3, 1) * (a2s > 0)
        d2 = da2[sl].astype(F32)
        wgrad("c2", d2, a1s, 4, 2)
        da1[sl] = conv_transpose_ref(d2, W2, 2) * (a1s > 0)
        wgrad("c1", da1[sl].astype(F32), np.ascontiguousarray(x[sl]), 8, 4)
    g, mag = {}, {}
    for k, s in shp.items():
        P = {"c3": NP3, "c2": NP2, "c1": NP1}[k]
        g[k + "W"], g[k + "b"] = gW[k].reshape(s).astype(F32), gb[k].astype(F32)
        mag[k + "W"], mag[k + "b"] = m[k].mm().reshape(s), np.full(s[0], m[k].X * np.sqrt(S * float(P)))
    return g, mag, da2, da1


def nature_heads_ref(rewards, dones, v, probs, logp, actions, Wpi, Wv, hfc, **kw):
    """returns_heads_ref at the heads' hidden width (512 on the Nature head) plus the
    heads' weight gradients with their bias, as the heads GEMM of nature_learn forms
    them from the f32 dlogits / dv: gpiW = dlogits^T h, gpib = sum_s dlogits, gvW =
    dv^T h, gvb = sum_s dv; hfc (T, N, H).  Returns {dlogits, dv, loss, dfc} float64
    and (g, mag) float32."""
    dl, dv, loss, dfc = returns_heads_ref(rewards, dones, v, probs, logp, actions, Wpi, Wv, hfc, **kw)
    S = dv.size
    dl32, dvc, hh = dl.reshape(S, -1).astype(F32), dv.reshape(S, 1).astype(F32), np.asarray(hfc).reshape(S, -1)
    g = {"piW": mm64(dl32.T, hh), "pib": dl32.sum(0, dtype=F64), "vW": mm64(dvc.T, hh), "vb": dvc.sum(0, dtype=F64)}
    mag = {"piW": O._mag_mm(dl32.T, hh), "pib": O._mag_sum(dl32), "vW": O._mag_mm(dvc.T, hh), "vb": O._mag_sum(dvc)}
    return {"dlogits": dl, "dv": dv, "loss": loss, "dfc": dfc}, {k: x.astype(F32) for k, x in g.items()}, mag


def nature_learn_ref(d, lam=1.0):
    """The whole of nature_learn on the operands of nature_data, chained: the heads
    (nature_heads_ref), the FC (nature_fc_bwd_ref on the f32 dfc) and the convs
    (nature_conv_bwd_ref on the f32 da3).  Returns (outs, g, mag): outs {dlogits, dv,
    loss, dfc} float64, the 12 gradient tensors and their scales."""
    T, S, p = d["T"], d["S"], d["p"]
    outs, g, mag = nature_heads_ref(d["rewards"], d["dones"], d["v"], d["probs"], d["logp"], d["actions"], p["1/0/W"],
                                    p["2/0/W"], d["hfc"][:T], lam=lam)
    a3 = d["a3"][:T].reshape(S, NA3)
    gf, mf = nature_fc_bwd_ref(outs["dfc"].reshape(S, NHID).astype(F32), a3, p["0/3/W"])
    da3 = gf.pop("da3").reshape(S, NC3, 7, 7)
    gc, mc, _, _ = nature_conv_bwd_ref(d["x"], d["a1"][:T].reshape(S, NC1, 20, 20), d["a2"][:T].reshape(S, NC2, 9, 9), da3,
                                       p["0/2/W"], p["0/1/W"])
    g.update(gf), g.update(gc), mag.update(mf), mag.update(mc)
    return outs, g, mag


# ---------------------------------------------------------------- data recipes
def ring_nvalid(rng, R, N, T):
    """nvalid as conv_data draws it: 1..4 per (slot, env), env 0 masked at slot 0 and at
    the bootstrap slot."""
    nvalid = rng.integers(1, 5, (R, N)).astype(np.uint8)
    nvalid[0, 0], nvalid[T, 0] = 2, 3
    return nvalid


def rolled(ring, start, R):
    """The ring array holding at slot (start + k) % R what `ring` holds at slot k: the
    same window under a step counter of `start`."""
    return np.roll(ring, start % R, axis=0)


def ring_starts(T):
    """The step counters of the ring-residue cases: R - 1, 2^32 - 3 and the first multiple of T above 2^40."""
    return [T + 3, 2 ** 32 - 3, (2 ** 40 // T + 1) * T]


def nature_data(n_envs, t_max, n_actions, seed=0):
    """Operands of every Nature stage and of nature_learn, at a step counter of 0:
    parameters as init_like_torch, frames / nvalid as conv_data (x: the window's T
    steps, x_fwd: with the bootstrap slot), post-ReLU a1 / a2 / a3 / hfc with the
    bootstrap slot a sentinel, da3, fresh_dfc(k), and the returns launch's inputs
    (returns_data's rewards, dones, v, probs, logp, actions)."""
    rng = np.random.default_rng([seed, n_envs, t_max, n_actions, 10])
    N, T, A, S, R = n_envs, t_max, n_actions, n_envs * t_max, t_max + 4
    d = {"N": N, "T": T, "A": A, "S": S, "R": R, "p": O.init_like_torch(O.ARCH_FF_NATURE, A, rng)}
    d["frames"] = rng.integers(0, 256, (R, N, 84, 84), dtype=np.uint8)
    d["nvalid"] = ring_nvalid(rng, R, N, T)
    d["x"] = RingX(d["frames"], d["nvalid"], N, T)
    d["x_fwd"] = RingX(d["frames"], d["nvalid"], N, T, steps=T + 1)
    for name, shape in (("a1", (NC1, 20, 20)), ("a2", (NC2, 9, 9)), ("a3", (NA3,)), ("hfc", (NHID,))):
        a = act_like(rng, (T + 1, N) + shape)
        a[T] = SENTINEL
        d[name] = a
    d["da3"] = grad_like(rng, (S, NC3, 7, 7))
    d["fresh_dfc"] = lambda k: grad_like(np.random.default_rng([seed, n_envs, t_max, n_actions, 11, k]), (S, NHID))
    r = returns_data(T, A, N, seed=seed)
    d.update({k: r[k] for k in ("rewards", "dones", "v", "probs", "logp", "actions")})
    return d


def states_data(n_envs, t_max, seed=0):
    """Operands of the two conv stages of an ARCH_STATES net at a step counter of 0:
    a (R, N, 4, 84, 84) ring of signed normal states (no image of uint8 frames) with
    the three slots past the bootstrap slot sentinels, the convs' weights and biases,
    a1 with the bootstrap slot a sentinel, da2; x: the window's T steps, x_fwd: with
    the bootstrap slot."""
    rng = np.random.default_rng([seed, n_envs, t_max, 12])
    N, T, S, R = n_envs, t_max, n_envs * t_max, t_max + 4
    frames = rng.standard_normal((R, N, 4, 84, 84), F32)
    frames[T + 1:] = SENTINEL
    a1 = act_like(rng, (T + 1, N, 16, 20, 20))
    a1[T] = SENTINEL
    d = {"N": N, "T": T, "S": S, "R": R, "frames": frames, "a1": a1, "da2": grad_like(rng, (S, 32, 9, 9)),
         "W1": weight_like(rng, (16, 4, 8, 8)), "W2": weight_like(rng, (32, 16, 4, 4))}
    d["b1"], d["b2"] = rng.uniform(-1 / 16, 1 / 16, 16).astype(F32), rng.uniform(-1 / 16, 1 / 16, 32).astype(F32)
    d["x"] = RingX(frames, None, N, T, "states")
    d["x_fwd"] = RingX(frames, None, N, T, "states", steps=T + 1)
    return d


# the cases of tests/test_gpu_gemm_stages.py; tests/test_stage_ref.py pins their launch geometry and runs the
# sensitivity checks on the same data
NATURE_CASES = [(1, 1, 4), (33, 5, 18), (67, 2, 6)]    # (n_envs, t_max, n_actions)
NATURE_HEADS_CASE = (41, 9, 4)                         # the heads and fc_bwd only
# the heads GEMM's M = A + 1 rows in 16-row tiles: one exact tile; the second tile holds the value row alone
NATURE_HEADS_EDGE_CASES = [(5, 3, 15), (5, 3, 16)]
NATURE_LEARN_CASES = [(33, 5, 18), NATURE_HEADS_CASE]
NATURE_RING_CASE = (33, 5, 18)
STATES_CASES = [(1, 1), (33, 5)]                       # (n_envs, t_max)
STATES_RING_CASE = (33, 5)
GAE_LAMBDAS = (1.0, 0.95)
TIE_SHARE_MAX = 1e-3                                   # of a tensor's elements the tie band may exempt
