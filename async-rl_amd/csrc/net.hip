// A3C FF / LSTM network on gfx950: batched-env forward, lockstep-window
// backward, parameter layout and workspace layout.
//
// Reference: a3c_ale.py:28-70 (A3CFF, A3CLSTM), dqn_head.py:31-52
// (NIPSDQNHead: conv 4->16 k8 s4, conv 16->32 k4 s2, Linear 2592->256, ReLU
// after each), policy.py:32-58, v_function.py:10-34, Chainer 1.8.1 L.LSTM /
// F.lstm (interleaved a,i,f,o gates), a3c.py:129-130 (backward of the window
// loss), a3c.py:144 (unchain_backward: truncated BPTT at the window edge).
//
// The window's launches in order (the kernels live in their own files):
// forward per step t: phi_ring (phi.hip) -> conv_fwd (conv_fwd.hip) -> fc_fwd
// (fc.hip) -> policy_fc (FF) or the LSTM gate kernel + policy (lstm.hip,
// policy.hip); learner: returns + heads dh (policy.hip), [LSTM BPTT + gate
// weight gradients], fc_bwd (fc_bwd.hip), conv_bwd + its slab reduce
// (conv_bwd.hip), then clip + RMSProp + the window advance (optim.hip).  The
// f32-state forward (pi_and_v) and the ARCH_STATES / Nature convolutions run on
// the generic implicit-GEMM template (gemm.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "arl_internal.hpp"
#include "gemm.hpp"
#include "layers.hpp"

namespace arl {

// ---------------------------------------------------------------- accessors

// (conv1 from the uint8 frame ring has dedicated kernels: conv1.hip)
struct Conv1F32A {      // same from an f32 (n,C,84,84) state tensor (dqn_phi output; C = 3 for RGB)
  const float* __restrict__ x;
  int C;
  __device__ float load(int m, int k) const {
    const int s = m / C1_P, p = m - s * C1_P;
    const int ic = k >> 6, ky = (k >> 3) & 7, kx = k & 7;
    const int oy = p / 20, ox = p - oy * 20;
    return x[((int64_t)s * C + ic) * PLANE + (4 * oy + ky) * 84 + 4 * ox + kx];
  }
};
struct Conv2A {         // A(m, k) = a1[s][ic][2oy+ky][2ox+kx], m = s*81 + p, k = ic*16+ky*4+kx
  const float* __restrict__ a1;
  __device__ float load(int m, int k) const {
    const int s = m / C2_P, p = m - s * C2_P;
    const int oy = p / 9, ox = p - oy * 9;
    const int ic = k >> 4, ky = (k >> 2) & 3, kx = k & 3;
    return a1[(int64_t)s * A1 + ic * C1_P + (2 * oy + ky) * 20 + 2 * ox + kx];
  }
};

// ---------------------------------------------------------------- elementwise
__device__ inline float sigm(float x) { return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-x))); }

// F.lstm backward of element i = (m, unit) at step t: dh = dL/dh_t (heads +
// carried), dcn in: dc carried from t+1 (first: none), out: dc carried to t-1.
__device__ inline void lstm_cell_bwd_elem(const float* __restrict__ gates, const float* __restrict__ c_t,
                                          const float* __restrict__ c_prev, bool rs, float dh, float* __restrict__ dcn,
                                          float* __restrict__ dG, bool first, int64_t i) {
  const float4 g = reinterpret_cast<const float4*>(gates)[i];
  const float a = tanhf(g.x), ig = sigm(g.y), fg = sigm(g.z), og = sigm(g.w);
  const float c = c_t[i];
  const float tc = tanhf(c);
  float dc = __fmul_rn(__fmul_rn(dh, og), __fsub_rn(1.f, __fmul_rn(tc, tc)));
  if (!first) dc = __fadd_rn(dc, dcn[i]);
  const float cp = rs ? 0.f : c_prev[i];
  float4 d;
  d.x = __fmul_rn(__fmul_rn(dc, ig), __fsub_rn(1.f, __fmul_rn(a, a)));
  d.y = __fmul_rn(__fmul_rn(__fmul_rn(dc, a), ig), __fsub_rn(1.f, ig));
  d.z = __fmul_rn(__fmul_rn(__fmul_rn(dc, cp), fg), __fsub_rn(1.f, fg));
  d.w = __fmul_rn(__fmul_rn(__fmul_rn(dh, tc), og), __fsub_rn(1.f, og));
  reinterpret_cast<float4*>(dG)[i] = d;
  dcn[i] = rs ? 0.f : __fmul_rn(dc, fg);
}

// F.lstm backward for step t.  dH: dL/dh_t from the heads; dhn/dcn: carried
// from step t+1 (ignored when first); writes dG (interleaved) and dcn for t-1.
__global__ void lstm_cell_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ c_t,
                                     const float* __restrict__ c_prev, const uint8_t* __restrict__ reset,
                                     const float* __restrict__ dH, const float* __restrict__ dhn,
                                     float* __restrict__ dcn, float* __restrict__ dG, int first, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t m = i / HID;
  const float dh = first ? dH[i] : __fadd_rn(dH[i], dhn[i]);
  lstm_cell_bwd_elem(gates, c_t, c_prev, reset[m] != 0, dh, dcn, dG, first != 0, i);
}

// dh[s][j] = sum_k dlogits[s][k] Wpi[k][j] + dv[s] Wv[j]; with mask: * (h > 0)
__global__ void heads_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ dv,
                                 const float* __restrict__ Wpi, const float* __restrict__ Wv, int A, int H,
                                 const float* __restrict__ mask, float* __restrict__ out, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t s = i / H;
  const int j = (int)(i - s * H);
  float acc = 0.f;
  for (int k = 0; k < A; ++k) acc = __fadd_rn(acc, __fmul_rn(dl[s * A + k], Wpi[k * H + j]));
  acc = __fadd_rn(acc, __fmul_rn(dv[s], Wv[j]));
  if (mask) acc = mask[i] > 0.f ? acc : 0.f;
  out[i] = acc;
}

hipError_t launch_heads_bwd(const float* dl, const float* dv, const float* Wpi, const float* Wv, int A, int H,
                            const float* mask, float* out, int64_t S, hipStream_t s) {
  const int64_t cnt = S * H;
  hipLaunchKernelGGL(heads_bwd_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, dl, dv, Wpi, Wv, A, H,
                     mask, out, cnt);
  return hipGetLastError();
}

__global__ void advance_kernel(int64_t* ctl, int T, uint8_t* reset, int n, float* hbuf, float* cbuf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) reset[i] = reset[(int64_t)T * n + i];
  if (hbuf != nullptr && i < (int64_t)n * HID) {
    hbuf[i] = hbuf[(int64_t)T * n * HID + i];
    cbuf[i] = cbuf[(int64_t)T * n * HID + i];
  }
  if (i == 0) {
    ctl[CTL_STEP] += T;
    ctl[CTL_WINDOW] += 1;
  }
}

static int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

bool net_init(Net& net, int arch, int n_actions, int n_envs, int t_max, int env_offset, uint64_t seed,
              std::string& err) {
  const bool rgb = (arch & ARCH_RGB) != 0;
  const bool stk = (arch & ARCH_STACK) != 0;
  const bool sts = (arch & ARCH_STATES) != 0;
  arch &= ~(ARCH_RGB | ARCH_STACK | ARCH_STATES);
  if ((rgb || stk || sts) && arch == ARCH_FF_NATURE) {
    err = "ARCH_RGB / ARCH_STACK / ARCH_STATES apply to the NIPS head (FF or LSTM) only";
    return false;
  }
  if ((int)rgb + (int)stk + (int)sts > 1) { err = "ARCH_RGB, ARCH_STACK and ARCH_STATES are exclusive"; return false; }
  net.rgb = rgb;
  net.stack = stk;
  net.states = sts;
  net.layout = rgb ? FRAMES_RGB : stk ? FRAMES_STACK : sts ? FRAMES_STATES : FRAMES_RING;
  if (arch != ARCH_FF && arch != ARCH_LSTM && arch != ARCH_FF_NATURE) {
    err = "arch must be 0 (FF), 1 (LSTM) or 2 (FF, Nature head), optionally | 16 (RGB), | 32 (STACK) or | 64 (STATES)";
    return false;
  }
  if (n_actions < 1 || n_actions > MAXA) { err = "n_actions must be in [1, 32]"; return false; }
  if (n_envs < 1 || n_envs > (1 << 20)) { err = "n_envs out of range"; return false; }
  if (t_max < 1 || t_max > 64) { err = "t_max must be in [1, 64]"; return false; }
  if ((int64_t)t_max * n_envs * C1_P >= (int64_t)1 << 31) { err = "t_max * n_envs too large"; return false; }
  net.arch = arch; net.A = n_actions; net.N = n_envs; net.T = t_max; net.R = t_max + 4;
  net.dR = fd_make((uint32_t)net.R); net.dN = fd_make((uint32_t)net.N);
  net.env_offset = env_offset; net.seed = seed;
  const bool NAT = arch == ARCH_FF_NATURE;
  net.hid = NAT ? NHID : HID;
  // ---- parameters, Chainer link order (a3c_ale.py:35,52)
  net.params.clear();
  int64_t off = 0;
  auto add = [&](const char* name, int64_t numel) {
    ParamInfo pi; pi.name = name; pi.offset = off; pi.numel = numel;
    net.params.push_back(pi);
    off = align_up(off + numel, 64);
    return pi.offset;
  };
  net.o_luW = net.o_lub = net.o_llW = net.o_c3W = net.o_c3b = -1;
  if (NAT) {   // dqn_head.py:16-20, then FCSoftmaxPolicy(512) / FCVFunction(512)
    net.o_c1W = add("0/0/W", NC1 * 4 * 8 * 8);
    net.o_c1b = add("0/0/b", NC1);
    net.o_c2W = add("0/1/W", NC2 * NC1 * 4 * 4);
    net.o_c2b = add("0/1/b", NC2);
    net.o_c3W = add("0/2/W", NC3 * NC2 * 3 * 3);
    net.o_c3b = add("0/2/b", NC3);
    net.o_fcW = add("0/3/W", (int64_t)NHID * NA3);
    net.o_fcb = add("0/3/b", NHID);
    net.o_piW = add("1/0/W", (int64_t)n_actions * NHID);
    net.o_pib = add("1/0/b", n_actions);
    net.o_vW = add("2/0/W", NHID);
    net.o_vb = add("2/0/b", 1);
  } else {
    net.o_c1W = add("0/0/W", 16 * (rgb ? 3 : 4) * 8 * 8);
    net.o_c1b = add("0/0/b", 16);
    net.o_c2W = add("0/1/W", 32 * 16 * 4 * 4);
    net.o_c2b = add("0/1/b", 32);
    net.o_fcW = add("0/2/W", (int64_t)HID * A2);
    net.o_fcb = add("0/2/b", HID);
  }
  if (arch == ARCH_FF) {
    net.o_piW = add("1/0/W", (int64_t)n_actions * HID);
    net.o_pib = add("1/0/b", n_actions);
    net.o_vW = add("2/0/W", HID);
    net.o_vb = add("2/0/b", 1);
  } else if (arch == ARCH_LSTM) {
    net.o_luW = add("1/upward/W", (int64_t)GATES * HID);
    net.o_lub = add("1/upward/b", GATES);
    net.o_llW = add("1/lateral/W", (int64_t)GATES * HID);
    net.o_piW = add("2/0/W", (int64_t)n_actions * HID);
    net.o_pib = add("2/0/b", n_actions);
    net.o_vW = add("3/0/W", HID);
    net.o_vb = add("3/0/b", 1);
  }
  net.param_floats = off;
  // the tensors NonbiasWeightDecay skips (nonbias_weight_decay.py:22: name == 'b' or name.endswith('/b'))
  net.decay = DecayArgs{};
  for (const ParamInfo& pi : net.params) {
    const std::string& nm = pi.name;
    if (nm != "b" && (nm.size() < 2 || nm.compare(nm.size() - 2, 2, "/b") != 0)) continue;
    if (net.decay.n_bias == DECAY_MAX_BIAS) { err = "more bias tensors than DECAY_MAX_BIAS"; return false; }
    net.decay.begin[net.decay.n_bias] = pi.offset;
    net.decay.end[net.decay.n_bias++] = pi.offset + pi.numel;
  }
  // ---- workspace
  const int64_t n = n_envs, T = t_max, T1 = T + 1, S = T * n, A = n_actions;
  net.norm_blocks = 256;
  int64_t slab = 0;
  slab = std::max(slab, (int64_t)FC_SPLIT * n * HID);
  slab = std::max(slab, conv_bwd_slab_floats((int)S));
  if (NAT) slab = nature_slab_floats(net);
  if (sts) slab = std::max(slab, states_slab_floats(net));
  net.slab_floats = slab;
  net.bufs.clear();
  int64_t wo = 0;
  auto buf = [&](const char* name, int64_t bytes) {
    Net::Buf b; b.name = name; b.off = wo; b.bytes = bytes;
    net.bufs.push_back(b);
    wo = align_up(wo + std::max<int64_t>(bytes, 1), 256);
    return b.off;
  };
  const bool L = arch == ARCH_LSTM;
  net.w_ctl = buf("ctl", CTL_SIZE * 8);
  net.w_frames = buf("frames", (int64_t)net.R * n * PLANE * (rgb ? 3 : stk ? 4 : sts ? 16 : 1));
  net.w_nvalid = buf("nvalid", (int64_t)net.R * n);
  net.w_reset = buf("reset", T1 * n);
  net.w_rewards = buf("rewards", S * 4);
  net.w_dones = buf("dones", S);
  const int64_t H = net.hid, nA1 = NAT ? NA1 : A1, nA2 = NAT ? NA2 : A2;
  net.w_a1 = buf("a1", T1 * n * nA1 * 4);
  net.w_a2 = buf("a2", T1 * n * nA2 * 4);
  // the FC backward's ReLU mask as bits, written by conv_fwd.hip (its f32-state / Nature paths write none)
  net.w_a2m = buf("a2_mask", (NAT || sts) ? 0 : T1 * n * A2W * 4);
  net.w_a3 = buf("a3", NAT ? T1 * n * NA3 * 4 : 0);
  net.w_hfc = buf("hfc", T1 * n * H * 4);
  net.w_gates = buf("gates", L ? T1 * n * GATES * 4 : 0);
  net.w_hbuf = buf("hbuf", L ? (T + 2) * n * HID * 4 : 0);
  net.w_cbuf = buf("cbuf", L ? (T + 2) * n * HID * 4 : 0);
  net.w_logits = buf("logits", T1 * n * A * 4);
  net.w_probs = buf("probs", T1 * n * A * 4);
  net.w_logp = buf("logp", T1 * n * A * 4);
  net.w_v = buf("v", T1 * n * 4);
  net.w_ent = buf("entropy", T1 * n * 4);
  net.w_logpa = buf("logp_a", T1 * n * 4);
  net.w_act = buf("actions", T1 * n * 4);
  net.w_dlogits = buf("dlogits", S * A * 4);
  net.w_dv = buf("dv", S * 4);
  net.w_dh = buf("dh", L ? S * HID * 4 : 0);
  net.w_dfc = buf("dfc", S * H * 4);
  net.w_dG = buf("dG", L ? S * GATES * 4 : 0);
  net.w_dhn = buf("dhn", L ? n * HID * 4 : 0);
  net.w_dcn = buf("dcn", L ? n * HID * 4 : 0);
  net.w_da2 = buf("da2", S * nA2 * 4);
  net.w_da1 = buf("da1", NAT ? S * NA1 * 4 : sts ? S * A1 * 4 : 0);
  net.w_da3 = buf("da3", NAT ? S * NA3 * 4 : 0);
  net.w_slab = buf("slab", slab * 4);
  net.w_norm = buf("norm_partials", (int64_t)NORM_SCRATCH * 8);   // partials, result, ticket (arl_internal.hpp)
  net.w_tick = buf("tickets", (int64_t)fc_fwd_tiles((int)n) * 4);
  net.w_fcb_part = buf("fc_bwd_partials", NAT ? 0 : fc_bwd_part_floats((int)S) * 4);
  net.w_fcb_tick = buf("fc_bwd_tickets", NAT ? 0 : (int64_t)fc_bwd_tickets() * 4);
  net.w_loss = buf("loss", n * 2 * 4);
  net.w_eval_h = buf("eval_h", L ? n * HID * 4 : 0);
  net.w_eval_c = buf("eval_c", L ? n * HID * 4 : 0);
  net.w_eval_hn = buf("eval_hn", L ? n * HID * 4 : 0);
  net.w_eval_cn = buf("eval_cn", L ? n * HID * 4 : 0);
  net.w_eval_reset = buf("eval_reset", L ? n : 0);
  net.w_zero = buf("zero_row", L ? ZERO_ROW_FLOATS * 4 : 0);
  net.w_fcplanes = buf("fc_planes", NAT ? 0 : FC_PLANES_BYTES);
  // window statistics (optim.hip window_stats_kernel): the ring of records and the count of records written
  net.w_win_log = buf("win_log", (int64_t)WINDOW_LOG * WINDOW_STAT_FIELDS * 8);
  net.w_win_count = buf("win_count", 8);
  // episode statistics: the 14 arrays of EpisodeView, in its order (episode_view computes the same offsets)
  net.w_episodes = wo;
  for (const char* nm : {"ep_run_ret", "ep_run_len", "ep_total", "ep_steps", "ep_count", "ep_sum", "ep_sumsq", "ep_min",
                         "ep_max", "ep_len_sum", "ep_log_count"})
    buf(nm, n * 8);
  for (const char* nm : {"ep_log_ret", "ep_log_len", "ep_log_step"}) buf(nm, (int64_t)EPISODE_LOG * n * 8);
  if (wo - net.w_episodes != episode_block_bytes(n)) { err = "episode statistics layout"; return false; }
  net.ws_bytes = wo;
  return true;
}

// ---------------------------------------------------------------- forward

// a2 > 0 bits of window slot t (conv_fwd.hip writes them, fc_bwd.hip's job B reads them as its ReLU
// mask); null for the nets whose conv forward is not conv_fwd.hip (Nature, f32 states)
static uint32_t* a2_mask(const Net& net, int t) {
  if (net.arch == ARCH_FF_NATURE || net.states) return nullptr;
  return net.at<uint32_t>(net.w_a2m) + (int64_t)t * net.N * A2W;
}

// the FC weight's split planes (fc.hip): rebuilt from the params when a writer bumped the parameter
// generation since they were built (bind, arl_net_params_changed); every update keeps them current
hipError_t ensure_fc_planes(Net& net, hipStream_t s) {
  if (net.planes_current() || net.arch == ARCH_FF_NATURE) return hipSuccess;
  ARL_TRY(launch_fc_planes(net.p + net.o_fcW, net.at<uint16_t>(net.w_fcplanes), s));
  net.planes_gen = net.param_gen;
  return hipSuccess;
}
static const uint16_t* fc_planes(const Net& net) { return net.at<uint16_t>(net.w_fcplanes); }

// head after conv1 (conv2 -> fc) for n rows, activations at a1/a2/hfc
static hipError_t fc_forward(const Net& net, int n, const float* a2, float* hfc, hipStream_t s) {
  return launch_fc_fwd(a2, n, fc_planes(net), net.p + net.o_fcb, net.at<float>(net.w_slab), net.at<int>(net.w_tick),
                       hfc, s, net.forms);
}

// policy / value heads of window slot t (rows of env e0, e0 + 1, ..) reading h
static PolicyArgs slot_policy_args(const Net& net, int t, int mode, int e0 = 0) {
  const float* P = net.p;
  const int A = net.A;
  const int64_t o = (int64_t)t * net.N + e0;
  return make_policy_args(P + net.o_piW, P + net.o_pib, P + net.o_vW, P + net.o_vb, A, net.seed,
                          net.at<int64_t>(net.w_ctl), t, net.env_offset + e0, mode, net.at<float>(net.w_logits) + o * A,
                          net.at<float>(net.w_probs) + o * A, net.at<float>(net.w_logp) + o * A,
                          net.at<float>(net.w_v) + o, net.at<float>(net.w_ent) + o, net.at<int32_t>(net.w_act) + o,
                          net.at<float>(net.w_logpa) + o);
}

// ---- the launches a window and its isolated stages (net_stage) share, each with its argument list here only

// conv1 + conv2 of window slot t from the frame ring for envs [e0, e0 + ne) (ne < 0: all).  bwd_outputs: also a1
// and the a2 > 0 bits, which only the backward reads (the ring-frame kernels skip those stores: 25.6 KB an env)
static hipError_t conv_fwd_slot(const Net& net, int t, int e0, int ne, bool bwd_outputs, hipStream_t s) {
  const float* P = net.p;
  const int n = net.N;
  return launch_conv_fwd(net.at<uint8_t>(net.w_frames), net.at<uint8_t>(net.w_nvalid), net.at<int64_t>(net.w_ctl), n,
                         net.dR, t, P + net.o_c1W, P + net.o_c1b, P + net.o_c2W, P + net.o_c2b,
                         bwd_outputs ? net.at<float>(net.w_a1) + (int64_t)t * n * A1 : nullptr,
                         net.at<float>(net.w_a2) + (int64_t)t * n * A2, s, net.forms, net.layout, e0, ne,
                         bwd_outputs ? a2_mask(net, t) : nullptr);
}

// The LSTM step of slot t for envs [e0, e0 + ne): the gates with the cell in their epilogue.  The FC's split-K
// partials are reduced + bias + relu in the gate kernel's staging (XRED) or were by the FC's last-arriver ticket
// (lstm_xred of the launch's env count); h goes to row t + 1 of hbuf
static hipError_t lstm_gates_step(const Net& net, int t, int e0, int ne, hipStream_t s) {
  const float* P = net.p;
  const int n = net.N;
  const bool xred = lstm_xred(net.forms, ne);
  const int64_t r0 = (int64_t)t * n + e0;
  float* hfc = net.at<float>(net.w_hfc) + r0 * HID;
  return launch_lstm_gates(xred ? nullptr : hfc, net.at<float>(net.w_hbuf) + r0 * HID,
                           net.at<uint8_t>(net.w_reset) + r0, P + net.o_luW, P + net.o_llW, P + net.o_lub,
                           net.at<float>(net.w_gates) + r0 * GATES, net.at<float>(net.w_cbuf) + r0 * HID,
                           net.at<float>(net.w_cbuf) + (r0 + n) * HID, net.at<float>(net.w_hbuf) + (r0 + n) * HID, ne,
                           true, s, xred ? net.at<float>(net.w_slab) + (int64_t)FC_SPLIT * e0 * HID : nullptr,
                           xred ? P + net.o_fcb : nullptr, xred ? hfc : nullptr);
}

// One BPTT step t -> t - 1 (t >= 1): dh_{t-1} = (dG_t Wl) * (no reset at t) and step t - 1's cell in one launch
// (lstm.hip)
static hipError_t lstm_bptt_step(const Net& net, int t, hipStream_t s) {
  const int n = net.N;
  const int64_t o = (int64_t)t * n, op = o - n;
  float* dG = net.at<float>(net.w_dG);
  const float* cbuf = net.at<float>(net.w_cbuf);
  const uint8_t* rs = net.at<uint8_t>(net.w_reset);
  return launch_lstm_bptt(dG + o * GATES, net.p + net.o_llW, rs + o, net.at<float>(net.w_gates) + op * GATES,
                          cbuf + (op + n) * HID, cbuf + op * HID, rs + op, net.at<float>(net.w_dh) + op * HID,
                          net.at<float>(net.w_dcn), dG + op * GATES, net.at<float>(net.w_dhn), n, true, s);
}

// the fused conv backward per sample (conv_bwd.hip), its slabs left for the reduce
static hipError_t conv_bwd_slabs(const Net& net, hipStream_t s) {
  return launch_conv_bwd(net.at<uint8_t>(net.w_frames), net.at<uint8_t>(net.w_nvalid), net.at<int64_t>(net.w_ctl),
                         net.dN, net.dR, net.T * net.N, net.at<float>(net.w_a1), net.at<float>(net.w_da2),
                         net.p + net.o_c2W, net.at<float>(net.w_slab), net.g + net.o_c2W, net.g + net.o_c2b,
                         net.g + net.o_c1W, net.g + net.o_c1b, s, net.forms, /*reduce=*/false, net.layout);
}
// and that reduce, with the folded clip norm's partials when nf.parts is set
static hipError_t conv_bwd_reduce(const Net& net, const NormFold& nf, hipStream_t s) {
  return launch_conv_reduce(net.at<float>(net.w_slab), net.T * net.N, net.g + net.o_c2W, net.g + net.o_c2b,
                            net.g + net.o_c1W, net.g + net.o_c1b, s, net.layout, nf);
}

// ---- the loss-gradient launches' arguments from the net (declared in arl_internal.hpp: nature.hip shares them)

ReturnsArgs window_returns_args(const Net& net, double gamma, float beta, float vcoef, int clip_reward) {
  ReturnsArgs ra{};
  ra.rewards = net.at<float>(net.w_rewards); ra.dones = net.at<uint8_t>(net.w_dones); ra.v = net.at<float>(net.w_v);
  ra.probs = net.at<float>(net.w_probs); ra.logp = net.at<float>(net.w_logp); ra.act = net.at<int32_t>(net.w_act);
  ra.T = net.T; ra.n = net.N; ra.A = net.A;
  ra.gamma = gamma; ra.clip_reward = clip_reward;
  ra.beta = beta; ra.vcoef = vcoef; ra.pcoef = net.pi_coef; ra.keep_scale = net.keep_scale;
  ra.dlogits = net.at<float>(net.w_dlogits); ra.dv = net.at<float>(net.w_dv); ra.loss = net.at<float>(net.w_loss);
  ra.ctl = net.at<int64_t>(net.w_ctl);   // every window launch snapshots the step counter
  return ra;
}

HeadsBwd window_heads_bwd(const Net& net) {
  const bool L = net.arch == ARCH_LSTM;
  return HeadsBwd{net.p + net.o_piW, net.p + net.o_vW, L ? nullptr : net.at<float>(net.w_hfc),
                  L ? net.at<float>(net.w_dh) : net.at<float>(net.w_dfc)};
}

// one PPO epoch's arguments: the window's slots (shared with window_returns_args), the snapshot's planes and the
// options as they stand
static PpoLossArgs window_ppo_args(const Net& net, float beta, float vcoef) {
  const int64_t S = (int64_t)net.T * net.N;
  float* snap = net.ppo_snap;
  PpoLossArgs p{};
  p.r = window_returns_args(net, 0.0, beta, vcoef, 0);
  p.lpo = snap; p.adv = snap + S; p.ret = snap + 2 * S; p.ratio = snap + 3 * S;
  p.lo = net.ppo_lo; p.hi = net.ppo_hi;
  p.vold = net.ppo_vold; p.ev = net.ppo_ev;   // (vold null: the form without value clipping)
  return p;
}

// One lockstep step (conv -> fc [-> LSTM] -> policy) for envs [e0, e0 + ne)
// of window slot t.  Disjoint env ranges touch disjoint rows of every buffer
// (the FC split-K slab and tickets included: e0 is a multiple of the FC's
// 32-row tile), so ranges can run concurrently on separate streams.
hipError_t net_act(Net& net, int t, int mode, hipStream_t s, int e0, int ne) {
  if (ne < 0) {
    e0 = 0;
    ne = net.N;
  }
  if (net.arch == ARCH_FF_NATURE) {
    if (e0 != 0 || ne != net.N || mode > 2) return hipErrorInvalidValue;
    return nature_act(net, t, mode, s);
  }
  const int n = net.N;
  const int part = mode & (ACT_CONV_ONLY | ACT_AFTER_CONV);
  mode &= 3;
  // an env range forks from the caller's stream: stale planes rebuilt on one chain's stream would race
  // the other chains' FC reads (the ABI refuses that case first, arl_act_envs)
  if (ne != n && !net.planes_current()) return hipErrorNotReady;
  ARL_TRY(ensure_fc_planes(net, s));
  // a fused bootstrap launch whose learn never followed (a dropped window) must not make a later
  // window's learn skip its returns: any act of a window's step t < T starts a new window
  if (t < net.T) net.returns_done = false;
  float* a2 = net.at<float>(net.w_a2) + (int64_t)t * n * A2;
  float* hfc = net.at<float>(net.w_hfc) + ((int64_t)t * n + e0) * HID;
  const float* P = net.p;
  if (!(part & ACT_AFTER_CONV) && net.states) {
    if (e0 != 0 || ne != n) return hipErrorInvalidValue;   // one launch over all envs
    ARL_TRY(states_conv_fwd(net, t, net.at<float>(net.w_a1) + (int64_t)t * n * A1, a2, s));
    ARL_TRY(stamp(net, STAGE_CONV_FWD, s));
  } else if (!(part & ACT_AFTER_CONV)) {
    // the bootstrap slot T feeds only the FC / heads forward: no backward reads its a1 or a2 mask
    ARL_TRY(conv_fwd_slot(net, t, e0, ne, t < net.T, s));
    ARL_TRY(stamp(net, STAGE_CONV_FWD, s));
  }
  if (part & ACT_CONV_ONLY) return hipSuccess;
  float* fc_slab = net.at<float>(net.w_slab) + (int64_t)FC_SPLIT * e0 * HID;
  const PolicyArgs pa = slot_policy_args(net, t, t < net.T ? mode : 0, e0);
  if (net.arch != ARCH_LSTM) {   // FF: split-K partials, reduce + relu + heads in one policy_fc launch
    ARL_TRY(launch_fc_fwd(a2 + (int64_t)e0 * A2, ne, fc_planes(net), P + net.o_fcb, fc_slab, nullptr, nullptr, s,
                          net.forms));
    ARL_TRY(stamp(net, STAGE_FC_FWD, s));
    // + the learner's returns (one env group); not while the update runs as PPO epochs (arl_ppo_begin / arl_ppo_learn)
    if (t == net.T && net.fuse_returns && net.ppo_snap == nullptr && e0 == 0 && ne == n) {
      const Net::ReturnsCfg& r = net.ret;
      ARL_TRY(launch_policy_fc_returns(fc_slab, ne, P + net.o_fcb, hfc, pa,
                                       window_returns_args(net, r.gamma, r.beta, r.vcoef, r.clip_reward),
                                       net.gae_lambda, window_heads_bwd(net), s));
      net.returns_done = true;
      net.norm_ready = false;   // a new gradient (as LEARN_RETURNS)
      note_returns_launch(net, r.gamma, r.clip_reward);
      return stamp(net, STAGE_POLICY, s);
    }
    ARL_TRY(launch_policy_fc(fc_slab, ne, P + net.o_fcb, hfc, pa, s));
    return stamp(net, STAGE_POLICY, s);
  }
  // LSTM: the FC's split-K partials, reduced + bias + relu either in the gate kernel's staging (XRED) or
  // by the FC's last-arriver ticket (lstm_xred); then the gates with the cell in their epilogue
  const bool xred = lstm_xred(net.forms, ne);
  ARL_TRY(launch_fc_fwd(a2 + (int64_t)e0 * A2, ne, fc_planes(net), P + net.o_fcb, fc_slab,
                        xred ? nullptr : net.at<int>(net.w_tick) + fc_fwd_tiles(e0), xred ? nullptr : hfc, s,
                        net.forms));
  ARL_TRY(stamp(net, STAGE_FC_FWD, s));
  ARL_TRY(lstm_gates_step(net, t, e0, ne, s));
  ARL_TRY(stamp(net, STAGE_LSTM_GATES, s));
  ARL_TRY(launch_policy_args(net.at<float>(net.w_hbuf) + ((int64_t)(t + 1) * n + e0) * HID, ne, pa, s, HID));
  return stamp(net, STAGE_POLICY, s);
}

// Policy arguments of a forward on explicit states (slot T): a sampled action
// draws from Philox stream 1 with a host counter, one per call, so repeated
// calls on the same state are independent draws and never collide with the
// window's draws (stream 0, counter = step + t).
PolicyArgs states_policy_args(Net& net, int mode) {
  PolicyArgs pa = slot_policy_args(net, net.T, mode);
  if (mode == 1) {
    pa.ctl = net.at<int64_t>(net.w_ctl) + CTL_ZERO;
    pa.step_off = net.eval_draws++;
    pa.stream = 1u;
  }
  return pa;
}

// Drop-in pi_and_v on explicit f32 states (dqn_phi output); results land in
// activation slot T (the bootstrap slot) of the workspace.  LSTM: the
// recurrent state is the pi_and_v state (eval_h / eval_c, reset flags
// eval_reset = "state is None"), separate from the lockstep window's; it
// advances unless keep (keep_same_state, a3c_ale.py:57-60).
hipError_t net_forward_f32(Net& net, const float* x, int n, int mode, hipStream_t s, bool keep) {
  if (net.arch == ARCH_FF_NATURE) return nature_forward_f32(net, x, n, mode, s);
  if (n > net.N) return hipErrorInvalidValue;
  const int T = net.T, N = net.N;
  float* a1 = net.at<float>(net.w_a1) + (int64_t)T * N * A1;
  float* a2 = net.at<float>(net.w_a2) + (int64_t)T * N * A2;
  float* hfc = net.at<float>(net.w_hfc) + (int64_t)T * N * HID;
  const float* P = net.p;
  ARL_TRY(ensure_fc_planes(net, s));
  const int K1 = (net.rgb ? 3 : 4) * 64;
  ARL_TRY((launch_gemm<64, 16, 32, 4, 1>(Conv1F32A{x, K1 / 64}, WeightT{P + net.o_c1W, K1},
                                                      EpiConv{a1, P + net.o_c1b, C1_OC, C1_P}, n * C1_P, C1_OC, K1,
                                                      1, s)));
  ARL_TRY((launch_gemm<32, 32, 32, 2, 2, GS, GK>(Conv2A{a1}, WeightT{P + net.o_c2W, 256},
                                                      EpiConv{a2, P + net.o_c2b, C2_OC, C2_P}, n * C2_P, C2_OC, 256,
                                                      1, s)));
  ARL_TRY(fc_forward(net, n, a2, hfc, s));
  const float* hpol = hfc;
  if (net.arch == ARCH_LSTM) {
    float* gates = net.at<float>(net.w_gates) + (int64_t)T * N * GATES;
    float* eh = net.at<float>(net.w_eval_h);
    float* ec = net.at<float>(net.w_eval_c);
    float* hn = net.at<float>(net.w_eval_hn);
    float* cn = net.at<float>(net.w_eval_cn);
    uint8_t* rs = net.at<uint8_t>(net.w_eval_reset);
    ARL_TRY(launch_lstm_gates(hfc, eh, rs, P + net.o_luW, P + net.o_llW, P + net.o_lub, gates, ec, cn, hn, n, true, s));
    const int64_t cnt = (int64_t)n * HID;
    if (!keep) {
      ARL_TRY(hipMemcpyAsync(eh, hn, cnt * 4, hipMemcpyDeviceToDevice, s));
      ARL_TRY(hipMemcpyAsync(ec, cn, cnt * 4, hipMemcpyDeviceToDevice, s));
      ARL_TRY(hipMemsetAsync(rs, 0, n, s));
    }
    hpol = hn;
  }
  const PolicyArgs pa = states_policy_args(net, mode);
  return launch_policy_args(hpol, n, pa, s, HID);
}

// A3CLSTM.reset_state (a3c_ale.py:65-66) for the pi_and_v state of rows [e0, e0 + n)
hipError_t net_reset_state(Net& net, int e0, int n, hipStream_t s) {
  if (net.arch != ARCH_LSTM) return hipSuccess;
  return hipMemsetAsync(net.at<uint8_t>(net.w_eval_reset) + e0, 1, n, s);
}

// ---------------------------------------------------------------- backward
// the folded clip norm's arguments (none unless arl_net_set_norm_fold): the
// conv tensors are [0, o_fcW) of the flat gradient, everything after is final
// before the conv slab reduce
static NormFold norm_fold_args(const Net& net) {
  if (!net.norm_fold) return NormFold{};
  return NormFold{net.at<double>(net.w_norm), net.g, net.o_fcW, net.param_floats, net.norm_rest_blocks};
}

// the fused conv backward (per-sample slabs) and its slab reduce (with the folded clip norm's
// partials when nf.parts is set): the learner's last part
static hipError_t conv_backward(Net& net, hipStream_t s, const NormFold& nf) {
  ARL_TRY(conv_bwd_slabs(net, s));
  ARL_TRY(stamp(net, STAGE_CONV_BWD, s));
  ARL_TRY(conv_bwd_reduce(net, nf, s));
  return stamp(net, STAGE_CONV_REDUCE, s);
}

hipError_t net_learn(Net& net, double gamma, float beta, float vcoef, int clip_reward, hipStream_t s) {
  if (net.arch == ARCH_FF_NATURE) return nature_learn(net, gamma, beta, vcoef, clip_reward, s);
  for (int part = 0; part < LEARN_CONV; ++part) ARL_TRY(net_learn_part(net, part, gamma, beta, vcoef, clip_reward, s));
  // the conv part last; with norm_fold its slab reduce also leaves the clip norm's partials
  // (every other gradient tensor is final by now: one stream)
  if (net.states) {   // the generic-GEMM conv backward has no folded norm: the update runs grad_sqnorm
    ARL_TRY(states_conv_bwd(net, s));
    net.norm_ready = false;
    return hipSuccess;
  }
  ARL_TRY(conv_backward(net, s, norm_fold_args(net)));
  net.norm_ready = net.norm_fold;
  return hipSuccess;
}

// PPO epochs (arl_net_set_ppo; FF nets, and LSTM nets with a carry buffer): the window's snapshot from the
// workspace, after its bootstrap forward
hipError_t net_ppo_begin(Net& net, double gamma, int clip_reward, hipStream_t s) {
  const int64_t S = (int64_t)net.T * net.N;
  float* snap = net.ppo_snap;
  const ReturnsArgs ra = window_returns_args(net, gamma, 0.f, 0.f, clip_reward);
  net.returns_done = false;
  note_returns_launch(net, gamma, clip_reward);   // the window statistics repeat the snapshot's returns
  ARL_TRY(launch_ppo_snapshot(ra, net.gae_lambda, snap, snap + S, snap + 2 * S, s));
  net.ppo_begun = true;
  net.ppo_epoch = 0;
  ARL_TRY(stamp(net, STAGE_OTHER, s));
  // LSTM: the rollout's (h_T, c_T), before the re-forwards of epochs >= 2 overwrite rows T (net_ppo_restore)
  if (net.arch == ARCH_LSTM) {
    if (net.ppo_carry == nullptr) return hipErrorInvalidValue;   // (arl_net_set_ppo refuses an LSTM without one)
    ARL_TRY(launch_ppo_carry(net.at<float>(net.w_hbuf), net.at<float>(net.w_cbuf), net.ppo_carry, net.T, net.N, false, s));
    ARL_TRY(stamp(net, STAGE_OTHER, s));
  }
  // arl_net_set_ppo_options: v_old of the window, then the adv plane normalised in place (each with a stamp
  // of its own; with the options off nothing more is launched)
  if (net.ppo_vold != nullptr) {
    ARL_TRY(launch_ppo_vold(ra.dones, ra.v, net.ppo_vold, net.T, net.N, s));
    ARL_TRY(stamp(net, STAGE_OTHER, s));
  }
  if (net.ppo_norm_adv) {
    ARL_TRY(launch_ppo_normalize_adv(ra.dones, snap + S, net.T, net.N, net.ppo_aux + 1, s));
    ARL_TRY(stamp(net, STAGE_OTHER, s));
  }
  return hipSuccess;
}

// One epoch's gradient: the PPO loss gradient + heads dh (it also snapshots the step counter, as the returns
// launch it stands in for), then the trunk and conv parts unchanged
hipError_t net_ppo_learn(Net& net, float beta, float vcoef, hipStream_t s) {
  const PpoLossArgs p = window_ppo_args(net, beta, vcoef);
  net.norm_ready = false;   // a new gradient, no folded norm
  net.returns_done = false;
  ARL_TRY(launch_ppo_heads(p, window_heads_bwd(net), s));
  ARL_TRY(stamp(net, STAGE_RETURNS, s));
  net.ppo_epoch += 1;
  if (net.ppo_aux != nullptr) {   // the epoch's record, while its ratio plane and the slots' log_probs / v stand
    ARL_TRY(launch_ppo_epoch_stats(p, net.at<int64_t>(net.w_ctl), 0.0, (double)net.ppo_epoch,
                                   reinterpret_cast<int64_t*>(net.ppo_aux), net.ppo_aux, s));
    ARL_TRY(stamp(net, STAGE_OTHER, s));
  }
  ARL_TRY(net_learn_part(net, LEARN_TRUNK, 0.0, beta, vcoef, 0, s));
  return net_learn_part(net, LEARN_CONV, 0.0, beta, vcoef, 0, s);
}

// LSTM gate weight gradients ([x | h_prev] operand, reset rows' h dropped) straight into the gradient
// and dfc = (dG Wu) * (hfc > 0), one launch (fc_bwd.hip's ShapeLSTM)
static hipError_t lstm_wgrad(Net& net, hipStream_t s) {
  const int S = net.T * net.N;
  return launch_lstm_wgrad(net.at<float>(net.w_dG), net.at<float>(net.w_hfc), net.at<float>(net.w_hbuf),
                           net.at<uint8_t>(net.w_reset), net.at<float>(net.w_zero), net.p + net.o_luW, S,
                           net.g + net.o_luW, net.g + net.o_llW, net.g + net.o_lub, net.at<float>(net.w_dfc),
                           net.at<float>(net.w_fcb_part), net.at<int>(net.w_fcb_tick), s);
}

// the heads' weight gradients ride on the FC backward launch (its job C)
static HeadsDW heads_dw(const Net& net) {
  const float* hh = net.arch == ARCH_LSTM ? net.at<float>(net.w_hbuf) + (int64_t)net.N * HID : net.at<float>(net.w_hfc);
  return HeadsDW{net.at<float>(net.w_dlogits), net.at<float>(net.w_dv), hh, net.A, net.g + net.o_piW,
                 net.g + net.o_pib, net.g + net.o_vW, net.g + net.o_vb};
}

static hipError_t fc_backward(Net& net, hipStream_t s) {
  const HeadsDW heads = heads_dw(net);
  return launch_fc_bwd(net.at<float>(net.w_dfc), net.at<float>(net.w_a2), net.p + net.o_fcW, net.T * net.N,
                       net.g + net.o_fcW, net.g + net.o_fcb, net.at<float>(net.w_da2), net.at<float>(net.w_fcb_part),
                       net.at<int>(net.w_fcb_tick), s, &heads, a2_mask(net, 0));
}

// One part of the NIPS learner (LEARN_* in arl_internal.hpp), in order on one stream
hipError_t net_learn_part(Net& net, int part, double gamma, float beta, float vcoef, int clip_reward, hipStream_t s) {
  if (net.arch == ARCH_FF_NATURE) return hipErrorInvalidValue;
  const int n = net.N, T = net.T;
  if (part == LEARN_RETURNS) {
    if (net.returns_done) {   // the bootstrap policy launch ran it (net_act, fuse_returns)
      net.returns_done = false;
      return hipSuccess;
    }
    // n-step returns + loss gradient wrt logits / v (a3c.py:82-126); also snapshots the step counter for
    // the optimizer's fused advance and, in the same launch, the heads' backward dh (FF: dfc = dh * (hfc > 0))
    net.norm_ready = false;   // a new gradient: no folded norm until net_learn's reduce
    note_returns_launch(net, gamma, clip_reward);
    ARL_TRY(launch_returns_heads(window_returns_args(net, gamma, beta, vcoef, clip_reward), net.gae_lambda,
                                 window_heads_bwd(net), s));
    return stamp(net, STAGE_RETURNS, s);
  }
  if (part == LEARN_CONV) {
    if (net.states) {
      ARL_TRY(states_conv_bwd(net, s));
      return stamp(net, STAGE_CONV_BWD, s);
    }
    // fused conv backward per sample (conv_bwd.hip): conv2 dW/db, da1 = conv_transpose(da2, W2) * (a1 > 0)
    // kept in LDS, conv1 dW/db straight from the frame ring; then its slab reduce
    return conv_backward(net, s, NormFold{});
  }
  if (part != LEARN_TRUNK) return hipErrorInvalidValue;
  // LSTM: truncated BPTT over the window (a3c.py:144), then the gate weight gradients and dfc
  if (net.arch == ARCH_LSTM) {
    const float* cbuf = net.at<float>(net.w_cbuf);
    const int64_t cnt = (int64_t)n * HID;
    // step T-1's cell, then one BPTT step per t = T-1 .. 1
    const int64_t oT = (int64_t)(T - 1) * n;
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s,
                       net.at<float>(net.w_gates) + oT * GATES, cbuf + (oT + n) * HID, cbuf + oT * HID,
                       net.at<uint8_t>(net.w_reset) + oT, net.at<float>(net.w_dh) + oT * HID, net.at<float>(net.w_dhn),
                       net.at<float>(net.w_dcn), net.at<float>(net.w_dG) + oT * GATES, 1, cnt);
    ARL_TRY(hipGetLastError());
    ARL_TRY(stamp(net, STAGE_LSTM_CELL, s));
    for (int t = T - 1; t > 0; --t) {
      ARL_TRY(lstm_bptt_step(net, t, s));
      ARL_TRY(stamp(net, STAGE_LSTM_BPTT, s));
    }
    ARL_TRY(lstm_wgrad(net, s));
    ARL_TRY(stamp(net, STAGE_LSTM_WGRAD, s));
  }
  // FC: dW + db straight into the gradient and da2 = (dfc W) * (a2 > 0), with the heads' weight
  // gradients, one launch (fc_bwd.hip)
  ARL_TRY(fc_backward(net, s));
  return stamp(net, STAGE_FC_BWD, s);
}

// One stage of a window on the current workspace contents (arl_run_stage):
// the same launches the window makes, isolated for timing.
hipError_t net_stage(Net& net, int stage, int t, hipStream_t s) {
  if (net.arch == ARCH_FF_NATURE) return nature_stage(net, stage, t, s);
  const int n = net.N;
  const float* P = net.p;
  float* slab = net.at<float>(net.w_slab);
  float* a2 = net.at<float>(net.w_a2);
  float* hfc = net.at<float>(net.w_hfc);
  if (net.states && (stage == STAGE_CONV_FWD || stage == STAGE_CONV_BWD || stage == STAGE_CONV_REDUCE)) {
    if (stage == STAGE_CONV_FWD)
      return states_conv_fwd(net, t, net.at<float>(net.w_a1) + (int64_t)t * n * A1, a2 + (int64_t)t * n * A2, s);
    return stage == STAGE_CONV_BWD ? states_conv_bwd(net, s) : hipSuccess;   // (no separate slab reduce)
  }
  switch (stage) {
    case STAGE_CONV_FWD:   // all envs, with the backward's outputs whatever the slot
      return conv_fwd_slot(net, t, 0, -1, true, s);
    case STAGE_FC_FWD:   // as in net_act: FF (and the LSTM's XRED gate kernel) reduce the partials downstream
      ARL_TRY(ensure_fc_planes(net, s));
      if (net.arch != ARCH_LSTM || lstm_xred(net.forms, n))
        return launch_fc_fwd(a2 + (int64_t)t * n * A2, n, fc_planes(net), P + net.o_fcb, slab, nullptr, nullptr, s,
                             net.forms);
      return fc_forward(net, n, a2 + (int64_t)t * n * A2, hfc + (int64_t)t * n * HID, s);
    case STAGE_POLICY: {
      const int64_t o = (int64_t)t * n;
      if (net.arch != ARCH_LSTM)
        return launch_policy_fc(slab, n, P + net.o_fcb, hfc + o * HID, slot_policy_args(net, t, 0), s);
      return launch_policy_args(net.at<float>(net.w_hbuf) + (o + n) * HID, n, slot_policy_args(net, t, 0), s, HID);
    }
    case STAGE_FC_BWD:   // with the heads' weight gradients (job C), as in LEARN_TRUNK
      return fc_backward(net, s);
    case STAGE_CONV_BWD:
      return conv_bwd_slabs(net, s);
    case STAGE_RETURNS:   // the LEARN_RETURNS launch (returns + loss gradient + heads dh), default coefficients
      return net_learn_part(net, LEARN_RETURNS, 0.99, 0.01f, 0.5f, 1, s);
    case STAGE_CONV_REDUCE:
      return conv_bwd_reduce(net, norm_fold_args(net), s);   // as arl_learn launches it
    case STAGE_GRAD_SQNORM:
      return launch_grad_sqnorm(net.g, net.param_floats, net.at<double>(net.w_norm), net.norm_blocks, s);
    case STAGE_LSTM_GATES:   // as net_act's LSTM step over all envs
      if (net.arch != ARCH_LSTM) return hipErrorInvalidValue;
      return lstm_gates_step(net, t, 0, n, s);
    case STAGE_LSTM_BPTT:    // the BPTT step t -> t - 1 (t = T - 1 when t is 0)
      if (net.arch != ARCH_LSTM || net.T < 2) return hipErrorInvalidValue;
      return lstm_bptt_step(net, t > 0 && t < net.T ? t : net.T - 1, s);
    case STAGE_LSTM_WGRAD:
      if (net.arch != ARCH_LSTM) return hipErrorInvalidValue;
      return lstm_wgrad(net, s);
    case STAGE_RMSPROP: {   // the update kernel as a window runs it (clip 40 from the last norm the window left), lr 0
      UpdateArgs u;
      u.norm_sq = net.at<double>(net.w_norm);
      u.nparts = net.norm_ready ? conv_norm_parts(net.norm_rest_blocks) : net.norm_blocks;
      u.clip = 40.f;
      u.t_max = net.T;
      return launch_rmsprop(net.p, net.ms, net.g, net.param_floats, 0.0, 0.99, 0.1, u, s);
    }
    default:
      return hipErrorInvalidValue;
  }
}

// The carry of a PPO window on the LSTM: rows T of hbuf / cbuf back to the rollout's (h_T, c_T) that
// net_ppo_begin saved, before anything advances -- the last epoch's BPTT and heads weight gradient read the
// re-forwarded rows T, so this belongs to the update, not to net_ppo_learn.  FF nets, and windows without a
// snapshot: nothing is launched.
static hipError_t net_ppo_restore(Net& net, hipStream_t s) {
  if (net.arch != ARCH_LSTM || !net.ppo_begun || net.ppo_carry == nullptr) return hipSuccess;
  ARL_TRY(launch_ppo_carry(net.at<float>(net.w_hbuf), net.at<float>(net.w_cbuf), net.ppo_carry, net.T, net.N, true, s));
  return stamp(net, STAGE_OTHER, s);
}

hipError_t net_optimize(Net& net, double lr0, int64_t total_steps, int64_t n_total, double alpha, double eps,
                        float clip, hipStream_t s, bool advance) {
  double* parts = net.at<double>(net.w_norm);
  if (advance) ARL_TRY(net_ppo_restore(net, s));
  const bool do_clip = clip > 0.f;
  // arl_learn left the step snapshot (returns kernel), so the update kernel
  // can also advance the window
  const bool fused = advance;
  const bool folded = do_clip && net.norm_ready;   // partials left by arl_learn's conv reduce
  net.norm_ready = false;
  // the window statistics record the squared norm even when the update does not clip
  if ((do_clip || net.window_stats) && !folded) {
    ARL_TRY(launch_grad_sqnorm(net.g, net.param_floats, parts, net.norm_blocks, s));
    ARL_TRY(stamp(net, STAGE_GRAD_SQNORM, s));
  }
  const bool L = net.arch == ARCH_LSTM;
  // the update rewrites the FC weight's split planes with the new W (all of them, so they are current
  // afterwards even if they were not before)
  uint16_t* planes = net.arch == ARCH_FF_NATURE ? nullptr : net.at<uint16_t>(net.w_fcplanes);
  const AdvanceArgs adv{fused ? net.at<int64_t>(net.w_ctl) : nullptr, planes, net.o_fcW, net.at<uint8_t>(net.w_reset),
                        L ? net.at<float>(net.w_hbuf) : nullptr, L ? net.at<float>(net.w_cbuf) : nullptr, net.T,
                        net.N};
  UpdateArgs u;   // of the record and of the update
  u.norm_sq = parts;
  u.nparts = folded ? conv_norm_parts(net.norm_rest_blocks) : net.norm_blocks;
  u.clip = clip;
  u.lr_ctl = total_steps > 0 ? net.at<int64_t>(net.w_ctl) : nullptr;
  u.total_steps = total_steps;
  u.n_total = n_total;
  u.t_max = net.T;
  u.adv = &adv;
  u.wd = &net.decay;
  AdamArgs ad{net.adam_beta1, net.adam_beta2, net.at<int64_t>(net.w_ctl), 0};
  if (net.window_stats) {   // one record of the window this update consumes, before anything advances
    const WindowStatsArgs w{net.at<float>(net.w_rewards), net.at<uint8_t>(net.w_dones), net.at<float>(net.w_v),
                            net.at<float>(net.w_ent), net.at<float>(net.w_loss), net.T, net.N, net.win_gamma,
                            net.win_clip_reward, net.at<int64_t>(net.w_ctl), net.at<double>(net.w_win_log),
                            net.at<int64_t>(net.w_win_count)};
    ARL_TRY(launch_window_stats(w, lr0, u, s, net.win_lambda));
    ad.stats_log = net.at<double>(net.w_win_log);   // (Adam: the record's lr becomes its step size, launch_adam)
    ad.stats_count = net.at<int64_t>(net.w_win_count);
  }
  if (!do_clip) u.norm_sq = nullptr;   // (the record took the norm; the update reads it only to clip)
  if (planes != nullptr) net.planes_gen = net.param_gen;
  // the net's optimizer (arl_net_set_adam): Adam takes lr0 as its alpha and ms as its second moment
  if (net.adam_m != nullptr)
    ARL_TRY(launch_adam(net.p, net.adam_m, net.ms, net.g, net.param_floats, lr0, eps, ad, u, s));
  else
    ARL_TRY(launch_rmsprop(net.p, net.ms, net.g, net.param_floats, lr0, alpha, eps, u, s));
  ARL_TRY(stamp(net, STAGE_RMSPROP, s));
  if (advance) net.ppo_begun = false;   // the next window's epochs need their own snapshot
  return advance && !fused ? net_advance(net, s) : hipSuccess;
}

hipError_t net_advance(Net& net, hipStream_t s) {
  const bool L = net.arch == ARCH_LSTM;
  const int64_t cnt = L ? (int64_t)net.N * HID : net.N;
  ARL_TRY(net_ppo_restore(net, s));
  net.ppo_begun = false;
  hipLaunchKernelGGL(advance_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, net.at<int64_t>(net.w_ctl),
                     net.T, net.at<uint8_t>(net.w_reset), net.N, L ? net.at<float>(net.w_hbuf) : nullptr,
                     L ? net.at<float>(net.w_cbuf) : nullptr);
  return hipGetLastError();
}

}  // namespace arl
