// Policy / value heads, softmax policy output and action sampling; n-step
// returns and the loss gradient of the A3C objective.
//
// Reference: policy.py:28-29,53-58 (FCSoftmaxPolicy: logits = h W^T + b),
// v_function.py:29-34 (FCVFunction), policy_output.py:12-61
// (SoftmaxPolicyOutput: softmax, log_softmax, entropy, sampled actions and
// their log-probs), a3c.py:69-70 (reward clip), a3c.py:82-126 (n-step
// return, advantage, pi/v/entropy losses).
//
// policy_kernel: one 4-wave workgroup per 4 env rows (C3 window 1.0642-1.0678 -> 1.0582-1.0588 ms
// against 16 rows, 1.0635-1.0641 at 1 row, r5am).  The A logits and the
// value are one small GEMM on the matrix cores: [16 rows x 256] . [256 x
// (A + 1)] with v_mfma_f32_16x16x4_f32 (exact f32 products; each lane's h and
// W fragments are 16-byte loads covering 4 k-steps, k permuted identically on
// both sides); the 4 waves take one K quarter each and the partial tiles are
// summed in wave order.  The rows go through LDS to one lane
// per env, which accumulates the softmax, log-softmax and entropy serially
// (k = 0..A-1, the order NumPy uses for small rows) so the sampler's f32 CDF
// is reproducible by the CPU oracle.  The draw is inverse-CDF on a
// counter-based Philox4x32-10 uniform keyed by (seed; env id, step), so
// sampling needs no RNG state and a captured graph replays with fresh
// numbers; mode 2 takes the first argmax instead (most_probable_actions,
// policy_output.py:37-39).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "arl_internal.hpp"
#include "policy_rows.hpp"

namespace arl {

// HW = hidden width (256: NIPS head / LSTM; 512: Nature head)
constexpr int PK_ROWS = 4;   // env rows a workgroup (the MFMA tile's other rows repeat the last: bit-identical)
template <int HW>
__global__ void __launch_bounds__(256)
policy_kernel(const float* __restrict__ h, int64_t n, PolicyArgs pa) {
  __shared__ float part[4][16][MAXA + 2];
  __shared__ float zs[16][MAXA + 2];
  policy_rows16<HW, false, false, PK_ROWS>(h, (int64_t)blockIdx.x * PK_ROWS, n, pa, part, zs);
}

hipError_t launch_policy_args(const float* h, int64_t n, const PolicyArgs& pa, hipStream_t s, int hid) {
  if (n <= 0) return hipSuccess;
  if (hid == 512)
    hipLaunchKernelGGL(policy_kernel<512>, dim3((unsigned)((n + PK_ROWS - 1) / PK_ROWS)), dim3(256), 0, s, h, n, pa);
  else if (hid == HID)
    hipLaunchKernelGGL(policy_kernel<HID>, dim3((unsigned)((n + PK_ROWS - 1) / PK_ROWS)), dim3(256), 0, s, h, n, pa);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// FF act step: the FC forward's split-K reduce moved here from fc_fwd_kernel's
// last arriver (fc.hip).  The 8 partial slabs of this group's rows are
// summed in split order 0..7 from 0.f, then + bias, relu -- the same f32 op
// sequence as the ticket path, so hfc is bit-identical -- written to hfc (the
// backward reads it) and to LDS, where the heads read it.
// PF_ROWS env rows per workgroup (1: 256 workgroups at 256 envs, each reading
// 8 KB of partials; measured 4.33 us vs 4.57 at 2 rows, 4.62 at 4, 5.56 at 16,
// where the reduce ran on 16 CUs)
constexpr int PF_ROWS = 1;
__global__ void __launch_bounds__(256)
policy_fc_kernel(const float* __restrict__ slab, int n, const float* __restrict__ fc_bias, float* __restrict__ hfc,
                 PolicyArgs pa) {
  __shared__ float part[4][16][MAXA + 2];
  __shared__ float zs[16][MAXA + 2];
  __shared__ __attribute__((aligned(16))) float hl[PF_ROWS * HID];
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * PF_ROWS;
  constexpr int NV = PF_ROWS * HID / 4;          // float4 per slab of this group
  constexpr int V4 = (NV + 255) / 256;           // per thread
  const HeadsPrefetch<HID> pf = heads_prefetch<HID>(pa);   // in flight with the slab loads
  f32x4v p[V4][FC_SPLIT];
#pragma unroll
  for (int z = 0; z < FC_SPLIT; ++z)
#pragma unroll
    for (int j = 0; j < V4; ++j) {
      const int idx = min(tid + 256 * j, NV - 1), r = idx / (HID / 4), c = 4 * (idx % (HID / 4));
      const int64_t m = min(row0 + r, (int64_t)n - 1);
      p[j][z] = *reinterpret_cast<const f32x4v*>(slab + ((int64_t)z * n + m) * HID + c);
    }
#pragma unroll
  for (int j = 0; j < V4; ++j) {
    const int idx = tid + 256 * j, r = idx / (HID / 4), c = 4 * (idx % (HID / 4));
    if (idx >= NV) break;
    f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int z = 0; z < FC_SPLIT; ++z)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], p[j][z][e]);
    const float4 b = *reinterpret_cast<const float4*>(fc_bias + c);
    float4 o;
    o.x = fmaxf(__fadd_rn(acc[0], b.x), 0.f); o.y = fmaxf(__fadd_rn(acc[1], b.y), 0.f);
    o.z = fmaxf(__fadd_rn(acc[2], b.z), 0.f); o.w = fmaxf(__fadd_rn(acc[3], b.w), 0.f);
    *reinterpret_cast<float4*>(hl + r * HID + c) = o;
    if (row0 + r < n) *reinterpret_cast<float4*>(hfc + (row0 + r) * HID + c) = o;
  }
  __syncthreads();
  policy_rows16<HID, false, true, PF_ROWS>(hl, row0, n, pa, part, zs, &pf);
}

hipError_t launch_policy_fc(const float* slab, int n, const float* fc_bias, float* hfc, const PolicyArgs& pa,
                            hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(policy_fc_kernel, dim3((unsigned)((n + PF_ROWS - 1) / PF_ROWS)), dim3(256), 0, s, slab, n, fc_bias, hfc, pa);
  return hipGetLastError();
}

hipError_t launch_policy(const float* h, int64_t n, const float* Wpi, const float* bpi, const float* Wv,
                         const float* bv, int A, uint64_t seed, const int64_t* ctl, int64_t step_off,
                         int env_offset, int mode, float* logits, float* probs, float* logp, float* v,
                         float* ent, int32_t* act, float* logp_a, hipStream_t s, int hid) {
  if (n <= 0) return hipSuccess;
  return launch_policy_args(h, n, make_policy_args(Wpi, bpi, Wv, bv, A, seed, ctl, step_off, env_offset, mode, logits,
                                                   probs, logp, v, ent, act, logp_a), s, hid);
}

// a3c.py:82-126 over a lockstep window, one thread per (step t, env).
// rewards/dones (T, n); v/probs/logp/act indexed (T+1, n[, A]) with row T =
// the bootstrap value v(s_T) computed with the pre-update parameters.
// R accumulates in float64 (Python float at a3c.py:83-92) and restarts at 0
// at every terminal (dones bit 0), so each episode segment in the window is
// one a3c update.  Thread (t, e) runs the reverse recurrence R = R*gamma + r
// from T-1 down to its own t -- the same operations in the same order as a
// sequential scan, so R_t is bit-identical -- with every reward / done of its
// env loaded up front (no dependent loads in the chain).  Steps flagged past
// the window's end (dones bit 1, arl_truncate_window: the reference's window
// closed early at a terminal, a3c.py:77-78) get no loss and a zero gradient.
// Loss scale (a3c.py:110-121): pi terms * pi_loss_coef, v terms * v_loss_coef,
// and with keep_loss_scale_same both * t_max / len for a segment that a
// terminal closed after len < t_max steps.  The per-env losses are then
// summed in the reference's order (t = T-1 .. 0) through LDS.  ctl != null:
// also snapshot the step counter (CTL_STEP_SNAP) for the optimizer's fused
// advance.  Block = EB envs x T steps (EB = 256 / T), env fastest.
// The arguments: ReturnsArgs (arl_internal.hpp; it stays arl::ReturnsArgs with its fields in that order -- the
// name is part of the kernels' mangled names and the layout is what they read) and the forms derived from it here.
// The launch's form G, compile time: the n-step advantage, the GAE one, or a clipped-surrogate (PPO) epoch on a
// window's snapshot (arl_net_set_ppo).  false / true in a template argument list are RF_NSTEP / RF_GAE.
// (ints, not an unnamed enum: the forms appear in the kernels' mangled names through ReturnsArgsT, and an unnamed
// type there is numbered differently by the host and the device compilation)
constexpr int RF_NSTEP = 0, RF_GAE = 1, RF_PPO = 2, RF_PPO_VC = 3;
// RF_PPO_VC: the PPO form with the clipped value loss (arl_net_set_ppo_options); rf_ppo: either PPO form
constexpr bool rf_ppo(int G) { return G == RF_PPO || G == RF_PPO_VC; }
// the GAE form's arguments (below): + gl = gamma * lambda.  ReturnsArgsT<RF_NSTEP> is ReturnsArgs itself.
struct ReturnsArgsGae : ReturnsArgs {
  double gl;
};
// the PPO form's arguments (below): + the snapshot's planes, the ratio's output (or null) and the clip range
// lo = (float)(1.0 - eps_clip), hi = (float)(1.0 + eps_clip); rewards and gamma are not read
struct ReturnsArgsPpo : ReturnsArgs {
  const float* lpo;
  const float* adv;
  const float* ret;
  float* ratio;
  float lo, hi;
};
// the value-clipped PPO form's arguments: + the values the rollout's policy gave (0 where a sample is not live)
// and ev = (float)vclip_eps, formed on the host
struct ReturnsArgsPpoVc : ReturnsArgsPpo {
  const float* vold;
  float ev;
};
template <int G>
using ReturnsArgsT = std::conditional_t<
    G == RF_PPO_VC, ReturnsArgsPpoVc,
    std::conditional_t<G == RF_PPO, ReturnsArgsPpo, std::conditional_t<G == RF_GAE, ReturnsArgsGae, ReturnsArgs>>>;

// dlogits / dv of (step t, env e); returns the two loss terms of the step
// (pi term without the sign, v term) through lpi / lv
// Every load of the thread is issued before the arithmetic that uses it
// (register arrays with static indices, clamped offsets): a load after a
// store the compiler cannot disambiguate, or under a per-lane branch, would
// wait for the one before it.  Windows up to RW steps keep their rewards /
// dones in registers; longer ones loop over memory.
constexpr int RW = 8;
// GAE form (G, compile time; the host picks it for lambda != 1, arl_net_set_gae): the policy term's advantage
// is the GAE(lambda) one (gae_step) instead of f32(Rf - v); the value target stays the n-step return.  It
// carries gl = gamma * lambda and the register window of v: v[0 .. RW-1] at clamped offsets beside vboot, the
// RW + 1 values v[k + 1] is taken from.  The G = false forms hold and do nothing more than they did.
// PPO form (RF_PPO; the host picks it while arl_net_set_ppo is on): the return and the advantage are the
// snapshot's (ppo_snapshot_kernel left there what the two forms above would form), the policy term is the clipped
// surrogate's with the ratio exp(lp[ac] - lpo).  It scans only the dones, for the segment of keep_loss_scale_same.
// Value-clipped PPO form (RF_PPO_VC; the host picks it while arl_net_set_ppo_options has vclip_eps > 0): the
// PPO form with one more load, vold, and a value tail of its own in returns_compute (vclip_step).  New
// instantiations only: the other three forms compile to the instructions they had (DESIGN.md "PPO options").
template <int G>
struct GaeIn {};
template <>
struct GaeIn<RF_GAE> {
  float vw[RW];
  double gl;
};
template <>
struct GaeIn<RF_PPO> {
  float lpo, adv, Rf;
};
template <>
struct GaeIn<RF_PPO_VC> : GaeIn<RF_PPO> {
  float vold;
};
// The clipped value loss 0.5 * max((v - R)^2, (v_clip - R)^2), v_clip = vold + clamp(v - vold, -ev, ev), for
// one sample (the header's "value clipping"; every operation f32 round-to-nearest, unfused): lsq = the square
// the loss takes; returns taken = the clipped square is the larger, so the value gets no gradient.  Within
// ev of vold (every sample in epoch 1) this is today's lsq = f32(dvv * dvv), not taken.  Shared by the loss
// gradient (returns_compute) and the per-epoch record (ppo_epoch_stats_kernel), as return_step / gae_step are.
__device__ inline bool vclip_step(float vi, float vold, float Rf, float ev, float dvv, float& lsq) {
  const float dvo = __fsub_rn(vi, vold);
  const float lu = __fmul_rn(dvv, dvv);
  lsq = lu;
  if (fabsf(dvo) <= ev) return false;
  const float vc = __fadd_rn(vold, dvo > 0.f ? ev : -ev);
  const float dvc = __fsub_rn(vc, Rf);
  const float lc = __fmul_rn(dvc, dvc);
  const bool taken = lc > lu;
  if (taken) lsq = lc;
  return taken;
}
// AM >= A: the action count the registers are sized for (4 / 8 / MAXA)
template <int AM, int G = RF_NSTEP>
struct RetIn : GaeIn<G> {   // everything returns_one reads of step (t, e)
  float pr[AM], lp[AM], rw[RW];
  int dn[RW];
  float vboot, vi;
  int ac, di;
};
template <int AM, int G>
__device__ inline void returns_load(const ReturnsArgsT<G>& a, int t, int e, RetIn<AM, G>& in) {
  const int T = a.T, n = a.n, A = a.A;
  const int64_t i = (int64_t)t * n + e;
#pragma unroll
  for (int k = 0; k < AM; ++k) {
    const int64_t o = i * A + min(k, A - 1);
    in.pr[k] = a.probs[o];
    in.lp[k] = a.logp[o];
  }
#pragma unroll
  for (int k = 0; k < RW; ++k) {
    const int64_t o = (int64_t)min(k, T - 1) * n + e;
    if constexpr (!rf_ppo(G)) in.rw[k] = a.rewards[o];
    in.dn[k] = a.dones[o];
    if constexpr (G == RF_GAE) in.vw[k] = a.v[o];
  }
  if constexpr (rf_ppo(G)) {
    in.lpo = a.lpo[i];
    in.adv = a.adv[i];
    in.Rf = a.ret[i];
    if constexpr (G == RF_PPO_VC) in.vold = a.vold[i];
  } else {
    in.vboot = a.v[(int64_t)T * n + e];
  }
  in.vi = a.v[i];
  in.ac = a.act[i];
  in.di = a.dones[i];
}
template <int AM, int G>
__device__ inline void returns_compute(const ReturnsArgsT<G>& a, int t, int e, const RetIn<AM, G>& in, float& lpi,
                                       float& lv, float* sdl) {
  const int T = a.T, n = a.n, A = a.A;
  const int64_t i = (int64_t)t * n + e;
  const float* pr = in.pr;
  const float* lp = in.lp;
  const float* rw = in.rw;
  const int* dn = in.dn;
  float vboot = 0.f;
  if constexpr (!rf_ppo(G)) vboot = in.vboot;
  const float vi = in.vi;
  const int ac = in.ac, di = in.di;
  float* dl = a.dlogits + i * A;
  if (di & 2) {   // past the end of this window
    for (int k = 0; k < A; ++k) dl[k] = 0.f;
    a.dv[i] = 0.f;
    if (sdl)
      for (int k = 0; k <= A; ++k) sdl[k] = 0.f;
    if constexpr (rf_ppo(G))
      if (a.ratio != nullptr) a.ratio[i] = 0.f;
    lpi = 0.f;
    lv = 0.f;
    return;
  }
  double R = (double)vboot;
  double Gl = 0.0;    // GAE form: the advantage's scan, beside R's
  int seg_end = -1;   // first terminal at or after t: closes t's segment
  int seg_start = 0;  // first step after the last terminal before t
  if (T <= RW) {
#pragma unroll
    for (int k = RW - 1; k >= 0; --k)
      if (k < T && k >= t) {
        if (dn[k] & 1) seg_end = k;
        if constexpr (!rf_ppo(G)) R = return_step(R, dn[k], rw[k], a.gamma, a.clip_reward);
        if constexpr (G == RF_GAE)   // v[k + 1]: the bootstrap value at the window's last step (k = RW - 1 is always that)
          Gl = gae_step(Gl, dn[k], rw[k], in.vw[k], k == T - 1 ? vboot : in.vw[k < RW - 1 ? k + 1 : k], a.gamma,
                        in.gl, a.clip_reward);
      }
#pragma unroll
    for (int k = 0; k < RW; ++k)
      if (k < t && (dn[k] & 1)) seg_start = k + 1;
  } else {
    for (int tt = T - 1; tt >= t; --tt) {
      const int64_t j = (int64_t)tt * n + e;
      if (a.dones[j] & 1) seg_end = tt;
      if constexpr (!rf_ppo(G)) R = return_step(R, a.dones[j], a.rewards[j], a.gamma, a.clip_reward);
      if constexpr (G == RF_GAE)
        Gl = gae_step(Gl, a.dones[j], a.rewards[j], a.v[j], tt == T - 1 ? vboot : a.v[j + n], a.gamma, in.gl,
                      a.clip_reward);
    }
    for (int tt = t - 1; tt >= 0; --tt)
      if (a.dones[(int64_t)tt * n + e] & 1) {
        seg_start = tt + 1;
        break;
      }
  }
  float pf = a.pcoef, vf = a.vcoef;
  if (a.keep_scale && seg_end >= 0) {
    const int len = seg_end - seg_start + 1;
    if (len < T) {
      const float factor = (float)((double)T / (double)len);
      pf = __fmul_rn(pf, factor);
      vf = __fmul_rn(vf, factor);
    }
  }
  float Rf, adv;
  if constexpr (rf_ppo(G)) {
    Rf = in.Rf;
    adv = in.adv;
  } else {
    Rf = (float)R;
    if constexpr (G == RF_GAE) adv = (float)Gl;
    else adv = __fsub_rn(Rf, vi);
  }
  float H = 0.f, lpa = 0.f;
#pragma unroll
  for (int k = 0; k < AM; ++k)
    if (k < A) {
      H = __fadd_rn(H, __fmul_rn(pr[k], lp[k]));
      if (k == ac) lpa = lp[k];
    }
  H = -H;
  // the policy term's weight w (of the gradient) and its loss term: adv and lp[ac] * adv, or the clipped
  // surrogate's (the header's "clipped-surrogate epochs"); rho == 1 leaves w == adv
  float w = adv, surr = 0.f;
  if constexpr (rf_ppo(G)) {
    const float rho = (float)exp((double)__fsub_rn(lpa, in.lpo));
    const bool active = adv >= 0.f ? rho <= a.hi : rho >= a.lo;
    w = active ? __fmul_rn(rho, adv) : 0.f;
    surr = active ? w : __fmul_rn(adv >= 0.f ? a.hi : a.lo, adv);
    if (a.ratio != nullptr) a.ratio[i] = rho;
  }
#pragma unroll
  for (int k = 0; k < AM; ++k)
    if (k < A) {
      const float oh = (k == ac) ? 1.f : 0.f;
      const float t1 = __fmul_rn(-w, __fsub_rn(oh, pr[k]));
      const float t2 = __fmul_rn(__fmul_rn(a.beta, pr[k]), __fadd_rn(lp[k], H));
      const float d = __fmul_rn(pf, __fadd_rn(t1, t2));
      dl[k] = d;
      if (sdl) sdl[k] = d;
    }
  const float dvv = __fsub_rn(vi, Rf);
  if constexpr (G == RF_PPO_VC) {   // the clipped value loss: its own tail, the other forms' below stays as it was
    float lsq;
    const bool taken = vclip_step(vi, in.vold, Rf, a.ev, dvv, lsq);
    const float dvc = taken ? 0.f : __fmul_rn(vf, dvv);
    a.dv[i] = dvc;
    if (sdl) sdl[A] = dvc;
    lpi = __fmul_rn(pf, __fadd_rn(surr, __fmul_rn(a.beta, H)));
    lv = __fmul_rn(vf, __fmul_rn(lsq, 0.5f));
    return;
  }
  const float dvo = __fmul_rn(vf, dvv);
  a.dv[i] = dvo;
  if (sdl) sdl[A] = dvo;
  float pterm;
  if constexpr (G == RF_PPO) pterm = surr;
  else pterm = __fmul_rn(lpa, adv);
  lpi = __fmul_rn(pf, __fadd_rn(pterm, __fmul_rn(a.beta, H)));
  lv = __fmul_rn(vf, __fmul_rn(__fmul_rn(dvv, dvv), 0.5f));
}
template <int G>
__device__ inline void returns_one(const ReturnsArgsT<G>& a, int t, int e, float& lpi, float& lv) {
  RetIn<MAXA, G> in;
  if constexpr (G == RF_GAE) in.gl = a.gl;
  returns_load<MAXA, G>(a, t, e, in);
  returns_compute<MAXA, G>(a, t, e, in, lpi, lv, nullptr);
}

// per-env losses summed in the reference's order (t = T-1 .. 0)
__device__ inline void env_loss(const ReturnsArgs& a, const float* lpi, const float* lv, int EB, int el, int e) {
  float pi_loss = 0.f, v_loss = 0.f;
  for (int tt = a.T - 1; tt >= 0; --tt) {
    pi_loss = __fsub_rn(pi_loss, lpi[tt * EB + el]);
    v_loss = __fadd_rn(v_loss, lv[tt * EB + el]);
  }
  a.loss[2 * e] = pi_loss;
  a.loss[2 * e + 1] = v_loss;
}

template <int G = RF_NSTEP>
__global__ void __launch_bounds__(256)
returns_kernel(ReturnsArgsT<G> a) {
  __shared__ float lpi[256], lv[256];
  if (a.ctl != nullptr && blockIdx.x == 0 && threadIdx.x == 0) a.ctl[CTL_STEP_SNAP] = a.ctl[CTL_STEP];
  const int EB = 256 / a.T;
  const int tid = threadIdx.x, t = tid / EB, el = tid - t * EB;
  const int e = blockIdx.x * EB + el;
  const bool on = t < a.T && e < a.n;
  if (on) returns_one<G>(a, t, e, lpi[tid], lv[tid]);
  if (a.loss == nullptr) return;
  __syncthreads();
  if (t == 0 && on) env_loss(a, lpi, lv, EB, el, e);
}

// The snapshot a window's PPO epochs share (arl_net_set_ppo), one thread per (step t, env) as returns_kernel:
// lpo = logp[t, e, act[t, e]], ret = Rf and adv as the G form of returns_compute forms them (the same loads, the
// same device functions in the same order), or 0, 0, 0 past a truncated window's end.  G: RF_NSTEP or RF_GAE.
struct SnapArgs : ReturnsArgsGae {   // probs: any readable (T, n, A) array (not used), dlogits / dv / loss: null
  float* lpo_out;
  float* adv_out;
  float* ret_out;
};
template <int G>
__global__ void __launch_bounds__(256)
ppo_snapshot_kernel(SnapArgs a) {
  const int EB = 256 / a.T;
  const int tid = threadIdx.x, t = tid / EB, el = tid - t * EB;
  const int e = blockIdx.x * EB + el;
  if (t >= a.T || e >= a.n) return;
  RetIn<1, G> in;
  if constexpr (G == RF_GAE) in.gl = a.gl;
  returns_load<1, G>(a, t, e, in);
  const int64_t i = (int64_t)t * a.n + e;
  const float lpa = a.logp[i * a.A + min(max(in.ac, 0), a.A - 1)];
  float lpo = 0.f, adv = 0.f, Rf = 0.f;
  if (!(in.di & 2)) {
    // returns_compute's scan of R (and Gl) without the segment bookkeeping -- its own copy: with the scan in a
    // function the two shared, the existing forms no longer compiled to the instructions they had
    const float vboot = in.vboot;
    double R = (double)vboot, Gl = 0.0;
    if (a.T <= RW) {
#pragma unroll
      for (int k = RW - 1; k >= 0; --k)
        if (k < a.T && k >= t) {
          R = return_step(R, in.dn[k], in.rw[k], a.gamma, a.clip_reward);
          if constexpr (G == RF_GAE)
            Gl = gae_step(Gl, in.dn[k], in.rw[k], in.vw[k], k == a.T - 1 ? vboot : in.vw[k < RW - 1 ? k + 1 : k],
                          a.gamma, in.gl, a.clip_reward);
        }
    } else {
      for (int tt = a.T - 1; tt >= t; --tt) {
        const int64_t j = (int64_t)tt * a.n + e;
        R = return_step(R, a.dones[j], a.rewards[j], a.gamma, a.clip_reward);
        if constexpr (G == RF_GAE)
          Gl = gae_step(Gl, a.dones[j], a.rewards[j], a.v[j], tt == a.T - 1 ? vboot : a.v[j + a.n], a.gamma, in.gl,
                        a.clip_reward);
      }
    }
    Rf = (float)R;
    if constexpr (G == RF_GAE) adv = (float)Gl;
    else adv = __fsub_rn(Rf, in.vi);
    lpo = lpa;
  }
  a.lpo_out[i] = lpo;
  a.adv_out[i] = adv;
  a.ret_out[i] = Rf;
}

// returns_kernel + the heads' backward (a3c.py:129-130 through policy.py /
// v_function.py): dh[s][j] = sum_k dlogits[s][k] Wpi[k][j] + dv[s] Wv[j],
// times (mask[s][j] > 0) when mask is given, for the T steps of one env per
// block -- the rows the block's own threads just produced, handed over in
// LDS.  Thread j of the block owns column j (HID = 256 = blockDim): its Wpi /
// Wv column and its mask entries are loaded up front, beside the returns' own
// loads.  rh_load issues every load of a block, rh_finish does the rest, so
// the bootstrap step's policy launch can run both around its own work
// (policy_fc_returns_kernel).
// AM >= A actions, RB rows (steps) per pass: the register arrays (mask
// entries, head-weight column, loaded probs / log-probs) are sized for the
// window, e.g. 5 rows and 4 actions at C2 instead of 32 and 32
template <int AM, int RB, int G = RF_NSTEP>
struct RhState {
  float mv[RB];
  int64_t so[RB];
  float wc[AM + 1];
  RetIn<AM, G> in;
};

// mask entries of rows r0 .. r0 + RB - 1 (row r = step r of env e) for column j = threadIdx.x
// (unconditional loads at clamped offsets: a load under a per-lane branch would wait for each one in turn)
template <int AM, int RB, int G>
__device__ inline void rh_rows(const ReturnsArgs& a, const float* __restrict__ mask, int e, int r0,
                               RhState<AM, RB, G>& st) {
  const int j = threadIdx.x;
#pragma unroll
  for (int u = 0; u < RB; ++u) {
    const int r = r0 + u;
    st.so[u] = (r < a.T && e < a.n) ? ((int64_t)r * a.n + e) * HID + j : -1;
  }
#pragma unroll
  for (int u = 0; u < RB; ++u) st.mv[u] = mask != nullptr ? mask[st.so[u] < 0 ? j : st.so[u]] : 1.f;
}

template <int AM, int RB, int G>
__device__ inline void rh_load(const ReturnsArgsT<G>& a, const float* __restrict__ Wpi, const float* __restrict__ Wv,
                               const float* __restrict__ mask, int e, RhState<AM, RB, G>& st) {
  const int T = a.T, A = a.A, j = threadIdx.x;
  rh_rows(a, mask, e, 0, st);
#pragma unroll
  for (int k = 0; k <= AM; ++k) st.wc[k] = k < A ? Wpi[min(k, A - 1) * HID + j] : Wv[j];
  returns_load<AM, G>(a, min((int)threadIdx.x, T - 1), min(e, a.n - 1), st.in);   // off threads: a valid step, discarded
}

// lpi / lv: 64 floats, sdl: 64 (AM + 1), w: (AM + 1) HID of LDS
template <int AM, int RB, int G>
__device__ inline void rh_finish(const ReturnsArgsT<G>& a, const float* __restrict__ mask, float* __restrict__ dh, int e,
                                 RhState<AM, RB, G>& st, float* lpi, float* lv, float* sdl, float* w) {
  const int T = a.T, A = a.A;
  const int tid = threadIdx.x, t = tid, j = tid;
  const bool on = t < T && e < a.n;
#pragma unroll
  for (int k = 0; k <= AM; ++k)
    if (k <= A) w[k * HID + j] = k < A ? st.wc[k] : st.wc[AM];   // thread j's own column
  if (on) returns_compute<AM, G>(a, t, e, st.in, lpi[tid], lv[tid], sdl + tid * (A + 1));   // row tid = step t
  __syncthreads();
  if (a.loss != nullptr && t == 0 && on) env_loss(a, lpi, lv, 1, 0, e);
  for (int r0 = 0; r0 < T; r0 += RB) {
    if (r0 > 0) rh_rows(a, mask, e, r0, st);   // T > RB: the next RB rows
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      if (st.so[u] < 0) continue;
      const float* d = sdl + (r0 + u) * (A + 1);
      float acc = 0.f;
      for (int k = 0; k < A; ++k) acc = __fadd_rn(acc, __fmul_rn(d[k], w[k * HID + j]));
      acc = __fadd_rn(acc, __fmul_rn(d[A], w[A * HID + j]));
      dh[st.so[u]] = st.mv[u] > 0.f ? acc : 0.f;
    }
  }
}

template <int AM, int RB, int G = RF_NSTEP>
__global__ void __launch_bounds__(256)
returns_heads_kernel(ReturnsArgsT<G> a, const float* __restrict__ Wpi, const float* __restrict__ Wv,
                     const float* __restrict__ mask, float* __restrict__ dh) {
  __shared__ float lpi[64], lv[64];
  __shared__ float sdl[64 * (AM + 1)];
  __shared__ float w[(AM + 1) * HID];
  if (a.ctl != nullptr && blockIdx.x == 0 && threadIdx.x == 0) a.ctl[CTL_STEP_SNAP] = a.ctl[CTL_STEP];
  RhState<AM, RB, G> st;
  if constexpr (G == RF_GAE) st.in.gl = a.gl;
  rh_load<AM, RB, G>(a, Wpi, Wv, mask, blockIdx.x, st);
  rh_finish<AM, RB, G>(a, mask, dh, blockIdx.x, st, lpi, lv, sdl, w);
}

// The FF window's bootstrap step (slot T, no draw) with the learner's first
// launch folded in: block e runs policy_fc_kernel's row e (the FC split-K
// reduce + relu + heads), then returns_heads_kernel's env e, whose bootstrap
// value v(s_T) is the row's own value head output, taken from LDS (the same
// f32 the policy stores to v).  Every load of the returns part is issued
// before the FC partials' loads.  Results are bit-identical to the two
// launches: the same per-element arithmetic in the same order.
// GAE form: v(s_T) from LDS as here; the other v rows (slots 0 .. T - 1, earlier launches' stores) from memory.
template <int AM, int RB, int G = RF_NSTEP>
__global__ void __launch_bounds__(256)
policy_fc_returns_kernel(const float* __restrict__ slab, int n, const float* __restrict__ fc_bias,
                         float* __restrict__ hfc, PolicyArgs pa, ReturnsArgsT<G> ra, const float* __restrict__ mask,
                         float* __restrict__ dh) {
  __shared__ float part[4][16][MAXA + 2];
  __shared__ float zs[16][MAXA + 2];
  __shared__ __attribute__((aligned(16))) float hl[HID];
  __shared__ float lpi[64], lv[64];
  __shared__ float sdl[64 * (AM + 1)];
  __shared__ float w[(AM + 1) * HID];
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x;
  const int e = blockIdx.x;
  if (ra.ctl != nullptr && e == 0 && tid == 0) ra.ctl[CTL_STEP_SNAP] = ra.ctl[CTL_STEP];
  RhState<AM, RB, G> st;
  if constexpr (G == RF_GAE) st.in.gl = ra.gl;
  rh_load<AM, RB, G>(ra, pa.Wpi, pa.Wv, mask, e, st);
  const HeadsPrefetch<HID> pf = heads_prefetch<HID>(pa);
  // policy_fc_kernel's row (PF_ROWS = 1): threads 0..63 hold one float4 column of the 8 partials
  const int c = 4 * (tid & 63);
  const int64_t m = min((int64_t)e, (int64_t)n - 1);
  f32x4v p[FC_SPLIT];
#pragma unroll
  for (int z = 0; z < FC_SPLIT; ++z) p[z] = *reinterpret_cast<const f32x4v*>(slab + ((int64_t)z * n + m) * HID + c);
  if (tid < HID / 4) {
    f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int z = 0; z < FC_SPLIT; ++z)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], p[z][k]);
    const float4 b = *reinterpret_cast<const float4*>(fc_bias + c);
    float4 o;
    o.x = fmaxf(__fadd_rn(acc[0], b.x), 0.f); o.y = fmaxf(__fadd_rn(acc[1], b.y), 0.f);
    o.z = fmaxf(__fadd_rn(acc[2], b.z), 0.f); o.w = fmaxf(__fadd_rn(acc[3], b.w), 0.f);
    *reinterpret_cast<float4*>(hl + c) = o;
    if (e < n) *reinterpret_cast<float4*>(hfc + (int64_t)e * HID + c) = o;
  }
  __syncthreads();
  policy_rows16<HID, false, true, 1>(hl, e, n, pa, part, zs, &pf);   // ends with a barrier
  st.in.vboot = zs[0][pa.A];   // v(s_T) of env e (heads_row_out stored zs[0][A] to v)
  rh_finish<AM, RB, G>(ra, mask, dh, e, st, lpi, lv, sdl, w);
}

// ---------------------------------------------------------------- the loss-gradient launches
// Each launcher picks its form G once (RF_NSTEP / RF_GAE by gae_on(lambda), RF_PPO / RF_PPO_VC by vold) and hands
// that form's arguments to its kernel's launch template below.
// gl = gamma * lambda: one f64 product, formed here on the host
static ReturnsArgsGae gae_args(const ReturnsArgs& ra, double lambda) {
  ReturnsArgsGae rg;
  static_cast<ReturnsArgs&>(rg) = ra;
  rg.gl = ra.gamma * lambda;
  return rg;
}

static ReturnsArgsPpo ppo_args(const PpoLossArgs& p) {
  ReturnsArgsPpo a;
  static_cast<ReturnsArgs&>(a) = p.r;
  a.rewards = nullptr; a.gamma = 0.0; a.clip_reward = 0;   // not read: the same launch whatever a caller left there
  a.lpo = p.lpo; a.adv = p.adv; a.ret = p.ret; a.ratio = p.ratio;
  a.lo = p.lo; a.hi = p.hi;
  return a;
}

// p.vold set: the value-clipped form's arguments
static ReturnsArgsPpoVc ppo_vc_args(const PpoLossArgs& p) {
  ReturnsArgsPpoVc a;
  static_cast<ReturnsArgsPpo&>(a) = ppo_args(p);
  a.vold = p.vold;
  a.ev = p.ev;
  return a;
}

// The register shapes of the heads kernels, the one place that chooses them: AM = the action count and RB = the
// rows (steps) a pass their register arrays are sized for (RhState).  f(AM, RB) launches, the two as
// std::integral_constants.
template <class F>
static hipError_t with_heads_shape(int T, int A, F&& f) {
  if (T < 1 || T > 64 || A < 1 || A > MAXA) return hipErrorInvalidValue;
  using std::integral_constant;
  if (T > 8) f(integral_constant<int, MAXA>{}, integral_constant<int, 32>{});
  else if (A <= 4) f(integral_constant<int, 4>{}, integral_constant<int, 8>{});
  else if (A <= 8) f(integral_constant<int, 8>{}, integral_constant<int, 8>{});
  else f(integral_constant<int, MAXA>{}, integral_constant<int, 8>{});
  return hipGetLastError();
}

template <int G>
static hipError_t returns_form(const ReturnsArgsT<G>& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.T < 1 || a.T > 256) return hipErrorInvalidValue;
  const int EB = 256 / a.T;
  hipLaunchKernelGGL(returns_kernel<G>, dim3((a.n + EB - 1) / EB), dim3(256), 0, s, a);
  return hipGetLastError();
}

template <int G>
static hipError_t returns_heads_form(const ReturnsArgsT<G>& a, const HeadsBwd& hb, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  return with_heads_shape(a.T, a.A, [&](auto am, auto rb) {
    hipLaunchKernelGGL((returns_heads_kernel<decltype(am)::value, decltype(rb)::value, G>), dim3(a.n), dim3(256), 0, s,
                       a, hb.Wpi, hb.Wv, hb.mask, hb.dh);
  });
}

template <int G>
static hipError_t policy_fc_returns_form(const float* slab, const float* fc_bias, float* hfc, const PolicyArgs& pa,
                                         const ReturnsArgsT<G>& ra, const HeadsBwd& hb, hipStream_t s) {
  return with_heads_shape(ra.T, ra.A, [&](auto am, auto rb) {
    hipLaunchKernelGGL((policy_fc_returns_kernel<decltype(am)::value, decltype(rb)::value, G>), dim3(ra.n), dim3(256),
                       0, s, slab, ra.n, fc_bias, hfc, pa, ra, hb.mask, hb.dh);
  });
}

hipError_t launch_returns(const ReturnsArgs& ra, double lambda, hipStream_t s) {
  return gae_on(lambda) ? returns_form<RF_GAE>(gae_args(ra, lambda), s) : returns_form<RF_NSTEP>(ra, s);
}

hipError_t launch_returns_heads(const ReturnsArgs& ra, double lambda, const HeadsBwd& hb, hipStream_t s) {
  return gae_on(lambda) ? returns_heads_form<RF_GAE>(gae_args(ra, lambda), hb, s)
                        : returns_heads_form<RF_NSTEP>(ra, hb, s);
}

// hb.Wpi / hb.Wv are not read: the heads' weights are the policy's own (pa)
hipError_t launch_policy_fc_returns(const float* slab, int n, const float* fc_bias, float* hfc, const PolicyArgs& pa,
                                    const ReturnsArgs& ra, double lambda, const HeadsBwd& hb, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (ra.n != n || ra.A != pa.A) return hipErrorInvalidValue;   // one set of rows, one set of heads
  return gae_on(lambda) ? policy_fc_returns_form<RF_GAE>(slab, fc_bias, hfc, pa, gae_args(ra, lambda), hb, s)
                        : policy_fc_returns_form<RF_NSTEP>(slab, fc_bias, hfc, pa, ra, hb, s);
}

hipError_t launch_ppo_snapshot(const ReturnsArgs& ra, double lambda, float* lpo, float* adv, float* ret, hipStream_t s) {
  if (ra.n <= 0) return hipSuccess;
  if (ra.T < 1 || ra.T > 256) return hipErrorInvalidValue;
  const int EB = 256 / ra.T;
  SnapArgs a{};   // the coefficients and dlogits / dv / loss / ctl stay 0 / null: the kernel has no use for them
  a.rewards = ra.rewards; a.dones = ra.dones; a.v = ra.v; a.logp = ra.logp; a.act = ra.act;
  a.probs = ra.logp;   // (any readable (T, n, A) array)
  a.T = ra.T; a.n = ra.n; a.A = ra.A;
  a.gamma = ra.gamma; a.clip_reward = ra.clip_reward; a.gl = ra.gamma * lambda;
  a.lpo_out = lpo; a.adv_out = adv; a.ret_out = ret;
  const dim3 grid((ra.n + EB - 1) / EB), blk(256);
  if (gae_on(lambda)) hipLaunchKernelGGL(ppo_snapshot_kernel<RF_GAE>, grid, blk, 0, s, a);
  else hipLaunchKernelGGL(ppo_snapshot_kernel<RF_NSTEP>, grid, blk, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ppo_lossgrad(const PpoLossArgs& p, hipStream_t s) {
  return p.vold != nullptr ? returns_form<RF_PPO_VC>(ppo_vc_args(p), s) : returns_form<RF_PPO>(ppo_args(p), s);
}

hipError_t launch_ppo_heads(const PpoLossArgs& p, const HeadsBwd& hb, hipStream_t s) {
  return p.vold != nullptr ? returns_heads_form<RF_PPO_VC>(ppo_vc_args(p), hb, s)
                           : returns_heads_form<RF_PPO>(ppo_args(p), hb, s);
}

// ---------------------------------------------------------------- PPO options (arl_net_set_ppo_options)
// The two one-workgroup kernels below follow window_stats_kernel's ordering rule (optim.hip): thread j of 256
// owns envs j, j + 256, ... ascending, and per env the steps t = 0 .. T - 1 ascending; its f64 partial sums
// start at +0.0 and a sample that is not live (dones bit 1) adds +0.0; partial 0, then partials 1 .. 255 are
// added in order.  Every f64 operation is an unfused round-to-nearest one, so a NumPy restatement in this
// order gives the same bits.

// partial 0 + partial 1 + ... + partial 255 of column f (stride S doubles a thread), the adds in that order;
// op 1 / 2: the column's max / min instead (one instruction stream for the lanes of a wave, whatever their op).
// The LDS reads of 32 partials at a time are in flight ahead of the chain that waits for them.
template <int S>
__device__ inline double ordered_total(const double* part, int f, int op = 0) {
  double sum = part[f];
  for (int q0 = 1; q0 < 256; q0 += 32) {
    double x[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) x[u] = part[min(q0 + u, 255) * S + f];
#pragma unroll
    for (int u = 0; u < 32; ++u)
      if (q0 + u < 256) {
        const double add = __dadd_rn(sum, x[u]), mx = fmax(sum, x[u]), mn = fmin(sum, x[u]);
        sum = op == 0 ? add : op == 1 ? mx : mn;
      }
  }
  return sum;
}

// v_old of a window (arl_ppo_begin with value clipping on): v[t, e] of a live sample, else 0
__global__ void __launch_bounds__(256)
ppo_vold_kernel(const uint8_t* __restrict__ dones, const float* __restrict__ v, float* __restrict__ vold, int64_t S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < S) vold[i] = (dones[i] & 2) ? 0.f : v[i];
}

// A thread's samples in the one-workgroup kernels' order, f(i, dones[i], adv[i]) for each: envs j, j + 256, ...,
// per env t ascending.  Windows up to PO_RW steps load an env's adv / dones into registers first (static
// indices, clamped offsets, as returns_load), so the loads of an env are in flight together and ahead of f's
// stores; longer windows loop over memory.
constexpr int PO_RW = 8;
template <class F>
__device__ inline void ppo_for_samples(const uint8_t* __restrict__ dones, const float* adv, int T, int n, F&& f) {
  for (int e = threadIdx.x; e < n; e += 256) {
    if (T <= PO_RW) {
      float a[PO_RW];
      int d[PO_RW];
#pragma unroll
      for (int k = 0; k < PO_RW; ++k) {
        const int64_t o = (int64_t)min(k, T - 1) * n + e;
        a[k] = adv[o];
        d[k] = dones[o];
      }
#pragma unroll
      for (int k = 0; k < PO_RW; ++k)
        if (k < T) f((int64_t)k * n + e, d[k], a[k]);
    } else {
      for (int t = 0; t < T; ++t) {
        const int64_t i = (int64_t)t * n + e;
        f(i, (int)dones[i], adv[i]);
      }
    }
  }
}

// Advantage normalisation (the header's definition): the snapshot's adv plane in place, over the live samples,
//   mean = S1 / n_live,  std = sqrt(S2 / n_live) (population),  adv' = (float)((adv - mean) / (std + 1e-8))
// in three passes; each thread reads and writes only its own envs' samples, and the two barriers order the
// partials.  Every thread forms the totals itself from the 256 partials in LDS (the same adds in the same
// order, so the same bits).  moments: n_live, mean, std.
__global__ void __launch_bounds__(256)
ppo_normalize_adv_kernel(const uint8_t* __restrict__ dones, float* adv, int T, int n, double* __restrict__ moments) {
  __shared__ double p1[256], p2[256];
  __shared__ int pc[256];
  const int j = threadIdx.x;
  double s1 = 0.0;
  int cnt = 0;
  ppo_for_samples(dones, adv, T, n, [&](int64_t, int d, float a) {
    const bool live = (d & 2) == 0;
    s1 = __dadd_rn(s1, live ? (double)a : 0.0);
    cnt += live ? 1 : 0;
  });
  p1[j] = s1;
  pc[j] = cnt;
  __syncthreads();
  int64_t n_live = 0;
  for (int q = 0; q < 256; ++q) n_live += pc[q];
  if (n_live == 0) {   // nothing to rewrite (the same branch in every thread)
    if (j == 0) moments[0] = moments[1] = moments[2] = 0.0;
    return;
  }
  const double nl = (double)n_live;
  const double mean = ordered_total<1>(p1, 0) / nl;
  double s2 = 0.0;
  ppo_for_samples(dones, adv, T, n, [&](int64_t, int d, float a) {
    const double dd = __dsub_rn((double)a, mean);
    s2 = __dadd_rn(s2, (d & 2) == 0 ? __dmul_rn(dd, dd) : 0.0);
  });
  p2[j] = s2;
  __syncthreads();
  const double sd = sqrt(ordered_total<1>(p2, 0) / nl);
  const double den = __dadd_rn(sd, 1e-8);
  ppo_for_samples(dones, adv, T, n, [&](int64_t i, int d, float a) {
    if ((d & 2) == 0) adv[i] = (float)(__dsub_rn((double)a, mean) / den);
  });
  if (j == 0) {
    moments[0] = nl;
    moments[1] = mean;
    moments[2] = sd;
  }
}

// The per-epoch record (the header's table): fields 2 .. 9 from one pass over the samples, combined by the
// first eight lanes (one field each); thread 0 writes the record.  count non-null: the record goes to slot
// *count % PPO_LOG of the ring at rec and the count is advanced; null: rec is the record itself.
struct EpochStatsArgs {
  const uint8_t* dones;
  const float *v, *logp;
  const int32_t* act;
  const float *lpo, *adv, *ret, *ratio, *vold;   // vold: null = no value clipping (vclipped = 0)
  int T, n, A;
  float lo, hi, ev;
  const int64_t* ctl;   // non-null: window = ctl[CTL_WINDOW]
  double window, epoch;
  int64_t* count;
  double* rec;
};
constexpr int ES_SUMS = 8;   // samples, clipped, kl_sum, ratio_max, ratio_min, vclipped, adv_sum, adv_sumsq
static_assert(2 + ES_SUMS == PPO_STAT_FIELDS, "epoch record layout");
__global__ void __launch_bounds__(256)
ppo_epoch_stats_kernel(EpochStatsArgs a) {
  __shared__ double part[256 * ES_SUMS];
  __shared__ double tot[ES_SUMS];
  const int j = threadIdx.x, T = a.T, n = a.n, A = a.A;
  double acc[ES_SUMS];
#pragma unroll
  for (int f = 0; f < ES_SUMS; ++f) acc[f] = 0.0;
  double rmax = -HUGE_VAL, rmin = HUGE_VAL;
  const bool vc = a.vold != nullptr;
  // one sample into the sums (values loaded by the caller)
  auto sample = [&](int dn, float lpa, float lpo, float rho, float adv, float vi, float Rf, float vo) {
    const bool live = (dn & 2) == 0;
    const float d = __fsub_rn(lpa, lpo);
    const bool cut = !(adv >= 0.f ? rho <= a.hi : rho >= a.lo);
    float lsq;
    const bool taken = vc && vclip_step(vi, vo, Rf, a.ev, __fsub_rn(vi, Rf), lsq);
    const double ad = (double)adv;
    acc[0] = __dadd_rn(acc[0], live ? 1.0 : 0.0);
    acc[1] = __dadd_rn(acc[1], live && cut ? 1.0 : 0.0);
    acc[2] = __dadd_rn(acc[2], live ? -(double)d : 0.0);
    acc[5] = __dadd_rn(acc[5], live && taken ? 1.0 : 0.0);
    acc[6] = __dadd_rn(acc[6], live ? ad : 0.0);
    acc[7] = __dadd_rn(acc[7], live ? __dmul_rn(ad, ad) : 0.0);
    rmax = live ? fmax(rmax, (double)rho) : rmax;
    rmin = live ? fmin(rmin, (double)rho) : rmin;
  };
  for (int e = j; e < n; e += 256) {
    if (T <= PO_RW) {   // the env's window in registers: two rounds of loads (the log-prob gather needs the action)
      int dn[PO_RW], ac[PO_RW];
      float lpa[PO_RW], lpo[PO_RW], rho[PO_RW], adv[PO_RW], vi[PO_RW], Rf[PO_RW], vo[PO_RW];
#pragma unroll
      for (int k = 0; k < PO_RW; ++k) {
        const int64_t o = (int64_t)min(k, T - 1) * n + e;
        dn[k] = a.dones[o];
        ac[k] = a.act[o];
        lpo[k] = a.lpo[o];
        rho[k] = a.ratio[o];
        adv[k] = a.adv[o];
        vi[k] = a.v[o];
        Rf[k] = a.ret[o];
        vo[k] = vc ? a.vold[o] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < PO_RW; ++k)
        lpa[k] = a.logp[((int64_t)min(k, T - 1) * n + e) * A + min(max(ac[k], 0), A - 1)];
#pragma unroll
      for (int k = 0; k < PO_RW; ++k)
        if (k < T) sample(dn[k], lpa[k], lpo[k], rho[k], adv[k], vi[k], Rf[k], vo[k]);
    } else {
      for (int t = 0; t < T; ++t) {
        const int64_t i = (int64_t)t * n + e;
        sample(a.dones[i], a.logp[i * A + min(max(a.act[i], 0), A - 1)], a.lpo[i], a.ratio[i], a.adv[i], a.v[i],
               a.ret[i], vc ? a.vold[i] : 0.f);
      }
    }
  }
  acc[3] = rmax;
  acc[4] = rmin;
#pragma unroll
  for (int f = 0; f < ES_SUMS; ++f) part[j * ES_SUMS + f] = acc[f];
  __syncthreads();
  if (j < ES_SUMS) tot[j] = ordered_total<ES_SUMS>(part, j, j == 3 ? 1 : j == 4 ? 2 : 0);
  __syncthreads();
  if (j != 0) return;
  double* rec = a.rec;
  int64_t cnt = 0;
  if (a.count != nullptr) {
    cnt = *a.count;
    rec += PPO_AUX_HEAD + (int64_t)((uint64_t)cnt % PPO_LOG) * PPO_STAT_FIELDS;
  }
  const bool any = tot[0] > 0.0;
  rec[0] = a.ctl != nullptr ? (double)a.ctl[CTL_WINDOW] : a.window;
  rec[1] = a.epoch;
  rec[2] = tot[0];
  rec[3] = tot[1];
  rec[4] = tot[2];
  rec[5] = any ? tot[3] : 0.0;
  rec[6] = any ? tot[4] : 0.0;
  rec[7] = tot[5];
  rec[8] = tot[6];
  rec[9] = tot[7];
  if (a.count != nullptr) *a.count = cnt + 1;
}

hipError_t launch_ppo_vold(const uint8_t* dones, const float* v, float* vold, int T, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t S = (int64_t)T * n;
  hipLaunchKernelGGL(ppo_vold_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, dones, v, vold, S);
  return hipGetLastError();
}

hipError_t launch_ppo_normalize_adv(const uint8_t* dones, float* adv, int T, int n, double* moments, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (T < 1 || T > 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppo_normalize_adv_kernel, dim3(1), dim3(256), 0, s, dones, adv, T, n, moments);
  return hipGetLastError();
}

hipError_t launch_ppo_epoch_stats(const PpoLossArgs& p, const int64_t* ctl, double window, double epoch, int64_t* count,
                                  double* rec, hipStream_t s) {
  const ReturnsArgs& r = p.r;
  if (r.n <= 0) return hipSuccess;
  if (r.T < 1 || r.T > 256 || r.A < 1 || r.A > MAXA || p.ratio == nullptr) return hipErrorInvalidValue;
  const EpochStatsArgs a{r.dones, r.v, r.logp, r.act, p.lpo, p.adv, p.ret, p.ratio, p.vold, r.T, r.n, r.A,
                         p.lo, p.hi, p.ev, ctl, window, epoch, count, rec};
  hipLaunchKernelGGL(ppo_epoch_stats_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace arl
