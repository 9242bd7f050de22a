// GradientClipping(40) + RMSpropAsync over one flat parameter buffer.
//
// Reference: a3c_ale.py:224-226 (RMSpropAsync(lr=7e-4, eps=1e-1, alpha=0.99)
// + GradientClipping(40) hook), rmsprop_async.py:23-29 (update_one_cpu) and
// the dormant CuPy kernel rmsprop_async.py:31-38; Chainer's GradientClipping
// (norm = sqrt(sum of per-array squared norms); if 40/norm < 1: g *= 40/norm).
//
// Two launches per update, both HBM-streaming over the padded flat buffer:
//   grad_sqnorm_kernel: per-block partial sum of g^2 (f64 per thread over a
//     grid-stride and across the block) -> partials[block] (the folded form:
//     reduce_conv_bwd_kernel leaves partials of f32 per-thread sums, conv_bwd.hip), so the
//     clip rate needs no host round trip and no extra launch;
//   the update kernel (update_body below, written once; rmsprop_kernel and adam_kernel are its entry points):
//     every block sums the partials in block order (their loads in flight with its first p / state / g
//     loads; a last-arriving block of the norm launch leaving one f64 instead measured 2-4 us slower a
//     window, r4c), then 4 parameters per thread per iteration: g' = clip ? g*f32(rate) : g, the decay
//     step, and the optimizer's rule on one element.  RMSProp's (rms1): ms = ms*alpha; ms += (c*g')*g';
//     p -= (lr*g') / sqrt(ms + eps) -- every op an explicit round-to-nearest f32 op in the reference's
//     order (NumPy f32 semantics, no FMA), so the result is bit-identical to update_one_cpu.  Then the FC
//     weight's split planes are rewritten from the new W, and the launch that ends a window advances it.
// 20 bytes move per parameter (read p, g, ms; write p, ms) + 4 for the norm.
// With arl_net_set_window_stats on, window_stats_kernel (below) runs between the two and records what
// the update is about to apply, through the same device functions (update_lr, partials_sum, clip_scale).
//
// NonbiasWeightDecay(rate) (a3c_ale.py:227-228, nonbias_weight_decay.py:4-28), the hook the reference adds
// after the clip: g += rate * p for every parameter whose name is not a bias, i.e. t = f32(f32(rate) * p),
// g = f32(g + t) (two roundings, NumPy's f32 array ops) on the clipped gradient.  The <DecayArgs> instantiations
// have that step between the clip scale and the rule: p is in registers already, the bias tensors
// come as [begin, end) float ranges in the kernel arguments, so the decay moves no extra byte.  The clip
// norm stays the norm of the gradient before the decay (the reference clips first).  rate == 0 launches
// the <NoDecay> instantiation, without the step (g + f32(0 * p) would also turn a -0 gradient into +0).
//
// Adam (arl_net_set_adam; an extension, off by default): the same body with Adam's rule (adam1) and a second
// state array, behind adam_kernel; 28 bytes per parameter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "arl_internal.hpp"

namespace arl {

__device__ inline double block_sum_f64(double x, double* sh) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sh[w] = x;
  __syncthreads();
  double t = 0.0;
  const int nw = blockDim.x >> 6;
  for (int i = 0; i < nw; ++i) t += sh[i];
  return t;
}

__global__ void __launch_bounds__(256)
grad_sqnorm_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partials) {
  __shared__ double sh[8];
  const int64_t n4 = n >> 2;
  // f64 throughout: an f32 square is exact in f64, so the sum is the f64 norm a host forms (oracle.clip_grads,
  // exact_norm) to about 1e-16, and f32(clip / norm) is the same f32.  With f32 sums per thread the scale could
  // come out one ulp off, which moves a parameter's last bit when the clip is active.
  double acc = 0.0;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = g4[i];
    const double x = v.x, y = v.y, z = v.z, w = v.w;
    acc += (x * x + y * y) + (z * z + w * w);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const double v = g[(n4 << 2) + threadIdx.x];
    acc += v * v;
  }
  const double t = block_sum_f64(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

struct RmsConst {   // (AdvanceArgs is declared in arl_internal.hpp)
  float lr, alpha, one_minus_alpha, eps;
  // optional on-device lr anneal (a3c_ale.py:111-112):
  // lr = (total - global_t - 1) / total * lr0, global_t = (ctl[STEP] + t_max) * n_total
  double lr0;
  int64_t total, n_total, t_max;
  const int64_t* ctl;
  int ctl_idx;              // CTL_STEP, or CTL_STEP_SNAP when this launch also advances
};

// The three pieces below are shared by the update kernels and window_stats_kernel, so that the recorded
// learning rate, squared norm and clip scale are bit for bit the ones the update applies.

// the anneal in f64 (only with the control block and a step budget): update_lr rounds it to f32, Adam's
// bias correction goes on in f64 (adam_lr)
__device__ inline double anneal_f64(const RmsConst& c) {
  const int64_t gt = (c.ctl[c.ctl_idx] + c.t_max) * c.n_total;
  // clamped at 0: the reference stops training once global_t passes the
  // step budget (run_a3c.py:64-68); a replay past it must not ascend
  return ((double)max(c.total - gt - 1, (int64_t)0) / (double)c.total) * c.lr0;
}
// the update's learning rate: c.lr, or the anneal when the control block and a step budget are given
__device__ inline float update_lr(const RmsConst& c) {
  if (c.ctl == nullptr || c.total <= 0) return c.lr;
  return (float)anneal_f64(c);
}

// the squared norm: re-reduce the partials [0, nparts) in block order (4 loads a thread in flight);
// sh: 8 doubles of LDS; every thread of the 256 gets the sum
__device__ inline double partials_sum(const double* __restrict__ norm_sq, int nparts, double* sh) {
  double t = 0.0, v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = norm_sq[min((int)threadIdx.x + 256 * k, nparts - 1)];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((int)threadIdx.x + 256 * k < nparts) t += v[k];
  return block_sum_f64(t, sh);
}

// GradientClipping: does the update scale the gradient, and by which f32 factor (else scale is left alone)
__device__ inline bool clip_scale(double sqnorm, float clip, float& scale) {
  const double norm = sqrt(sqnorm);
  const double rate = (double)clip / norm;
  if (norm > 0.0 && rate < 1.0) {
    scale = (float)rate;
    return true;
  }
  return false;
}

__device__ inline void rms1(float& p, float& ms, float g, const RmsConst& c) {
  ms = __fmul_rn(ms, c.alpha);                                   // ms *= alpha
  ms = __fadd_rn(ms, __fmul_rn(__fmul_rn(c.one_minus_alpha, g), g));   // ms += (1-a)*g*g
  // sqrtf (not __fsqrt_rn = native approx sqrt) is the correctly rounded one under hipcc defaults
  p = __fsub_rn(p, __fdiv_rn(__fmul_rn(c.lr, g), sqrtf(__fadd_rn(ms, c.eps))));  // p -= lr*g/sqrt(ms+eps)
}

// is element e (the first of its float4: tensors start on 64-float boundaries, so a float4 lies in one
// tensor or in the padding after it) inside one of the bias ranges?
__device__ inline bool in_bias(const DecayArgs& wd, int64_t e) {
  bool b = false;
#pragma unroll
  for (int k = 0; k < DECAY_MAX_BIAS; ++k) b |= k < wd.n_bias && e >= wd.begin[k] && e < wd.end[k];
  return b;
}

__device__ inline float decay1(float g, float p, float rate) { return __fadd_rn(g, __fmul_rn(rate, p)); }

// Adam (arl_net_set_adam, arl_adam; an extension, the reference has none): Chainer 1.8.1's optimizers.Adam
// as NumPy evaluates it on f32 arrays, restated in include/asyncrl_hip.h ("Adam").  State m, v (f32); for
// update number t: lr_t = (float)(alpha * sqrt(1 - beta2^t) / (1 - beta1^t)) in f64, then per element
//   m += c1 * (g - m); v += c2 * (g * g - v); p -= (lr_t * m) / (sqrt(v) + eps)
// every op an explicit round-to-nearest f32 op in that order (adam1), c1 = f32(1 - beta1), c2 = f32(1 - beta2).
// adam_kernel is update_body (below) with this rule and a second state array; 28 bytes move per parameter
// (read p, m, v, g; write p, m, v).
// t lives on the device, so that a captured update replays with a fresh bias correction (as the lr anneal
// does): ctl[CTL_ADAM_T] holds the updates made so far.  No workgroup may read a word another workgroup of
// the launch writes (the CTL_STEP / CTL_STEP_SNAP hazard), so the count moves in a launch of its own:
// adam_tick_kernel (one thread, before the update on the same stream) adds 1, and adam_kernel only reads it;
// every workgroup computes lr_t for that t itself in f64 while its first loads are in flight.  (The count moved
// by the update kernel's last workgroup to finish, a ticket on a second ctl slot, measured 19 us a window at C4
// -- 662 agent-scope releases and atomics on one word; the extra launch measures 4.6 us: DESIGN.md.)
// beta^t is binary exponentiation in explicit f64 multiplies (exact at t = 1, a relative error below 2 log2(t)
// ulp, which leaves the f32 lr_t within 1 ulp of Python's): two pow calls in every workgroup cost 2.3 us.
struct AdamConst {
  RmsConst lr;            // lr0 = Adam's alpha with update_lr's anneal arguments (lr.alpha / one_minus_alpha / eps unused)
  float c1, c2, eps;
  double beta1, beta2;
  const int64_t* tctl;    // the control block: t = tctl[CTL_ADAM_T]; null: lr_t below is the host's for its t
  float lr_t;
};

// the bias-corrected step size of update t (>= 1), shared by adam_kernel and adam_tick_kernel's record
__device__ inline float adam_lr(const AdamConst& a, int64_t t) {
  const double alpha = (a.lr.ctl == nullptr || a.lr.total <= 0) ? a.lr.lr0 : anneal_f64(a.lr);
  double r1 = 1.0, r2 = 1.0, b1 = a.beta1, b2 = a.beta2;   // beta1^t, beta2^t
  for (int64_t k = t; k > 0; k >>= 1) {
    if (k & 1) {
      r1 = __dmul_rn(r1, b1);
      r2 = __dmul_rn(r2, b2);
    }
    b1 = __dmul_rn(b1, b1);
    b2 = __dmul_rn(b2, b2);
  }
  const double fix1 = 1.0 - r1, fix2 = 1.0 - r2;
  return (float)(alpha * sqrt(fix2) / fix1);
}

__device__ inline void adam1(float& p, float& m, float& v, float g, const AdamConst& a, float lr) {
  m = __fadd_rn(m, __fmul_rn(a.c1, __fsub_rn(g, m)));                    // m += (1-b1)*(g-m)
  v = __fadd_rn(v, __fmul_rn(a.c2, __fsub_rn(__fmul_rn(g, g), v)));      // v += (1-b2)*(g*g-v)
  p = __fsub_rn(p, __fdiv_rn(__fmul_rn(lr, m), __fadd_rn(sqrtf(v), a.eps)));   // p -= lr_t*m/(sqrt(v)+eps)
}

// The per-element rules of update_body: the constants, the set-up every thread runs once while its first
// loads are in flight, and one element's step on (p, s1, s2, g).  STATES: the state arrays beside p.
struct RmsRule {
  static constexpr int STATES = 1;   // ms
  RmsConst c;
  __device__ void setup() { c.lr = update_lr(c); }
  __device__ void step(float& p, float& ms, float&, float g) const { rms1(p, ms, g, c); }
};
struct AdamRule {
  static constexpr int STATES = 2;   // m, v
  AdamConst a;
  float lr;
  // (adam_tick_kernel has counted this update; nothing in this launch writes the word)
  __device__ void setup() { lr = a.tctl != nullptr ? adam_lr(a, a.tctl[CTL_ADAM_T]) : a.lr_t; }
  __device__ void step(float& p, float& m, float& v, float g) const { adam1(p, m, v, g, a, lr); }
};

struct NoDecay {};   // the decay-free instantiations' (empty) last kernel argument

// The fused update, written once for both optimizers: one float4 of p / s1 (/ s2) / g per thread and pass,
// the first pass's loads in flight with the norm's; then the tail, then the window advance.
// Decay = DecayArgs: the NonbiasWeightDecay step on every element outside wd's bias ranges (NoDecay: none).
// s2 is read and written only by a rule with two state arrays (compiled out otherwise).
template <class Rule, class Decay>
__device__ __forceinline__ void update_body(Rule& rule, float* __restrict__ p, float* __restrict__ s1,
                                            float* __restrict__ s2, const float* __restrict__ g, int64_t n,
                                            const double* __restrict__ norm_sq, int nparts, float clip,
                                            const AdvanceArgs& adv, const Decay& wd, int64_t i0, int64_t gsz) {
  constexpr bool WD = std::is_same<Decay, DecayArgs>::value;
  constexpr bool S2 = Rule::STATES == 2;
  __shared__ double sh[8];
  const int64_t n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* a4 = reinterpret_cast<float4*>(s1);
  float4* b4 = reinterpret_cast<float4*>(s2);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  // the first pass's float4s are in flight with the squared norm's loads (n4 == 0: none; past the end: a
  // clamped duplicate, never stored)
  float4 pv, av, bv, gv;
  bool bias0 = false;   // WD: the first pass's float4 lies in a bias tensor
  if (n4 > 0) {
    const int64_t i = min(i0, n4 - 1);
    pv = p4[i];
    av = a4[i];
    if constexpr (S2) bv = b4[i];
    gv = g4[i];
    // decided here so that the range table's kernel-argument loads (two cache lines no other argument
    // shares) are issued with the first arguments': read first before the loop, the decay arm cost
    // 1.1 us over the decay-free kernel's 7.8 us at C4, this way 0.5 us
    if constexpr (WD) bias0 = in_bias(wd, 4 * i);
  }
  rule.setup();
  float scale = 1.f;
  bool do_clip = false;
  if (norm_sq != nullptr) do_clip = clip_scale(partials_sum(norm_sq, nparts, sh), clip, scale);
  for (int64_t ib = i0; ib < n4; ib += gsz) {
    if (ib != i0) {
      pv = p4[ib];
      av = a4[ib];
      if constexpr (S2) bv = b4[ib];
      gv = g4[ib];
    }
    if (do_clip) {
      gv.x = __fmul_rn(gv.x, scale); gv.y = __fmul_rn(gv.y, scale);
      gv.z = __fmul_rn(gv.z, scale); gv.w = __fmul_rn(gv.w, scale);
    }
    if constexpr (WD) {   // after the clip, as Chainer runs the two hooks
      if (!(ib == i0 ? bias0 : in_bias(wd, 4 * ib))) {
        gv.x = decay1(gv.x, pv.x, wd.rate); gv.y = decay1(gv.y, pv.y, wd.rate);
        gv.z = decay1(gv.z, pv.z, wd.rate); gv.w = decay1(gv.w, pv.w, wd.rate);
      }
    }
    rule.step(pv.x, av.x, bv.x, gv.x);
    rule.step(pv.y, av.y, bv.y, gv.y);
    rule.step(pv.z, av.z, bv.z, gv.z);
    rule.step(pv.w, av.w, bv.w, gv.w);
    p4[ib] = pv;
    a4[ib] = av;
    if constexpr (S2) b4[ib] = bv;
    const int64_t e = 4 * ib - adv.fc_w0;   // the FC weight's split planes follow their f32 W (fc.hip)
    if (adv.fc_planes != nullptr && e >= 0 && e < (int64_t)HID * A2) fc_planes_store(adv.fc_planes, (int)e, pv);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t j = (n4 << 2) + threadIdx.x;
    float gt = g[j];
    if (do_clip) gt = __fmul_rn(gt, scale);
    float pt = p[j], at = s1[j], bt = 0.f;
    if constexpr (S2) bt = s2[j];
    if constexpr (WD)
      if (!in_bias(wd, j)) gt = decay1(gt, pt, wd.rate);
    rule.step(pt, at, bt, gt);
    p[j] = pt;
    s1[j] = at;
    if constexpr (S2) s2[j] = bt;
  }
  if (adv.ctl == nullptr) return;   // (no window advance)
  for (int64_t i = i0; i < adv.n; i += gsz) adv.reset[i] = adv.reset[(int64_t)adv.T * adv.n + i];
  if (adv.hbuf != nullptr)
    for (int64_t i = i0; i < (int64_t)adv.n * HID; i += gsz) {
      adv.hbuf[i] = adv.hbuf[(int64_t)adv.T * adv.n * HID + i];
      adv.cbuf[i] = adv.cbuf[(int64_t)adv.T * adv.n * HID + i];
    }
  if (i0 == 0) {
    adv.ctl[CTL_STEP] += adv.T;
    adv.ctl[CTL_WINDOW] += 1;
  }
}

// The two entry points (profiles, the timeline scripts and bench.py know the update by these names).  They
// compute i0, this thread's first float4, and gsz, the launch's thread count: read in a __global__ function
// the workgroup size is a scalar kernel-argument load, read inside update_body it became a vector load.
template <class Decay>
__global__ void __launch_bounds__(256)
rmsprop_kernel(float* __restrict__ p, float* __restrict__ ms, const float* __restrict__ g, int64_t n, RmsConst c,
               const double* __restrict__ norm_sq, int nparts, float clip, AdvanceArgs adv, Decay wd) {
  RmsRule rule{c};
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (int64_t)gridDim.x * blockDim.x;
  update_body(rule, p, ms, nullptr, g, n, norm_sq, nparts, clip, adv, wd, i0, gsz);
}

template <class Decay>
__global__ void __launch_bounds__(256)
adam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g, int64_t n,
            AdamConst a, const double* __restrict__ norm_sq, int nparts, float clip, AdvanceArgs adv, Decay wd) {
  AdamRule rule{a, 0.f};
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (int64_t)gridDim.x * blockDim.x;
  update_body(rule, p, m, v, g, n, norm_sq, nparts, clip, adv, wd, i0, gsz);
}

// One thread, before adam_kernel on its stream: count the update (the only writer of ctl[CTL_ADAM_T] besides
// arl_net_set_adam_t and arl_net_reset).  With window statistics on (log non-null; window_stats_kernel ran just
// before and left count at its record's index + 1) field 16 of that record becomes this update's Adam lr_t.
__global__ void adam_tick_kernel(int64_t* ctl, AdamConst a, double* __restrict__ log,
                                 const int64_t* __restrict__ count) {
  const int64_t t = ctl[CTL_ADAM_T] + 1;
  ctl[CTL_ADAM_T] = t;
  if (log == nullptr) return;
  const int64_t cnt = *count;
  if (cnt < 1) return;
  log[(int64_t)((uint64_t)(cnt - 1) % WINDOW_LOG) * WINDOW_STAT_FIELDS + 16] = (double)adam_lr(a, t);
}

__global__ void ctl_write_kernel(int64_t* ctl, int idx, int64_t value) { ctl[idx] = value; }

// Per-window training statistics (arl_net_set_window_stats; semantics in include/asyncrl_hip.h, "window
// statistics"): one record per update, launched by net_optimize between the norm's partials and the update
// kernel.  One workgroup of 256: thread j owns envs j, j + 256, ...; per env one reverse scan of the
// learner's return recurrence (return_step) gives (float)R_t, then t ascends over the steps; the twelve
// f64 partial sums (fields 2..13) go through LDS, and lane f of the first wave adds partials 1..255 of
// field 2 + f to partial 0 in order (twelve lanes, one instruction stream: one thread walking all twelve
// chains issued twelve times the f64 adds and measured 10 us longer).  The lr, the squared norm and the
// clip scale come from rmsprop_kernel's own device functions on the arguments the update gets.
// Windows up to WS_RW steps keep an env's rewards / dones / v / entropy and its R_t in registers (static
// indices, clamped offsets, as returns_load); longer ones loop over memory with the R_t in LDS.
// Dynamic LDS, reused in turn: block_sum_f64's scratch, the R_t columns (T x 256 f32, T > WS_RW), the
// partials (256 x WS_SUMS f64).
constexpr int WS_SUMS = 12, WS_RW = 8;
static_assert(2 + WS_SUMS + 3 == WINDOW_STAT_FIELDS, "window record layout");

// one env's window in registers (T <= WS_RW): static indices, clamped offsets, as returns_load (policy.hip)
struct WsEnv {
  float rw[WS_RW], vv[WS_RW], en[WS_RW], vboot, l0, l1;
  int dn[WS_RW];
};
__device__ inline void ws_load(const WindowStatsArgs& w, int e, WsEnv& x) {
#pragma unroll
  for (int k = 0; k < WS_RW; ++k) {
    const int64_t o = (int64_t)min(k, w.T - 1) * w.n + e;
    x.rw[k] = w.rewards[o];
    x.dn[k] = w.dones[o];
    x.vv[k] = w.v[o];
    x.en[k] = w.entropy[o];
  }
  x.vboot = w.v[(int64_t)w.T * w.n + e];
  x.l0 = w.loss[2 * e];
  x.l1 = w.loss[2 * e + 1];
}

// the per-env terms: pi_loss, v_loss
__device__ inline void ws_env(double* acc, float pi_loss, float v_loss) {
  acc[3] = __dadd_rn(acc[3], (double)pi_loss);
  acc[4] = __dadd_rn(acc[4], (double)v_loss);
}

// One sample (t, e) into the sums, without a branch.  A sample past a truncated window's end (dones bit
// 1) adds +0.0 to every sum, which leaves its bits alone: the sums start at +0.0, and a round-to-nearest
// sum that started there is never -0.0, the only value x + 0.0 would change.
// G (the kernel's GAE form, below): the advantage is af, the GAE one the learner used, instead of f32(rf - vi).
template <bool G>
__device__ inline void ws_sample(double* acc, int d, float r, float vi, float ent, float rf, float af,
                                 int clip_reward) {
  const bool live = (d & 2) == 0;
  const double vd = (double)vi, rd = (double)rf, ad = G ? (double)af : (double)__fsub_rn(rf, vi);
  const double x[WS_SUMS] = {1.0, (d & 1) ? 1.0 : 0.0, clip_reward_f64(r, clip_reward), 0.0, 0.0, (double)ent,
                             vd, __dmul_rn(vd, vd), rd, __dmul_rn(rd, rd), ad, __dmul_rn(ad, ad)};
#pragma unroll
  for (int f = 0; f < WS_SUMS; ++f)
    if (f != 3 && f != 4) acc[f] = __dadd_rn(acc[f], live ? x[f] : 0.0);
}

// GAE form (G, compile time; the host picks it for lambda != 1): adv_sum / adv_sumsq are the sums of the GAE
// advantage, the f32 the learner used, from the same gae_step on the same values.  The register path scans it
// beside R.  The memory path has one LDS column per thread, so after an env's samples are summed with a zero
// advantage (+0.0 leaves the two sums' bits alone, as above) a second reverse scan puts the advantages in the
// column and a second ascent adds them: each sum still sees its terms in the order t ascending, env by env.
struct WindowStatsArgsGae : WindowStatsArgs {
  double gl;   // gamma * lambda
};
template <bool G>
using WindowStatsArgsT = std::conditional_t<G, WindowStatsArgsGae, WindowStatsArgs>;
template <bool G = false>
__global__ void __launch_bounds__(256)
window_stats_kernel(WindowStatsArgsT<G> w, RmsConst c, const double* __restrict__ norm_sq, int nparts, float clip) {
  extern __shared__ double dyn[];
  const int j = threadIdx.x, T = w.T, n = w.n;
  // what only the record's writer needs, loaded first so that it is there by the end
  const int64_t cnt = *w.count, window = w.ctl[CTL_WINDOW], step = w.ctl[c.ctl_idx];
  const double sqnorm = partials_sum(norm_sq, nparts, dyn);
  float scale = 1.f;
  if (clip > 0.f) clip_scale(sqnorm, clip, scale);   // (clip <= 0: the update gets no partials and does not clip)
  const float lr = update_lr(c);
  __syncthreads();   // block_sum_f64's scratch is read: the R_t columns may overwrite it
  double acc[WS_SUMS];
#pragma unroll
  for (int f = 0; f < WS_SUMS; ++f) acc[f] = 0.0;
  if (T <= WS_RW) {   // an env's window in registers, the next env's loads in flight while this one is summed
    WsEnv cur, nxt;
    if (j < n) ws_load(w, j, cur);
    for (int e = j; e < n; e += 256) {
      ws_load(w, e + 256 < n ? e + 256 : e, nxt);   // (past the last env: this one again, unused)
      float rf[WS_RW], af[WS_RW] = {};
      double R = (double)cur.vboot;
      double Gl = 0.0;
#pragma unroll
      for (int k = WS_RW - 1; k >= 0; --k)
        if (k < T) {
          R = return_step(R, cur.dn[k], cur.rw[k], w.gamma, w.clip_reward);
          rf[k] = (float)R;
          if constexpr (G) {
            Gl = gae_step(Gl, cur.dn[k], cur.rw[k], cur.vv[k], k == T - 1 ? cur.vboot : cur.vv[k < WS_RW - 1 ? k + 1 : k],
                          w.gamma, w.gl, w.clip_reward);
            af[k] = (float)Gl;
          }
        }
      ws_env(acc, cur.l0, cur.l1);
#pragma unroll
      for (int k = 0; k < WS_RW; ++k)
        if (k < T) ws_sample<G>(acc, cur.dn[k], cur.rw[k], cur.vv[k], cur.en[k], rf[k], af[k], w.clip_reward);
      cur = nxt;
    }
  } else {            // longer windows: loops over memory, the R_t of the reverse scan in the thread's LDS column
    float* Rf = reinterpret_cast<float*>(dyn);
    for (int e = j; e < n; e += 256) {
      double R = (double)w.v[(int64_t)T * n + e];
      for (int t = T - 1; t >= 0; --t) {
        const int64_t i = (int64_t)t * n + e;
        R = return_step(R, w.dones[i], w.rewards[i], w.gamma, w.clip_reward);
        Rf[t * 256 + j] = (float)R;
      }
      ws_env(acc, w.loss[2 * e], w.loss[2 * e + 1]);
      for (int t = 0; t < T; ++t) {
        const int64_t i = (int64_t)t * n + e;
        ws_sample<G>(acc, w.dones[i], w.rewards[i], w.v[i], w.entropy[i], Rf[t * 256 + j], 0.f, w.clip_reward);
      }
      if constexpr (G) {
        const float vboot = w.v[(int64_t)T * n + e];
        double Gl = 0.0;
        for (int t = T - 1; t >= 0; --t) {
          const int64_t i = (int64_t)t * n + e;
          Gl = gae_step(Gl, w.dones[i], w.rewards[i], w.v[i], t == T - 1 ? vboot : w.v[i + n], w.gamma, w.gl,
                        w.clip_reward);
          Rf[t * 256 + j] = (float)Gl;
        }
        for (int t = 0; t < T; ++t) {
          const double ad = (w.dones[(int64_t)t * n + e] & 2) ? 0.0 : (double)Rf[t * 256 + j];
          acc[10] = __dadd_rn(acc[10], ad);
          acc[11] = __dadd_rn(acc[11], __dmul_rn(ad, ad));
        }
      }
    }
  }
  __syncthreads();   // every R_t column is read: the partials may overwrite them
#pragma unroll
  for (int f = 0; f < WS_SUMS; ++f) dyn[j * WS_SUMS + f] = acc[f];
  __syncthreads();
  if (j >= WS_SUMS) return;
  // lane f of the first wave combines field 2 + f: partial 0, then 1 .. 255 in order
  // (the LDS reads of 32 partials at a time are in flight ahead of the chain of adds that waits for them)
  double sum = dyn[j];
  for (int q0 = 1; q0 < 256; q0 += 32) {
    double x[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) x[u] = dyn[min(q0 + u, 255) * WS_SUMS + j];
#pragma unroll
    for (int u = 0; u < 32; ++u)
      if (q0 + u < 256) sum = __dadd_rn(sum, x[u]);
  }
  double* rec = w.log + (int64_t)((uint64_t)cnt % WINDOW_LOG) * WINDOW_STAT_FIELDS;
  rec[2 + j] = sum;
  if (j != 0) return;
  rec[0] = (double)window;
  rec[1] = (double)step;
  rec[14] = sqnorm;
  rec[15] = (double)scale;
  rec[16] = (double)lr;
  *w.count = cnt + 1;
}

static int stream_blocks(int64_t n) {
  int64_t b = (n / 4 + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

hipError_t launch_grad_sqnorm(const float* g, int64_t n, double* partials, int blocks, hipStream_t s) {
  if (blocks < 1 || blocks > NORM_MAX_PARTS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(blocks), dim3(256), 0, s, g, n, partials);
  return hipGetLastError();
}

// each Python-float hyperparameter meets the f32 arrays as f32(value); the lr reads the learner's step
// snapshot when the launch also ends the window
static RmsConst rms_const(double lr, double alpha, double eps, const UpdateArgs& u) {
  RmsConst c;
  c.lr = (float)lr;
  c.alpha = (float)alpha;
  c.one_minus_alpha = (float)(1.0 - alpha);   // (1 - self.alpha) in Python double, then f32
  c.eps = (float)eps;
  c.lr0 = lr;
  c.total = u.total_steps;
  c.n_total = u.n_total;
  c.t_max = u.t_max;
  c.ctl = u.lr_ctl;
  c.ctl_idx = u.adv != nullptr && u.adv->ctl != nullptr ? CTL_STEP_SNAP : CTL_STEP;
  return c;
}

hipError_t launch_window_stats(const WindowStatsArgs& w, double lr, const UpdateArgs& u, hipStream_t s, double lambda) {
  if (w.T < 1 || w.T > 64 || w.n < 1) return hipErrorInvalidValue;   // (the R_t columns: at most 64 KB of LDS)
  if (u.norm_sq == nullptr || u.nparts < 1 || u.nparts > NORM_MAX_PARTS) return hipErrorInvalidValue;
  const RmsConst c = rms_const(lr, 0.0, 0.0, u);   // alpha / eps do not enter the record
  const size_t lds = std::max(w.T > WS_RW ? (size_t)w.T * 256 * sizeof(float) : 0, (size_t)WS_SUMS * 256 * sizeof(double));
  if (gae_on(lambda)) {
    WindowStatsArgsGae wg;
    static_cast<WindowStatsArgs&>(wg) = w;
    wg.gl = w.gamma * lambda;
    hipLaunchKernelGGL(window_stats_kernel<true>, dim3(1), dim3(256), lds, s, wg, c, u.norm_sq, u.nparts, u.clip);
  } else {
    hipLaunchKernelGGL(window_stats_kernel<false>, dim3(1), dim3(256), lds, s, w, c, u.norm_sq, u.nparts, u.clip);
  }
  return hipGetLastError();
}

// What launch_rmsprop and launch_adam share: the checks, the empty array, and the choice of the instantiation.
// launch(adv, wd) issues the optimizer's kernel(s) for wd, a DecayArgs or NoDecay{}, and returns their status.
template <class Launch>
static hipError_t launch_update(int64_t n, const UpdateArgs& u, Launch&& launch) {
  if (u.wd != nullptr && (u.wd->n_bias < 0 || u.wd->n_bias > DECAY_MAX_BIAS)) return hipErrorInvalidValue;
  if (u.norm_sq != nullptr && (u.nparts < 1 || u.nparts > NORM_MAX_PARTS)) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  AdvanceArgs adv{};
  if (u.adv != nullptr) adv = *u.adv;
  if (u.wd != nullptr && u.wd->rate != 0.f) return launch(adv, *u.wd);
  return launch(adv, NoDecay{});
}

hipError_t launch_rmsprop(float* p, float* ms, const float* g, int64_t n, double lr, double alpha, double eps,
                          const UpdateArgs& u, hipStream_t s) {
  const RmsConst c = rms_const(lr, alpha, eps, u);
  return launch_update(n, u, [&](const AdvanceArgs& adv, auto wd) {
    hipLaunchKernelGGL(rmsprop_kernel<decltype(wd)>, dim3(stream_blocks(n)), dim3(256), 0, s, p, ms, g, n, c, u.norm_sq,
                       u.nparts, u.clip, adv, wd);
    return hipGetLastError();
  });
}

// ad.tctl null: lr_t for the host's ad.t from the host's libm, in Python's order (bit-identical to Adam.lr)
static AdamConst adam_const(double lr, double eps, const AdamArgs& ad, const UpdateArgs& u) {
  AdamConst a;
  a.lr = rms_const(lr, 0.0, 0.0, u);
  a.c1 = (float)(1.0 - ad.beta1);
  a.c2 = (float)(1.0 - ad.beta2);
  a.eps = (float)eps;
  a.beta1 = ad.beta1;
  a.beta2 = ad.beta2;
  a.tctl = ad.tctl;
  a.lr_t = 0.f;
  if (ad.tctl == nullptr) {
    const double fix1 = 1.0 - std::pow(ad.beta1, (double)ad.t), fix2 = 1.0 - std::pow(ad.beta2, (double)ad.t);
    a.lr_t = (float)(lr * std::sqrt(fix2) / fix1);
  }
  return a;
}

hipError_t launch_adam(float* p, float* m, float* v, const float* g, int64_t n, double lr, double eps,
                       const AdamArgs& ad, const UpdateArgs& u, hipStream_t s) {
  if (ad.tctl == nullptr && ad.t < 1) return hipErrorInvalidValue;
  return launch_update(n, u, [&](const AdvanceArgs& adv, auto wd) {
    const AdamConst a = adam_const(lr, eps, ad, u);
    if (ad.tctl != nullptr) {   // count the update (and, with a window record, note its lr_t) ahead of the kernel
      hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, s, ad.tctl, a, ad.stats_log, ad.stats_count);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(adam_kernel<decltype(wd)>, dim3(stream_blocks(n)), dim3(256), 0, s, p, m, v, g, n, a, u.norm_sq,
                       u.nparts, u.clip, adv, wd);
    return hipGetLastError();
  });
}

hipError_t launch_ctl_write(int64_t* ctl, int idx, int64_t value, hipStream_t s) {
  if (idx < 0 || idx >= CTL_SIZE) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctl_write_kernel, dim3(1), dim3(1), 0, s, ctl, idx, value);
  return hipGetLastError();
}

// HBM stream-copy peak (measurement only; SURVEY 8(d) "also report vs the
// measured stream-copy peak").  Two forms, the bench keeps the faster:
//   mode 0: grid-stride, four 16-byte loads in flight per lane before the
//           first store (addresses one grid apart);
//   mode 1: each workgroup copies contiguous 64 KB blocks (block-stride over
//           the buffer), every lane 4 consecutive-in-wave 16-byte loads in
//           flight, non-temporal loads / stores (a once-read stream).
__global__ void __launch_bounds__(256)
stream_copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst, int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const float4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    dst[i] = a;
    dst[i + stride] = b;
    dst[i + 2 * stride] = c;
    dst[i + 3 * stride] = d;
  }
  for (; i < n4; i += stride) dst[i] = src[i];
}

typedef float cp_f32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256)
stream_copy_blocks_kernel(const cp_f32x4* __restrict__ src, cp_f32x4* __restrict__ dst, int64_t n4) {
  constexpr int U = 16;                         // 16-byte vectors per lane per block: 256 x 16 x 16 B = 64 KB
  const int64_t nblk = n4 / (256 * U);
  for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    const cp_f32x4* s = src + b * (256 * U) + threadIdx.x;
    cp_f32x4* d = dst + b * (256 * U) + threadIdx.x;
    cp_f32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(s + 256 * u);
#pragma unroll
    for (int u = 0; u < U; ++u) __builtin_nontemporal_store(v[u], d + 256 * u);
  }
  for (int64_t i = nblk * (256 * U) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
    dst[i] = src[i];
}

//   mode 2 / 3: a one-shot grid, one 16-byte load and store per lane (bytes / 4 KB workgroups of 256);
//           mode 3 with non-temporal loads / stores -- the fastest form on MI355X (scripts/copy_sweep.hip:
//           6.47 TB/s non-temporal, 6.25 plain at 1 GiB; 8 loads a lane in flight ran 4.3 TB/s)
template <bool NT>
__global__ void __launch_bounds__(256)
stream_copy_chunk_kernel(const cp_f32x4* __restrict__ src, cp_f32x4* __restrict__ dst, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  if (NT) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
  else dst[i] = src[i];
}

hipError_t launch_stream_copy(const void* src, void* dst, int64_t bytes, int blocks, int mode, hipStream_t s) {
  const float4* a = reinterpret_cast<const float4*>(src);
  float4* b = reinterpret_cast<float4*>(dst);
  if (mode >= 2) {
    const int64_t grid = (bytes / 16 + 255) / 256;
    if (grid > 0x7fffffff) return hipErrorInvalidValue;
    if (mode == 3)
      hipLaunchKernelGGL(stream_copy_chunk_kernel<true>, dim3((unsigned)grid), dim3(256), 0, s,
                         reinterpret_cast<const cp_f32x4*>(src), reinterpret_cast<cp_f32x4*>(dst), bytes / 16);
    else
      hipLaunchKernelGGL(stream_copy_chunk_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s,
                         reinterpret_cast<const cp_f32x4*>(src), reinterpret_cast<cp_f32x4*>(dst), bytes / 16);
    return hipGetLastError();
  }
  if (mode == 1)
    hipLaunchKernelGGL(stream_copy_blocks_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const cp_f32x4*>(src),
                       reinterpret_cast<cp_f32x4*>(dst), bytes / 16);
  else hipLaunchKernelGGL(stream_copy_kernel, dim3(blocks), dim3(256), 0, s, a, b, bytes / 16);
  return hipGetLastError();
}

}  // namespace arl
