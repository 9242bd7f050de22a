/*
 * asyncrl_hip.h -- C ABI of libasyncrl_hip.so, the MI355X (gfx950) hot path of
 * batched A3C (phi + forward + sample + n-step update) for PeerM/async-rl.
 *
 * Every entry point takes plain device pointers, sizes and a hipStream_t
 * (passed as void*; NULL = the default stream).  Calls are asynchronous on
 * that stream, never allocate, never synchronise, and are graph-capturable.
 * Return value: 0 (ARL_OK) or an error code; arl_last_error() describes the
 * last failure of the calling thread.
 *
 * Each function names the reference interface it replaces (file:line in
 * PeerM/async-rl @ v0).  INTEGRATION.md shows the ctypes binding a maintainer
 * adds on the reference side.
 */
#ifndef ASYNCRL_HIP_H
#define ASYNCRL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARL_ABI_VERSION 4

#define ARL_OK 0
#define ARL_EINVAL 1   /* bad argument (shape, pointer, alignment) */
#define ARL_EHIP 2     /* HIP runtime error (launch failure) */
#define ARL_ESTATE 3   /* handle not bound / wrong arch for this call */

#define ARL_ARCH_FF 0     /* A3CFF   (a3c_ale.py:28-40) */
#define ARL_ARCH_LSTM 1   /* A3CLSTM (a3c_ale.py:43-70) */
#define ARL_ARCH_FF_NATURE 2  /* A3CFF with NatureDQNHead (dqn_head.py:6-28) instead of NIPSDQNHead */
#define ARL_ARCH_RGB 16   /* flag for FF / LSTM: the ViZDoom models of train_a3c_doom.py:25-63
                             (NIPSDQNHead(n_input_channels=3) on one RGB screen, no frame stack);
                             observations come through arl_observe_rgb */
#define ARL_ARCH_STACK 32 /* flag for FF / LSTM: observations are whole 4-screen stacks (ale.py:91-94
                             ALE.state, as A3C.act receives them, a3c.py:67,72-73), one per ring
                             slot; they come through arl_observe_stack */
#define ARL_ARCH_STATES 64 /* flag for FF / LSTM: observations are float32 (4, 84, 84) states -- the
                              output of A3C's phi plugin (a3c.py:34,50,73; identity by default) --
                              one per ring slot; they come through arl_observe_states */

#define ARL_RESIZE_SCALAR 0  /* OpenCV FixedPtCast vertical pass (canonical) */
#define ARL_RESIZE_SIMD 1    /* OpenCV VResizeLinearVec_32s8u (mulhi) pass */
#define ARL_RESIZE_CROP 2    /* flag: ale.py:73-82 crop_or_scale='crop' (84x110 resize, rows 18..101) */

int arl_abi_version(void);
const char* arl_last_error(void);

/* ------------------------------------------------------------------ phi */

/* ale.py:59-89 ALE.current_screen (crop_or_scale='scale'), batched.
 * rgb_cur, rgb_prev: (n, 210, 160, 3) uint8, 16-byte aligned.
 * out: (n, 84, 84) uint8.  max -> fp64 luminance -> uint8 -> 84x84 resize. */
int arl_current_screen(const uint8_t* rgb_cur, const uint8_t* rgb_prev, uint8_t* out, int64_t n,
                       int resize_mode, void* stream);

/* ale.py:62-69 alone: np.maximum of the two frames + float64 luminance +
 * astype(uint8), for npix pixels (rgb: (npix, 3) uint8) -> gray (npix,). */
int arl_max_luminance(const uint8_t* rgb_cur, const uint8_t* rgb_prev, uint8_t* gray, int64_t npix,
                      void* stream);

/* ale.py:135 + ale.py:155-158 (frame-stack deque), batched, materialised.
 * rgb_pairs: (n, 2, 210, 160, 3) uint8 (frame 4 and frame 3 of the skip);
 * prev_stack, out_stack: (n, 4, 84, 84) uint8, must not alias;
 * reset: (n,) uint8 or NULL -- 1 = episode start: [0, 0, 0, new]. */
int arl_phi_stack(const uint8_t* rgb_pairs, const uint8_t* prev_stack, const uint8_t* reset,
                  uint8_t* out_stack, int64_t n, int resize_mode, void* stream);

/* dqn_phi.py:4-17 dqn_phi, batched: (n, 4, 84, 84) uint8 -> float32 / 255. */
int arl_dqn_phi(const uint8_t* stack_u8, float* out, int64_t n, void* stream);

/* train_a3c_doom.py:21-23 phi, batched: cv2.resize(image_buffer, (84, 84))
 * per channel (INTER_LINEAR fixed point, resize_mode as above, no crop),
 * transpose(2, 0, 1), float32 / 255.  imgs: (n, H, W, 3) uint8 RGB24
 * (doom_env.py:47), 16-byte aligned, W % 16 == 0, W <= 2048; out: (n, 3,
 * 84, 84) f32. */
int arl_rgb_phi(const uint8_t* imgs, int64_t n, int H, int W, float* out, int resize_mode, void* stream);

/* ------------------------------------------------------------------ net */
typedef struct arl_net arl_net;

/* Describe an A3C model + lockstep actor-learner over n_envs envs and
 * t_max-step windows (a3c.py:33-61 A3C.__init__, a3c_ale.py:219-229).
 * env_offset: global id of this rank's env 0 (RNG stream); seed: Philox key. */
int arl_net_create(arl_net** out, int arch, int n_actions, int n_envs, int t_max, int env_offset,
                   uint64_t seed);
void arl_net_destroy(arl_net* net);

/* Flat parameter layout (Chainer namedparams order, each tensor 64-float
 * aligned).  The same layout is used for params, grads and RMSProp ms. */
int64_t arl_net_param_floats(const arl_net* net);
int arl_net_param_count(const arl_net* net);
int arl_net_param_info(const arl_net* net, int idx, int64_t* offset, int64_t* numel, char* name, int name_cap);

/* Caller-owned device workspace (activations, frame ring, rollout buffers). */
int64_t arl_net_workspace_bytes(const arl_net* net);
int arl_net_buffer(const arl_net* net, const char* name, int64_t* offset, int64_t* bytes);

/* Bind caller-owned device memory: params/grads/ms (param_floats f32 each,
 * 16-byte aligned; grads must be zeroed once by the caller) and workspace. */
int arl_net_bind(arl_net* net, float* params, float* grads, float* ms, void* workspace);

/* Parameter generations (ABI 4).  The FC forward reads the FC weight as bf16
 * split planes derived from the bound params; every arl_optimize* /
 * arl_run_window update keeps them current.  Any OTHER writer of the bound
 * params -- a checkpoint load, a copy from another model (copy_param.py,
 * serializers), arl_rmsprop on the params -- must bump the generation with
 * arl_net_params_changed; arl_net_bind bumps it too.  A forward over all envs
 * rebuilds stale planes on its own stream; arl_net_prepare rebuilds them on a
 * given stream (call it on the stream env-range chains fork from, and before
 * replaying a captured window after such a write: a replay has no rebuild);
 * arl_act_envs over a proper env range refuses stale planes with ARL_ESTATE.
 * arl_net_param_generation reads both generations (planes current iff equal).
 * No reference counterpart: the reference's forward reads the f32 params. */
int arl_net_params_changed(arl_net* net);
int arl_net_prepare(arl_net* net, void* stream);
int arl_net_param_generation(const arl_net* net, uint64_t* param_gen, uint64_t* planes_gen);

/* Reset the control block (step counters) and the frame ring; call once
 * before the first observation (async). */
int arl_net_reset(arl_net* net, void* stream);

/* Input pools (no reference counterpart: the reference's actors hand one frame
 * at a time to A3C.act).  The observation calls below read entry (control-block
 * step + t) % pool_len of caller-owned device pools, and a pointer carries no
 * extent, so the net keeps the extent of every pool it may read: register each
 * pool with its size in bytes before observing from it (kind ARL_POOL_FRAMES:
 * the frame-pair / image / stack / state pool; ARL_POOL_REWARDS; ARL_POOL_DONES;
 * up to 8 pools per kind, a later registration of the same base replaces the
 * earlier one, bytes == 0 removes it).  An observation whose non-NULL pool is
 * not inside a registered one, or whose pool_len entries of n_envs rows do not
 * fit before its end, fails with ARL_EINVAL before anything is launched. */
#define ARL_POOL_FRAMES 0
#define ARL_POOL_REWARDS 1
#define ARL_POOL_DONES 2
int arl_net_set_pool(arl_net* net, int kind, const void* pool, int64_t bytes);

/* Observation at window step t (0..t_max): phi of the env's frame pair into
 * the ring + stack bookkeeping + ingest of the reward/done that came with it
 * (a3c.py:69-75; ale.py:111-139).  Pools hold pool_len steps; the step used
 * is (control-block step + t) % pool_len.  pair_pool: (pool_len, n, 2, 210,
 * 160, 3) uint8; reward_pool: (pool_len, n) f32; done_pool: (pool_len, n)
 * uint8 (1 = the transition into this obs ended the episode, which also
 * resets the frame stack and LSTM state).  force_reset: treat every env as
 * starting an episode (first observation). */
int arl_observe(arl_net* net, int t, const uint8_t* pair_pool, const float* reward_pool,
                const uint8_t* done_pool, int64_t pool_len, int force_reset, int resize_mode, void* stream);

/* arl_observe for an ARL_ARCH_RGB net: the observation is the env's RGB
 * screen, img_pool (pool_len, n, H, W, 3) uint8 (W % 16 == 0, W <= 2048),
 * resized to 3 planes as arl_rgb_phi; same reward / done / reset handling
 * (the reset clears the LSTM state; there is no frame stack). */
int arl_observe_rgb(arl_net* net, int t, const uint8_t* img_pool, int H, int W, const float* reward_pool,
                    const uint8_t* done_pool, int64_t pool_len, int force_reset, int resize_mode, void* stream);

/* arl_observe for an ARL_ARCH_STACK net: stack_pool (pool_len, n, 4, 84, 84)
 * uint8 (ale.py:91-94 ALE.state: the 4 screens oldest first, zeros before
 * an episode's first screen), conv input = dqn_phi of it (dqn_phi.py:4-17).
 * stack_pool == NULL (t >= 1): ingest only the reward / done of the
 * transition into a terminal observation, whose state the reference never
 * feeds to the model (a3c.py:72-73, 165-167). */
int arl_observe_stack(arl_net* net, int t, const uint8_t* stack_pool, const float* reward_pool,
                      const uint8_t* done_pool, int64_t pool_len, int force_reset, void* stream);

/* arl_observe for an ARL_ARCH_STATES net: state_pool (pool_len, n, 4, 84, 84)
 * f32 (16-byte aligned), the conv input as phi returns it (a3c.py:73
 * np.expand_dims(self.phi(state), 0)); NULL (t >= 1): reward / done only, as
 * arl_observe_stack. */
int arl_observe_states(arl_net* net, int t, const float* state_pool, const float* reward_pool,
                       const uint8_t* done_pool, int64_t pool_len, int force_reset, void* stream);

/* The reference's early window end (a3c.py:77-78: an update at a terminal
 * after t_len < t_max steps): window steps [t_len, t_max) carry no loss and
 * no gradient in the next arl_learn (their done flags get bit 1, rewards 0).
 * Observations of the next window overwrite the flags again. */
int arl_truncate_window(arl_net* net, int t_len, void* stream);

/* Loss options of A3C.__init__ (a3c.py:33-36, 110-121): pi_loss_coef scales
 * the policy + entropy terms; keep_loss_scale_same scales both losses of a
 * segment that a terminal closed after len < t_max steps by t_max / len.
 * Host state of the handle, read when arl_learn launches (defaults 1, 0). */
int arl_net_set_loss(arl_net* net, double pi_loss_coef, int keep_loss_scale_same);

/* NonbiasWeightDecay(rate) (a3c_ale.py:204,227-228, nonbias_weight_decay.py),
 * the hook the reference adds after GradientClipping: per update, after the
 * clip (whose norm is the norm of the gradient BEFORE the decay) and before
 * update_one, g += rate * p -- t = f32(f32(rate) * p), g = f32(g + t), two
 * roundings -- for every parameter whose name is not 'b' and does not end in
 * '/b'.  The update kernel does it on the p / g it holds in registers (no
 * extra byte moved); the bias tensors come from the names arl_net_param_info
 * serves.  Every architecture and flag, the Nature head included.
 * Host state of the handle, like arl_net_set_loss (works on an unbound handle),
 * read when arl_optimize / arl_optimize_advance / arl_run_window launches the
 * update; default 0 = no hook: the decay-free kernel runs (a rate whose f32
 * value is 0 does too).  rate < 0 or not finite (as f32): ARL_EINVAL.  The
 * rate is a kernel argument, so a captured graph keeps the rate it was
 * captured with (as it keeps lr0): changing it needs a re-capture.
 * arl_run_stage(ARL_STAGE_RMSPROP) stays the decay-free timing form. */
int arl_net_set_weight_decay(arl_net* net, double rate);

/* Adam (Kingma & Ba 2015) as a second fused update kernel.  An extension,
 * off by default: the reference has RMSpropAsync only, whose hyperparameters
 * were tuned for one Hogwild process; the batched learner steps once per window
 * on the gradient of all envs.  The arithmetic is Chainer 1.8.1's
 * optimizers.Adam as NumPy evaluates it on float32 arrays.  State m, v: f32,
 * zero-initialised.  For update number t (1 for the first update):
 *   fix1 = 1 - beta1**t;  fix2 = 1 - beta2**t                     (float64)
 *   lr_t = (float)(alpha_a * sqrt(fix2) / fix1)     (float64, left to right, one rounding)
 *   m = f32(m + f32(c1 * f32(g - m)))               c1 = (float)(1.0 - beta1)
 *   v = f32(v + f32(c2 * f32(f32(g * g) - v)))      c2 = (float)(1.0 - beta2)
 *   p = f32(p - f32(f32(lr_t * m) / f32(sqrtf(v) + (float)eps)))
 * every elementwise operation round-to-nearest f32, unfused, in this order.
 * alpha_a is the call's lr0 as a double, or with total_steps > 0 the anneal of
 * arl_optimize in f64: max(total - global_t - 1, 0) / total * lr0.  g is the
 * gradient after GradientClipping and NonbiasWeightDecay, exactly as they feed
 * the RMSProp update.
 *
 * arl_net_set_adam(net, m, beta1, beta2): while m is set, every update of the
 * net (arl_optimize, arl_optimize_advance, arl_run_window) runs the Adam kernel
 * instead of the RMSProp one, with the same side duties (the FC weight's split
 * planes, the fused window advance).  m: param_floats f32, caller-owned,
 * 16-byte aligned, zeroed by the caller; the bound ms buffer holds v.  The
 * update call's lr0 is Adam's alpha and its eps Adam's eps; its alpha argument
 * (RMSProp's decay) is ignored.  m == NULL switches back to RMSpropAsync.  Host
 * state of the handle, like arl_net_set_weight_decay; ARL_EINVAL for a
 * misaligned m or a beta outside [0, 1) (NaN included).  A captured update keeps
 * the optimizer (and m, beta1, beta2) it was captured with.
 * arl_run_stage(ARL_STAGE_RMSPROP) keeps launching the RMSProp kernel.
 *
 * The update number lives on the device, so that a captured window replays
 * with a fresh bias correction: slot ARL_CTL_ADAM_T of the control block
 * (arl_net_buffer "ctl", int64[16]) holds the number of Adam updates made so
 * far; an update adds 1 (a one-thread launch ahead of the update kernel, so
 * that no workgroup reads a word its own launch writes) and uses the new count
 * as t.  Every workgroup computes lr_t itself in f64, beta**t by binary
 * exponentiation (exact at t = 1); against Python's pow the f32 lr_t can
 * differ by at most 1 ulp, and almost never does.
 * arl_net_reset zeroes the counter with the rest of the control block.
 * arl_net_set_adam_t: asynchronous write of the counter on `stream` (checkpoint
 * resume); read it through the "ctl" buffer.  ARL_ESTATE on an unbound net. */
#define ARL_CTL_ADAM_T 3
int arl_net_set_adam(arl_net* net, float* m, double beta1, double beta2);
int arl_net_set_adam_t(arl_net* net, int64_t t, void* stream);

/* Generalized advantage estimation, GAE(lambda) (Schulman et al. 2016), for
 * the policy term.  An extension: the reference has only the n-step advantage.
 * With lambda != 1 the learner's returns kernel also scans, per env and in
 * float64 with unfused round-to-nearest operations, k = t_max - 1 .. t:
 *   r_k   = (double)rewards[k, e], clipped to [-1, 1] iff clip_reward
 *   vn    = dones[k, e] bit 0 ? 0.0 : (double)v[k + 1, e]    (v[t_max, e]: the bootstrap value)
 *   d_k   = (r_k + gamma * vn) - (double)v[k, e]
 *   G     = dones[k, e] bit 0 ? 0.0 : G                      (G = 0.0 before the scan)
 *   G     = d_k + gl * G,       gl = gamma * lambda, one float64 product of the host
 *   adv_t = (float)G after k = t
 * and adv_t replaces f32(Rf - v) in dlogits and in the pi_loss term.  The value
 * target stays the n-step return, so R, dv and v_loss are bit for bit what
 * they are without it; pi_loss_coef, keep_loss_scale_same, beta and a
 * truncated window (dones bit 1) behave as before, and a terminal cuts the
 * scan, so steps past a truncated window's end do not reach a live step.
 * lambda == 1 (the default) is not routed through this: the n-step kernels
 * run with the arguments they always had.
 * Host state of the handle, like arl_net_set_loss (works on an unbound handle),
 * read at every returns launch: arl_learn, arl_learn_part(LEARN_RETURNS), the
 * returns fused into the bootstrap step, arl_run_window, every architecture.
 * gl is a kernel argument, so a captured graph keeps the lambda it was
 * captured with (as it keeps gamma and the weight-decay rate): changing it
 * needs a re-capture.  lambda outside [0, 1] or not finite: ARL_EINVAL.
 * Addition to ABI 4. */
int arl_net_set_gae(arl_net* net, double lambda);

/* Clipped-surrogate epochs (PPO, Schulman et al. 2017): several gradient steps
 * from one window's rollout.  An extension, off by default: the reference takes
 * one step per window and discards the samples.  With it off every call makes
 * exactly the launches it made before.  Additions to ABI 4.
 *
 * The rollout of a window runs as always: all t_max + 1 forwards with the
 * pre-update parameters theta_old.  A snapshot (arl_ppo_begin) then fixes, per
 * sample (t, e), t < t_max:
 *   lpo = log_probs[t, e, actions[t, e]]      as theta_old left it
 *   Rf  = (float)R_t                          the learner's n-step return
 *   adv = f32(Rf - v[t, e])                   at lambda == 1
 *       = the GAE adv_t                       at lambda != 1 (arl_net_set_gae)
 * Rf and adv come from the returns launch's own device functions in its order,
 * so they are bit for bit the values it forms.  A sample with dones bit 1 (past
 * a truncated window's end) stores 0, 0, 0.
 *
 * Loss gradient of an epoch (arl_ppo_learn).  For a live sample take the slot's
 * current pr[k], lp[k], vi -- the rollout's in epoch 1, those of the last
 * re-forward (arl_act_mode(net, t, 0)) later -- and ac = actions[t, e], lpo, adv,
 * Rf from the snapshot.  Every operation round-to-nearest f32 and unfused
 * unless marked:
 *   d      = f32(lp[ac] - lpo)
 *   rho    = (float)exp((double)d)            one float64 exp, one rounding
 *   lo, hi = (float)(1.0 - clip_eps), (float)(1.0 + clip_eps)     formed on the host
 *   active = adv >= 0 ? rho <= hi : rho >= lo     (min(rho A, clip(rho) A) has a gradient)
 *   w      = active ? f32(rho * adv) : 0.0f
 *   surr   = active ? w : f32((adv >= 0 ? hi : lo) * adv)
 *   H, t2_k as the returns launch forms them:  H = -sum_k f32(pr[k] * lp[k]) (k ascending),
 *            t2_k = f32(f32(beta * pr[k]) * f32(lp[k] + H))
 *   dlogits[k] = f32(pf * f32(f32(-w * f32(oh_k - pr[k])) + t2_k))       oh_k = (k == ac)
 *   dv         = f32(vf * dvv),  dvv = f32(vi - Rf)
 *   lpi = f32(pf * f32(surr + f32(beta * H)))
 *   lv  = f32(vf * f32(f32(dvv * dvv) * 0.5f))
 * pf, vf = pi_loss_coef, v_loss_coef, times the keep_loss_scale_same segment
 * factor (arl_net_set_loss); the per-env losses loss[2e] = 0 - lpi_{T-1} - ... -
 * lpi_0, loss[2e + 1] = 0 + lv_{T-1} + ... + lv_0 as arl_learn sums them.  At
 * rho == 1 (epoch 1: d == 0 exactly) w == adv, so epoch 1's dlogits and dv are
 * bit for bit those of arl_learn (n-step or GAE).  ratio[t, e] = rho (0 for a
 * sample that is not live).  The device's exp and the C library's can differ
 * in the last float64 bit, so rho is within 1 f32 ulp of a host replay.
 *
 * arl_net_set_ppo(net, snap, clip_eps): snap = 4 * t_max * n_envs f32,
 * caller-owned, 16-byte aligned, planes (t_max, n_envs) in this order: logp_old,
 * adv, ret, ratio.  NULL switches it off.  Host state of the handle, like
 * arl_net_set_adam (works on an unbound handle).  clip_eps not finite or outside
 * (0, 1), a misaligned snap: ARL_EINVAL.  FF nets with the NIPS head, and LSTM
 * nets that have a carry buffer (arl_net_set_ppo_state below), whatever their
 * observation flag; an LSTM without one and the Nature head: ARL_ESTATE.
 * While set, the bootstrap arl_act does not fuse the returns
 * (arl_net_set_returns_fusion is ignored) and arl_run_window returns ARL_ESTATE:
 * a single-call window has no epochs.
 *
 * A window with K epochs:
 *   observe / act slots 0 .. t_max as always (the bootstrap forward included)
 *   arl_ppo_begin(net, gamma, clip_reward, stream)        the snapshot, with the net's lambda
 *   for j = 1 .. K:
 *     j > 1: arl_act_mode(net, t, 0, stream), t = 0 .. t_max - 1    re-forward from the frame ring;
 *            mode 0 touches neither actions nor the Philox counters; the bootstrap slot is not
 *            re-forwarded (ret and adv are fixed).  LSTM: t ascending is part of the contract,
 *            slot t reads the state slot t - 1 wrote
 *     arl_ppo_learn(net, beta, v_loss_coef, stream)       loss gradient + heads dh, then
 *                                                         ARL_LEARN_TRUNK and ARL_LEARN_CONV
 *     arl_optimize (j < K) / arl_optimize_advance (j == K)
 * arl_ppo_begin sets the gamma / clip_reward / lambda the window statistics use,
 * as a returns launch does.  arl_ppo_learn's first launch writes the step
 * snapshot the update's fused advance reads, as the returns launch it replaces;
 * it never folds the clip norm (the update runs its own squared-norm launch).
 * ARL_ESTATE from either on an unbound net or with PPO off, and from
 * arl_ppo_learn without an arl_ppo_begin since the last window advance.
 * Window statistics: one record per update, K per window; in epochs >= 2 fields
 * 5-13 describe the slots' current contents (the re-forwarded v and entropy,
 * that epoch's losses; returns and advantages recomputed from the current v).
 * Fields 12 / 13 (adv_sum, adv_sumsq) stay the un-normalised advantage whatever
 * arl_net_set_ppo_options sets.
 *
 * The LSTM (ARL_ARCH_LSTM).  Rollout, snapshot, loss gradient and epoch record
 * are the FF net's: they read v, log_probs, probs, actions and dones only.
 *   Re-forward.  The LSTM step of slot t reads rows t of hbuf / cbuf / reset and
 * writes rows t + 1, and nothing writes rows 0 between two advances; so
 * arl_act_mode(net, t, 0, stream) for t = 0 .. t_max - 1 ascending recomputes the
 * window from the window's own initial state (rows 0 and the reset rows as the
 * rollout left them) with the current parameters.  Reset flags and the frame
 * ring are not touched.  BPTT is truncated to the window, as in arl_learn, on the
 * re-forwarded gates / cbuf / hbuf rows.
 *   Carry.  The state that enters the next window is the rollout's (h_T, c_T),
 * computed at theta_old: the rows the advance copies when no epoch re-forwards.
 * arl_ppo_begin saves rows T of hbuf and cbuf into the carry buffer (one launch,
 * after the snapshot's); the advancing update (arl_optimize_advance, or
 * arl_advance after arl_optimize) puts them back before anything advances (one
 * launch, before the window statistics and the update), when arl_ppo_begin ran in
 * this window.  The last epoch's BPTT and heads weight gradient read the
 * re-forwarded rows T, which is why the restore belongs to the update: the call
 * sequence above is the FF one unchanged.  After arl_truncate_window the same rows
 * are saved and restored, so row 0 after the advance is bit for bit what one
 * gradient step per window leaves.  The pi_and_v evaluation state is not touched.
 *
 * arl_net_set_ppo_state(net, carry): carry = 2 * n_envs * 256 f32, caller-owned,
 * 16-byte aligned, planes h then c.  Host state of the handle (works on an
 * unbound handle).  It is the LSTM's opt-in: arl_net_set_ppo and
 * arl_net_set_ppo_options accept an LSTM net only once a carry buffer is set.
 * Not an LSTM net: ARL_ESTATE.  A misaligned carry: ARL_EINVAL.  NULL unsets it;
 * NULL while PPO is set on the net: ARL_ESTATE (switch PPO off first).
 * Not built: the Nature head, minibatches within an epoch, several ranks. */
int arl_net_set_ppo(arl_net* net, float* snap, double clip_eps);
int arl_net_set_ppo_state(arl_net* net, float* carry);
int arl_ppo_begin(arl_net* net, double gamma, int clip_reward, void* stream);
int arl_ppo_learn(arl_net* net, double beta, double v_loss_coef, void* stream);

/* Options of the PPO epochs: advantage normalisation, the clipped value loss and
 * a device-side record per epoch.  All off by default, (0, 0.0, NULL, NULL):
 * every call then makes exactly the launches it made before.  Host state of the
 * handle, like arl_net_set_ppo (works on an unbound handle); read when
 * arl_ppo_begin / arl_ppo_learn launch, inert while PPO is off; a captured window
 * keeps what it was captured with.  Additions to ABI 4.
 *
 * A thread order shared by the two one-workgroup kernels below ("ordered sum"):
 * thread j of 256 owns envs j, j + 256, ... ascending and, per env, the steps
 * t = 0 .. t_max - 1 ascending; its float64 partial starts at +0.0, a sample that
 * is not live (dones bit 1) adds +0.0; the total is partial 0 + partial 1 + ... +
 * partial 255 in that order.  Every float64 operation is unfused round-to-nearest.
 *
 * norm_adv != 0 -- advantage normalisation.  arl_ppo_begin, right after the
 * snapshot, rewrites the snapshot's adv plane in place (logp_old and ret stay, so
 * the value target does not change):
 *   n_live = the count of live samples,  S1 = ordered sum of (double)adv
 *   mean = S1 / (double)n_live
 *   S2 = ordered sum of dd * dd,  dd = (double)adv - mean
 *   std = sqrt(S2 / (double)n_live)               the population form
 *   adv' = (float)(((double)adv - mean) / (std + 1e-8))   live samples, one rounding
 * A sample that is not live stays 0.  n_live == 0: nothing is rewritten and the
 * moments are 0, 0, 0.  (n_live, mean, std) go to aux[1..3].  Needs aux.
 *
 * vclip_eps > 0 -- the clipped value loss 0.5 * max((v - R)^2, (v_clip - R)^2),
 * v_clip = v_old + clamp(v - v_old, -eps, eps).  v_old: t_max * n_envs f32,
 * caller-owned, 16-byte aligned; arl_ppo_begin writes v_old[t, e] = v[t, e] of a
 * live sample, 0 otherwise (one small launch).  In arl_ppo_learn only the value
 * tail changes; with ev = (float)vclip_eps formed on the host, f32 unfused:
 *   dvv = f32(vi - Rf)                     as without it
 *   do  = f32(vi - vold);  inside = fabsf(do) <= ev
 *   inside:  dv = f32(vf * dvv);  lv = f32(vf * f32(f32(dvv * dvv) * 0.5f))
 *   outside: vc = f32(vold + (do > 0 ? ev : -ev));  dvc = f32(vc - Rf)
 *            lu = f32(dvv * dvv);  lc = f32(dvc * dvc);  taken = lc > lu
 *            dv = taken ? 0.0f : f32(vf * dvv)
 *            lv = f32(vf * f32((taken ? lc : lu) * 0.5f))
 * In epoch 1 vi == vold, so every sample is inside and dv, dlogits are bit for
 * bit those without value clipping.  vclip_eps == 0 switches it off (v_old is
 * then ignored).
 *
 * aux != NULL -- ARL_PPO_AUX_DOUBLES doubles, caller-owned, 8-byte aligned, zeroed
 * by the caller (arl_net_reset does not own it).  Word 0 is an int64: the count of
 * epoch records ever written.  Words 1..3: n_live, mean, std of the last
 * normalisation.  Words 4..7 reserved.  Record r sits at
 * 8 + (r % ARL_PPO_LOG) * ARL_PPO_STAT_FIELDS.  arl_ppo_learn launches the record's
 * kernel right after its loss-gradient launch (stream order: it sees that epoch's
 * ratio plane and the slots' log_probs / v).  Fields, sums ordered as above:
 *   0 window     the control block's window counter, read on the device
 *   1 epoch      1-based, counted on the host from arl_ppo_begin
 *   2 samples    live samples
 *   3 clipped    live samples with !(adv >= 0 ? rho <= hi : rho >= lo), rho from
 *                the ratio plane: the learner's decision
 *   4 kl_sum     sum of -(double)d, d = f32(lp[ac] - lpo)
 *   5 ratio_max  over live samples, 0 when there are none
 *   6 ratio_min  over live samples, 0 when there are none
 *   7 vclipped   live samples with `taken` above; 0 with value clipping off
 *   8 adv_sum    sum of (double)adv as the epoch used it (after normalisation)
 *   9 adv_sumsq  sum of its float64 square
 *
 * ARL_EINVAL: vclip_eps negative or not finite; vclip_eps > 0 with a NULL v_old;
 * norm_adv with a NULL aux; a misaligned pointer.  ARL_ESTATE: any option on for a
 * net arl_net_set_ppo refuses. */
#define ARL_PPO_LOG 16            /* epoch records kept */
#define ARL_PPO_STAT_FIELDS 10
#define ARL_PPO_AUX_DOUBLES (8 + ARL_PPO_LOG * ARL_PPO_STAT_FIELDS)
int arl_net_set_ppo_options(arl_net* net, int norm_adv, double vclip_eps, float* v_old, double* aux);

/* GradientClipping's squared norm (a3c_ale.py:226) folded into arl_learn:
 * with on != 0, arl_learn's conv slab reduce also leaves the f64 partial
 * sums of squares of the whole gradient (the conv tensors it writes, and the
 * rest, final by then), and the next arl_optimize / arl_optimize_advance
 * uses them instead of its own squared-norm launch.  Only valid when nothing
 * changes the gradient in between (turn it off when the gradient is
 * all-reduced across ranks); arl_learn_part never folds.  Default off. */
int arl_net_set_norm_fold(arl_net* net, int on);

/* Kernel forms.  Four launches have two bit-identical kernels each, and the net
 * picks between them per launch:
 *   ARL_FORM_CONV_EPW     envs per conv forward workgroup: 1 or 2.  Auto: 2 in nets
 *                         of >= 512 envs (the net's count, whatever the launch covers)
 *   ARL_FORM_FC_BIG       1 = the FC forward's 64-row tiles, 0 = its 32-row tiles.
 *                         Auto: 1 for launches over >= 512 envs
 *   ARL_FORM_LSTM_XRED    1 = the LSTM gate kernel reduces the FC's split-K partials
 *                         in its staging, 0 = the FC's last-arriver ticket does.
 *                         Auto: 1 for launches over < 512 envs
 *   ARL_FORM_CONV_BWD_WS  1 = the wave-specialised conv backward, 0 = the 512-thread
 *                         kernel.  Auto: 1
 * arl_net_set_form sets one of them to a concrete value or back to ARL_FORM_AUTO
 * (the default).  It sets host state of the handle only (no bind needed), and is
 * accepted without effect where the net never runs that kernel (the Nature head;
 * ARL_FORM_LSTM_XRED on FF nets).  arl_net_form returns in *value the concrete form
 * a launch over launch_envs envs of this net would run now (ARL_FORM_CONV_EPW
 * ignores launch_envs), through the rule the launches themselves use.
 *
 * A form is read when a launch is issued: a captured graph keeps the forms it was
 * captured with, and changing a form between windows of a bound net is allowed.
 * All combinations share one workspace layout (the ticket buffer is sized by the
 * 32-row tiling and the kernels reset it), so nothing is reallocated.
 *
 * ARL_EINVAL: a null net or value pointer, an unknown form, launch_envs < 1, or a
 * value that is neither ARL_FORM_AUTO nor one of the form's two. */
#define ARL_FORM_AUTO (-1)
#define ARL_FORM_CONV_EPW 0
#define ARL_FORM_FC_BIG 1
#define ARL_FORM_LSTM_XRED 2
#define ARL_FORM_CONV_BWD_WS 3
int arl_net_set_form(arl_net* net, int form, int value);
int arl_net_form(const arl_net* net, int form, int launch_envs, int* value);

/* The learner's returns + loss gradient + heads backward (arl_learn_part
 * ARL_LEARN_RETURNS, a3c.py:82-130) folded into the bootstrap step's policy
 * launch: with on != 0, the next arl_act / arl_act_mode at t == t_max over all
 * envs of an FF net with the NIPS head runs them in that launch with these
 * arguments, bit-identical, and the window's ARL_LEARN_RETURNS part (or
 * arl_learn's first launch) is then skipped.  arl_run_window does this
 * internally.  Host state of the handle; default off. */
int arl_net_set_returns_fusion(arl_net* net, int on, double gamma, double beta, double v_loss_coef, int clip_reward);

/* A3C.act forward + sample at window step t (a3c.py:154-164): pi_and_v of
 * the ring state, softmax policy output, Philox inverse-CDF action.  t ==
 * t_max is the bootstrap value of the window end (a3c.py:85, pre-update
 * params, LSTM state kept: a3c_ale.py:57-60); it samples nothing. */
int arl_act(arl_net* net, int t, void* stream);

/* arl_act with an explicit action mode: 0 = forward only (no action), 1 =
 * sample (as arl_act), 2 = greedy, the first argmax of the probabilities
 * (SoftmaxPolicyOutput.most_probable_actions, policy_output.py:37-39; the
 * evaluation policy of a3c_ale.py:73-89 / demo_a3c_ale.py:15-30). */
int arl_act_mode(arl_net* net, int t, int mode, void* stream);

/* Env groups: arl_observe / arl_observe_rgb and arl_act_mode restricted to
 * envs [e0, e0 + ne) of the net (no reference counterpart: the batched
 * form of running a3c.py:67-167 for a subset of the actors).  Disjoint
 * ranges touch disjoint workspace rows, so ranges issued on different
 * streams run concurrently (A3C.run_window(env_groups=G) forks one stream
 * per group for the T + 1 forward steps and joins before arl_learn).
 * e0 must be a multiple of ARL_ENV_GROUP_ALIGN; H, W are the screen size of
 * an ARL_ARCH_RGB net (ignored otherwise).  The Nature head accepts only
 * the full range. */
#define ARL_ENV_GROUP_ALIGN 32
int arl_observe_envs(arl_net* net, int t, int e0, int ne, const uint8_t* pool, int H, int W,
                     const float* reward_pool, const uint8_t* done_pool, int64_t pool_len, int force_reset,
                     int resize_mode, void* stream);
/* mode for arl_act_envs: 0 / 1 / 2 as arl_act_mode, optionally | one of
 * ARL_ACT_CONV_ONLY (launch only the step's conv layers) or
 * ARL_ACT_AFTER_CONV (the rest of the step): a stream can then record an
 * event between the two, which is how run_window staggers the groups. */
#define ARL_ACT_CONV_ONLY 4
#define ARL_ACT_AFTER_CONV 8
int arl_act_envs(arl_net* net, int t, int e0, int ne, int mode, void* stream);

/* Window update, gradient part (a3c.py:82-130): n-step returns with R = 0 at
 * terminals, advantage / entropy / value loss gradient, backward through
 * heads, [LSTM BPTT], FC, conv2, conv1 -> grads (overwritten). */
int arl_learn(arl_net* net, double gamma, double beta, double v_loss_coef, int clip_reward, void* stream);

/* arl_learn in parts (NIPS FF / LSTM heads; not the Nature head): parts 0..2
 * in order on one stream equal arl_learn (without its folded clip norm).
 * Part 0: returns + loss gradient + the heads' dh; part 1: LSTM BPTT and gate
 * weight gradients, the FC backward (dW, db, da2) and the heads' weight
 * gradients; part 2: the conv backward and its slab reduce, which write only
 * the conv tensors [0, offset of "0/2/W") of the gradient -- everything after
 * is final once part 1 is done (the N > 1 window all-reduces it meanwhile). */
#define ARL_LEARN_RETURNS 0
#define ARL_LEARN_TRUNK 1
#define ARL_LEARN_CONV 2
int arl_learn_part(arl_net* net, int part, double gamma, double beta, double v_loss_coef, int clip_reward,
                   void* stream);

/* GradientClipping(clip) + RMSpropAsync update (a3c_ale.py:224-226,
 * rmsprop_async.py:23-29) of the bound params / ms from the bound grads.
 * total_steps > 0 anneals lr on device (a3c_ale.py:111-112) with global_t =
 * (step + t_max) * n_total; otherwise lr = lr0.  clip <= 0 disables clipping.
 * After arl_net_set_adam the update is Adam's instead: lr0 is its alpha (annealed
 * the same way), eps its eps, and the alpha argument is ignored. */
int arl_optimize(arl_net* net, double lr0, int64_t total_steps, int64_t n_total, double alpha, double eps,
                 double clip, void* stream);

/* One stage of a window, run alone on the current workspace contents (the
 * same launches arl_act / arl_learn make), for per-kernel timing and
 * profiling.  t selects the window step for the forward stages.  Stages 1-11
 * and ARL_STAGE_RMSPROP. */
enum {
  ARL_STAGE_CONV_FWD = 1,   /* fused conv1 + conv2 forward from the frame ring */
  ARL_STAGE_FC_FWD = 2,     /* Linear(2592, 256): FF nets write the 8 split-K partials only; LSTM
                               nets reduce + bias + relu in the same launch */
  ARL_STAGE_POLICY = 3,     /* pi / v heads + softmax policy output (no action); FF nets first
                               reduce the FC partials + bias + relu into h (as in a window step) */
  ARL_STAGE_FC_BWD = 4,     /* FC dW / db and da2 GEMMs (+ the pi / v heads dW / db) */
  ARL_STAGE_CONV_BWD = 5,   /* fused conv backward (conv2 dW, convT, conv1 dW) into per-block slabs */
  ARL_STAGE_RETURNS = 6,    /* n-step returns + loss gradient + heads dh (gamma 0.99, beta 0.01, v coef 0.5,
                               clipped rewards): the learner's first launch */
  ARL_STAGE_CONV_REDUCE = 7,  /* the conv backward's slab reduce into the conv gradients */
  ARL_STAGE_GRAD_SQNORM = 8,  /* squared-norm partials of the whole gradient (GradientClipping) */
  ARL_STAGE_LSTM_GATES = 9,   /* LSTM: the gate kernel of slot t (cell in its epilogue) */
  ARL_STAGE_LSTM_BPTT = 10,   /* LSTM: one truncated-BPTT step (dh GEMM + the previous step's cell backward) */
  ARL_STAGE_LSTM_WGRAD = 11,  /* LSTM: the gate weight gradients + dfc (one launch) */
  /* timeline-only stages (arl_stamps_*, not arl_run_stage) */
  ARL_STAGE_PHI = 12,         /* the observation (phi into the frame ring) */
  ARL_STAGE_RMSPROP = 13,     /* clip + RMSProp (+ the window advance); arl_run_stage: the update
                                 kernel alone, lr 0, clip 40 at the norm the last window left */
  ARL_STAGE_LSTM_CELL = 14,   /* the LSTM cell backward of the window's last step */
  ARL_STAGE_HOST = 15,        /* a caller's stamp (arl_stamp), e.g. after a collective */
  ARL_STAGE_OTHER = 16
};
int arl_run_stage(arl_net* net, int stage, int t, void* stream);

/* Window timeline (measurement; no reference counterpart).  After
 * arl_stamps_begin(net, cap) every stage launch of the window (arl_observe*,
 * arl_act*, arl_learn*, arl_optimize*) records a timing event on its stream
 * right after its kernel(s), with the stage it closes (ARL_STAGE_*), up to cap
 * events; arl_stamp records one for the caller.  arl_stamps_end stops and
 * returns the count.  arl_stamps_read waits for stamp i0 + n - 1 and returns,
 * for i in [i0, i0 + n), ms[i - i0] = the time from stamp i - 1 to stamp i (0
 * for i = 0) and stage[i - i0]: consecutive intervals split an eager window
 * into its stages as it ran, launch boundaries included.
 * arl_stamps_sparse(net, P), right after arl_stamps_begin, for windows of P
 * stamp calls: window w records only its calls t - 1 and t, t = w mod P, so
 * each window carries at most two events and P windows time every stage once
 * nearly unperturbed; arl_stamps_read then returns ms = -1 for an interval
 * that is not between consecutive calls. */
int arl_stamps_begin(arl_net* net, int cap);
int arl_stamps_sparse(arl_net* net, int period);
int arl_stamp(arl_net* net, int stage, void* stream);
int arl_stamps_end(arl_net* net, int* count);
int arl_stamps_read(arl_net* net, int i0, int n, float* ms, int* stage);

/* One whole lockstep window in one call, for frame-pair nets with the NIPS
 * head (FF / LSTM): t = 0..t_max: arl_observe(t) (slot 0 only when first != 0,
 * with force_reset) + arl_act(t) (sampled; slot t_max the bootstrap forward,
 * a3c.py:85), then arl_learn and arl_optimize_advance (a3c.py:88-144) -- the
 * same launches in the same order as those calls one by one, issued without a
 * host round trip per step (A3C.run_window's single-chain window without
 * collectives). */
int arl_run_window(arl_net* net, const uint8_t* pair_pool, const float* reward_pool, const uint8_t* done_pool,
                   int64_t pool_len, int first, int resize_mode, double gamma, double beta, double v_loss_coef,
                   int clip_reward, double lr0, int64_t total_steps, int64_t n_total, double alpha, double eps,
                   double clip, void* stream);

/* End of window: advance step counters, carry reset flags / LSTM state. */
int arl_advance(arl_net* net, void* stream);

/* arl_optimize followed by arl_advance (the end of a3c.py's update,
 * a3c.py:139-144) in one call; for the NIPS models the update kernel also
 * advances the window (one launch fewer). */
int arl_optimize_advance(arl_net* net, double lr0, int64_t total_steps, int64_t n_total, double alpha, double eps,
                         double clip, void* stream);

/* A3CFF / A3CLSTM.pi_and_v on explicit f32 states (a3c_ale.py:38-40,55-63;
 * input from dqn_phi), rows 0..n-1, n <= n_envs; outputs in the workspace's
 * bootstrap slot.  mode as arl_act_mode: 0 no action, 1 sampled
 * (action_indices from Philox stream 1, counter = number of sampling
 * forward_states calls so far on this handle: repeated calls draw afresh),
 * 2 greedy (most_probable_actions).  LSTM: the recurrent state is the
 * handle's pi_and_v state (not the lockstep window's); it advances unless
 * mode | ARL_FWD_KEEP_STATE (keep_same_state, a3c_ale.py:57-60). */
#define ARL_FWD_KEEP_STATE 16
int arl_forward_states(arl_net* net, const float* states, int64_t n, int mode, void* stream);

/* A3CLSTM.reset_state (a3c_ale.py:65-66) of the pi_and_v state, rows
 * [e0, e0 + n): the next forward starts from h = c = None.  No-op for FF. */
int arl_reset_state(arl_net* net, int64_t e0, int64_t n, void* stream);

/* ------------------------------------------------------------------ episode statistics */

/* Device-side episode statistics: the learning curve of train_loop
 * (a3c_ale.py:95-96,114-124: episode_r += env.reward, printed and zeroed at every
 * terminal; total_r) without copying a step's rewards or dones to the host.
 * Off by default; additions to ABI 4.  While on, the thread that ingests env
 * e's reward / done in arl_observe* / arl_observe_envs / arl_run_window also
 * accumulates them; an observation at window slot t >= 1 carries (r, d):
 *   run_ret[e] += r, run_len[e] += 1, total[e] += r, steps[e] += 1
 *   d != 0, the episode is complete with return G = run_ret, length L = run_len:
 *     count[e] += 1, sum[e] += G, sumsq[e] += G * G, len_sum[e] += L,
 *     min[e] = min(min[e], G), max[e] = max(max[e], G);
 *     (G, L, k) -> env e's log entry (count before) % ARL_EPISODE_LOG, where
 *     k = control-block step + t is the global observation index;
 *     log_count[e] += 1; run_ret[e] = 0, run_len[e] = 0.
 * r is the raw float32 reward, never clipped, whatever clip_reward says (the
 * reference sums env.reward; clipping happens only in the returns).  Slot 0
 * carries no reward.  force_reset abandons the running episode (run_ret =
 * run_len = 0 after the above) and does not count as an episode.  Observing
 * the same slot twice counts its reward twice.
 * All sums are float64 with unfused round-to-nearest adds / multiplies in
 * env-step order; lengths, counts and steps are int64; one thread owns one
 * env (no atomics), so a NumPy float64 replay is bit-identical, env-range
 * launches on several streams and graph replays included.
 * The arrays are the last arl_net_buffer entries of the workspace, 8-byte
 * elements, (n_envs,) each: ep_run_ret, ep_total, ep_sum, ep_sumsq, ep_min,
 * ep_max (f64); ep_run_len, ep_steps, ep_count, ep_len_sum, ep_log_count
 * (int64); and the logs, (ARL_EPISODE_LOG, n_envs): ep_log_ret (f64),
 * ep_log_len, ep_log_step (int64).  arl_net_reset zeroes the block (with
 * count 0: min = +inf, max = -inf), whether the feature is on or not.
 *
 * arl_net_set_episode_stats: on / off for the observations launched (or
 * captured) from now on.  arl_episode_stats_reset: zero the whole block.
 * arl_episode_stats: reduce over the envs, stream-ordered behind the
 * observations that fed it, into 8 doubles of device memory (8-byte aligned):
 *   [episodes, return_sum, return_sumsq, return_min, return_max, length_sum,
 *    steps, reward_sum]
 * in a fixed order (one 256-thread workgroup: thread j sums envs j, j + 256,
 * ... ascending, thread 0 then combines partials 0..255 in order).  clear != 0
 * also zeroes the cumulative per-env arrays it read (ep_count, ep_sum,
 * ep_sumsq, ep_min, ep_max, ep_len_sum, ep_steps, ep_total; not the running
 * episode, not the log): "statistics since the last read".
 * All three: ARL_ESTATE on an unbound net; arl_episode_stats also ARL_ESTATE
 * while the feature is off, ARL_EINVAL for a null or misaligned out8_device. */
#define ARL_EPISODE_LOG 8
int arl_net_set_episode_stats(arl_net* net, int on);
int arl_episode_stats_reset(arl_net* net, void* stream);
int arl_episode_stats(arl_net* net, double* out8_device, int clear, void* stream);

/* ------------------------------------------------------------------ window statistics */

/* Device-side per-window training statistics: what the reference's learner
 * logs at every update -- pi_loss / v_loss (a3c.py:123-124), the gradient norm
 * before the clip (a3c.py:136-141), entropy and value per step
 * (a3c.py:161-163), the annealed learning rate -- without a host sync per
 * window and inside a graph replay.  Off by default; additions to ABI 4.
 * While on, every update of the net (arl_optimize, arl_optimize_advance,
 * arl_run_window) appends one record of ARL_WINDOW_STAT_FIELDS doubles to a
 * ring log in the workspace: one extra single-workgroup launch, stream-ordered
 * (and graph-capturable) after the clip norm's partials exist and before the
 * update kernel, so the control block is not yet advanced.  The record
 * describes the window whose gradient the update consumes.  A sample (t, e),
 * t < t_max, is live when dones[t, e] bit 1 is clear (not past a truncated
 * window's end).
 *    0 window        ctl window counter before the update
 *    1 step          the per-env step counter the update's lr anneal reads
 *    2 samples       number of live samples
 *    3 terminals     live samples with dones bit 0
 *    4 reward_sum    sum over live of the reward as the learner uses it:
 *                    (double)r, clipped to [-1, 1] iff the window's clip_reward
 *    5 pi_loss       sum over envs of (double)loss[2e]
 *    6 v_loss        sum over envs of (double)loss[2e + 1]
 *    7 entropy_sum   sum over live of (double)entropy[t, e]
 *    8, 9   value_sum, value_sumsq     of (double)v[t, e] and its f64 square
 *   10, 11  return_sum, return_sumsq   of (double)Rf and its f64 square, Rf =
 *                    (float)R_t the learner's n-step return: f64 recurrence from
 *                    v[t_max, e], R = 0 at bit-0 terminals, R = R * gamma + clip(r)
 *   12, 13  adv_sum, adv_sumsq         of (double)adv, adv = f32(Rf - v), and its f64 square;
 *                    with arl_net_set_gae(lambda != 1) adv is the GAE adv_t the learner
 *                    used (the same device function on the same values)
 *   14 grad_sqnorm   squared norm of the gradient the update consumes, from the
 *                    partials the update kernel reads (with several ranks: of
 *                    the all-reduced gradient)
 *   15 clip_scale    (double) of the f32 scale the update applies; 1.0 when it does not clip
 *   16 lr            (double) of the f32 learning rate the update uses, anneal included;
 *                    with arl_net_set_adam the bias-corrected lr_t of this update, from
 *                    the Adam kernel's own device function (written by the one-thread
 *                    launch that counts the update)
 * gamma, clip_reward and the GAE lambda are those of the last returns launch of the net
 * (arl_learn, arl_learn_part(LEARN_RETURNS), the returns fused into the
 * bootstrap step, arl_run_window); 0.99 and 1 before any.  With clip <= 0 the
 * update still launches the squared-norm kernel while the feature is on, so
 * field 14 is always filled; field 15 is then 1.0.
 * All sums are float64 with unfused round-to-nearest adds / multiplies, in a
 * fixed order: one 256-thread workgroup; thread j walks envs j, j + 256, ...
 * ascending and, for each env, t = 0 .. t_max - 1 ascending (after one reverse
 * scan for the R_t); each field's partials 0 .. 255 are then combined in
 * order (partial 0, plus partial 1, ...).  A sample that is not live adds
 * +0.0, which changes no bit.  Counts are exact integers stored as doubles.  A NumPy float64 replay in that
 * order is bit-identical for fields 0-13; the return recurrence, the clip
 * scale and the lr anneal are the learner's and the update kernel's own device
 * functions, so fields 10-13, 15 and 16 are bit for bit what they use.
 * Storage: two arl_net_buffer entries before the episode block, both 256-byte
 * aligned: win_log, (ARL_WINDOW_LOG, ARL_WINDOW_STAT_FIELDS) float64, and
 * win_count, one int64: records ever written; a record goes to slot
 * count % ARL_WINDOW_LOG.  Read them through their offsets, as the episode
 * log.  arl_net_reset zeroes both, whether the feature is on or not.
 *
 * arl_net_set_window_stats: on / off for the updates launched (or captured)
 * from now on; off: no extra launch, the same kernels with the same arguments.
 * arl_window_stats_reset: zero win_log and win_count.
 * Both: ARL_ESTATE on an unbound net. */
#define ARL_WINDOW_LOG 64
#define ARL_WINDOW_STAT_FIELDS 17
int arl_net_set_window_stats(arl_net* net, int on);
int arl_window_stats_reset(arl_net* net, void* stream);

/* ------------------------------------------------------------------ device environment */

/* A device-resident Catch, so that the actor-learner loop closes without the
 * host: env -> phi -> forward -> sample -> env -> ... -> update, eagerly or as
 * one replayed graph.  An extension (the reference's envs are host emulators,
 * ale.py / doom_env.py); additions to ABI 4.  One launch per env-step does the
 * transition and the render of real 210 x 160 x 3 frame pairs into the pools
 * arl_observe reads, with the reward and done the learner ingests.
 *
 * The game (exact in integer arithmetic; tests/catch_ref.py restates it).
 * Screen 210 rows x 160 columns, RGB uint8, HWC, black.  Paddle 16 x 4 on rows
 * 190..193, colour (200, 72, 72), left edge px in [0, 144].  Ball 8 x 8, colour
 * (236, 236, 236), left edge bx in [0, 152], top edge by; a pixel inside both
 * takes the ball's colour.  Action 2 moves right, 3 left, every other value is
 * a no-op (Breakout's NOOP / FIRE / RIGHT / LEFT; any n_actions >= 4).
 * One env-step is up to 4 emulator frames; frame f = 0..3:
 *   1. right: px = min(px + 3, 144); left: px = max(px - 3, 0)
 *   2. bx += vx; bx < 0: bx = -bx, vx = -vx; else bx > 152: bx = 304 - bx, vx = -vx
 *   3. by += 3
 *   4. by + 8 >= 190: the episode ends in this frame and the skip loop breaks
 *      (ale.py:111-139); reward +1 if bx + 8 > px && bx < px + 16, else -1.
 * Non-terminal step: reward 0.0f, done 0, pair[0] = the screen after frame 4,
 * pair[1] = the screen after frame 3 (the order arl_observe documents).
 * Terminal step: reward +-1.0f, done 1, the env starts its next episode at once
 * and both frames of the pair are that episode's first screen (the reference's
 * episode start, ale.py:141-161; the terminal screen is never shown).
 * Episode start (the per-env episode counter starts at 0 and advances at every
 * terminal): by = 18, px = 72, steps_in_episode = 0, and with (w0, w1, ., .) =
 * philox4x32_10(counter = (env_offset + e, episode, 0, 2), key = (seed &
 * 0xffffffff, seed >> 32)): bx = w0 % 153, vx = (int)(w1 % 5) - 2.  Counter
 * word 3 = 2 is a stream beside 0 (window draws) and 1 (pi_and_v draws).
 * Every episode lasts 14 env-steps; the optimal return is +1, a uniform random
 * policy scores about -0.70.
 *
 * Env state: caller-owned device memory, (2, n_envs, 8) int32, 16-byte aligned,
 * [bx, by, vx, px, episode, steps_in_episode, 0, 0] per env, double-buffered by
 * the parity of the global observation index: the launch for observation
 * k -> k + 1 reads half k & 1 and writes half (k + 1) & 1.  Every workgroup of
 * an env recomputes the transition from the old half and one of them writes the
 * new half, the reward and the done, so no workgroup reads a word another
 * workgroup of its launch writes.
 *
 * Granular calls (no net): arl_catch_state_bytes(n_envs) = the state's size;
 * arl_catch_reset: episode 0 of every env into half `parity`, the first screens
 * (twice) into pair_out (n, 2, 210, 160, 3), rewards 0.0f (n,), dones 0 (n,);
 * arl_catch_step: one env-step from actions (n,) int32 and half parity_in into
 * half 1 - parity_in and the outputs.  n <= 65535; ARL_EINVAL for a null or
 * misaligned pointer (state, frames 16 bytes) or a parity other than 0 / 1. */
#define ARL_ENV_CATCH 1
int64_t arl_catch_state_bytes(int64_t n_envs);
int arl_catch_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int parity, uint8_t* pair_out,
                    float* reward_out, uint8_t* done_out, void* stream);
int arl_catch_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                   uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* stream);

/* A device-resident Breakout, the second device environment: the game the
 * reference's published numbers are about, with what Catch lacks -- episodes
 * of different lengths (terminals out of phase between envs), rewards above 1
 * (clip_reward has work to do), lives (the reference's
 * treat_life_lost_as_terminal, ale.py:96-131) and bricks that persist across
 * an episode boundary.  Same launch shape, pools and state protocol as Catch;
 * additions to ABI 4.
 *
 * The game (exact in integer arithmetic; tests/breakout_ref.py restates it).
 * Screen 210 rows x 160 columns, RGB uint8, HWC, black.
 * Bricks: 6 rows x 20 columns, each 8 wide and 6 tall; brick (r, c) covers
 *   columns 8c .. 8c+7 and rows 57+6r .. 62+6r.  Bit i = 20r + c lives in four
 *   uint32 words: word i >> 5, bit i & 31.  Row colours, r = 0..5: (200,72,72),
 *   (198,108,58), (180,122,48), (162,162,42), (72,160,72), (66,72,200).  Row
 *   values: 7, 7, 4, 4, 1, 1.
 * Paddle: 16 x 4 on rows 190..193, colour (200,72,72), px in [0, 144].
 * Ball: 4 x 4, colour (236,236,236), bx in [0, 156]; a ball pixel covers
 *   anything under it.
 * Actions: 2 = right, 3 = left, anything else a no-op (n_actions >= 4).  There
 *   is no FIRE: the ball serves itself.
 * Serve: by = 100, vy = +4, and with (w0, w1, ., .) = philox4x32_10(counter =
 *   (env_offset + e, serves, 0, 3), key = (seed & 0xffffffff, seed >> 32)):
 *   bx = w0 % 157, vx = (-2, -1, 1, 2)[w1 % 4]; then serves += 1.  serves
 *   counts every serve of the env and starts at 0.  Counter word 3 = 3 is a
 *   stream beside 0 (window draws), 1 (pi_and_v draws) and 2 (Catch).
 * New game: all 120 bricks present, lives = 5, px = 72, game_steps = 0,
 *   score = 0, then a serve.
 * One env-step is up to 4 frames; frame f does, in order:
 *   1. right: px = min(px + 3, 144); left: px = max(px - 3, 0)
 *   2. bx += vx; bx < 0: bx = -bx, vx = -vx; else bx > 156: bx = 312 - bx,
 *      vx = -vx
 *   3. by += vy; by < 32: by = 64 - by, vy = -vy
 *   4. brick test: cx = bx + 2, cy = by if vy < 0 else by + 3; if
 *      57 <= cy < 93: r = (cy - 57) / 6, c = cx >> 3; if the bit is set: clear
 *      it, reward += value[r], vy = -vy, bricks_left -= 1
 *   5. paddle test, only if vy > 0 && by + 4 >= 190: if bx + 4 > px &&
 *      bx < px + 16: by = 372 - by, vy = -vy, vx = (-2,-1,1,2)[clamp(bx + 2 -
 *      px, 0, 15) >> 2]; otherwise a life is lost: lives -= 1
 *   6. the skip loop breaks in the frame where a life is lost or
 *      bricks_left == 0 (ale.py:111-139).
 * After the frames: game_steps += 1, score += reward.  The game is over when
 * lives == 0 || bricks_left == 0 || game_steps >= 1000; a new game then starts
 * at once (game += 1).  On a life loss that does not end the game the ball is
 * re-served at once; bricks, lives, score and px are kept.  In both cases both
 * frames of the pair are the first screen after the serve (Catch's rule: the
 * losing screen is never shown).  Otherwise pair[0] is the screen after frame
 * 4 and pair[1] the screen after frame 3.
 * Done: by default a life loss is terminal (ale.py:98-99): done = life lost ||
 * game over.  With ARL_ENV_GAME_OVER_ONLY done = game over only (the
 * reference's evaluation env, a3c_ale.py:75-76).  The two modes differ in
 * nothing but the done byte and steps_in_episode (which counts the env-steps
 * since the last done); state, rewards and frames are identical.  The reward
 * is the raw float sum of the step's brick values (it can be 14): clipping is
 * the learner's business (clip_reward), the episode statistics count it raw.
 * A uniform random policy scores about 0.15 per life (88 % of lives score 0,
 * a life lasts 6 env-steps and more); tracking the ball scores hundreds per
 * game and runs into the 1000-step cap.
 *
 * Env state: caller-owned device memory, (2, n_envs, 16) int32, 16-byte
 * aligned, [bx, by, vx, vy, px, lives, serves, steps_in_episode, game,
 * game_steps, score, bricks_left, b0, b1, b2, b3] per env, double-buffered by
 * the parity of the observation index exactly as Catch's.
 *
 * Granular calls: Catch's trio; arl_breakout_step takes flags = 0 or
 * ARL_ENV_GAME_OVER_ONLY (anything else: ARL_EINVAL). */
#define ARL_ENV_BREAKOUT 2
#define ARL_ENV_GAME_OVER_ONLY 0x100
int64_t arl_breakout_state_bytes(int64_t n_envs);
int arl_breakout_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int parity, uint8_t* pair_out,
                       float* reward_out, uint8_t* done_out, void* stream);
int arl_breakout_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                      int flags, uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* stream);

/* A device-resident Pong, the third device environment: the game the A3C paper
 * leads with, with what the other two lack -- rewards of both signs inside an
 * episode that do not end it (the n-step return and the GAE recurrence run
 * through a -1 that does not close the segment), an opponent (part of the
 * dynamics is not the agent's), games of hundreds of env-steps (almost every
 * window bootstraps, and the step cap is reached), a background that is not
 * black, and ALE Pong's six-action minimal set with its aliased actions.  Same
 * launch shape, pools and state protocol as Catch; additions to ABI 4.
 *
 * The game (exact in integer arithmetic; tests/pong_ref.py restates it).
 * Screen 210 rows x 160 columns, RGB uint8, HWC.
 * Background (144,72,17) everywhere not listed below.
 * Walls (236,236,236): rows 24..33 and rows 194..203, full width.
 * Opponent paddle (213,130,74): 4 x 16, columns 16..19, rows oy..oy+15, oy in
 *   [34, 178].
 * Agent paddle (92,186,92): 4 x 16, columns 140..143, rows py..py+15, py in
 *   [34, 178].
 * Ball (236,236,236): 4 x 4, left edge bx, top edge by in [34, 190].
 * Draw order: the ball over a paddle, a paddle over the background.
 * Actions (NOOP, FIRE, UP, DOWN, UPFIRE, DOWNFIRE): 2 and 4 move the agent up,
 *   3 and 5 down, every other value is a no-op (any n_actions >= 4).  There is
 *   no FIRE: the ball serves itself.
 * One env-step is up to 4 frames; frame f does, in order:
 *   1. up: py = max(py - 4, 34); down: py = min(py + 4, 178)
 *   2. opponent: c = by + 2 - (oy + 8); c > 2: oy = min(oy + 2, 178); c < -2:
 *      oy = max(oy - 2, 34) (it follows the ball at half the agent's speed,
 *      with a dead zone)
 *   3. by += vy; by < 34: by = 68 - by, vy = -vy; else by > 190: by = 380 - by,
 *      vy = -vy
 *   4. bx += vx
 *   5. paddles: if vx > 0 && 136 <= bx < 139, and by + 4 > py && by < py + 16:
 *      bx = 272 - bx, vx = -3, vy = 2 * (clamp(by + 2 - py, 0, 15) >> 2) - 3
 *      (one of -3, -1, 1, 3); else if vx < 0 && 16 < bx <= 19, and by + 4 > oy
 *      && by < oy + 16: bx = 40 - bx, vx = +3, vy from oy in the same way.
 *      |vx| = 3 and the three-column windows: each crossing is tested once.
 *   6. point: bx < 0: reward +1 (the agent scored); bx > 156: reward -1.  The
 *      skip loop breaks in that frame.
 * After the frames: game_steps += 1, and a point raises the scorer's count.
 * The game is over when either count reaches `points` (1..21) or game_steps >=
 * 5000; a new game then starts at once.
 * New game: py = oy = 106, both counts 0, game_steps = 0, then a serve.  game
 *   counts the games finished: 0 after the reset, += 1 at every game over.
 * A point that does not end the game: a serve only; the paddles stay.
 * Serve: with (w0, w1, w2, .) = philox4x32_10(counter = (env_offset + e,
 *   serves, 0, 4), key = (seed & 0xffffffff, seed >> 32)): bx = 78, by = 34 +
 *   w0 % 157, vy = 2 * (w1 % 4) - 3; in a new game vx = (w2 & 1) ? 3 : -3,
 *   after a point vx points toward the side that conceded (-3 after a +1);
 *   then serves += 1.  serves counts every serve of the env and starts at 0.
 *   Counter word 3 = 4 is a stream beside 0 (window draws), 1 (pi_and_v
 *   draws), 2 (Catch) and 3 (Breakout).
 * Done = game over; there are no lives, so no ARL_ENV_GAME_OVER_ONLY.
 * A step that serves -- a point, terminal or not, or the step cap -- writes
 * both frames of the pair as the first screen after the serve (Catch's rule:
 * a done observation is the first of the next episode).  Every other step
 * writes pair[0] = the screen after frame 4, pair[1] = the screen after frame
 * 3.  The reward is the raw +-1.0f or 0.0f.  steps_in_episode counts the
 * env-steps since the last done.
 * At points = 1 a uniform random policy scores about -0.37 and a game lasts
 * about 11 env-steps; at 21 about -17 and 230.
 *
 * Env state: caller-owned device memory, (2, n_envs, 12) int32, 16-byte
 * aligned, [bx, by, vx, vy, py, oy, serves, steps_in_episode, game,
 * game_steps, score_agent, score_opp] per env, double-buffered by the parity
 * of the observation index exactly as Catch's.
 *
 * The kind is ARL_ENV_PONG | ARL_ENV_PONG_POINTS(p), p in 1..21; p = 0 means
 * 21.  Any other bit (0x100 included): ARL_EINVAL.
 * Granular calls: Catch's trio; arl_pong_step takes points (1..21, anything
 * else: ARL_EINVAL) where arl_breakout_step takes its flags. */
#define ARL_ENV_PONG 4
#define ARL_ENV_PONG_POINTS(p) ((p) << 16)
int64_t arl_pong_state_bytes(int64_t n_envs);
int arl_pong_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int parity, uint8_t* pair_out,
                   float* reward_out, uint8_t* done_out, void* stream);
int arl_pong_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                  int points, uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* stream);

/* A device-resident T-maze, the fourth device environment: a cue-recall task,
 * with what the other three lack -- partial observability.  Catch, Breakout
 * and Pong can be read off the 4-observation stack, so the FF model does on
 * them whatever the LSTM does; here a cue is shown on an episode's first
 * screen only and has to be named L env-steps later, after it has left the
 * stack: the recurrent state has to carry it.  Same launch shape, pools and
 * state protocol as Catch; additions to ABI 4.
 *
 * The game (exact in integer arithmetic; tests/tmaze_ref.py restates it).
 * Screen 210 rows x 160 columns, RGB uint8, HWC, background (0,0,0).  L = the
 * corridor's length, 1..8.
 * Floor (84,84,84): rows 96..111, columns 0..16L+15.
 * Arms (84,84,84): rows 48..159, columns 16L..16L+15.
 * Agent (92,186,92): 8 x 8, rows 100..107, left edge ax.
 * Cue, 16 x 16, columns 0..15, drawn only on an episode's first screen:
 *   cue 0 ("up"): rows 72..87, colour (200,72,72);
 *   cue 1 ("down"): rows 120..135, colour (66,72,200).
 * Draw order: the agent over the floor over the background; the cue overlaps
 *   nothing.
 * Episode start: pos = 0, ax = 4, steps_in_episode = 0, and with (w0, ., ., .)
 *   = philox4x32_10(counter = (env_offset + e, episode, 0, 5), key = (seed &
 *   0xffffffff, seed >> 32)): cue = w0 & 1.  Counter word 3 = 5 is a stream
 *   beside 0 (window draws), 1 (pi_and_v draws), 2 (Catch), 3 (Breakout) and 4
 *   (Pong).  episode starts at 0 and advances at every terminal.
 * Actions: 2 = up, 3 = down, anything else is no choice (any n_actions >= 4).
 * One env-step with pos < L: four frames, each ax += 4; after the step
 *   pos += 1, so ax = 4 + 16 pos.  Reward 0, done 0.  pair[0] is the screen
 *   after frame 4 and pair[1] the screen after frame 3; neither shows the cue.
 *   The action is ignored.
 * One env-step with pos == L (the junction): reward +1 if the choice equals
 *   the cue, -1 if it is the other arm, 0.0 if no choice was made; done = 1 in
 *   all three cases.  The hits, misses and lapses counters advance,
 *   episode += 1, and the next episode starts at once: both frames of the pair
 *   are its first screen, with its cue (Catch's rule: the terminal screen is
 *   never shown).
 * So every episode lasts L + 1 env-steps and the optimum is +1.  A uniform
 * policy over A actions scores mean 0 with P(+1) = P(-1) = 1 / A, and any
 * policy whose action at the junction does not depend on the cue has expected
 * return exactly 0.  The cue leaves the 4-observation stack at observation 4,
 * so for L >= 4 the FF model's input at the junction is the same for both
 * cues.  With the default L = 4 an episode is exactly one t_max = 5 window.
 *
 * Env state: caller-owned device memory, (2, n_envs, 8) int32, 16-byte
 * aligned, [pos, cue, length, steps_in_episode, episode, hits, misses, lapses]
 * per env, double-buffered by the parity of the observation index exactly as
 * Catch's.  The reset stores L in the row; a step keeps the L of its call
 * there.
 *
 * The kind is ARL_ENV_TMAZE | ARL_ENV_TMAZE_LENGTH(l), l in 1..8; l = 0 means
 * 4.  Any other bit (0x100 included): ARL_EINVAL.
 * Granular calls: Catch's trio; arl_tmaze_reset and arl_tmaze_step take the
 * length (1..8, anything else: ARL_EINVAL), the same in both. */
#define ARL_ENV_TMAZE 8
#define ARL_ENV_TMAZE_LENGTH(l) ((l) << 16)
int64_t arl_tmaze_state_bytes(int64_t n_envs);
int arl_tmaze_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int length, int parity,
                    uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* stream);
int arl_tmaze_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                   int length, uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* stream);

/* A device-resident grid maze with procedurally generated levels, the fifth
 * device environment.  The other four are single tasks: a policy is trained on
 * the very episodes it is scored on.  Here the layout, the start and the goal
 * are drawn per episode from a numbered set of levels: levels = L trains on L
 * fixed tasks, levels = 0 draws from all of them, and the difference between
 * the two scores is a generalisation gap.  A view knob hides everything
 * outside a small window around the agent, which makes the same game an
 * exploration task under partial observability.  Same launch shape, pools and
 * state protocol as Catch; additions to ABI 4.
 *
 * The game (exact in integer arithmetic; tests/maze_ref.py restates it).
 * Screen 210 rows x 160 columns, RGB uint8, HWC, background (0,0,0).
 * Geometry: rooms = R in 2..4; the maze is G x G tiles, G = 2R + 1, a tile 16
 *   x 16 pixels: tile (ty, tx) covers rows 32 + 16 ty .. + 15 and columns
 *   16 tx .. + 15 (16 x 11 exceeds 160 columns, hence R <= 4).
 * Rooms and carving (a binary-tree maze): the rooms are the tiles (2i + 1,
 *   2j + 1), i, j in 0..R-1, i = 0 the top row.  Room (0, R-1) carves nothing;
 *   the other rooms of row 0 carve east; the other rooms of column R-1 carve
 *   north; every other room carves north if bit k = (i - 1)(R - 1) + j of
 *   `bits` is set, else east.  North opens tile (2i, 2j + 1), east opens tile
 *   (2i + 1, 2j + 2); everything else is wall.  That is 2 R^2 - 1 open tiles
 *   and a spanning tree of the rooms: every goal is reachable.
 * Level to task: with (w0, w1, w2, .) = philox4x32_10(counter = (level, 0, 1,
 *   6), key = (seed & 0xffffffff, seed >> 32)) and mulhi(a, b) = (uint64(a) *
 *   b) >> 32: bits = w0 & (2^((R-1)^2) - 1); start room s = mulhi(w1, R^2);
 *   goal room g = s + 1 + mulhi(w2, R^2 - 1), minus R^2 if that is >= R^2 (so
 *   g != s).  Room index = i R + j.
 * Episode to level: with w0 of philox4x32_10(counter = (env_offset + e,
 *   episode, 0, 6), same key): level = levels ? mulhi(w0, levels) : w0, levels
 *   in 0..1023.  Counter word 3 = 6 is a stream beside 0 (window draws), 1
 *   (pi_and_v draws), 2 (Catch), 3 (Breakout), 4 (Pong) and 5 (T-maze).
 *   episode starts at 0 and advances at every terminal.
 * Episode start: the agent on the start room's tile, steps_in_episode = 0.
 * Actions: a & 3: 0 up, 1 down, 2 right, 3 left (any n_actions >= 4).
 * One env-step: steps_in_episode += 1.  If the target tile is open the agent
 *   moves there in four frames of 4 px: pair[0] shows it on the target tile,
 *   pair[1] 4 px short of it.  If the target is a wall both screens show the
 *   unmoved agent.  If the agent is now on the goal: reward 1, done.  Else if
 *   steps_in_episode == 8R: reward 0, done.  On done, wins or timeouts
 *   advances, episode += 1, and the next episode starts at once: both frames
 *   of the pair are its first screen (Catch's rule: the terminal screen is
 *   never shown).
 * Drawing: open tile (40,40,40), wall tile (96,96,96), goal tile
 *   (236,236,120), agent (92,186,92): 8 x 8 at offset (4, 4) inside its tile,
 *   drawn over the tile.  view = V in 0..2; V = 0 shows the whole maze.  With
 *   V >= 1 a tile whose Chebyshev distance from the agent's tile after the
 *   step exceeds V is black on both screens of the pair, the goal's included;
 *   the agent is always drawn.
 * The longest shortest path from a start to a goal is 8R - 10 env-steps, so
 * every level is solvable within the cap of 8R and the optimum return is 1.
 *
 * Env state: caller-owned device memory, (2, n_envs, 8) int32, 16-byte
 * aligned, [pos | goal << 8, bits, steps_in_episode, episode, wins, timeouts,
 * level, cfg] per env, pos and goal as 16 ty + tx, double-buffered by the
 * parity of the observation index exactly as Catch's.  cfg = R | V << 3 |
 * levels << 5: the reset stores it in the row; a step keeps the one of its
 * call there.
 *
 * The kind is ARL_ENV_MAZE | ARL_ENV_MAZE_ROOMS(r) | ARL_ENV_MAZE_VIEW(v) |
 * ARL_ENV_MAZE_LEVELS(l): r in 2..4, r = 0 means 3; v in 0..2; l in 0..1023.
 * Any other bit (0x100 included), r = 1 or 5..7, v = 3: ARL_EINVAL.
 * Granular calls: Catch's trio; arl_maze_reset and arl_maze_step take rooms
 * (2..4), view (0..2) and levels (0..1023), anything else: ARL_EINVAL, the
 * same in both. */
#define ARL_ENV_MAZE 32
#define ARL_ENV_MAZE_ROOMS(r) ((r) << 16)
#define ARL_ENV_MAZE_VIEW(v) ((v) << 19)
#define ARL_ENV_MAZE_LEVELS(l) ((l) << 21)
int64_t arl_maze_state_bytes(int64_t n_envs);
int arl_maze_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int rooms, int view, int levels,
                   int parity, uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* stream);
int arl_maze_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                  int rooms, int view, int levels, uint8_t* pair_out, float* reward_out, uint8_t* done_out,
                  void* stream);

/* Attached to a net (host state of the handle, like arl_net_set_adam; works on
 * an unbound handle): arl_net_set_env(net, kind, state) with kind =
 * ARL_ENV_CATCH, ARL_ENV_BREAKOUT, ARL_ENV_BREAKOUT | ARL_ENV_GAME_OVER_ONLY,
 * ARL_ENV_PONG | ARL_ENV_PONG_POINTS(p), ARL_ENV_TMAZE |
 * ARL_ENV_TMAZE_LENGTH(l) or ARL_ENV_MAZE | ARL_ENV_MAZE_ROOMS(r) |
 * ARL_ENV_MAZE_VIEW(v) | ARL_ENV_MAZE_LEVELS(l)
 * (any other value, the flag on Catch included: ARL_EINVAL) and state as above
 * for that env, the net's n_envs, its env_offset and seed; state == NULL
 * detaches.  arl_env_reset, arl_env_step and arl_run_window launch the
 * attached kind.
 * Only frame-pair nets (FF, LSTM, FF_NATURE without the RGB / STACK / STATES
 * flags), else ARL_ESTATE; n_actions < 4 or a misaligned state: ARL_EINVAL.
 *
 * arl_env_reset: the reset into pool entry ctl[CTL_STEP] % pool_len and state
 * half ctl[CTL_STEP] & 1, both read on the device; the window that follows runs
 * with first != 0.  arl_env_step: steps envs [e0, e0 + ne) (the range rules of
 * arl_observe_envs, so env-group chains on several streams stay independent)
 * from row t of the workspace's "actions" buffer, 0 <= t < t_max, into entry
 * (k + 1) % pool_len, k = ctl[CTL_STEP] + t: what arl_observe(t + 1) reads.
 * While an env is attached, arl_run_window issues the step itself after each
 * arl_act(t), t < t_max (writing the pools it takes as const).  A captured
 * window keeps the env, and the flag, it was captured with.
 *
 * The pools are written here: all three are needed, each inside a registered
 * pool (arl_net_set_pool) with room for pool_len entries, and pool_len >= 2;
 * otherwise ARL_EINVAL before any launch.  ARL_ESTATE without an attached env
 * or on an unbound net.  With no env attached every other call makes exactly
 * the launches it made before, with the same arguments. */
int arl_net_set_env(arl_net* net, int kind, int32_t* state);
int arl_env_reset(arl_net* net, uint8_t* pair_pool, float* reward_pool, uint8_t* done_pool, int64_t pool_len,
                  void* stream);
int arl_env_step(arl_net* net, int t, int e0, int ne, uint8_t* pair_pool, float* reward_pool, uint8_t* done_pool,
                 int64_t pool_len, void* stream);

/* Direct-to-ring device env: the env-step and the observation that follows it
 * as ONE launch that never materialises the frame pair.  Every screen of the
 * five games is a function of the env's handful of integers, so the launch
 * evaluates arl_observe's arithmetic (max of the two screens, float64
 * luminance, the fixed-point resize of resize_mode) on bytes it produces in
 * registers and stores the 84 x 84 plane into the frame ring, with the
 * observation's bookkeeping (nvalid, reset flag, reward, done, episode
 * statistics) from the reward and done it just computed.  The ring, the
 * window buffers, the env state and everything downstream are bit for bit
 * what arl_env_step + arl_observe_envs leave; the pools do not exist.
 * Additions to ABI 4; opt-in, off by default: with it off every call makes
 * exactly the launches it made before, with the same arguments.
 *
 * arl_net_set_env_direct(net, on): host state of the handle.  on != 0 needs an
 * attached env (else ARL_ESTATE); a net with the RGB / STACK / STATES flag is
 * refused with ARL_ESTATE as arl_net_set_env refuses it.  Detaching the env
 * (arl_net_set_env(net, kind, NULL)) turns it off.
 *
 * arl_env_reset_observe(net, resize_mode, stream): arl_env_reset +
 * arl_observe(0, force_reset = 1) -- episode 0 of every env into state half
 * ctl[CTL_STEP] & 1, its first screen (as both frames) into ring slot
 * ctl[CTL_STEP] % R, nvalid 1, reset_flags[0] = 1, the running episode of the
 * episode statistics abandoned.
 * arl_env_step_observe(net, t, e0, ne, resize_mode, stream): arl_env_step(t) +
 * arl_observe_envs(t + 1) of envs [e0, e0 + ne) (arl_env_step's range rules):
 * from row t of the "actions" buffer and state half k & 1, k = ctl[CTL_STEP] +
 * t read on the device, into half (k + 1) & 1, ring slot (k + 1) % R,
 * rewards[t], dones[t], reset_flags[t + 1].  The reward stored is the raw one
 * (the learner clips).
 * Both: ARL_ESTATE on an unbound net, without an attached env or with direct
 * mode off; ARL_EINVAL for t outside [0, t_max), a bad range or a resize_mode
 * outside the four of arl_observe, before any launch.  Each launch is stamped
 * ARL_STAGE_PHI.
 *
 * arl_run_window with direct mode on ignores the three pools and pool_len
 * (NULL, 0 are fine) and issues act(t), step_observe(t) for t < t_max, then the
 * bootstrap act(t_max); with first != 0 the reset form goes first (no
 * arl_env_reset before it).  With direct mode off it is unchanged.
 *
 * arl_env_step_screen: the granular form, no net -- arl_<game>_step followed by
 * arl_current_screen on the pair it would have written: one env-step from
 * actions (n,) and half parity_in into half 1 - parity_in, screen_out (n, 84,
 * 84) uint8, the raw rewards (n,) and dones (n,).  kind as arl_net_set_env
 * takes it (Breakout's flag, Pong's points, the T-maze's length, the maze's fields).  n <=
 * 65535; ARL_EINVAL for an unknown kind, a parity other than 0 / 1, a bad
 * resize_mode, a null or misaligned pointer (state 16 bytes; screens,
 * rewards, actions 4). */
int arl_net_set_env_direct(arl_net* net, int on);
int arl_env_reset_observe(arl_net* net, int resize_mode, void* stream);
int arl_env_step_observe(arl_net* net, int t, int e0, int ne, int resize_mode, void* stream);
int arl_env_step_screen(int kind, int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset,
                        uint64_t seed, int resize_mode, uint8_t* screen_out, float* reward_out, uint8_t* done_out,
                        void* stream);

/* ------------------------------------------------------------------ granular ops */

/* RMSpropAsync.update_one (rmsprop_async.py:23-38) on flat f32 arrays, with
 * optional Chainer GradientClipping (norm over g, scale if clip/norm < 1).
 * norm_partials: device f64[1024] scratch (needed when clip > 0): the norm
 * pass's per-block partials. */
int arl_rmsprop(float* param, float* ms, const float* grad, int64_t n, double lr, double alpha, double eps,
                double clip, double* norm_partials, void* stream);

/* arl_rmsprop with NonbiasWeightDecay(weight_decay) on the whole array: after
 * the clip (norm of grad as given), g' = f32(g + f32(f32(weight_decay) *
 * param)) feeds update_one; grad itself is not written.  The reference's hook
 * loops over the arrays and skips the biases: pass 0 for a bias array (that is
 * arl_rmsprop).  weight_decay < 0 or not finite: ARL_EINVAL. */
int arl_rmsprop_wd(float* param, float* ms, const float* grad, int64_t n, double lr, double alpha, double eps,
                   double clip, double* norm_partials, double weight_decay, void* stream);

/* One Adam update (the arithmetic of arl_net_set_adam above) on flat f32
 * arrays, the counterpart of arl_rmsprop / arl_rmsprop_wd: param, m, v updated
 * from grad (read only) for update number t >= 1, which comes from the caller;
 * lr_t is computed on the host in double with the C library's pow / sqrt (what
 * Python uses), so it is bit-identical to the formula evaluated there.  clip,
 * norm_partials as arl_rmsprop; weight_decay as arl_rmsprop_wd (0: none).
 * t < 1, a beta outside [0, 1), a bad weight_decay: ARL_EINVAL. */
int arl_adam(float* param, float* m, float* v, const float* grad, int64_t n, double alpha, double beta1, double beta2,
             double eps, int64_t t, double clip, double* norm_partials, double weight_decay, void* stream);

/* SoftmaxPolicyOutput (policy_output.py:32-61) + FCSoftmaxPolicy / FCVFunction
 * heads (policy.py:53-58, v_function.py:29-34) for h: (n, 256) f32.  Samples
 * with Philox(seed; env_offset + row, step) when sample == 1 (step = *step_dev +
 * step_off); sample == 2 takes the first argmax (most_probable_actions);
 * sample == 0 writes no action. */
int arl_policy(const float* h, int64_t n, const float* W_pi, const float* b_pi, const float* W_v,
               const float* b_v, int n_actions, uint64_t seed, const int64_t* step_dev, int64_t step_off,
               int env_offset, int sample, float* logits, float* probs, float* log_probs, float* v,
               float* entropy, int32_t* actions, float* action_log_probs, void* stream);

/* a3c.py:82-126: returns + loss gradient over a (t_max, n) window. v, probs,
 * log_probs, actions are (t_max+1, n[, A]) with row t_max = bootstrap.
 * dones: bit 0 = the transition t -> t+1 ended the episode (R = 0), bit 1 =
 * step t is past the window's end (no loss).  loss: (n, 2) pi / v loss or
 * NULL. */
int arl_returns_lossgrad(const float* rewards, const uint8_t* dones, const float* v, const float* probs,
                         const float* log_probs, const int32_t* actions, int t_max, int64_t n, int n_actions,
                         double gamma, double beta, double pi_loss_coef, double v_loss_coef,
                         int keep_loss_scale_same, int clip_reward, float* dlogits, float* dv, float* loss,
                         void* stream);

/* arl_returns_lossgrad with the GAE(lambda) advantage in the policy term
 * (arl_net_set_gae has the definition); lambda == 1 launches
 * arl_returns_lossgrad's kernel with its arguments.  lambda outside [0, 1] or
 * not finite: ARL_EINVAL.  Addition to ABI 4. */
int arl_returns_lossgrad_gae(const float* rewards, const uint8_t* dones, const float* v, const float* probs,
                             const float* log_probs, const int32_t* actions, int t_max, int64_t n, int n_actions,
                             double gamma, double lambda, double beta, double pi_loss_coef, double v_loss_coef,
                             int keep_loss_scale_same, int clip_reward, float* dlogits, float* dv, float* loss,
                             void* stream);

/* The snapshot of arl_ppo_begin on explicit arrays (arl_net_set_ppo has the
 * definition): rewards, dones (t_max, n); v (t_max + 1, n), log_probs and
 * actions (t_max + 1, n[, A]) with row t_max = bootstrap; logp_old, adv, ret
 * (t_max, n) out.  lambda == 1: the n-step advantage.  t_max <= 256.
 * Addition to ABI 4. */
int arl_ppo_snapshot(const float* rewards, const uint8_t* dones, const float* v, const float* log_probs,
                     const int32_t* actions, int t_max, int64_t n, int n_actions, double gamma, double lambda,
                     int clip_reward, float* logp_old, float* adv, float* ret, void* stream);

/* The loss gradient of one PPO epoch on explicit arrays (arl_net_set_ppo has
 * the definition), the counterpart of arl_returns_lossgrad: v, probs,
 * log_probs, actions as there (the current policy's), logp_old / adv / ret the
 * snapshot.  loss: (n, 2) or NULL; ratio_out: (t_max, n) or NULL.  clip_eps
 * not finite or outside (0, 1): ARL_EINVAL.  Addition to ABI 4. */
int arl_ppo_lossgrad(const uint8_t* dones, const float* v, const float* probs, const float* log_probs,
                     const int32_t* actions, const float* logp_old, const float* adv, const float* ret, int t_max,
                     int64_t n, int n_actions, double clip_eps, double beta, double pi_loss_coef, double v_loss_coef,
                     int keep_loss_scale_same, float* dlogits, float* dv, float* loss, float* ratio_out,
                     void* stream);

/* arl_ppo_lossgrad with the clipped value loss (arl_net_set_ppo_options has the
 * definition).  The two added arguments stand beside their kin: v_old (t_max, n)
 * closes the snapshot's planes, after ret; vclip_eps follows clip_eps.  vclip_eps
 * not finite or <= 0, a NULL v_old: ARL_EINVAL.  Addition to ABI 4. */
int arl_ppo_lossgrad_vclip(const uint8_t* dones, const float* v, const float* probs, const float* log_probs,
                           const int32_t* actions, const float* logp_old, const float* adv, const float* ret,
                           const float* v_old, int t_max, int64_t n, int n_actions, double clip_eps,
                           double vclip_eps, double beta, double pi_loss_coef, double v_loss_coef,
                           int keep_loss_scale_same, float* dlogits, float* dv, float* loss, float* ratio_out,
                           void* stream);

/* The advantage normalisation of arl_ppo_begin on explicit arrays
 * (arl_net_set_ppo_options has the definition): adv (t_max, n) in place,
 * moments3_device = (n_live, mean, std), 3 doubles on the device.  One workgroup.
 * t_max <= 256; n == 0 returns ARL_OK without a launch.  Addition to ABI 4. */
int arl_ppo_normalize_adv(const uint8_t* dones, float* adv, int t_max, int64_t n, double* moments3_device,
                          void* stream);

/* One epoch's record on explicit arrays (arl_net_set_ppo_options has the fields):
 * v, log_probs, actions the current policy's (rows 0 .. t_max - 1 are read),
 * logp_old / adv / ret / ratio the snapshot's planes after arl_ppo_lossgrad,
 * v_old or NULL (then vclip_eps is not read and vclipped = 0); window and epoch
 * are stored as given; record10_device: ARL_PPO_STAT_FIELDS doubles on the device.
 * One workgroup.  t_max <= 256, n_actions <= 32; n == 0 returns ARL_OK without a
 * launch.  Addition to ABI 4. */
int arl_ppo_epoch_stats(const uint8_t* dones, const float* v, const float* log_probs, const int32_t* actions,
                        const float* logp_old, const float* adv, const float* ret, const float* ratio,
                        const float* v_old, int t_max, int64_t n, int n_actions, double clip_eps, double vclip_eps,
                        double window, double epoch, double* record10_device, void* stream);

/* ------------------------------------------------------------------ measurement */

/* Device-to-device copy of `bytes` (a multiple of 16, 16-byte aligned
 * buffers) by a grid of `blocks` 256-thread workgroups, 16-byte loads: the HBM
 * stream-copy peak the bench reports beside the 8 TB/s spec (SURVEY 8(d);
 * no reference counterpart).  mode 0: grid-stride, 4 loads in flight per lane;
 * mode 1: 64 KB blocks per workgroup, 16 non-temporal loads in flight per lane;
 * mode 2 / 3: a one-shot grid of bytes / 4 KB workgroups (`blocks` ignored), one
 * 16-byte load and store per lane (3: non-temporal). */
int arl_stream_copy(const void* src, void* dst, int64_t bytes, int blocks, int mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ASYNCRL_HIP_H */
