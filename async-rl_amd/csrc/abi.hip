// C ABI of libasyncrl_hip.so (declared in include/asyncrl_hip.h).
// Argument validation lives here; kernels assume validated shapes.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <string.h>

#include <initializer_list>
#include <string>

#include "../../include/asyncrl_hip.h"
#include "arl_internal.hpp"

struct arl_net {
  arl::Net net;
  bool bound = false;
  struct Pool {
    uintptr_t base = 0;
    int64_t bytes = 0;
  };
  Pool pools[3][8];   // registered input pools per kind (arl_net_set_pool)
};

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int hip_status(hipError_t e, const char* what) {
  if (e == hipSuccess) return ARL_OK;
  return fail(ARL_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
// a weight-decay rate the update can take: >= 0 (not NaN) and finite as f32
bool decay_rate_ok(double rate) { return rate >= 0.0 && rate <= (double)FLT_MAX; }
}  // namespace

extern "C" {

int arl_abi_version(void) { return ARL_ABI_VERSION; }
const char* arl_last_error(void) { return g_err.c_str(); }

int arl_current_screen(const uint8_t* cur, const uint8_t* prev, uint8_t* out, int64_t n, int mode, void* s) {
  if (n < 0 || (n > 0 && (!cur || !prev || !out))) return fail(ARL_EINVAL, "current_screen: null pointer / n < 0");
  if (!aligned(cur, 16) || !aligned(prev, 16) || !aligned(out, 4))
    return fail(ARL_EINVAL, "current_screen: frames must be 16-byte aligned, out 4-byte aligned");
  if (mode < 0 || mode > (ARL_RESIZE_SIMD | ARL_RESIZE_CROP)) return fail(ARL_EINVAL, "bad resize_mode");
  if (n > 65535) return fail(ARL_EINVAL, "current_screen: n > 65535 per call");
  return hip_status(arl::launch_current_screen(cur, prev, out, n, mode, S(s)), "current_screen");
}

int arl_max_luminance(const uint8_t* cur, const uint8_t* prev, uint8_t* gray, int64_t npix, void* s) {
  if (npix < 0 || (npix > 0 && (!cur || !prev || !gray))) return fail(ARL_EINVAL, "max_luminance: null / npix < 0");
  if (npix > ((int64_t)1 << 31) * 255) return fail(ARL_EINVAL, "max_luminance: npix too large");
  return hip_status(arl::launch_max_luminance(cur, prev, gray, npix, S(s)), "max_luminance");
}

int arl_phi_stack(const uint8_t* pairs, const uint8_t* prev_stack, const uint8_t* reset, uint8_t* out_stack,
                  int64_t n, int mode, void* s) {
  if (n < 0 || (n > 0 && (!pairs || !prev_stack || !out_stack)))
    return fail(ARL_EINVAL, "phi_stack: null pointer / n < 0");
  if (!aligned(pairs, 16) || !aligned(prev_stack, 16) || !aligned(out_stack, 16))
    return fail(ARL_EINVAL, "phi_stack: buffers must be 16-byte aligned");
  if (prev_stack == out_stack && n > 0) return fail(ARL_EINVAL, "phi_stack: prev_stack and out_stack alias");
  if (mode < 0 || mode > (ARL_RESIZE_SIMD | ARL_RESIZE_CROP)) return fail(ARL_EINVAL, "bad resize_mode");
  if (n > 65535) return fail(ARL_EINVAL, "phi_stack: n > 65535 per call");
  return hip_status(arl::launch_phi_stack(pairs, prev_stack, reset, out_stack, n, mode, S(s)), "phi_stack");
}

int arl_dqn_phi(const uint8_t* in, float* out, int64_t n, void* s) {
  if (n < 0 || (n > 0 && (!in || !out))) return fail(ARL_EINVAL, "dqn_phi: null pointer / n < 0");
  if (!aligned(in, 4) || !aligned(out, 16)) return fail(ARL_EINVAL, "dqn_phi: in 4-byte, out 16-byte aligned");
  return hip_status(arl::launch_dqn_phi(in, out, n * 4 * arl::PLANE, S(s)), "dqn_phi");
}

static int check_rgb_dims(int H, int W) {
  if (H < 2 || W < 16 || W % 16 != 0 || W > arl::RGB_MAX_W || H > 65535)
    return fail(ARL_EINVAL, "rgb: need H >= 2, W % 16 == 0, 16 <= W <= 2048");
  return ARL_OK;
}

int arl_rgb_phi(const uint8_t* imgs, int64_t n, int H, int W, float* out, int mode, void* s) {
  if (n < 0 || (n > 0 && (!imgs || !out))) return fail(ARL_EINVAL, "rgb_phi: null pointer / n < 0");
  if (int rc = check_rgb_dims(H, W)) return rc;
  if (n > 65535) return fail(ARL_EINVAL, "rgb_phi: n > 65535");
  if (!aligned(imgs, 16) || !aligned(out, 16)) return fail(ARL_EINVAL, "rgb_phi: 16-byte alignment");
  if (mode < 0 || mode > ARL_RESIZE_SIMD) return fail(ARL_EINVAL, "rgb_phi: resize_mode must be 0 or 1");
  return hip_status(arl::launch_rgb_phi(imgs, n, H, W, out, mode, S(s)), "rgb_phi");
}

int arl_net_create(arl_net** out, int arch, int n_actions, int n_envs, int t_max, int env_offset, uint64_t seed) {
  if (!out) return fail(ARL_EINVAL, "net_create: out is null");
  arl_net* h = new arl_net();
  std::string err;
  if (!arl::net_init(h->net, arch, n_actions, n_envs, t_max, env_offset, seed, err)) {
    delete h;
    return fail(ARL_EINVAL, "net_create: " + err);
  }
  *out = h;
  return ARL_OK;
}

void arl_net_destroy(arl_net* h) {
  if (h && h->net.stamps) {
    for (hipEvent_t e : h->net.stamps->ev) (void)hipEventDestroy(e);
    delete h->net.stamps;
  }
  delete h;
}

int64_t arl_net_param_floats(const arl_net* h) { return h ? h->net.param_floats : -1; }
int arl_net_param_count(const arl_net* h) { return h ? (int)h->net.params.size() : -1; }

int arl_net_param_info(const arl_net* h, int idx, int64_t* offset, int64_t* numel, char* name, int cap) {
  if (!h || idx < 0 || idx >= (int)h->net.params.size()) return fail(ARL_EINVAL, "param_info: bad index");
  const arl::ParamInfo& p = h->net.params[idx];
  if (offset) *offset = p.offset;
  if (numel) *numel = p.numel;
  if (name && cap > 0) {
    strncpy(name, p.name.c_str(), (size_t)cap - 1);
    name[cap - 1] = 0;
  }
  return ARL_OK;
}

int64_t arl_net_workspace_bytes(const arl_net* h) { return h ? h->net.ws_bytes : -1; }

int arl_net_buffer(const arl_net* h, const char* name, int64_t* offset, int64_t* bytes) {
  if (!h || !name) return fail(ARL_EINVAL, "net_buffer: null");
  for (const auto& b : h->net.bufs)
    if (strcmp(b.name, name) == 0) {
      if (offset) *offset = b.off;
      if (bytes) *bytes = b.bytes;
      return ARL_OK;
    }
  return fail(ARL_EINVAL, std::string("net_buffer: unknown buffer ") + name);
}

int arl_net_bind(arl_net* h, float* params, float* grads, float* ms, void* ws) {
  if (!h || !params || !grads || !ms || !ws) return fail(ARL_EINVAL, "net_bind: null pointer");
  if (!aligned(params, 16) || !aligned(grads, 16) || !aligned(ms, 16) || !aligned(ws, 256))
    return fail(ARL_EINVAL, "net_bind: params/grads/ms 16-byte aligned, workspace 256-byte aligned");
  h->net.p = params;
  h->net.g = grads;
  h->net.ms = ms;
  h->net.ws = reinterpret_cast<char*>(ws);
  ++h->net.param_gen;   // new parameter memory: derived state (the FC planes) is stale
  h->bound = true;
  return ARL_OK;
}

int arl_net_params_changed(arl_net* h) {
  if (!h) return fail(ARL_EINVAL, "null net");
  ++h->net.param_gen;
  return ARL_OK;
}

int arl_net_param_generation(const arl_net* h, uint64_t* param_gen, uint64_t* planes_gen) {
  if (!h) return fail(ARL_EINVAL, "null net");
  if (param_gen) *param_gen = h->net.param_gen;
  if (planes_gen) *planes_gen = h->net.planes_gen;
  return ARL_OK;
}

#define NEED_BOUND(h)                                                         \
  do {                                                                        \
    if (!(h)) return fail(ARL_EINVAL, "null net");                            \
    if (!(h)->bound) return fail(ARL_ESTATE, "net not bound (arl_net_bind)"); \
  } while (0)

int arl_net_prepare(arl_net* h, void* s) {
  NEED_BOUND(h);
  return hip_status(arl::ensure_fc_planes(h->net, S(s)), "net_prepare");
}

// win_log and win_count (adjacent 256-byte aligned buffers: one memset through the padding between them)
static hipError_t window_stats_zero(arl::Net& n, hipStream_t s) {
  return hipMemsetAsync(n.ws + n.w_win_log, 0, (size_t)(n.w_win_count + 8 - n.w_win_log), s);
}

int arl_net_reset(arl_net* h, void* s) {
  NEED_BOUND(h);
  arl::Net& n = h->net;
  hipError_t e = hipMemsetAsync(n.ws + n.w_ctl, 0, arl::CTL_SIZE * 8, S(s));
  if (e == hipSuccess) e = hipMemsetAsync(n.ws + n.w_nvalid, 0, (size_t)n.R * n.N, S(s));
  if (e == hipSuccess) e = hipMemsetAsync(n.ws + n.w_reset, 1, (size_t)(n.T + 1) * n.N, S(s));
  if (e == hipSuccess) e = hipMemsetAsync(n.ws + n.w_tick, 0, (size_t)arl::fc_fwd_tiles(n.N) * 4, S(s));
  if (e == hipSuccess) e = hipMemsetAsync(n.ws + n.w_norm, 0, (size_t)arl::NORM_SCRATCH * 8, S(s));
  if (e == hipSuccess && n.w_fcb_tick)
    e = hipMemsetAsync(n.ws + n.w_fcb_tick, 0, (size_t)arl::fc_bwd_tickets() * 4, S(s));
  n.returns_done = false;
  n.ppo_begun = false;
  if (e == hipSuccess && n.arch == arl::ARCH_LSTM) {
    e = hipMemsetAsync(n.ws + n.w_hbuf, 0, (size_t)(n.T + 2) * n.N * arl::HID * 4, S(s));
    if (e == hipSuccess) e = hipMemsetAsync(n.ws + n.w_cbuf, 0, (size_t)(n.T + 2) * n.N * arl::HID * 4, S(s));
    if (e == hipSuccess) e = hipMemsetAsync(n.ws + n.w_eval_reset, 1, (size_t)n.N, S(s));
    if (e == hipSuccess) e = hipMemsetAsync(n.ws + n.w_zero, 0, arl::ZERO_ROW_FLOATS * 4, S(s));
  }
  if (e == hipSuccess) e = arl::launch_episode_reset(n.ws + n.w_episodes, n.N, S(s));
  if (e == hipSuccess) e = window_stats_zero(n, S(s));
  return hip_status(e, "net_reset");
}

static_assert(arl::EPISODE_LOG == ARL_EPISODE_LOG, "episode log depth");

int arl_net_set_episode_stats(arl_net* h, int on) {
  NEED_BOUND(h);
  h->net.episode_stats = on != 0;
  return ARL_OK;
}

int arl_episode_stats_reset(arl_net* h, void* s) {
  NEED_BOUND(h);
  arl::Net& n = h->net;
  return hip_status(arl::launch_episode_reset(n.ws + n.w_episodes, n.N, S(s)), "episode_stats_reset");
}

int arl_episode_stats(arl_net* h, double* out8_device, int clear, void* s) {
  NEED_BOUND(h);
  arl::Net& n = h->net;
  if (!n.episode_stats) return fail(ARL_ESTATE, "episode_stats: the feature is off (arl_net_set_episode_stats)");
  if (!out8_device || !aligned(out8_device, 8)) return fail(ARL_EINVAL, "episode_stats: out8 null / not 8-byte aligned");
  return hip_status(arl::launch_episode_reduce(n.ws + n.w_episodes, n.N, out8_device, clear ? 1 : 0, S(s)),
                    "episode_stats");
}

static_assert(arl::WINDOW_LOG == ARL_WINDOW_LOG && arl::WINDOW_STAT_FIELDS == ARL_WINDOW_STAT_FIELDS,
              "window statistics record");

int arl_net_set_window_stats(arl_net* h, int on) {
  NEED_BOUND(h);
  h->net.window_stats = on != 0;
  return ARL_OK;
}

int arl_window_stats_reset(arl_net* h, void* s) {
  NEED_BOUND(h);
  return hip_status(window_stats_zero(h->net, S(s)), "window_stats_reset");
}

int arl_net_set_pool(arl_net* h, int kind, const void* pool, int64_t bytes) {
  if (!h) return fail(ARL_EINVAL, "null net");
  if (kind < ARL_POOL_FRAMES || kind > ARL_POOL_DONES) return fail(ARL_EINVAL, "set_pool: unknown pool kind");
  if (!pool || bytes < 0) return fail(ARL_EINVAL, "set_pool: null pool / bytes < 0");
  const uintptr_t b = reinterpret_cast<uintptr_t>(pool);
  arl_net::Pool* tab = h->pools[kind];
  int slot = -1;
  for (int i = 0; i < 8; ++i)
    if (tab[i].base == b) slot = i;
  if (slot < 0) {   // a free slot, else replace the oldest registration (slots shift down)
    for (int i = 0; i < 8 && slot < 0; ++i)
      if (tab[i].bytes == 0) slot = i;
    if (slot < 0) {
      for (int i = 0; i < 7; ++i) tab[i] = tab[i + 1];
      slot = 7;
    }
  }
  tab[slot].base = bytes > 0 ? b : 0;
  tab[slot].bytes = bytes;
  // a registration overlapping the new one belongs to memory that was freed and reused: drop it
  for (int i = 0; i < 8 && bytes > 0; ++i)
    if (i != slot && tab[i].bytes > 0 && tab[i].base < b + (uintptr_t)bytes && b < tab[i].base + (uintptr_t)tab[i].bytes)
      tab[i] = arl_net::Pool{};
  return ARL_OK;
}

// a non-null pool must lie inside a registered pool of its kind with pool_len * rows * unit bytes
// before that pool's end (0 = ok)
static int check_pool(const arl_net* h, int kind, const void* pool, int64_t pool_len, int64_t unit, const char* what) {
  if (!pool) return 0;
  const uintptr_t p = reinterpret_cast<uintptr_t>(pool);
  // the registration with the greatest base <= p whose range holds p: a stale, larger registration of a
  // freed pool that also spans p never lends its room to a newer pool allocated inside it
  const arl_net::Pool* best = nullptr;
  for (const arl_net::Pool& r : h->pools[kind]) {
    if (r.bytes <= 0 || p < r.base || p >= r.base + (uintptr_t)r.bytes) continue;
    if (!best || r.base > best->base) best = &r;
  }
  if (!best) return fail(ARL_EINVAL, std::string("observe: the ") + what + " pool is not registered (arl_net_set_pool)");
  const int64_t room = (int64_t)(best->base + (uintptr_t)best->bytes - p);
  if (unit > 0 && pool_len > room / unit)
    return fail(ARL_EINVAL, std::string("observe: pool_len ") + std::to_string(pool_len) + " exceeds the " + what +
                                " pool (" + std::to_string(room / unit) + " entries registered)");
  return 0;
}

// validates an observation and fills its ring arguments (0 = ok)
static int ring_args(arl_net* h, int t, const uint8_t* pool, const float* reward_pool, const uint8_t* done_pool,
                     int64_t pool_len, int force_reset, int mode, int H, int W, int e0, int ne, arl::RingArgs& a) {
  arl::Net& n = h->net;
  if (t < 0 || t > n.T) return fail(ARL_EINVAL, "observe: t out of [0, t_max]");
  if ((!pool && n.layout != arl::FRAMES_STACK && n.layout != arl::FRAMES_STATES) || pool_len < 1)
    return fail(ARL_EINVAL, "observe: need the frame pool and pool_len >= 1");
  if (!aligned(pool, 16)) return fail(ARL_EINVAL, "observe: the frame pool must be 16-byte aligned");
  if (n.N > 65535) return fail(ARL_EINVAL, "observe: n_envs > 65535");
  const int64_t frame_unit = n.layout == arl::FRAMES_RGB ? (int64_t)H * W * 3
                             : n.layout == arl::FRAMES_STACK ? 4 * arl::PLANE
                             : n.layout == arl::FRAMES_STATES ? 16 * arl::PLANE
                                                             : arl::PAIR;
  if (int rc = check_pool(h, ARL_POOL_FRAMES, pool, pool_len, frame_unit * n.N, "frame")) return rc;
  if (int rc = check_pool(h, ARL_POOL_REWARDS, reward_pool, pool_len, 4 * (int64_t)n.N, "reward")) return rc;
  if (int rc = check_pool(h, ARL_POOL_DONES, done_pool, pool_len, (int64_t)n.N, "done")) return rc;
  a.pair_pool = pool;
  a.reward_pool = reward_pool;
  a.done_pool = done_pool;
  a.pool_len = pool_len;
  // the kernels reduce the step counter by pool_len through these constants (divisors below 2^31); without
  // any pool (a bookkeeping-only stack observation) no pool entry is read and the divisor is immaterial
  const bool any_pool = pool || reward_pool || done_pool;
  if (any_pool && pool_len > INT32_MAX) return fail(ARL_EINVAL, "observe: pool_len above 2^31 - 1");
  a.dpool = arl::fd_make(any_pool ? (uint32_t)pool_len : 1u);
  a.dR = n.dR;
  a.frames = n.at<uint8_t>(n.w_frames);
  a.nvalid = n.at<uint8_t>(n.w_nvalid);
  a.reset_flags = n.at<uint8_t>(n.w_reset);
  a.rewards = n.at<float>(n.w_rewards);
  a.dones = n.at<uint8_t>(n.w_dones);
  a.ctl = n.at<int64_t>(n.w_ctl);
  a.n = n.N;
  a.R = n.R;
  a.t = t;
  a.mode = mode;
  a.force_reset = force_reset ? 1 : 0;
  a.H = H;
  a.W = W;
  a.e0 = e0;
  a.ne = ne;
  a.esize = n.layout == arl::FRAMES_STATES ? 4 : 1;
  a.episodes = n.episode_stats ? n.ws + n.w_episodes : nullptr;
  return 0;
}

static int observe_common(arl_net* h, int t, const uint8_t* pool, const float* reward_pool,
                          const uint8_t* done_pool, int64_t pool_len, int force_reset, int mode, int H, int W,
                          void* s, int e0 = 0, int ne = -1) {
  arl::RingArgs a;
  if (int rc = ring_args(h, t, pool, reward_pool, done_pool, pool_len, force_reset, mode, H, W, e0, ne, a)) return rc;
  const arl::Net& n = h->net;
  hipError_t e = n.layout == arl::FRAMES_RGB ? arl::launch_rgb_ring(a, S(s))
                 : (n.layout == arl::FRAMES_STACK || n.layout == arl::FRAMES_STATES) ? arl::launch_stack_ring(a, S(s))
                                                                                    : arl::launch_phi_ring(a, S(s));
  if (e == hipSuccess) e = arl::stamp(n, arl::STAGE_PHI, S(s));
  return hip_status(e, "observe");
}

int arl_observe(arl_net* h, int t, const uint8_t* pair_pool, const float* reward_pool, const uint8_t* done_pool,
                int64_t pool_len, int force_reset, int mode, void* s) {
  NEED_BOUND(h);
  if (h->net.rgb) return fail(ARL_ESTATE, "observe: RGB net, use arl_observe_rgb");
  if (h->net.stack) return fail(ARL_ESTATE, "observe: ARL_ARCH_STACK net, use arl_observe_stack");
  if (h->net.states) return fail(ARL_ESTATE, "observe: ARL_ARCH_STATES net, use arl_observe_states");
  if (mode < 0 || mode > (ARL_RESIZE_SIMD | ARL_RESIZE_CROP)) return fail(ARL_EINVAL, "bad resize_mode");
  return observe_common(h, t, pair_pool, reward_pool, done_pool, pool_len, force_reset, mode, 0, 0, s);
}

int arl_observe_rgb(arl_net* h, int t, const uint8_t* img_pool, int H, int W, const float* reward_pool,
                    const uint8_t* done_pool, int64_t pool_len, int force_reset, int mode, void* s) {
  NEED_BOUND(h);
  if (!h->net.rgb) return fail(ARL_ESTATE, "observe_rgb: net was not created with ARL_ARCH_RGB");
  if (mode < 0 || mode > ARL_RESIZE_SIMD) return fail(ARL_EINVAL, "observe_rgb: resize_mode must be 0 or 1");
  if (int rc = check_rgb_dims(H, W)) return rc;
  return observe_common(h, t, img_pool, reward_pool, done_pool, pool_len, force_reset, mode, H, W, s);
}

int arl_observe_stack(arl_net* h, int t, const uint8_t* stack_pool, const float* reward_pool,
                      const uint8_t* done_pool, int64_t pool_len, int force_reset, void* s) {
  NEED_BOUND(h);
  if (!h->net.stack) return fail(ARL_ESTATE, "observe_stack: net was not created with ARL_ARCH_STACK");
  if (!stack_pool && t < 1) return fail(ARL_EINVAL, "observe_stack: a frameless observation needs t >= 1");
  return observe_common(h, t, stack_pool, reward_pool, done_pool, pool_len, force_reset, 0, 0, 0, s);
}

int arl_observe_states(arl_net* h, int t, const float* state_pool, const float* reward_pool,
                       const uint8_t* done_pool, int64_t pool_len, int force_reset, void* s) {
  NEED_BOUND(h);
  if (!h->net.states) return fail(ARL_ESTATE, "observe_states: net was not created with ARL_ARCH_STATES");
  if (!state_pool && t < 1) return fail(ARL_EINVAL, "observe_states: a stateless observation needs t >= 1");
  return observe_common(h, t, reinterpret_cast<const uint8_t*>(state_pool), reward_pool, done_pool, pool_len,
                        force_reset, 0, 0, 0, s);
}

int arl_truncate_window(arl_net* h, int t_len, void* s) {
  NEED_BOUND(h);
  arl::Net& n = h->net;
  if (t_len < 1 || t_len > n.T) return fail(ARL_EINVAL, "truncate_window: t_len out of [1, t_max]");
  n.returns_done = false;   // a truncated window's learn runs its own returns
  if (t_len == n.T) return ARL_OK;
  const size_t rows = (size_t)(n.T - t_len) * n.N;
  hipError_t e = hipMemsetAsync(n.ws + n.w_dones + (size_t)t_len * n.N, 2, rows, S(s));
  if (e == hipSuccess) e = hipMemsetAsync(n.ws + n.w_rewards + (size_t)t_len * n.N * 4, 0, rows * 4, S(s));
  return hip_status(e, "truncate_window");
}

int arl_net_set_norm_fold(arl_net* h, int on) {
  if (!h) return fail(ARL_EINVAL, "null net");
  h->net.norm_fold = on != 0;
  h->net.norm_ready = false;
  return ARL_OK;
}

// the net's field of an ARL_FORM_* id (null: unknown) and its smallest concrete value (the other is lo + 1)
static int* form_field(arl::Forms& f, int form, int* lo, const char** name) {
  switch (form) {
    case ARL_FORM_CONV_EPW: *lo = 1; *name = "ARL_FORM_CONV_EPW"; return &f.conv_epw;
    case ARL_FORM_FC_BIG: *lo = 0; *name = "ARL_FORM_FC_BIG"; return &f.fc_big;
    case ARL_FORM_LSTM_XRED: *lo = 0; *name = "ARL_FORM_LSTM_XRED"; return &f.lstm_xred;
    case ARL_FORM_CONV_BWD_WS: *lo = 0; *name = "ARL_FORM_CONV_BWD_WS"; return &f.conv_bwd_ws;
  }
  return nullptr;
}

int arl_net_set_form(arl_net* h, int form, int value) {
  if (!h) return fail(ARL_EINVAL, "null net");
  int lo = 0;
  const char* name = nullptr;
  int* field = form_field(h->net.forms, form, &lo, &name);
  if (!field) return fail(ARL_EINVAL, "net_set_form: unknown form " + std::to_string(form));
  if (value != ARL_FORM_AUTO && value != lo && value != lo + 1)
    return fail(ARL_EINVAL, std::string("net_set_form: ") + name + " takes ARL_FORM_AUTO, " + std::to_string(lo) +
                                " or " + std::to_string(lo + 1) + ", not " + std::to_string(value));
  *field = value;
  return ARL_OK;
}

int arl_net_form(const arl_net* h, int form, int launch_envs, int* value) {
  if (!h || !value) return fail(ARL_EINVAL, "net_form: null net / value");
  if (launch_envs < 1) return fail(ARL_EINVAL, "net_form: launch_envs < 1");
  const arl::Forms& f = h->net.forms;
  switch (form) {
    case ARL_FORM_CONV_EPW: *value = arl::conv_fwd_epw(f, h->net.N); return ARL_OK;
    case ARL_FORM_FC_BIG: *value = arl::fc_fwd_big(f, launch_envs); return ARL_OK;
    case ARL_FORM_LSTM_XRED: *value = arl::lstm_xred(f, launch_envs); return ARL_OK;
    case ARL_FORM_CONV_BWD_WS: *value = arl::conv_bwd_ws(f); return ARL_OK;
  }
  return fail(ARL_EINVAL, "net_form: unknown form " + std::to_string(form));
}

int arl_net_set_returns_fusion(arl_net* h, int on, double gamma, double beta, double v_loss_coef, int clip_reward) {
  if (!h) return fail(ARL_EINVAL, "null net");
  arl::Net& n = h->net;
  n.fuse_returns = on != 0 && n.arch == arl::ARCH_FF;
  if (on) {   // (turning it off keeps returns_done: the window's learn still skips what the act ran)
    n.returns_done = false;
    n.ret = arl::Net::ReturnsCfg{gamma, (float)beta, (float)v_loss_coef, clip_reward};
  }
  return ARL_OK;
}

int arl_net_set_loss(arl_net* h, double pi_loss_coef, int keep_loss_scale_same) {
  if (!h) return fail(ARL_EINVAL, "null net");
  h->net.pi_coef = (float)pi_loss_coef;
  h->net.keep_scale = keep_loss_scale_same ? 1 : 0;
  return ARL_OK;
}

int arl_net_set_weight_decay(arl_net* h, double rate) {
  if (!h) return fail(ARL_EINVAL, "null net");
  if (!decay_rate_ok(rate)) return fail(ARL_EINVAL, "set_weight_decay: rate must be finite and >= 0");
  h->net.decay.rate = (float)rate;
  return ARL_OK;
}

static_assert(arl::CTL_ADAM_T == ARL_CTL_ADAM_T, "control block layout");
static bool adam_beta_ok(double b) { return b >= 0.0 && b < 1.0; }   // (nan fails both)

int arl_net_set_adam(arl_net* h, float* m, double beta1, double beta2) {
  if (!h) return fail(ARL_EINVAL, "null net");
  if (!m) {   // back to RMSpropAsync
    h->net.adam_m = nullptr;
    return ARL_OK;
  }
  if (!aligned(m, 16)) return fail(ARL_EINVAL, "set_adam: m must be 16-byte aligned");
  if (!adam_beta_ok(beta1) || !adam_beta_ok(beta2)) return fail(ARL_EINVAL, "set_adam: beta1 and beta2 must be in [0, 1)");
  h->net.adam_m = m;
  h->net.adam_beta1 = beta1;
  h->net.adam_beta2 = beta2;
  return ARL_OK;
}

int arl_net_set_adam_t(arl_net* h, int64_t t, void* s) {
  NEED_BOUND(h);
  if (t < 0) return fail(ARL_EINVAL, "set_adam_t: t < 0");
  return hip_status(arl::launch_ctl_write(h->net.at<int64_t>(h->net.w_ctl), arl::CTL_ADAM_T, t, S(s)), "set_adam_t");
}

static bool gae_lambda_ok(double lambda) { return lambda >= 0.0 && lambda <= 1.0; }   // (nan fails both)

int arl_net_set_gae(arl_net* h, double lambda) {
  if (!h) return fail(ARL_EINVAL, "null net");
  if (!gae_lambda_ok(lambda)) return fail(ARL_EINVAL, "set_gae: lambda must be finite and in [0, 1]");
  h->net.gae_lambda = lambda;
  return ARL_OK;
}

// the nets that run PPO epochs: FF with the NIPS head; the LSTM once it has a carry buffer (arl_net_set_ppo_state)
static bool ppo_arch_ok(const arl::Net& n) {
  return n.arch == arl::ARCH_FF || (n.arch == arl::ARCH_LSTM && n.ppo_carry != nullptr);
}
static const char* const PPO_ARCH_REFUSAL =
    "FF nets with the NIPS head only (the LSTM needs a carry buffer first, arl_net_set_ppo_state; not the Nature head)";

int arl_net_set_ppo_state(arl_net* h, float* carry) {
  if (!h) return fail(ARL_EINVAL, "null net");
  arl::Net& n = h->net;
  if (n.arch != arl::ARCH_LSTM) return fail(ARL_ESTATE, "set_ppo_state: LSTM nets only (an FF net carries no state)");
  if (!carry) {
    if (n.ppo_snap) return fail(ARL_ESTATE, "set_ppo_state: PPO is set on the net, switch it off first (arl_net_set_ppo)");
    n.ppo_carry = nullptr;
    return ARL_OK;
  }
  if (!aligned(carry, 16)) return fail(ARL_EINVAL, "set_ppo_state: carry must be 16-byte aligned");
  n.ppo_carry = carry;
  return ARL_OK;
}

int arl_net_set_ppo(arl_net* h, float* snap, double clip_eps) {
  if (!h) return fail(ARL_EINVAL, "null net");
  arl::Net& n = h->net;
  if (!snap) {   // back to one gradient step per window
    n.ppo_snap = nullptr;
    n.ppo_begun = false;
    return ARL_OK;
  }
  if (!(clip_eps > 0.0 && clip_eps < 1.0)) return fail(ARL_EINVAL, "set_ppo: clip_eps must be finite and in (0, 1)");
  if (!aligned(snap, 16)) return fail(ARL_EINVAL, "set_ppo: snap must be 16-byte aligned");
  if (!ppo_arch_ok(n)) return fail(ARL_ESTATE, std::string("set_ppo: ") + PPO_ARCH_REFUSAL);
  n.ppo_snap = snap;
  n.ppo_lo = (float)(1.0 - clip_eps);
  n.ppo_hi = (float)(1.0 + clip_eps);
  n.ppo_begun = false;
  return ARL_OK;
}

static bool vclip_ok(double e) { return e >= 0.0 && e <= 1.7976931348623157e308; }   // finite, >= 0 (nan fails both)

int arl_net_set_ppo_options(arl_net* h, int norm_adv, double vclip_eps, float* v_old, double* aux) {
  if (!h) return fail(ARL_EINVAL, "null net");
  arl::Net& n = h->net;
  if (!vclip_ok(vclip_eps)) return fail(ARL_EINVAL, "set_ppo_options: vclip_eps must be finite and >= 0");
  if (vclip_eps > 0.0 && !v_old) return fail(ARL_EINVAL, "set_ppo_options: value clipping needs v_old");
  if (norm_adv && !aux) return fail(ARL_EINVAL, "set_ppo_options: advantage normalisation needs aux");
  if (!aligned(v_old, 16) || !aligned(aux, 8))
    return fail(ARL_EINVAL, "set_ppo_options: v_old must be 16-byte and aux 8-byte aligned");
  const bool on = norm_adv || vclip_eps > 0.0 || aux;
  if (on && !ppo_arch_ok(n)) return fail(ARL_ESTATE, std::string("set_ppo_options: ") + PPO_ARCH_REFUSAL);
  n.ppo_norm_adv = norm_adv != 0;
  n.ppo_vold = vclip_eps > 0.0 ? v_old : nullptr;
  n.ppo_ev = (float)vclip_eps;
  n.ppo_aux = aux;
  return ARL_OK;
}

int arl_ppo_begin(arl_net* h, double gamma, int clip_reward, void* s) {
  NEED_BOUND(h);
  if (!h->net.ppo_snap) return fail(ARL_ESTATE, "ppo_begin: PPO is off (arl_net_set_ppo)");
  return hip_status(arl::net_ppo_begin(h->net, gamma, clip_reward, S(s)), "ppo_begin");
}

int arl_ppo_learn(arl_net* h, double beta, double vcoef, void* s) {
  NEED_BOUND(h);
  if (!h->net.ppo_snap) return fail(ARL_ESTATE, "ppo_learn: PPO is off (arl_net_set_ppo)");
  if (!h->net.ppo_begun) return fail(ARL_ESTATE, "ppo_learn: no arl_ppo_begin since the last window advance");
  return hip_status(arl::net_ppo_learn(h->net, (float)beta, (float)vcoef, S(s)), "ppo_learn");
}

int arl_act(arl_net* h, int t, void* s) {
  NEED_BOUND(h);
  if (t < 0 || t > h->net.T) return fail(ARL_EINVAL, "act: t out of [0, t_max]");
  return hip_status(arl::net_act(h->net, t, 1, S(s)), "act");
}

// ---------------------------------------------------------------- device environment
static int64_t env_state_bytes(int kind, int64_t n_envs) {
  return n_envs < 0 ? -1 : 2 * n_envs * arl::env_state_ints(kind) * (int64_t)sizeof(int32_t);
}

int64_t arl_catch_state_bytes(int64_t n_envs) { return env_state_bytes(ARL_ENV_CATCH, n_envs); }

int64_t arl_breakout_state_bytes(int64_t n_envs) { return env_state_bytes(ARL_ENV_BREAKOUT, n_envs); }

// the granular calls: explicit pointers, one pool entry, the parity from the host; kind: ARL_ENV_* | flags
static int env_granular(const char* who, int kind, int32_t* state, int parity, const int32_t* actions, bool step,
                        int64_t n, int env_offset, uint64_t seed, uint8_t* pair, float* reward, uint8_t* done,
                        void* s) {
  const std::string w = who;
  if (n < 0 || n > 65535) return fail(ARL_EINVAL, w + ": n out of [0, 65535]");
  if (parity != 0 && parity != 1) return fail(ARL_EINVAL, w + ": parity must be 0 or 1");
  if (n == 0) return ARL_OK;
  if (!state || !pair || !reward || !done || (step && !actions)) return fail(ARL_EINVAL, w + ": null pointer");
  if (!aligned(state, 16) || !aligned(pair, 16) || !aligned(reward, 4) || (step && !aligned(actions, 4)))
    return fail(ARL_EINVAL, w + ": state and frames 16-byte aligned, rewards and actions 4-byte aligned");
  arl::EnvArgs a{};
  a.state = state;
  a.actions = step ? actions : nullptr;
  a.ctl = nullptr;
  a.t = parity;
  a.dpool = arl::fd_make(1u);
  a.pair_pool = pair;
  a.reward_pool = reward;
  a.done_pool = done;
  a.n = (int)n;
  a.e0 = 0;
  a.ne = -1;
  a.env_offset = env_offset;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  return hip_status(arl::launch_env(kind, a, S(s)), who);
}

int arl_catch_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int parity, uint8_t* pair_out,
                    float* reward_out, uint8_t* done_out, void* s) {
  return env_granular("catch_reset", ARL_ENV_CATCH, state, parity, nullptr, false, n, env_offset, seed, pair_out,
                      reward_out, done_out, s);
}

int arl_catch_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                   uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* s) {
  return env_granular("catch_step", ARL_ENV_CATCH, state, parity_in, actions, true, n, env_offset, seed, pair_out,
                      reward_out, done_out, s);
}

int arl_breakout_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int parity, uint8_t* pair_out,
                       float* reward_out, uint8_t* done_out, void* s) {
  return env_granular("breakout_reset", ARL_ENV_BREAKOUT, state, parity, nullptr, false, n, env_offset, seed, pair_out,
                      reward_out, done_out, s);
}

int arl_breakout_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                      int flags, uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* s) {
  if (flags & ~ARL_ENV_GAME_OVER_ONLY)
    return fail(ARL_EINVAL, "breakout_step: flags must be 0 or ARL_ENV_GAME_OVER_ONLY");
  return env_granular("breakout_step", ARL_ENV_BREAKOUT | flags, state, parity_in, actions, true, n, env_offset, seed,
                      pair_out, reward_out, done_out, s);
}

int64_t arl_pong_state_bytes(int64_t n_envs) { return env_state_bytes(ARL_ENV_PONG, n_envs); }

int arl_pong_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int parity, uint8_t* pair_out,
                   float* reward_out, uint8_t* done_out, void* s) {
  return env_granular("pong_reset", ARL_ENV_PONG, state, parity, nullptr, false, n, env_offset, seed, pair_out,
                      reward_out, done_out, s);
}

int arl_pong_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                  int points, uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* s) {
  if (points < 1 || points > arl::PONG_POINTS_MAX) return fail(ARL_EINVAL, "pong_step: points out of [1, 21]");
  return env_granular("pong_step", ARL_ENV_PONG | ARL_ENV_PONG_POINTS(points), state, parity_in, actions, true, n,
                      env_offset, seed, pair_out, reward_out, done_out, s);
}

int64_t arl_tmaze_state_bytes(int64_t n_envs) { return env_state_bytes(ARL_ENV_TMAZE, n_envs); }

static bool tmaze_length_ok(int length) { return length >= 1 && length <= arl::TMAZE_LENGTH_MAX; }

int arl_tmaze_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int length, int parity, uint8_t* pair_out,
                    float* reward_out, uint8_t* done_out, void* s) {
  if (!tmaze_length_ok(length)) return fail(ARL_EINVAL, "tmaze_reset: length out of [1, 8]");
  return env_granular("tmaze_reset", ARL_ENV_TMAZE | ARL_ENV_TMAZE_LENGTH(length), state, parity, nullptr, false, n,
                      env_offset, seed, pair_out, reward_out, done_out, s);
}

int arl_tmaze_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                   int length, uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* s) {
  if (!tmaze_length_ok(length)) return fail(ARL_EINVAL, "tmaze_step: length out of [1, 8]");
  return env_granular("tmaze_step", ARL_ENV_TMAZE | ARL_ENV_TMAZE_LENGTH(length), state, parity_in, actions, true, n,
                      env_offset, seed, pair_out, reward_out, done_out, s);
}

int64_t arl_maze_state_bytes(int64_t n_envs) { return env_state_bytes(ARL_ENV_MAZE, n_envs); }

// the kind of a maze call from its explicit fields, or -1 with the error set
static int maze_kind(const char* who, int rooms, int view, int levels) {
  if (!arl::maze_fields_ok(rooms, view, levels)) {
    fail(ARL_EINVAL, std::string(who) + ": rooms out of [2, 4], view out of [0, 2] or levels out of [0, 1023]");
    return -1;
  }
  return ARL_ENV_MAZE | ARL_ENV_MAZE_ROOMS(rooms) | ARL_ENV_MAZE_VIEW(view) | ARL_ENV_MAZE_LEVELS(levels);
}

int arl_maze_reset(int32_t* state, int64_t n, int env_offset, uint64_t seed, int rooms, int view, int levels, int parity,
                   uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* s) {
  const int kind = maze_kind("maze_reset", rooms, view, levels);
  if (kind < 0) return ARL_EINVAL;
  return env_granular("maze_reset", kind, state, parity, nullptr, false, n, env_offset, seed, pair_out, reward_out,
                      done_out, s);
}

int arl_maze_step(int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset, uint64_t seed,
                  int rooms, int view, int levels, uint8_t* pair_out, float* reward_out, uint8_t* done_out, void* s) {
  const int kind = maze_kind("maze_step", rooms, view, levels);
  if (kind < 0) return ARL_EINVAL;
  return env_granular("maze_step", kind, state, parity_in, actions, true, n, env_offset, seed, pair_out, reward_out,
                      done_out, s);
}

int arl_net_set_env(arl_net* h, int kind, int32_t* state) {
  if (!h) return fail(ARL_EINVAL, "null net");
  if (!arl::env_kind_ok(kind))
    return fail(ARL_EINVAL,
                "set_env: unknown env kind (ARL_ENV_CATCH, ARL_ENV_BREAKOUT [| ARL_ENV_GAME_OVER_ONLY], "
                "ARL_ENV_PONG | ARL_ENV_PONG_POINTS(0..21), ARL_ENV_TMAZE | ARL_ENV_TMAZE_LENGTH(0..8), or ARL_ENV_MAZE | "
                "ARL_ENV_MAZE_ROOMS(0, 2..4) | ARL_ENV_MAZE_VIEW(0..2) | ARL_ENV_MAZE_LEVELS(0..1023))");
  if (!state) {   // detach
    h->net.env_state = nullptr;
    h->net.env_direct = false;
    return ARL_OK;
  }
  const arl::Net& n = h->net;
  if (n.rgb || n.stack || n.states)
    return fail(ARL_ESTATE, "set_env: the env renders frame pairs (FF / LSTM / FF_NATURE nets without a frames flag)");
  if (n.A < 4)
    return fail(ARL_EINVAL,
                "set_env: the env needs n_actions >= 4 (NOOP / FIRE / RIGHT / LEFT; Pong and the T-maze: NOOP / FIRE / "
                "UP / DOWN; the maze: UP / DOWN / RIGHT / LEFT)");
  if (!aligned(state, 16)) return fail(ARL_EINVAL, "set_env: state must be 16-byte aligned");
  h->net.env_state = state;
  h->net.env_kind = kind;
  return ARL_OK;
}

// validates an env launch of a bound net and fills its arguments (0 = ok); step == false: the reset
static int env_args(arl_net* h, bool step, int t, int e0, int ne, uint8_t* pair_pool, float* reward_pool,
                    uint8_t* done_pool, int64_t pool_len, arl::EnvArgs& a) {
  arl::Net& n = h->net;
  if (!n.env_state) return fail(ARL_ESTATE, "env: no env attached (arl_net_set_env)");
  if (step && (t < 0 || t >= n.T)) return fail(ARL_EINVAL, "env_step: t out of [0, t_max)");
  if (pool_len < 2 || pool_len > INT32_MAX) return fail(ARL_EINVAL, "env: pool_len out of [2, 2^31 - 1]");
  if (!pair_pool || !reward_pool || !done_pool) return fail(ARL_EINVAL, "env: the env writes all three pools");
  if (!aligned(pair_pool, 16) || !aligned(reward_pool, 4))
    return fail(ARL_EINVAL, "env: the frame pool must be 16-byte aligned, the reward pool 4-byte aligned");
  if (n.N > 65535) return fail(ARL_EINVAL, "env: n_envs > 65535");
  if (int rc = check_pool(h, ARL_POOL_FRAMES, pair_pool, pool_len, (int64_t)arl::PAIR * n.N, "frame")) return rc;
  if (int rc = check_pool(h, ARL_POOL_REWARDS, reward_pool, pool_len, 4 * (int64_t)n.N, "reward")) return rc;
  if (int rc = check_pool(h, ARL_POOL_DONES, done_pool, pool_len, (int64_t)n.N, "done")) return rc;
  a = arl::EnvArgs{};
  a.state = n.env_state;
  a.actions = step ? n.at<int32_t>(n.w_act) + (int64_t)t * n.N : nullptr;
  a.ctl = n.at<int64_t>(n.w_ctl);
  a.t = step ? t : 0;
  a.dpool = arl::fd_make((uint32_t)pool_len);
  a.pair_pool = pair_pool;
  a.reward_pool = reward_pool;
  a.done_pool = done_pool;
  a.n = n.N;
  a.e0 = e0;
  a.ne = ne;
  a.env_offset = n.env_offset;
  a.seed_lo = (uint32_t)n.seed;
  a.seed_hi = (uint32_t)(n.seed >> 32);
  return 0;
}

static int env_launch(const arl::Net& n, const arl::EnvArgs& a, void* s, const char* what) {
  hipError_t e = arl::launch_env(n.env_kind, a, S(s));
  if (e == hipSuccess) e = arl::stamp(n, arl::STAGE_OTHER, S(s));
  return hip_status(e, what);
}

int arl_env_reset(arl_net* h, uint8_t* pair_pool, float* reward_pool, uint8_t* done_pool, int64_t pool_len, void* s) {
  NEED_BOUND(h);
  arl::EnvArgs a;
  if (int rc = env_args(h, false, 0, 0, -1, pair_pool, reward_pool, done_pool, pool_len, a)) return rc;
  return env_launch(h->net, a, s, "env_reset");
}

int arl_act_mode(arl_net* h, int t, int mode, void* s) {
  NEED_BOUND(h);
  if (t < 0 || t > h->net.T) return fail(ARL_EINVAL, "act: t out of [0, t_max]");
  if (mode < 0 || mode > 2) return fail(ARL_EINVAL, "act: mode must be 0 (none), 1 (sample) or 2 (greedy)");
  return hip_status(arl::net_act(h->net, t, mode, S(s)), "act");
}

static int check_env_range(const arl::Net& n, int e0, int ne) {
  if (ne < 1 || e0 < 0 || e0 > n.N - ne) return fail(ARL_EINVAL, "env range [e0, e0 + ne) outside [0, n_envs)");
  if (e0 % ARL_ENV_GROUP_ALIGN) return fail(ARL_EINVAL, "env range: e0 must be a multiple of ARL_ENV_GROUP_ALIGN");
  if ((n.arch == arl::ARCH_FF_NATURE || n.states) && (e0 != 0 || ne != n.N))
    return fail(ARL_EINVAL, "env range: Nature-head and ARL_ARCH_STATES nets run all envs in one launch");
  return 0;
}

int arl_observe_envs(arl_net* h, int t, int e0, int ne, const uint8_t* pool, int H, int W, const float* reward_pool,
                     const uint8_t* done_pool, int64_t pool_len, int force_reset, int mode, void* s) {
  NEED_BOUND(h);
  if (int rc = check_env_range(h->net, e0, ne)) return rc;
  if (h->net.rgb) {
    if (mode < 0 || mode > ARL_RESIZE_SIMD) return fail(ARL_EINVAL, "observe_rgb: resize_mode must be 0 or 1");
    if (int rc = check_rgb_dims(H, W)) return rc;
  } else if (h->net.stack || h->net.states) {
    H = W = mode = 0;
  } else {
    if (mode < 0 || mode > (ARL_RESIZE_SIMD | ARL_RESIZE_CROP)) return fail(ARL_EINVAL, "bad resize_mode");
    H = W = 0;
  }
  return observe_common(h, t, pool, reward_pool, done_pool, pool_len, force_reset, mode, H, W, s, e0, ne);
}

int arl_env_step(arl_net* h, int t, int e0, int ne, uint8_t* pair_pool, float* reward_pool, uint8_t* done_pool,
                 int64_t pool_len, void* s) {
  NEED_BOUND(h);
  if (int rc = check_env_range(h->net, e0, ne)) return rc;
  arl::EnvArgs a;
  if (int rc = env_args(h, true, t, e0, ne, pair_pool, reward_pool, done_pool, pool_len, a)) return rc;
  return env_launch(h->net, a, s, "env_step");
}

// ---------------------------------------------------------------- direct-to-ring device env
int arl_net_set_env_direct(arl_net* h, int on) {
  if (!h) return fail(ARL_EINVAL, "null net");
  arl::Net& n = h->net;
  if (n.rgb || n.stack || n.states)
    return fail(ARL_ESTATE,
                "set_env_direct: the env renders frame pairs (FF / LSTM / FF_NATURE nets without a frames flag)");
  if (on && !n.env_state) return fail(ARL_ESTATE, "set_env_direct: no env attached (arl_net_set_env)");
  n.env_direct = on != 0;
  return ARL_OK;
}

static int bad_resize_mode(int mode) {
  return (mode < 0 || mode > (ARL_RESIZE_SIMD | ARL_RESIZE_CROP)) ? fail(ARL_EINVAL, "bad resize_mode") : 0;
}

// the ring half of a direct launch: the observation at window slot t of the bound net (no pools)
static void direct_ring(const arl::Net& n, int t, int force_reset, int mode, arl::RingArgs& a) {
  a = arl::RingArgs{};
  a.dpool = arl::fd_make(1u);
  a.dR = n.dR;
  a.frames = n.at<uint8_t>(n.w_frames);
  a.nvalid = n.at<uint8_t>(n.w_nvalid);
  a.reset_flags = n.at<uint8_t>(n.w_reset);
  a.rewards = n.at<float>(n.w_rewards);
  a.dones = n.at<uint8_t>(n.w_dones);
  a.ctl = n.at<int64_t>(n.w_ctl);
  a.n = n.N;
  a.R = n.R;
  a.t = t;
  a.mode = mode;
  a.force_reset = force_reset;
  a.episodes = n.episode_stats ? n.ws + n.w_episodes : nullptr;
}

// validates a direct launch of a bound net and fills its arguments (0 = ok); step == false: the reset form
static int direct_args(arl_net* h, bool step, int t, int e0, int ne, int mode, arl::DirectArgs& a) {
  arl::Net& n = h->net;
  if (!n.env_state) return fail(ARL_ESTATE, "env: no env attached (arl_net_set_env)");
  if (!n.env_direct) return fail(ARL_ESTATE, "env: direct mode is off (arl_net_set_env_direct)");
  if (step && (t < 0 || t >= n.T)) return fail(ARL_EINVAL, "env_step_observe: t out of [0, t_max)");
  if (int rc = bad_resize_mode(mode)) return rc;
  if (n.N > 65535) return fail(ARL_EINVAL, "env: n_envs > 65535");
  a = arl::DirectArgs{};
  a.env.state = n.env_state;
  a.env.actions = step ? n.at<int32_t>(n.w_act) + (int64_t)t * n.N : nullptr;
  a.env.ctl = n.at<int64_t>(n.w_ctl);
  a.env.t = step ? t : 0;
  a.env.dpool = arl::fd_make(1u);
  a.env.n = n.N;
  a.env.e0 = e0;
  a.env.ne = ne;
  a.env.env_offset = n.env_offset;
  a.env.seed_lo = (uint32_t)n.seed;
  a.env.seed_hi = (uint32_t)(n.seed >> 32);
  direct_ring(n, step ? t + 1 : 0, step ? 0 : 1, mode, a.ring);
  a.ring.e0 = e0;
  a.ring.ne = ne;
  return 0;
}

static int direct_launch(const arl::Net& n, const arl::DirectArgs& a, void* s, const char* what) {
  hipError_t e = arl::launch_env_direct(n.env_kind, a, S(s));
  if (e == hipSuccess) e = arl::stamp(n, arl::STAGE_PHI, S(s));
  return hip_status(e, what);
}

int arl_env_reset_observe(arl_net* h, int resize_mode, void* s) {
  NEED_BOUND(h);
  arl::DirectArgs a;
  if (int rc = direct_args(h, false, 0, 0, -1, resize_mode, a)) return rc;
  return direct_launch(h->net, a, s, "env_reset_observe");
}

int arl_env_step_observe(arl_net* h, int t, int e0, int ne, int resize_mode, void* s) {
  NEED_BOUND(h);
  if (!h->net.env_state) return fail(ARL_ESTATE, "env: no env attached (arl_net_set_env)");
  if (!h->net.env_direct) return fail(ARL_ESTATE, "env: direct mode is off (arl_net_set_env_direct)");
  if (int rc = check_env_range(h->net, e0, ne)) return rc;
  arl::DirectArgs a;
  if (int rc = direct_args(h, true, t, e0, ne, resize_mode, a)) return rc;
  return direct_launch(h->net, a, s, "env_step_observe");
}

int arl_env_step_screen(int kind, int32_t* state, int parity_in, const int32_t* actions, int64_t n, int env_offset,
                        uint64_t seed, int resize_mode, uint8_t* screen_out, float* reward_out, uint8_t* done_out,
                        void* s) {
  if (!arl::env_kind_ok(kind))
    return fail(ARL_EINVAL,
                "env_step_screen: unknown env kind (ARL_ENV_CATCH, ARL_ENV_BREAKOUT [| ARL_ENV_GAME_OVER_ONLY], "
                "ARL_ENV_PONG | ARL_ENV_PONG_POINTS(0..21), ARL_ENV_TMAZE | ARL_ENV_TMAZE_LENGTH(0..8), or ARL_ENV_MAZE | "
                "ARL_ENV_MAZE_ROOMS(0, 2..4) | ARL_ENV_MAZE_VIEW(0..2) | ARL_ENV_MAZE_LEVELS(0..1023))");
  if (n < 0 || n > 65535) return fail(ARL_EINVAL, "env_step_screen: n out of [0, 65535]");
  if (parity_in != 0 && parity_in != 1) return fail(ARL_EINVAL, "env_step_screen: parity must be 0 or 1");
  if (int rc = bad_resize_mode(resize_mode)) return rc;
  if (n == 0) return ARL_OK;
  if (!state || !actions || !screen_out || !reward_out || !done_out)
    return fail(ARL_EINVAL, "env_step_screen: null pointer");
  if (!aligned(state, 16) || !aligned(screen_out, 4) || !aligned(reward_out, 4) || !aligned(actions, 4))
    return fail(ARL_EINVAL, "env_step_screen: state 16-byte aligned, screens, rewards and actions 4-byte aligned");
  arl::DirectArgs a{};
  a.env.state = state;
  a.env.actions = actions;
  a.env.ctl = nullptr;
  a.env.t = parity_in;
  a.env.dpool = arl::fd_make(1u);
  a.env.n = (int)n;
  a.env.env_offset = env_offset;
  a.env.seed_lo = (uint32_t)seed;
  a.env.seed_hi = (uint32_t)(seed >> 32);
  a.ring.dpool = a.ring.dR = arl::fd_make(1u);
  a.ring.frames = screen_out;
  a.ring.n = (int)n;
  a.ring.R = 1;
  a.ring.mode = resize_mode;
  a.reward_out = reward_out;
  a.done_out = done_out;
  return hip_status(arl::launch_env_direct(kind, a, S(s)), "env_step_screen");
}

int arl_act_envs(arl_net* h, int t, int e0, int ne, int mode, void* s) {
  NEED_BOUND(h);
  if (t < 0 || t > h->net.T) return fail(ARL_EINVAL, "act: t out of [0, t_max]");
  const int part = mode & ~3;
  if (mode < 0 || (mode & 3) > 2 || (part != 0 && part != ARL_ACT_CONV_ONLY && part != ARL_ACT_AFTER_CONV))
    return fail(ARL_EINVAL, "act: mode must be 0 / 1 / 2, optionally | ARL_ACT_CONV_ONLY or ARL_ACT_AFTER_CONV");
  if (int rc = check_env_range(h->net, e0, ne)) return rc;
  if (part != 0 && h->net.arch == arl::ARCH_FF_NATURE) return fail(ARL_EINVAL, "act: Nature head has no conv split");
  if (ne != h->net.N && !h->net.planes_current() && h->net.arch != arl::ARCH_FF_NATURE)
    return fail(ARL_ESTATE, "act: the params changed since the FC weight planes were built; call arl_net_prepare on "
                            "the stream the env-range chains fork from before issuing them");
  return hip_status(arl::net_act(h->net, t, mode, S(s), e0, ne), "act");
}

int arl_run_stage(arl_net* h, int stage, int t, void* s) {
  NEED_BOUND(h);
  if (stage < ARL_STAGE_CONV_FWD || (stage > ARL_STAGE_LSTM_WGRAD && stage != ARL_STAGE_RMSPROP))
    return fail(ARL_EINVAL, "run_stage: unknown stage");
  if (stage >= ARL_STAGE_RETURNS && h->net.arch == arl::ARCH_FF_NATURE)
    return fail(ARL_EINVAL, "run_stage: returns / conv reduce / grad sqnorm stages are NIPS-head only");
  if (stage >= ARL_STAGE_LSTM_GATES && stage <= ARL_STAGE_LSTM_WGRAD && h->net.arch != arl::ARCH_LSTM)
    return fail(ARL_EINVAL, "run_stage: the LSTM stages need an LSTM net");
  if (t < 0 || t > h->net.T) return fail(ARL_EINVAL, "run_stage: t out of [0, t_max]");
  return hip_status(arl::net_stage(h->net, stage, t, S(s)), "run_stage");
}

int arl_stamps_begin(arl_net* h, int cap) {
  NEED_BOUND(h);
  if (cap < 1 || cap > (1 << 20)) return fail(ARL_EINVAL, "stamps_begin: cap out of [1, 2^20]");
  arl::Net& n = h->net;
  if (!n.stamps) n.stamps = new arl::Stamps();
  arl::Stamps& st = *n.stamps;
  while ((int)st.ev.size() < cap) {
    hipEvent_t e;
    // timing events without the system-scope fence (cache writeback / invalidate) a default event
    // record performs: the stamps perturb the window they measure less
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess)
      return fail(ARL_EHIP, "stamps_begin: hipEventCreateWithFlags");
    st.ev.push_back(e);
  }
  st.stage.assign(st.ev.size(), 0);
  st.seq.assign(st.ev.size(), 0);
  st.count = 0;
  st.calls = 0;
  st.period = 0;
  st.on = true;
  return ARL_OK;
}

int arl_stamps_sparse(arl_net* h, int period) {
  NEED_BOUND(h);
  arl::Stamps* st = h->net.stamps;
  if (!st || !st->on || st->calls != 0) return fail(ARL_EINVAL, "stamps_sparse: call right after arl_stamps_begin");
  if (period < 0 || period > 4096) return fail(ARL_EINVAL, "stamps_sparse: period out of [0, 4096]");
  st->period = period;
  return ARL_OK;
}

int arl_stamp(arl_net* h, int stage, void* s) {
  NEED_BOUND(h);
  if (stage < 0 || stage > arl::STAGE_OTHER) return fail(ARL_EINVAL, "stamp: unknown stage");
  return hip_status(arl::stamp(h->net, stage, S(s)), "stamp");
}

int arl_stamps_end(arl_net* h, int* count) {
  NEED_BOUND(h);
  arl::Stamps* st = h->net.stamps;
  if (st) st->on = false;
  if (count) *count = st ? st->count : 0;
  return ARL_OK;
}

int arl_stamps_read(arl_net* h, int i0, int n, float* ms, int* stage) {
  NEED_BOUND(h);
  arl::Stamps* st = h->net.stamps;
  if (!st || i0 < 0 || n < 0 || i0 + n > st->count) return fail(ARL_EINVAL, "stamps_read: range outside the stamps");
  if (n == 0) return ARL_OK;
  if (!ms || !stage) return fail(ARL_EINVAL, "stamps_read: null output");
  hipError_t e = hipEventSynchronize(st->ev[i0 + n - 1]);
  for (int i = i0; i < i0 + n && e == hipSuccess; ++i) {
    float t = 0.f;
    if (i > 0 && st->seq[i] != st->seq[i - 1] + 1) t = -1.f;   // (sparse: not one stage's interval)
    else if (i > 0) e = hipEventElapsedTime(&t, st->ev[i - 1], st->ev[i]);
    ms[i - i0] = t;
    stage[i - i0] = st->stage[i];
  }
  return hip_status(e, "stamps_read");
}

int arl_learn(arl_net* h, double gamma, double beta, double vcoef, int clip_reward, void* s) {
  NEED_BOUND(h);
  return hip_status(arl::net_learn(h->net, gamma, (float)beta, (float)vcoef, clip_reward, S(s)), "learn");
}

int arl_learn_part(arl_net* h, int part, double gamma, double beta, double vcoef, int clip_reward, void* s) {
  NEED_BOUND(h);
  if (part < 0 || part >= arl::LEARN_PARTS) return fail(ARL_EINVAL, "learn_part: part out of range");
  if (h->net.arch == arl::ARCH_FF_NATURE) return fail(ARL_ESTATE, "learn_part: the Nature learner is one call");
  return hip_status(arl::net_learn_part(h->net, part, gamma, (float)beta, (float)vcoef, clip_reward, S(s)),
                    "learn_part");
}

int arl_optimize(arl_net* h, double lr0, int64_t total_steps, int64_t n_total, double alpha, double eps, double clip,
                 void* s) {
  NEED_BOUND(h);
  return hip_status(arl::net_optimize(h->net, lr0, total_steps, n_total, alpha, eps, (float)clip, S(s)), "optimize");
}

int arl_run_window(arl_net* h, const uint8_t* pair_pool, const float* reward_pool, const uint8_t* done_pool,
                   int64_t pool_len, int first, int resize_mode, double gamma, double beta, double vcoef,
                   int clip_reward, double lr0, int64_t total_steps, int64_t n_total, double alpha, double eps,
                   double clip, void* s) {
  NEED_BOUND(h);
  arl::Net& n = h->net;
  if (n.ppo_snap) return fail(ARL_ESTATE, "run_window: a single-call window has no epochs (arl_net_set_ppo is on)");
  if (n.rgb || n.stack || n.states || n.arch == arl::ARCH_FF_NATURE)
    return fail(ARL_ESTATE, "run_window: frame-pair nets with the NIPS head only (FF / LSTM)");
  if (resize_mode < 0 || resize_mode > (ARL_RESIZE_SIMD | ARL_RESIZE_CROP)) return fail(ARL_EINVAL, "bad resize_mode");
  // a direct env (arl_net_set_env_direct) answers act(t) with observation t + 1 in one launch: no pools are read
  const bool direct = n.env_state != nullptr && n.env_direct;
  arl::DirectArgs da;
  if (direct) {
    if (int rc = direct_args(h, true, 0, 0, -1, resize_mode, da)) return rc;
  } else {   // every observation of the window reads the same pools: check them before the first launch
    arl::RingArgs a;
    if (int rc = ring_args(h, 0, pair_pool, reward_pool, done_pool, pool_len, 0, resize_mode, 0, 0, 0, -1, a)) return rc;
  }
  // an attached env steps after every act(t), t < T, into the pools the next observation reads (so it writes
  // them: the signature keeps the observing calls' const)
  const bool env = n.env_state != nullptr && !direct;
  arl::EnvArgs ea;
  if (env)
    if (int rc = env_args(h, true, 0, 0, -1, const_cast<uint8_t*>(pair_pool), const_cast<float*>(reward_pool),
                          const_cast<uint8_t*>(done_pool), pool_len, ea))
      return rc;
  // FF: the learner's returns + heads backward run in the bootstrap step's policy launch
  const bool fuse_was = n.fuse_returns;
  const arl::Net::ReturnsCfg ret_was = n.ret;
  n.fuse_returns = n.arch == arl::ARCH_FF;
  n.returns_done = false;
  n.ret = arl::Net::ReturnsCfg{gamma, (float)beta, (float)vcoef, clip_reward};
  for (int t = 0; t <= n.T; ++t) {
    if (direct) {
      if (t == 0 && first) {   // the reset form: episode 0 of every env, its first screen as observation 0
        arl::DirectArgs ra;
        int rc = direct_args(h, false, 0, 0, -1, resize_mode, ra);
        if (rc == ARL_OK) rc = direct_launch(n, ra, s, "run_window: env_reset_observe");
        if (rc != ARL_OK) {
          n.fuse_returns = fuse_was;
          n.ret = ret_was;
          return rc;
        }
      }
    } else if (t > 0 || first) {   // slot 0 of a continuing window: the previous window's bootstrap observation
      const int rc = observe_common(h, t, pair_pool, reward_pool, done_pool, pool_len, t == 0 ? 1 : 0, resize_mode, 0,
                                    0, s);
      if (rc != ARL_OK) {
        n.fuse_returns = fuse_was;
        n.ret = ret_was;
        return rc;
      }
    }
    const hipError_t e = arl::net_act(n, t, 1, S(s));   // (slot T: the bootstrap forward, no draw)
    if (e != hipSuccess) {
      n.fuse_returns = fuse_was;
      n.ret = ret_was;
      return hip_status(e, "run_window: act");
    }
    if (direct && t < n.T) {   // the env-step and observation t + 1
      da.env.t = t;
      da.env.actions = n.at<int32_t>(n.w_act) + (int64_t)t * n.N;
      da.ring.t = t + 1;
      if (const int rc = direct_launch(n, da, s, "run_window: env_step_observe")) {
        n.fuse_returns = fuse_was;
        n.ret = ret_was;
        return rc;
      }
    }
    if (env && t < n.T) {
      ea.t = t;
      ea.actions = n.at<int32_t>(n.w_act) + (int64_t)t * n.N;
      if (const int rc = env_launch(n, ea, s, "run_window: env_step")) {
        n.fuse_returns = fuse_was;
        n.ret = ret_was;
        return rc;
      }
    }
  }
  n.fuse_returns = fuse_was;
  n.ret = ret_was;
  hipError_t e = arl::net_learn(n, gamma, (float)beta, (float)vcoef, clip_reward, S(s));
  if (e == hipSuccess) e = arl::net_optimize(n, lr0, total_steps, n_total, alpha, eps, (float)clip, S(s), true);
  return hip_status(e, "run_window");
}

int arl_optimize_advance(arl_net* h, double lr0, int64_t total_steps, int64_t n_total, double alpha, double eps,
                         double clip, void* s) {
  NEED_BOUND(h);
  return hip_status(arl::net_optimize(h->net, lr0, total_steps, n_total, alpha, eps, (float)clip, S(s), true),
                    "optimize_advance");
}

int arl_advance(arl_net* h, void* s) {
  NEED_BOUND(h);
  return hip_status(arl::net_advance(h->net, S(s)), "advance");
}

int arl_forward_states(arl_net* h, const float* x, int64_t n, int mode, void* s) {
  NEED_BOUND(h);
  const bool keep = (mode & ARL_FWD_KEEP_STATE) != 0;
  mode &= ~ARL_FWD_KEEP_STATE;
  if (mode < 0 || mode > 2) return fail(ARL_EINVAL, "forward_states: mode must be 0, 1 or 2 (| ARL_FWD_KEEP_STATE)");
  if (!x || n < 1 || n > h->net.N) return fail(ARL_EINVAL, "forward_states: need 1 <= n <= n_envs");
  if (!aligned(x, 16)) return fail(ARL_EINVAL, "forward_states: states must be 16-byte aligned");
  return hip_status(arl::net_forward_f32(h->net, x, (int)n, mode, S(s), keep), "forward_states");
}

int arl_reset_state(arl_net* h, int64_t e0, int64_t n, void* s) {
  NEED_BOUND(h);
  if (e0 < 0 || n < 0 || e0 + n > h->net.N) return fail(ARL_EINVAL, "reset_state: rows outside [0, n_envs)");
  if (n == 0) return ARL_OK;
  return hip_status(arl::net_reset_state(h->net, (int)e0, (int)n, S(s)), "reset_state");
}

// The one-array updates (arl_rmsprop, arl_rmsprop_wd, arl_adam) share two steps; who: their error texts' prefix.
// 1. the arrays: none null unless n == 0, all 16-byte aligned
static int update_arrays_ok(const std::string& who, std::initializer_list<const void*> arrays, int64_t n) {
  bool null = false, align = true;
  for (const void* a : arrays) {
    null |= a == nullptr;
    align &= aligned(a, 16);
  }
  if (n < 0 || (n > 0 && null)) return fail(ARL_EINVAL, who + ": null pointer / n < 0");
  if (!align) return fail(ARL_EINVAL, who + ": 16-byte alignment");
  return ARL_OK;
}
// 2. the clip's scratch and its norm launch; leaves in u (and wd, the decay of the whole array at `rate`, no bias
// ranges) what the optimizer's launch takes
static int update_array_args(const std::string& who, const float* g, int64_t n, double clip, double* parts,
                             double rate, void* s, arl::DecayArgs& wd, arl::UpdateArgs& u) {
  if (clip > 0 && !parts) return fail(ARL_EINVAL, who + ": clip needs norm_partials scratch");
  wd.rate = (float)rate;
  u.norm_sq = clip > 0 ? parts : nullptr;
  u.nparts = 256;
  u.clip = (float)clip;
  u.wd = &wd;
  return clip > 0 ? hip_status(arl::launch_grad_sqnorm(g, n, parts, u.nparts, S(s)), who.c_str()) : ARL_OK;
}

static int rmsprop_array(float* p, float* ms, const float* g, int64_t n, double lr, double alpha, double eps,
                         double clip, double* parts, double rate, void* s) {
  arl::DecayArgs wd{};
  arl::UpdateArgs u;
  if (const int rc = update_arrays_ok("rmsprop", {p, ms, g}, n)) return rc;
  if (const int rc = update_array_args("rmsprop", g, n, clip, parts, rate, s, wd, u)) return rc;
  return hip_status(arl::launch_rmsprop(p, ms, g, n, lr, alpha, eps, u, S(s)), "rmsprop");
}

int arl_rmsprop(float* p, float* ms, const float* g, int64_t n, double lr, double alpha, double eps, double clip,
                double* parts, void* s) {
  return rmsprop_array(p, ms, g, n, lr, alpha, eps, clip, parts, 0.0, s);
}

int arl_rmsprop_wd(float* p, float* ms, const float* g, int64_t n, double lr, double alpha, double eps, double clip,
                   double* parts, double weight_decay, void* s) {
  if (!decay_rate_ok(weight_decay))
    return fail(ARL_EINVAL, "rmsprop_wd: weight_decay must be finite and >= 0");
  return rmsprop_array(p, ms, g, n, lr, alpha, eps, clip, parts, weight_decay, s);
}

int arl_adam(float* p, float* m, float* v, const float* g, int64_t n, double alpha, double beta1, double beta2,
             double eps, int64_t t, double clip, double* parts, double weight_decay, void* s) {
  if (const int rc = update_arrays_ok("adam", {p, m, v, g}, n)) return rc;
  if (t < 1) return fail(ARL_EINVAL, "adam: t must be >= 1 (the number of this update)");
  if (!adam_beta_ok(beta1) || !adam_beta_ok(beta2)) return fail(ARL_EINVAL, "adam: beta1 and beta2 must be in [0, 1)");
  if (!decay_rate_ok(weight_decay)) return fail(ARL_EINVAL, "adam: weight_decay must be finite and >= 0");
  const arl::AdamArgs ad{beta1, beta2, nullptr, t};
  arl::DecayArgs wd{};
  arl::UpdateArgs u;
  if (const int rc = update_array_args("adam", g, n, clip, parts, weight_decay, s, wd, u)) return rc;
  return hip_status(arl::launch_adam(p, m, v, g, n, alpha, eps, ad, u, S(s)), "adam");
}

int arl_policy(const float* hh, int64_t n, const float* Wpi, const float* bpi, const float* Wv, const float* bv,
               int A, uint64_t seed, const int64_t* step_dev, int64_t step_off, int env_offset, int sample,
               float* logits, float* probs, float* logp, float* v, float* ent, int32_t* act, float* logp_a,
               void* s) {
  if (n < 0 || A < 1 || A > arl::MAXA) return fail(ARL_EINVAL, "policy: bad n / n_actions");
  if (n > 0 && (!hh || !Wpi || !bpi || !Wv || !bv || !logits || !probs || !logp || !v || !ent))
    return fail(ARL_EINVAL, "policy: null pointer");
  if (sample < 0 || sample > 2) return fail(ARL_EINVAL, "policy: sample must be 0, 1 (Philox draw) or 2 (argmax)");
  if (sample == 1 && !step_dev) return fail(ARL_EINVAL, "policy: sampling needs the device step counter");
  if (sample && (!act || !logp_a)) return fail(ARL_EINVAL, "policy: sampling needs act/logp_a");
  if (!aligned(hh, 16) || !aligned(Wpi, 16) || !aligned(Wv, 16)) return fail(ARL_EINVAL, "policy: 16-byte alignment");
  return hip_status(arl::launch_policy(hh, n, Wpi, bpi, Wv, bv, A, seed, step_dev, step_off, env_offset, sample,
                                       logits, probs, logp, v, ent, act, logp_a, S(s)),
                    "policy");
}

// arl_returns_lossgrad is arl_returns_lossgrad_gae at lambda = 1 (gae_on(1.0) is false: the n-step kernel it always
// launched); who: their error texts' prefix
static int returns_lossgrad(const char* who_, const float* rewards, const uint8_t* dones, const float* v,
                            const float* probs, const float* logp, const int32_t* act, int T, int64_t n, int A,
                            double gamma, double lambda, double beta, double pi_loss_coef, double vcoef,
                            int keep_loss_scale_same, int clip_reward, float* dlogits, float* dv, float* loss,
                            void* s) {
  const std::string who = who_;
  if (T < 1 || n < 0 || A < 1) return fail(ARL_EINVAL, who + ": bad T / n / A");
  if (n > 0 && (!rewards || !dones || !v || !probs || !logp || !act || !dlogits || !dv))
    return fail(ARL_EINVAL, who + ": null pointer");
  if (!gae_lambda_ok(lambda)) return fail(ARL_EINVAL, who + ": lambda must be finite and in [0, 1]");
  arl::ReturnsArgs ra{};   // (no step snapshot: ctl stays null)
  ra.rewards = rewards; ra.dones = dones; ra.v = v; ra.probs = probs; ra.logp = logp; ra.act = act;
  ra.T = T; ra.n = (int)n; ra.A = A;
  ra.gamma = gamma; ra.clip_reward = clip_reward;
  ra.beta = (float)beta; ra.vcoef = (float)vcoef; ra.pcoef = (float)pi_loss_coef;
  ra.keep_scale = keep_loss_scale_same ? 1 : 0;
  ra.dlogits = dlogits; ra.dv = dv; ra.loss = loss;
  return hip_status(arl::launch_returns(ra, lambda, S(s)), who_);
}

int arl_returns_lossgrad(const float* rewards, const uint8_t* dones, const float* v, const float* probs,
                         const float* logp, const int32_t* act, int T, int64_t n, int A, double gamma, double beta,
                         double pi_loss_coef, double vcoef, int keep_loss_scale_same, int clip_reward, float* dlogits,
                         float* dv, float* loss, void* s) {
  return returns_lossgrad("returns", rewards, dones, v, probs, logp, act, T, n, A, gamma, 1.0, beta, pi_loss_coef,
                          vcoef, keep_loss_scale_same, clip_reward, dlogits, dv, loss, s);
}

int arl_returns_lossgrad_gae(const float* rewards, const uint8_t* dones, const float* v, const float* probs,
                             const float* logp, const int32_t* act, int T, int64_t n, int A, double gamma,
                             double lambda, double beta, double pi_loss_coef, double vcoef, int keep_loss_scale_same,
                             int clip_reward, float* dlogits, float* dv, float* loss, void* s) {
  return returns_lossgrad("returns_gae", rewards, dones, v, probs, logp, act, T, n, A, gamma, lambda, beta,
                          pi_loss_coef, vcoef, keep_loss_scale_same, clip_reward, dlogits, dv, loss, s);
}

int arl_ppo_snapshot(const float* rewards, const uint8_t* dones, const float* v, const float* logp, const int32_t* act,
                     int T, int64_t n, int A, double gamma, double lambda, int clip_reward, float* logp_old,
                     float* adv, float* ret, void* s) {
  if (T < 1 || T > 256 || n < 0 || n > INT32_MAX / 256 || A < 1) return fail(ARL_EINVAL, "ppo_snapshot: bad T / n / A");
  if (n > 0 && (!rewards || !dones || !v || !logp || !act || !logp_old || !adv || !ret))
    return fail(ARL_EINVAL, "ppo_snapshot: null pointer");
  if (!gae_lambda_ok(lambda)) return fail(ARL_EINVAL, "ppo_snapshot: lambda must be finite and in [0, 1]");
  arl::ReturnsArgs ra{};   // what the snapshot reads of it
  ra.rewards = rewards; ra.dones = dones; ra.v = v; ra.logp = logp; ra.act = act;
  ra.T = T; ra.n = (int)n; ra.A = A;
  ra.gamma = gamma; ra.clip_reward = clip_reward;
  return hip_status(arl::launch_ppo_snapshot(ra, lambda, logp_old, adv, ret, S(s)), "ppo_snapshot");
}

// The three granular PPO entries (arl_ppo_lossgrad, arl_ppo_lossgrad_vclip, arl_ppo_epoch_stats) share their
// shape and clip-range checks and the arguments all of them give; who: their error texts' prefix
static int ppo_dims_ok(const std::string& who, int T, int64_t n, int A) {
  if (T < 1 || T > 256 || n < 0 || n > INT32_MAX / 256 || A < 1 || A > arl::MAXA)
    return fail(ARL_EINVAL, who + ": bad T / n / A");
  return ARL_OK;
}
static int clip_eps_ok(const std::string& who, double clip_eps) {
  if (!(clip_eps > 0.0 && clip_eps < 1.0)) return fail(ARL_EINVAL, who + ": clip_eps must be finite and in (0, 1)");
  return ARL_OK;
}
static arl::PpoLossArgs ppo_entry_args(const uint8_t* dones, const float* v, const float* logp, const int32_t* act,
                                       const float* logp_old, const float* adv, const float* ret, int T, int64_t n,
                                       int A, double clip_eps) {
  arl::PpoLossArgs p{};   // the rest stays 0 / null until the entry names it
  p.r.dones = dones; p.r.v = v; p.r.logp = logp; p.r.act = act;
  p.r.T = T; p.r.n = (int)n; p.r.A = A;
  p.lpo = logp_old; p.adv = adv; p.ret = ret;
  p.lo = (float)(1.0 - clip_eps); p.hi = (float)(1.0 + clip_eps);
  return p;
}

// arl_ppo_lossgrad is arl_ppo_lossgrad_vclip without v_old (vclip false: v_old / vclip_eps are not looked at)
static int ppo_lossgrad(const char* who_, bool vclip, const uint8_t* dones, const float* v, const float* probs,
                        const float* logp, const int32_t* act, const float* logp_old, const float* adv,
                        const float* ret, const float* v_old, int T, int64_t n, int A, double clip_eps,
                        double vclip_eps, double beta, double pi_loss_coef, double vcoef, int keep_loss_scale_same,
                        float* dlogits, float* dv, float* loss, float* ratio_out, void* s) {
  const std::string who = who_;
  if (const int rc = ppo_dims_ok(who, T, n, A)) return rc;
  if (n > 0 && (!dones || !v || !probs || !logp || !act || !logp_old || !adv || !ret || (vclip && !v_old) ||
                !dlogits || !dv))
    return fail(ARL_EINVAL, who + ": null pointer");
  if (const int rc = clip_eps_ok(who, clip_eps)) return rc;
  if (vclip && !(vclip_ok(vclip_eps) && vclip_eps > 0.0))
    return fail(ARL_EINVAL, who + ": vclip_eps must be finite and > 0");
  arl::PpoLossArgs p = ppo_entry_args(dones, v, logp, act, logp_old, adv, ret, T, n, A, clip_eps);
  p.r.probs = probs;
  p.r.beta = (float)beta; p.r.vcoef = (float)vcoef; p.r.pcoef = (float)pi_loss_coef;
  p.r.keep_scale = keep_loss_scale_same ? 1 : 0;
  p.r.dlogits = dlogits; p.r.dv = dv; p.r.loss = loss; p.ratio = ratio_out;
  if (vclip) { p.vold = v_old; p.ev = (float)vclip_eps; }
  return hip_status(arl::launch_ppo_lossgrad(p, S(s)), who_);
}

int arl_ppo_lossgrad(const uint8_t* dones, const float* v, const float* probs, const float* logp, const int32_t* act,
                     const float* logp_old, const float* adv, const float* ret, int T, int64_t n, int A,
                     double clip_eps, double beta, double pi_loss_coef, double vcoef, int keep_loss_scale_same,
                     float* dlogits, float* dv, float* loss, float* ratio_out, void* s) {
  return ppo_lossgrad("ppo_lossgrad", false, dones, v, probs, logp, act, logp_old, adv, ret, nullptr, T, n, A, clip_eps,
                      0.0, beta, pi_loss_coef, vcoef, keep_loss_scale_same, dlogits, dv, loss, ratio_out, s);
}

int arl_ppo_lossgrad_vclip(const uint8_t* dones, const float* v, const float* probs, const float* logp,
                           const int32_t* act, const float* logp_old, const float* adv, const float* ret,
                           const float* v_old, int T, int64_t n, int A, double clip_eps, double vclip_eps, double beta,
                           double pi_loss_coef, double vcoef, int keep_loss_scale_same, float* dlogits, float* dv,
                           float* loss, float* ratio_out, void* s) {
  return ppo_lossgrad("ppo_lossgrad_vclip", true, dones, v, probs, logp, act, logp_old, adv, ret, v_old, T, n, A,
                      clip_eps, vclip_eps, beta, pi_loss_coef, vcoef, keep_loss_scale_same, dlogits, dv, loss,
                      ratio_out, s);
}

int arl_ppo_normalize_adv(const uint8_t* dones, float* adv, int T, int64_t n, double* moments3_device, void* s) {
  if (T < 1 || T > 256 || n < 0 || n > INT32_MAX / 256) return fail(ARL_EINVAL, "ppo_normalize_adv: bad T / n");
  if (n > 0 && (!dones || !adv || !moments3_device)) return fail(ARL_EINVAL, "ppo_normalize_adv: null pointer");
  if (!aligned(moments3_device, 8)) return fail(ARL_EINVAL, "ppo_normalize_adv: moments must be 8-byte aligned");
  return hip_status(arl::launch_ppo_normalize_adv(dones, adv, T, (int)n, moments3_device, S(s)), "ppo_normalize_adv");
}

int arl_ppo_epoch_stats(const uint8_t* dones, const float* v, const float* logp, const int32_t* act,
                        const float* logp_old, const float* adv, const float* ret, const float* ratio,
                        const float* v_old, int T, int64_t n, int A, double clip_eps, double vclip_eps, double window,
                        double epoch, double* record10_device, void* s) {
  if (const int rc = ppo_dims_ok("ppo_epoch_stats", T, n, A)) return rc;
  if (n > 0 && (!dones || !v || !logp || !act || !logp_old || !adv || !ret || !ratio || !record10_device))
    return fail(ARL_EINVAL, "ppo_epoch_stats: null pointer");
  if (const int rc = clip_eps_ok("ppo_epoch_stats", clip_eps)) return rc;
  if (!vclip_ok(vclip_eps) || (v_old && !(vclip_eps > 0.0)))
    return fail(ARL_EINVAL, "ppo_epoch_stats: vclip_eps must be finite and >= 0, > 0 with v_old");
  if (!aligned(record10_device, 8)) return fail(ARL_EINVAL, "ppo_epoch_stats: the record must be 8-byte aligned");
  arl::PpoLossArgs p = ppo_entry_args(dones, v, logp, act, logp_old, adv, ret, T, n, A, clip_eps);
  p.ratio = const_cast<float*>(ratio);   // (read only)
  p.vold = v_old;
  p.ev = (float)vclip_eps;
  return hip_status(arl::launch_ppo_epoch_stats(p, nullptr, window, epoch, nullptr, record10_device, S(s)),
                    "ppo_epoch_stats");
}

int arl_stream_copy(const void* src, void* dst, int64_t bytes, int blocks, int mode, void* s) {
  if (bytes < 0 || (bytes > 0 && (!src || !dst))) return fail(ARL_EINVAL, "stream_copy: null pointer / bytes < 0");
  if (bytes % 16 || !aligned(src, 16) || !aligned(dst, 16)) return fail(ARL_EINVAL, "stream_copy: 16-byte units");
  if (mode < 0 || mode > 3) return fail(ARL_EINVAL, "stream_copy: mode must be 0, 1, 2 or 3");
  if (mode < 2 && (blocks < 1 || blocks > 65535)) return fail(ARL_EINVAL, "stream_copy: blocks out of [1, 65535]");
  if (bytes == 0) return ARL_OK;
  return hip_status(arl::launch_stream_copy(src, dst, bytes, blocks, mode, S(s)), "stream_copy");
}

}  // extern "C"
