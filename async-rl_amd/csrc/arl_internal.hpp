// Internal declarations shared by the HIP translation units of libasyncrl_hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/asyncrl_hip.h"
#include "fastdiv.hpp"

// propagate a failed launch / runtime call out of a function that returns hipError_t
#define ARL_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return _e; } while (0)

namespace arl {

// control block (device int64[16]), read by kernels so that a captured window
// replays with advancing step counters (no frozen kernel arguments)
// CTL_STEP_SNAP: the step counter as the learner saw it (written at learn start),
// read by the fused optimizer for the lr anneal so it can advance CTL_STEP itself
// CTL_ZERO: never written (0 after arl_net_reset); the step base of draws keyed by a host counter
// CTL_ADAM_T: Adam updates made so far (adam_tick_kernel counts, adam_kernel reads; optim.hip)
enum { CTL_STEP = 0, CTL_WINDOW = 1, CTL_STEP_SNAP = 2, CTL_ADAM_T = 3, CTL_ZERO = 15, CTL_SIZE = 16 };

enum Arch { ARCH_FF = 0, ARCH_LSTM = 1, ARCH_FF_NATURE = 2 };
// arch flag: RGB (Doom) observations, train_a3c_doom.py:25-63 (NIPSDQNHead(n_input_channels=3)
// on one RGB screen); conv1 sees [0, R, G, B] so the fused kernels keep K = 256
constexpr int ARCH_RGB = 16;
// arch flag: observations are whole 4-screen stacks (ale.py:91-94 ALE.state), one per ring slot
// (frames (R, n, 4, 84, 84)) -- the layout of the reference-semantics A3C.act drop-in
constexpr int ARCH_STACK = 32;
// arch flag: observations are float32 (4, 84, 84) states -- whatever the A3C phi plugin returns
// (a3c.py:34,50,73; identity by default), one per ring slot (frames (R, n, 4, 84, 84) f32); the
// convs run on the generic implicit-GEMM template (states.hip)
constexpr int ARCH_STATES = 64;
// frame layout of the ring, as the conv kernels read it (conv input plane c of window step t):
// (the kernels reduce the device counter once, rs = k mod R through the host's FastDiv of R, and wrap
// window-local offsets such as rs + R - 3 + c with a compare and subtract: no runtime-divisor % in device code)
//   FRAMES_RING  one screen per slot, plane c = slot (k - 3 + c) % R   (k = ctl[STEP] + t)
//   FRAMES_RGB   three planes per slot [0, R, G, B] of slot k % R
//   FRAMES_STACK four planes per slot, plane c of slot k % R
//   FRAMES_STATES four f32 planes per slot (ARCH_STATES), plane c of slot k % R
enum FrameLayout { FRAMES_RING = 0, FRAMES_RGB = 1, FRAMES_STACK = 2, FRAMES_STATES = 3 };
// index (in 84 x 84 planes) of conv input plane c of env e at the obs step in ring slot rs = k mod R, for the three
// uint8 layouts; selects only, so the four plane loads of a thread go out back to back (RGB: plane 0 is the
// zero pad and re-reads plane 1's bytes, which the caller zeroes through nvalid = 3)
__device__ inline int64_t ring_plane(int layout, int rs, int R, int n, int e, int c) {
  const int slot = layout == FRAMES_RING ? fd_wrap(rs + R - 3 + c, R) : rs;
  const int mult = layout == FRAMES_STACK ? 4 : layout == FRAMES_RGB ? 3 : 1;
  const int sub = layout == FRAMES_STACK ? c : layout == FRAMES_RGB ? (c > 0 ? c - 1 : 0) : 0;
  return ((int64_t)slot * n + e) * mult + sub;
}

constexpr int PLANE = 84 * 84;         // 7056 B per screen
constexpr int PAIR = 2 * 210 * 160 * 3; // 201,600 B per frame pair
constexpr int C1_OC = 16, C1_P = 400;  // conv1: 16 x 20 x 20
constexpr int C2_OC = 32, C2_P = 81;   // conv2: 32 x 9 x 9
constexpr int A1 = C1_OC * C1_P;       // 6400
constexpr int A2 = C2_OC * C2_P;       // 2592
constexpr int A2W = A2 / 32;             // 81 u32 words of a2 > 0 bits per env-step (fc_bwd job B mask)
static_assert(A2 % 32 == 0, "mask words");
constexpr int HID = 256;
constexpr int GATES = 4 * HID;
constexpr int ZERO_ROW_FLOATS = 64;     // LSTM: the zero row a reset sample's h_prev is DMA'd from (fc_bwd.hip)
constexpr int MAXA = 32;               // max actions supported by the policy kernel
// NatureDQNHead (dqn_head.py:6-28): 4->32 k8 s4 (20x20), 32->64 k4 s2 (9x9),
// 64->64 k3 s1 (7x7), Linear 3136 -> 512
constexpr int NC1 = 32, NP1 = 400, NC2 = 64, NP2 = 81, NC3 = 64, NP3 = 49;
constexpr int NA1 = NC1 * NP1, NA2 = NC2 * NP2, NA3 = NC3 * NP3;   // 12800, 5184, 3136
constexpr int NHID = 512;

struct RingArgs {
  const uint8_t* pair_pool;   // (pool_len, n, 2, 210, 160, 3)
  const float* reward_pool;   // (pool_len, n) or null
  const uint8_t* done_pool;   // (pool_len, n) or null
  int64_t pool_len;
  FastDiv dpool, dR;          // pool_len and R as divisors of the step counter (fastdiv.hpp), filled by the host
  FastDiv dchunks;            // RGB nets: 16-byte chunks of a source row, W * 3 / 16 (launch_rgb_ring fills it)
  uint8_t* frames;            // (R, n, 84, 84)
  uint8_t* nvalid;            // (R, n)
  uint8_t* reset_flags;       // (T+1, n)
  float* rewards;             // (T, n)
  uint8_t* dones;             // (T, n)
  const int64_t* ctl;
  int n, R, t, mode, force_reset;
  int H = 0, W = 0;           // RGB nets: pair_pool is an image pool (pool_len, n, H, W, 3)
  int e0 = 0, ne = -1;        // env range of this launch: e0 + blockIdx.y, ne envs (-1: all n)
  int esize = 1;              // stack_ring_kernel: bytes per stack element (1 uint8 screens, 4 f32 states)
  char* episodes = nullptr;   // episode-statistics block (EpisodeView below); null: the feature is off
};

// Device-side episode statistics (arl_net_set_episode_stats; a3c_ale.py:95-96,114-124: episode_r / total_r of
// train_loop).  One block at the end of the workspace, 14 arrays of 8-byte elements, each starting 256-byte
// aligned in this order: 11 per-env arrays (n) and 3 logs (EPISODE_LOG, n).  The env's bookkeeping thread of the
// ring kernels is the only writer of column e (no atomics); all sums are f64 with explicit *_rn ops, so a NumPy
// f64 replay in env-step order is bit-identical.
constexpr int EPISODE_LOG = 8;
constexpr int EP_ENV_ARRAYS = 11, EP_LOG_ARRAYS = 3;
__host__ __device__ constexpr int64_t ep_align(int64_t b) { return (b + 255) / 256 * 256; }
__host__ __device__ constexpr int64_t episode_block_bytes(int64_t n) {
  return EP_ENV_ARRAYS * ep_align(n * 8) + EP_LOG_ARRAYS * ep_align(EPISODE_LOG * n * 8);
}
struct EpisodeView {
  double* run_ret;      // return of the running episode
  int64_t* run_len;     // its length so far
  double* total;        // sum of every reward ingested (total_r)
  int64_t* steps;       // rewards ingested
  int64_t* count;       // episodes completed
  double *sum, *sumsq, *mn, *mx;   // of the completed episodes' returns (count 0: mn = +inf, mx = -inf)
  int64_t* len_sum;     // sum of their lengths
  int64_t* log_count;   // episodes ever appended to the log (not cleared by a reduce)
  double* log_ret;      // (EPISODE_LOG, n): entry count % EPISODE_LOG of env e = (return, length, obs index)
  int64_t *log_len, *log_step;
};
__host__ __device__ inline EpisodeView episode_view(char* base, int64_t n) {
  const int64_t se = ep_align(n * 8), sl = ep_align(EPISODE_LOG * n * 8);
  EpisodeView v;
  v.run_ret = reinterpret_cast<double*>(base);
  v.run_len = reinterpret_cast<int64_t*>(base + se);
  v.total = reinterpret_cast<double*>(base + 2 * se);
  v.steps = reinterpret_cast<int64_t*>(base + 3 * se);
  v.count = reinterpret_cast<int64_t*>(base + 4 * se);
  v.sum = reinterpret_cast<double*>(base + 5 * se);
  v.sumsq = reinterpret_cast<double*>(base + 6 * se);
  v.mn = reinterpret_cast<double*>(base + 7 * se);
  v.mx = reinterpret_cast<double*>(base + 8 * se);
  v.len_sum = reinterpret_cast<int64_t*>(base + 9 * se);
  v.log_count = reinterpret_cast<int64_t*>(base + 10 * se);
  char* lg = base + EP_ENV_ARRAYS * se;
  v.log_ret = reinterpret_cast<double*>(lg);
  v.log_len = reinterpret_cast<int64_t*>(lg + sl);
  v.log_step = reinterpret_cast<int64_t*>(lg + 2 * sl);
  return v;
}
// zero the whole block of n envs (mn = +inf, mx = -inf)
hipError_t launch_episode_reset(char* block, int n, hipStream_t s);
// out8 = [episodes, return_sum, return_sumsq, return_min, return_max, length_sum, steps, reward_sum] over the n
// envs in a fixed order (phi.hip episode_reduce_kernel); clear: also zero the cumulative per-env arrays
hipError_t launch_episode_reduce(char* block, int n, double* out8, int clear, hipStream_t s);

// Device-resident envs (env_kernel.hpp, with the games in catch.hip, breakout.hip, pong.hip, tmaze.hip and maze.hip; the header's "device
// environment"): one launch = one env-step (or the reset) of envs [e0, e0 + ne): transition + render into pool
// entry (k + 1) % pool_len (reset: k % pool_len), k = ctl[CTL_STEP] + t read on the device; the state half read
// is k & 1, the half written (k + 1) & 1.
constexpr int CATCH_STATE_INTS = 8;       // [bx, by, vx, px, episode, steps_in_episode, 0, 0]
constexpr int BREAKOUT_STATE_INTS = 16;   // [bx, by, vx, vy, px, lives, serves, steps_in_episode, game, game_steps,
                                          //  score, bricks_left, b0, b1, b2, b3]
constexpr int PONG_STATE_INTS = 12;       // [bx, by, vx, vy, py, oy, serves, steps_in_episode, game, game_steps,
                                          //  score_agent, score_opp]
constexpr int TMAZE_STATE_INTS = 8;       // [pos, cue, length, steps_in_episode, episode, hits, misses, lapses]
constexpr int MAZE_STATE_INTS = 8;        // [pos | goal << 8, bits, steps_in_episode, episode, wins, timeouts, level, cfg]
struct EnvArgs {
  int32_t* state;            // (2, n, the game's STATE_INTS), 16-byte aligned
  const int32_t* actions;    // (n): the actions of observation k; null: reset (episode 0 into half k & 1)
  const int64_t* ctl;        // the control block; null: k = t (the granular calls: t = the parity, pool_len 1)
  int64_t t;
  FastDiv dpool;             // pool_len as a divisor of the step counter, filled by the host
  uint8_t* pair_pool;        // (pool_len, n, 2, 210, 160, 3)
  float* reward_pool;        // (pool_len, n)
  uint8_t* done_pool;        // (pool_len, n)
  int n;
  int e0 = 0, ne = -1;       // env range of this launch: e0 + blockIdx.y, ne envs (-1: all n)
  int env_offset = 0;
  uint32_t seed_lo = 0, seed_hi = 0;
  int flags = 0;             // filled by launch_env from the kind: Breakout's ARL_ENV_GAME_OVER_ONLY or 0, Pong's
                             // points (1..21), the T-maze's length (1..8), the maze's packed (rooms, view, levels); Catch ignores it
};
struct Catch;      // the games: catch.hip, breakout.hip, pong.hip, tmaze.hip and maze.hip each instantiate their launch_game
struct Breakout;
struct Pong;
struct TMaze;
struct Maze;
template <class Game> hipError_t launch_game(const EnvArgs& a, hipStream_t s);   // env_kernel.hpp
extern template hipError_t launch_game<Catch>(const EnvArgs&, hipStream_t);
extern template hipError_t launch_game<Breakout>(const EnvArgs&, hipStream_t);
extern template hipError_t launch_game<Pong>(const EnvArgs&, hipStream_t);
extern template hipError_t launch_game<TMaze>(const EnvArgs&, hipStream_t);
extern template hipError_t launch_game<Maze>(const EnvArgs&, hipStream_t);

// The library's only look at an env kind (ARL_ENV_*, a Breakout's with an optional ARL_ENV_GAME_OVER_ONLY, a
// Pong's with its points in bits 16 and up: 1..21, 0 = 21, a T-maze's with its length there: 1..8, 0 = 4, a
// maze's with its rooms in bits 16..18: 2..4, 0 = 3, its view in bits 19..20: 0..2, and its levels in bits 21..30;
// no other bit).
constexpr int PONG_POINTS_MAX = 21;
constexpr int TMAZE_LENGTH_MAX = 8, TMAZE_LENGTH_DEFAULT = 4;
constexpr bool env_is_breakout(int kind) { return (kind & ~ARL_ENV_GAME_OVER_ONLY) == ARL_ENV_BREAKOUT; }
constexpr bool env_is_pong(int kind) {
  return kind >= 0 && (kind & 0xffff) == ARL_ENV_PONG && (kind >> 16) <= PONG_POINTS_MAX;
}
constexpr int pong_points(int kind) { return (kind >> 16) ? (kind >> 16) : PONG_POINTS_MAX; }
constexpr bool env_is_tmaze(int kind) {
  return kind >= 0 && (kind & 0xffff) == ARL_ENV_TMAZE && (kind >> 16) <= TMAZE_LENGTH_MAX;
}
constexpr int tmaze_length(int kind) { return (kind >> 16) ? (kind >> 16) : TMAZE_LENGTH_DEFAULT; }
constexpr int MAZE_ROOMS_MIN = 2, MAZE_ROOMS_MAX = 4, MAZE_ROOMS_DEFAULT = 3, MAZE_VIEW_MAX = 2, MAZE_LEVELS_MAX = 1023;
constexpr bool maze_fields_ok(int rooms, int view, int levels) {
  return rooms >= MAZE_ROOMS_MIN && rooms <= MAZE_ROOMS_MAX && view >= 0 && view <= MAZE_VIEW_MAX && levels >= 0 &&
         levels <= MAZE_LEVELS_MAX;
}
constexpr int maze_rooms(int kind) { return ((kind >> 16) & 7) ? ((kind >> 16) & 7) : MAZE_ROOMS_DEFAULT; }
constexpr bool env_is_maze(int kind) {
  return kind >= 0 && (kind & 0xffff) == ARL_ENV_MAZE && maze_fields_ok(maze_rooms(kind), (kind >> 19) & 3, kind >> 21);
}
// what the kernel takes as its flags and keeps in the state row: rooms | view << 3 | levels << 5
constexpr int maze_cfg(int kind) { return ((kind >> 16) & ~7) | maze_rooms(kind); }
constexpr bool env_kind_ok(int kind) {
  return kind == ARL_ENV_CATCH || env_is_breakout(kind) || env_is_pong(kind) || env_is_tmaze(kind) || env_is_maze(kind);
}
constexpr int env_state_ints(int kind) {
  return env_is_maze(kind)       ? MAZE_STATE_INTS
         : env_is_tmaze(kind)    ? TMAZE_STATE_INTS
         : env_is_pong(kind)     ? PONG_STATE_INTS
         : env_is_breakout(kind) ? BREAKOUT_STATE_INTS
                                 : CATCH_STATE_INTS;
}
inline hipError_t launch_env(int kind, const EnvArgs& a, hipStream_t s) {
  EnvArgs f = a;
  if (env_is_maze(kind)) {
    f.flags = maze_cfg(kind);
    return launch_game<Maze>(f, s);
  }
  if (env_is_tmaze(kind)) {
    f.flags = tmaze_length(kind);
    return launch_game<TMaze>(f, s);
  }
  if (env_is_pong(kind)) {
    f.flags = pong_points(kind);
    return launch_game<Pong>(f, s);
  }
  f.flags = kind & ARL_ENV_GAME_OVER_ONLY;
  return env_is_breakout(kind) ? launch_game<Breakout>(f, s) : launch_game<Catch>(f, s);
}

// The direct-to-ring launch (env_direct.hpp; arl_net_set_env_direct): the env-step and its observation in one launch,
// no pools.  env: launch_env's arguments without the pools (actions null: the reset form).  ring: the observation
// this launch produces -- ring.t = env.t + 1 (the reset: 0, with force_reset), ring.n = env.n; its pools are not
// read.  The granular call (arl_env_step_screen): ring.nvalid == null, ring.dR = 1, the planes go to ring.frames
// (n, 84, 84) and the raw reward / done to reward_out / done_out.
struct DirectArgs {
  EnvArgs env;
  RingArgs ring;
  float* reward_out = nullptr;
  uint8_t* done_out = nullptr;
};
template <class Game> hipError_t launch_game_direct(const DirectArgs& a, hipStream_t s);   // env_direct.hpp
extern template hipError_t launch_game_direct<Catch>(const DirectArgs&, hipStream_t);
extern template hipError_t launch_game_direct<Breakout>(const DirectArgs&, hipStream_t);
extern template hipError_t launch_game_direct<Pong>(const DirectArgs&, hipStream_t);
extern template hipError_t launch_game_direct<TMaze>(const DirectArgs&, hipStream_t);
extern template hipError_t launch_game_direct<Maze>(const DirectArgs&, hipStream_t);
inline hipError_t launch_env_direct(int kind, const DirectArgs& a, hipStream_t s) {
  DirectArgs f = a;
  if (env_is_maze(kind)) {
    f.env.flags = maze_cfg(kind);
    return launch_game_direct<Maze>(f, s);
  }
  if (env_is_tmaze(kind)) {
    f.env.flags = tmaze_length(kind);
    return launch_game_direct<TMaze>(f, s);
  }
  if (env_is_pong(kind)) {
    f.env.flags = pong_points(kind);
    return launch_game_direct<Pong>(f, s);
  }
  f.env.flags = kind & ARL_ENV_GAME_OVER_ONLY;
  return env_is_breakout(kind) ? launch_game_direct<Breakout>(f, s) : launch_game_direct<Catch>(f, s);
}

// RGB (Doom) observations, train_a3c_doom.py:21-23 / doom_env.py:47
constexpr int RGB_MAX_W = 2048;  // staged source rows: 12 x W x 3 bytes of LDS
hipError_t launch_rgb_phi(const uint8_t* imgs, int64_t n, int H, int W, float* out, int mode, hipStream_t s);
hipError_t launch_rgb_ring(const RingArgs& a, hipStream_t s);
hipError_t launch_stack_ring(const RingArgs& a, hipStream_t s);   // ARCH_STACK / ARCH_STATES nets

hipError_t launch_current_screen(const uint8_t* cur, const uint8_t* prev, uint8_t* out, int64_t n,
                                 int mode, hipStream_t s);
hipError_t launch_phi_stack(const uint8_t* pairs, const uint8_t* prev_stack, const uint8_t* reset,
                            uint8_t* out_stack, int64_t n, int mode, hipStream_t s);
hipError_t launch_phi_ring(const RingArgs& a, hipStream_t s);
hipError_t launch_max_luminance(const uint8_t* cur, const uint8_t* prev, uint8_t* gray, int64_t npix,
                                hipStream_t s);
hipError_t launch_dqn_phi(const uint8_t* in, float* out, int64_t count, hipStream_t s);

// ---------------------------------------------------------------- network
// NonbiasWeightDecay folded into the update (optim.hip): g += rate * p after the clip, except inside the
// bias tensors' float ranges [begin[k], end[k]) of the flat layout (k < n_bias; net_init builds them from
// the parameter names).  n_bias == 0: every element decays (one array, arl_rmsprop_wd).
constexpr int DECAY_MAX_BIAS = 8;
struct DecayArgs {
  float rate;               // f32(rate), as the Python float meets the f32 arrays; 0: no decay
  int n_bias;
  int64_t begin[DECAY_MAX_BIAS], end[DECAY_MAX_BIAS];
};

struct ParamInfo {
  std::string name;   // Chainer namedparam / HDF5 path, e.g. "0/0/W"
  int64_t offset;     // floats into the flat buffer (64-float aligned)
  int64_t numel;
};

// window timeline (measurement, arl_stamps_*): while `on`, every stage launch of a window records a
// timing event on its stream right after the kernel(s) and remembers the stage (Stage) it closes, so
// the intervals between consecutive stamps split one eager window into its stages as it ran
struct Stamps {
  std::vector<hipEvent_t> ev;
  std::vector<int> stage;
  std::vector<int64_t> seq;   // the stamp call each recorded event answers
  int count = 0;
  bool on = false;
  int period = 0;             // > 0: sparse (arl_stamps_sparse): window w records only calls t - 1, t of its
  int64_t calls = 0;          //   period, t = w mod period
};

// Kernel forms of a net (arl_net_set_form): ARL_FORM_AUTO or a concrete value each.  The resolvers below are the
// only place a form is decided: the launches (conv_fwd.hip, fc.hip, net.hip, conv_bwd.hip) and arl_net_form call
// them at issue time.  All forms of a launch are bit-identical (tests/test_gpu_parity.py).
struct Forms {
  int conv_epw = ARL_FORM_AUTO, fc_big = ARL_FORM_AUTO, lstm_xred = ARL_FORM_AUTO, conv_bwd_ws = ARL_FORM_AUTO;
};
// conv forward: two envs a workgroup (16 waves sharing the weight planes) in nets of >= 512 envs, whether the
// launch covers all of them or one env group's range (C4 0.513 -> 0.503 ms, C3 1.227 -> 1.212 ms at two groups,
// profiles/r03/r3k)
inline int conv_fwd_epw(const Forms& f, int net_envs) {
  return f.conv_epw != ARL_FORM_AUTO ? f.conv_epw : (net_envs >= 512 ? 2 : 1);
}
// FC forward: launches over >= 512 envs on the 64-row tiles (C4 0.503 -> 0.497 ms at one env group, C3 1.215 ->
// 1.162 ms; at 256-env launches, 128 workgroups of them lose: profiles/r03/r3l)
inline bool fc_fwd_big(const Forms& f, int launch_envs) {
  return f.fc_big != ARL_FORM_AUTO ? f.fc_big == 1 : launch_envs >= 512;
}
// Where the LSTM step's FC split-K partials are reduced: in the gate kernel's staging (XRED) for launches under
// 512 envs, by the FC's last-arriver ticket for 512 and more (fc_fwd_kernel's tail; the gate kernel then stages
// hfc: every one of its 16 column-tile workgroups of a row block otherwise re-reads the block's 8 partial slabs
// -- C3 1.185 -> 1.160 ms, profiles/r03/r3aa)
inline bool lstm_xred(const Forms& f, int launch_envs) {
  return f.lstm_xred != ARL_FORM_AUTO ? f.lstm_xred == 1 : launch_envs < 512;
}
// conv backward: the wave-specialised kernel; 0 = the 512-thread kernel it is bit-identical to (conv_bwd 106.7 ->
// 89.1 us in the C4 window, profiles/r06/ws)
inline bool conv_bwd_ws(const Forms& f) { return f.conv_bwd_ws != 0; }

struct Net {
  int arch, A, N, T, R;
  Forms forms;                // arl_net_set_form
  FastDiv dR, dN;             // R and N as device-side divisors (net_init)
  Stamps* stamps = nullptr;   // null / off: stamp() is a no-op
  bool rgb = false;        // ARCH_RGB: 3 planes per obs step in the ring, conv1 W (16, 3, 8, 8)
  bool stack = false;      // ARCH_STACK: 4 planes (a whole stack) per obs step in the ring
  bool states = false;     // ARCH_STATES: 4 f32 planes (phi's output) per obs step in the ring
  int layout = FRAMES_RING;
  // loss options (a3c.py:110-121): pi_loss_coef, keep_loss_scale_same (arl_net_set_loss)
  float pi_coef = 1.f;
  int keep_scale = 0;
  // NonbiasWeightDecay of the update: the rate (arl_net_set_weight_decay; 0 = the hook is not installed)
  // and the bias tensors it skips, from the names in `params` (net_init)
  DecayArgs decay{};
  // arl_net_set_adam: non-null = every update of the net runs adam_kernel (first moment here, the second
  // in ms, the update count in ctl[CTL_ADAM_T]) instead of rmsprop_kernel
  float* adam_m = nullptr;
  double adam_beta1 = 0.9, adam_beta2 = 0.999;
  // arl_net_set_env: non-null = a device-resident env steps from the actions buffer (arl_env_step, and
  // arl_run_window after every arl_act(t), t < T); its double-buffered state (2, N, env_state_ints(env_kind))
  // and the kind it was attached as (ARL_ENV_*, with ARL_ENV_GAME_OVER_ONLY or'ed in)
  int32_t* env_state = nullptr;
  int env_kind = 0;
  // arl_net_set_env_direct: the attached env renders straight into the frame ring (arl_env_reset_observe,
  // arl_env_step_observe, and arl_run_window without pools); cleared when the env is detached
  bool env_direct = false;
  int64_t eval_draws = 0;  // sampling forward_states calls so far (Philox stream 1 counter)
  // clip norm folded into the learner's conv reduce (arl_net_set_norm_fold; only valid when
  // nothing changes the gradient between arl_learn and the update, e.g. no all-reduce):
  // norm_ready = the last arl_learn left the partials, consumed by the next update
  bool norm_fold = false, norm_ready = false;
  // parameter generations: every writer of the params the library does not make itself bumps param_gen
  // (arl_net_bind, arl_net_params_changed); planes_gen = the generation the FC weight's split planes
  // (w_fcplanes) were built from.  A forward over all envs rebuilds stale planes on its own stream
  // (fc_planes_kernel); an env-range forward refuses them (arl_net_prepare first, before the streams
  // fork); every in-window update rewrites all planes from the new W (rmsprop_kernel).
  uint64_t param_gen = 1, planes_gen = 0;
  bool planes_current() const { return planes_gen == param_gen; }
  // the learner's returns folded into the bootstrap step's policy launch (FF, arl_run_window):
  // fuse_returns = on, with the learn arguments below, for the window's slot-T forward; returns_done = that
  // launch ran, so the window's LEARN_RETURNS part is a no-op
  struct ReturnsCfg { double gamma; float beta, vcoef; int clip_reward; };
  bool fuse_returns = false, returns_done = false;
  ReturnsCfg ret{};
  int norm_rest_blocks = 64;
  bool episode_stats = false;   // arl_net_set_episode_stats: the observations accumulate into w_episodes
  // arl_net_set_window_stats: every net_optimize appends a record to w_win_log (window_stats_kernel, optim.hip);
  // win_gamma / win_clip_reward = those of the net's last returns launch, which the record's returns repeat
  bool window_stats = false;
  double win_gamma = 0.99;
  int win_clip_reward = 1;
  // GAE(lambda) advantages of the policy term (arl_net_set_gae; 1 = the n-step advantage, today's kernels):
  // read at every returns launch; win_lambda = that of the net's last returns launch, beside win_gamma
  double gae_lambda = 1.0, win_lambda = 1.0;
  // arl_net_set_ppo: non-null = the window's update runs as clipped-surrogate epochs (arl_ppo_begin, arl_ppo_learn)
  // on this snapshot, 4 planes of T * N f32: logp_old, adv, ret, ratio; ppo_lo / ppo_hi = the clip range as f32;
  // ppo_begun = arl_ppo_begin took the snapshot of the current window (cleared by the window advance)
  float* ppo_snap = nullptr;
  float ppo_lo = 0.8f, ppo_hi = 1.2f;
  bool ppo_begun = false;
  // arl_net_set_ppo_options, read when arl_ppo_begin / arl_ppo_learn launch: ppo_norm_adv = normalise the
  // snapshot's advantages; ppo_vold non-null = value clipping within ppo_ev = (float)vclip_eps of it (T * N f32);
  // ppo_aux non-null = the moments and the per-epoch records (ARL_PPO_AUX_DOUBLES f64); ppo_epoch = epochs
  // launched since the last arl_ppo_begin (the record's 1-based epoch)
  bool ppo_norm_adv = false;
  float* ppo_vold = nullptr;
  float ppo_ev = 0.f;
  double* ppo_aux = nullptr;
  int ppo_epoch = 0;
  // arl_net_set_ppo_state (LSTM): non-null = the carry buffer, 2 planes (h, c) of N * HID f32.  arl_ppo_begin saves
  // rows T of hbuf / cbuf there; the advancing update puts them back before anything advances (net_ppo_restore)
  float* ppo_carry = nullptr;
  int hid;              // width of the layer the heads read (256 NIPS / LSTM, 512 Nature)
  int env_offset;          // global id of env 0 on this rank (RNG stream)
  uint64_t seed;
  std::vector<ParamInfo> params;
  int64_t param_floats;    // padded flat length
  // parameter offsets (floats)
  int64_t o_c1W, o_c1b, o_c2W, o_c2b, o_fcW, o_fcb, o_luW, o_lub, o_llW, o_piW, o_pib, o_vW, o_vb;
  int64_t o_c3W = -1, o_c3b = -1;   // Nature head only
  // workspace layout (byte offsets)
  struct Buf { const char* name; int64_t off, bytes; };
  std::vector<Buf> bufs;
  int64_t ws_bytes;
  int64_t w_ctl, w_frames, w_nvalid, w_reset, w_rewards, w_dones, w_a1, w_a2, w_hfc, w_gates, w_hbuf,
      w_cbuf, w_logits, w_probs, w_logp, w_v, w_ent, w_logpa, w_act, w_dlogits, w_dv, w_dh, w_dfc,
      w_dG, w_dhn, w_dcn, w_da2, w_slab, w_norm, w_loss, w_tick, w_fcb_part = 0, w_fcb_tick = 0, w_zero = 0,
      w_a2m = 0,   // (T+1, N, 81) a2 > 0 bits (ring-frame NIPS nets; 0: none)
      w_fcplanes = 0;   // FC_PLANES_BYTES: the FC weight's bf16 split planes (NIPS nets)
  int64_t w_win_log = 0, w_win_count = 0;   // (WINDOW_LOG, WINDOW_STAT_FIELDS) f64 ring of records; int64 records written
  int64_t w_episodes = 0;   // episode_block_bytes(N): the episode statistics (EpisodeView), last in the workspace
  int64_t w_a3 = 0, w_da1 = 0, w_da3 = 0;   // Nature head only (w_da1 also ARCH_STATES)
  // LSTM recurrent state of pi_and_v on explicit states (A3CLSTM.pi_and_v, a3c_ale.py:55-63):
  // h, c (n, 256), the step's outputs hn, cn, and reset flags (1 = state is None)
  int64_t w_eval_h = 0, w_eval_c = 0, w_eval_hn = 0, w_eval_cn = 0, w_eval_reset = 0;
  int64_t slab_floats;
  int norm_blocks;
  // bound pointers
  float* p = nullptr;
  float* g = nullptr;
  float* ms = nullptr;
  char* ws = nullptr;
  template <class T> T* at(int64_t off) const { return reinterpret_cast<T*>(ws + off); }
};

bool net_init(Net& net, int arch, int n_actions, int n_envs, int t_max, int env_offset, uint64_t seed,
              std::string& err);
// mode: 0 none, 1 sample, 2 greedy, | ACT_CONV_ONLY / ACT_AFTER_CONV (env-group staggering:
// the step split after its conv launch); envs [e0, e0 + ne) (ne < 0: all)
constexpr int ACT_CONV_ONLY = 4, ACT_AFTER_CONV = 8;
hipError_t net_act(Net& net, int t, int mode, hipStream_t s, int e0 = 0, int ne = -1);
hipError_t ensure_fc_planes(Net& net, hipStream_t s);   // rebuild the FC weight planes if stale (net.hip)
// learner parts (net_learn_part), in this order on one stream
enum { LEARN_RETURNS = 0, LEARN_TRUNK, LEARN_CONV, LEARN_PARTS };
hipError_t net_learn_part(Net& net, int part, double gamma, float beta, float vcoef, int clip_reward, hipStream_t s);
hipError_t net_learn(Net& net, double gamma, float beta, float vcoef, int clip_reward, hipStream_t s);
// what every returns launch of a net (or the PPO snapshot standing in for one) leaves for the window statistics
inline void note_returns_launch(Net& net, double gamma, int clip_reward) {
  net.win_gamma = gamma;
  net.win_clip_reward = clip_reward;
  net.win_lambda = net.gae_lambda;
}
// PPO epochs (net.ppo_snap set, FF): the window's snapshot after its bootstrap forward, and one epoch's gradient
// from the slots' current contents (loss gradient + heads dh, LEARN_TRUNK, LEARN_CONV; no folded clip norm)
hipError_t net_ppo_begin(Net& net, double gamma, int clip_reward, hipStream_t s);
hipError_t net_ppo_learn(Net& net, float beta, float vcoef, hipStream_t s);
// advance: also end the window, folded into the update kernel (arl_learn
// snapshots the step counter, so the update's lr anneal does not race it).
hipError_t net_optimize(Net& net, double lr0, int64_t total_steps, int64_t n_total, double alpha, double eps,
                        float clip, hipStream_t s, bool advance = false);
hipError_t net_advance(Net& net, hipStream_t s);
enum Stage { STAGE_CONV_FWD = 1, STAGE_FC_FWD = 2, STAGE_POLICY = 3, STAGE_FC_BWD = 4, STAGE_CONV_BWD = 5,
             STAGE_RETURNS = 6, STAGE_CONV_REDUCE = 7, STAGE_GRAD_SQNORM = 8,
             STAGE_LSTM_GATES = 9, STAGE_LSTM_BPTT = 10, STAGE_LSTM_WGRAD = 11,
             // stamp-only stages (timeline, not arl_run_stage): the observation, the update kernel,
             // the separate LSTM cell launches, a caller's stamp (e.g. after a collective), others
             STAGE_PHI = 12, STAGE_RMSPROP = 13, STAGE_LSTM_CELL = 14, STAGE_HOST = 15, STAGE_OTHER = 16 };
// record the stamp closing `stage` on stream s (no-op unless the net's timeline is on)
inline hipError_t stamp(const Net& net, int stage, hipStream_t s) {
  Stamps* st = net.stamps;
  if (st == nullptr || !st->on || st->count >= (int)st->ev.size()) return hipSuccess;
  const int64_t q = st->calls++;
  if (st->period > 0) {
    const int64_t P = st->period, i = q % P, t = (q / P) % P;
    if (i != t && i != t - 1) return hipSuccess;
  }
  st->stage[st->count] = stage;
  st->seq[st->count] = q;
  return hipEventRecord(st->ev[st->count++], s);
}
hipError_t net_stage(Net& net, int stage, int t, hipStream_t s);
// keep: LSTM keep_same_state (the pi_and_v recurrent state is not advanced)
hipError_t net_forward_f32(Net& net, const float* x, int n, int mode, hipStream_t s, bool keep = false);
hipError_t net_reset_state(Net& net, int e0, int n, hipStream_t s);

// Nature head (nature.hip)
int64_t nature_slab_floats(const Net& net);
hipError_t nature_act(Net& net, int t, int mode, hipStream_t s);
hipError_t nature_forward_f32(Net& net, const float* x, int n, int mode, hipStream_t s);
hipError_t nature_learn(Net& net, double gamma, float beta, float vcoef, int clip_reward, hipStream_t s);
hipError_t nature_stage(Net& net, int stage, int t, hipStream_t s);

// ARCH_STATES nets (states.hip): conv1 + conv2 forward of window slot t from the f32
// state ring (all envs), and the conv backward of the window (conv2 dW / db,
// da1, conv1 dW / db) on the generic GEMM, gradients straight into net.g
hipError_t states_conv_fwd(const Net& net, int t, float* a1, float* a2, hipStream_t s);
hipError_t states_conv_bwd(Net& net, hipStream_t s);
int64_t states_slab_floats(const Net& net);

// LSTM gate GEMM + bias (+ the F.lstm cell when cell) for rows [0, n) (lstm.hip)
hipError_t launch_lstm_bptt(const float* dG, const float* Wl, const uint8_t* rs_t, const float* gates, const float* c_t,
                            const float* c_prev, const uint8_t* rs, const float* dH, float* dcn, float* dG_out,
                            float* dhn, int n, bool cell, hipStream_t s);
hipError_t launch_lstm_gates(const float* x, const float* h, const uint8_t* reset, const float* Wu, const float* Wl,
                             const float* b, float* gates, const float* c_prev, float* c_out, float* h_out, int n,
                             bool cell, hipStream_t s, const float* fc_slab = nullptr, const float* fc_b = nullptr,
                             float* hfc = nullptr);

// shared pieces of the heads' backward (net.hip)
hipError_t launch_heads_bwd(const float* dl, const float* dv, const float* Wpi, const float* Wv, int A, int H,
                            const float* mask, float* out, int64_t S, hipStream_t s);

// layout: FrameLayout of the ring (FRAMES_RGB: conv1 W (16, 3, 8, 8) on input planes 1..3)
hipError_t launch_conv_fwd(const uint8_t* frames, const uint8_t* nvalid, const int64_t* ctl, int n, const FastDiv& R,
                           int t,
                           const float* W1, const float* b1, const float* W2, const float* b2, float* a1, float* a2,
                           hipStream_t s, const Forms& forms, int layout = FRAMES_RING, int e0 = 0, int ne = -1,
                           uint32_t* a2m = nullptr);
// the gradient's squared norm folded into the conv slab reduce (parts == null: not folded)
struct NormFold {
  double* parts;            // NORM_SCRATCH f64: conv_norm_parts(rest_blocks) partials
  const float* g;           // the flat gradient
  int64_t rest_begin, rest_end;   // floats of g outside the conv tensors (final before the reduce)
  int rest_blocks;
};
int conv_norm_parts(int rest_blocks);
hipError_t launch_conv_bwd(const uint8_t* frames, const uint8_t* nvalid, const int64_t* ctl, const FastDiv& n,
                           const FastDiv& R, int S,
                           const float* a1, const float* da2, const float* W2, float* slab, float* gW2, float* gb2,
                           float* gW1, float* gb1, hipStream_t s, const Forms& forms, bool reduce = true,
                           int layout = FRAMES_RING, const NormFold& nf = NormFold{});
int64_t conv_bwd_slab_floats(int S);
int conv_bwd_blocks(int S);       // workgroups (= slab slices) of launch_conv_bwd
// the slab reduce launch_conv_bwd(reduce = true) ends with, alone
hipError_t launch_conv_reduce(const float* slab, int S, float* gW2, float* gb2, float* gW1, float* gb1, hipStream_t s,
                              int layout, const NormFold& nf = NormFold{});

// arguments of the softmax policy / value heads (policy_rows.hpp)
struct PolicyArgs {
  const float *Wpi, *bpi, *Wv, *bv;
  int A;
  uint32_t seed_lo, seed_hi;
  const int64_t* ctl;       // step counter (Philox counter = ctl[STEP] + step_off)
  int64_t step_off;
  int env_offset, mode;     // mode: 0 none, 1 sample, 2 greedy
  uint32_t stream;          // Philox counter word 3: 0 = window draws, 1 = pi_and_v draws
  float *logits, *probs, *logp, *v, *ent;
  int32_t* act;
  float* logp_a;
};
inline PolicyArgs make_policy_args(const float* Wpi, const float* bpi, const float* Wv, const float* bv, int A,
                                   uint64_t seed, const int64_t* ctl, int64_t step_off, int env_offset, int mode,
                                   float* logits, float* probs, float* logp, float* v, float* ent, int32_t* act,
                                   float* logp_a) {
  return PolicyArgs{Wpi, bpi, Wv, bv, A, (uint32_t)seed, (uint32_t)(seed >> 32), ctl, step_off, env_offset, mode, 0u,
                    logits, probs, logp, v, ent, act, logp_a};
}

constexpr int FC_SPLIT = 8;   // fc forward split-K (one slice per XCD)
// The FC weight as three exact bf16 split planes (bf16split.hpp), the B operand of fc_fwd_kernel (fc.hip):
// [3][256][FC_PLANE_LD] bf16; split z's 324 columns at z * FC_PLANE_SLICE (16-byte aligned slices, 4 pad
// columns each), the first 320 of a slice permuted within each 32-block so that lane quarter g of a 16x16x32
// fragment reads its 8 k as one 16-byte run: stored 8 g + 4 h + r holds column k = 16 h + 4 g + r.
// Written by fc_planes_kernel (fc.hip) and, for every W the update changes, by rmsprop_kernel (optim.hip).
constexpr int FC_PLANE_SLICE = A2 / FC_SPLIT + 4, FC_PLANE_LD = FC_SPLIT * FC_PLANE_SLICE;   // 328, 2624
constexpr int64_t FC_PLANES_BYTES = (int64_t)3 * HID * FC_PLANE_LD * 2;
__host__ __device__ constexpr int fc_plane_pos(int local) {   // stored position of slice column `local`
  return local >= 320 ? local : (local & ~31) + 8 * ((local >> 2) & 3) + 4 * ((local >> 4) & 1) + (local & 3);
}
// 4 consecutive W elements (flat index e % 4 == 0 within the (256, 2592) tensor) -> 8 bytes per plane
__device__ inline void fc_planes_store(uint16_t* planes, int e, float4 w) {
  const int j = e / A2, k = e - j * A2, z = k / (A2 / FC_SPLIT), loc = k - z * (A2 / FC_SPLIT);
  const int64_t o = (int64_t)j * FC_PLANE_LD + z * FC_PLANE_SLICE + fc_plane_pos(loc);   // 4 consecutive stored
  const float v[4] = {w.x, w.y, w.z, w.w};
  uint32_t h[4], m[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t hb = __float_as_uint(v[i]) & 0xffff0000u;
    const float r1 = __fsub_rn(v[i], __uint_as_float(hb));
    const uint32_t mb = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = __fsub_rn(r1, __uint_as_float(mb));
    h[i] = hb >> 16;
    m[i] = mb >> 16;
    l[i] = __float_as_uint(r2) >> 16;
  }
  constexpr int64_t P = (int64_t)HID * FC_PLANE_LD;
  *reinterpret_cast<uint2*>(planes + o) = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
  *reinterpret_cast<uint2*>(planes + P + o) = make_uint2(m[0] | (m[1] << 16), m[2] | (m[3] << 16));
  *reinterpret_cast<uint2*>(planes + 2 * P + o) = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
}
hipError_t launch_fc_planes(const float* W, uint16_t* planes, hipStream_t s);
int fc_fwd_tiles(int n);      // tickets needed for n envs
// Wp: the FC weight's split planes (FC_PLANE_LD above); tickets == null: split-K partials only (the
// consumer reduces them); else the last-arriver reduce + bias + relu -> hfc in the same launch; 64- or 32-row
// tiles by fc_fwd_big(forms, n)
hipError_t launch_fc_fwd(const float* a2, int n, const uint16_t* Wp, const float* b, float* slab, int* tickets,
                         float* hfc, hipStream_t s, const Forms& forms);
// FC backward (fc_bwd.hip): dW / db straight into the gradient, da2 = (dfc W) * (a2 > 0)
// weight gradients of the policy / value heads (a3c.py:126-130 through
// policy.py / v_function.py Linear layers): rows a < A from dlogits, row A
// from dv, over the S samples of h (fc_bwd's job C)
struct HeadsDW {
  const float* dl;   // (S, A)
  const float* dv;   // (S)
  const float* h;    // (S, HID) fed to the heads
  int A;
  float *gWpi, *gbpi, *gWv, *gbv;
};
hipError_t launch_fc_bwd(const float* dfc, const float* a2, const float* W, int S, float* gW, float* gb, float* da2,
                         float* part, int* tick, hipStream_t s, const HeadsDW* heads = nullptr,
                         const uint32_t* a2m = nullptr);
// LSTM gate weight gradients (upward W / b, lateral W) + dfc = (dG Wu) * (hfc > 0), the same kernel
hipError_t launch_lstm_wgrad(const float* dG, const float* hfc, const float* hprev, const uint8_t* reset,
                             const float* zero, const float* Wu, int S, float* gWu, float* gWl, float* gbu, float* dfc,
                             float* part, int* tick, hipStream_t s);
int64_t fc_bwd_part_floats(int S);   // workspace of its in-launch split reduction (both launches)
int fc_bwd_tickets();                 // int counters, zero before the first launch (re-armed by it)
hipError_t launch_policy_args(const float* h, int64_t n, const PolicyArgs& pa, hipStream_t s, int hid);
// policy arguments of a forward on explicit states (arl_forward_states): slot
// T, a sampled action from Philox stream 1 keyed by a per-call host counter
PolicyArgs states_policy_args(Net& net, int mode);
// FC split-K reduce (partials of launch_fc_fwd with tickets == nullptr) + bias
// + relu -> hfc, then the policy / value heads on the same 16 rows
hipError_t launch_policy_fc(const float* slab, int n, const float* fc_bias, float* hfc, const PolicyArgs& pa,
                            hipStream_t s);

// x / 255 correctly rounded, i.e. __fdiv_rn(x, 255.f), in three ops instead of the ~10 of the
// general division: q = x * RN(1/255), the exact residual r = x - 255 q (fma), q + r * RN(1/255)
// (fma).  scripts/div255_check.c compares it with IEEE division over every finite f32: equal
// except x = -0 (+0 instead of -0), which no caller passes (byte values; MFMA sums from +0
// accumulators).  Needs f32 denormals on (the kernels' default float_denorm_mode 3).
__device__ inline float div255(float x) {
  constexpr float inv = 1.f / 255.f;
  const float q = __fmul_rn(x, inv);
  return __fmaf_rn(__fmaf_rn(-q, 255.f, x), inv, q);
}

// end-of-window advance folded into the update (NIPS learner): the lr reads
// the learner's snapshot CTL_STEP_SNAP, so no workgroup reads CTL_STEP and one
// thread can move it without a ticket; reset flags (and the LSTM h / c carry)
// are copied grid-stride by all workgroups (optim.hip).
struct AdvanceArgs {
  int64_t* ctl;             // null: no advance
  uint16_t* fc_planes;      // non-null: also rewrite the FC weight's split planes ([fc_w0, fc_w0 + 256 x 2592))
  int64_t fc_w0;
  uint8_t* reset;           // (T+1, n): row T -> row 0
  float* hbuf;              // LSTM: (T+2, n, 256), row T -> row 0 (else null)
  float* cbuf;
  int T, n;
};
// GradientClipping's squared norm: f64 partials [0, nparts) (nparts <= NORM_MAX_PARTS) of the launch
// that sums them (grad_sqnorm_kernel, or reduce_conv_bwd_kernel with a NormFold), one per block;
// every block of the update kernel re-reduces them in block order
constexpr int NORM_MAX_PARTS = 1000, NORM_SCRATCH = 1024;
// What one update's launches share (launch_rmsprop, launch_adam and, for the record of that update,
// launch_window_stats), whichever optimizer runs it.
struct UpdateArgs {
  const double* norm_sq = nullptr;   // the norm's partials [0, nparts), re-reduced by every block; null: no clip
  int nparts = 0;
  float clip = 0.f;
  const int64_t* lr_ctl = nullptr;   // the lr anneal (update_lr, optim.hip): the control block with total_steps > 0,
  int64_t total_steps = 0;           //   else null: the lr as given
  int64_t n_total = 0;
  int t_max = 0;
  const AdvanceArgs* adv = nullptr;  // null: no advance, no FC planes
  const DecayArgs* wd = nullptr;     // null or rate == 0: the decay-free kernel
};
hipError_t launch_rmsprop(float* p, float* ms, const float* g, int64_t n, double lr, double alpha, double eps,
                          const UpdateArgs& u, hipStream_t s);
// Adam (Chainer 1.8.1 optimizers.Adam restated in include/asyncrl_hip.h) with launch_rmsprop's hooks and side
// duties: lr = Adam's alpha (annealed as launch_rmsprop's lr), v = the second moment.  tctl = the control block:
// a one-thread launch ahead of the update kernel adds 1 to tctl[CTL_ADAM_T], the update number the kernel then
// reads; with stats_log set (launch_window_stats ran just before) it also makes field 16 of that record the Adam
// step size.  tctl null: the host's t >= 1 (flat arrays: the f32 step size then comes from the host's libm).
struct AdamArgs {
  double beta1, beta2;
  int64_t* tctl;
  int64_t t;
  double* stats_log = nullptr;
  const int64_t* stats_count = nullptr;
};
hipError_t launch_adam(float* p, float* m, float* v, const float* g, int64_t n, double lr, double eps,
                       const AdamArgs& ad, const UpdateArgs& u, hipStream_t s);
hipError_t launch_ctl_write(int64_t* ctl, int idx, int64_t value, hipStream_t s);
hipError_t launch_grad_sqnorm(const float* g, int64_t n, double* partials, int blocks, hipStream_t s);
// Per-window training statistics (arl_net_set_window_stats; the header's "window statistics"): one record
// of WINDOW_STAT_FIELDS doubles per update, slot count % WINDOW_LOG of the ring `log`.
constexpr int WINDOW_LOG = 64, WINDOW_STAT_FIELDS = 17;
struct WindowStatsArgs {
  const float* rewards;     // (T, n)
  const uint8_t* dones;     // (T, n)
  const float* v;           // (T + 1, n), row T = the bootstrap value
  const float* entropy;     // (T + 1, n)
  const float* loss;        // (n, 2)
  int T, n;
  double gamma;
  int clip_reward;
  const int64_t* ctl;       // the control block, not yet advanced
  double* log;
  int64_t* count;
};
// One 256-thread workgroup (optim.hip window_stats_kernel).  lr and u are those of the update that follows, so
// that the recorded lr and clip scale come from the values (and the device functions) the update kernel uses;
// u.norm_sq is always given, u.clip <= 0: the update does not clip.
// lambda != 1: adv_sum / adv_sumsq are those of the GAE advantage (gae_step), another kernel; 1: today's launch
hipError_t launch_window_stats(const WindowStatsArgs& w, double lr, const UpdateArgs& u, hipStream_t s,
                               double lambda = 1.0);
hipError_t launch_stream_copy(const void* src, void* dst, int64_t bytes, int blocks, int mode, hipStream_t s);
hipError_t launch_policy(const float* h, int64_t n, const float* Wpi, const float* bpi, const float* Wv,
                         const float* bv, int A, uint64_t seed, const int64_t* ctl, int64_t step_off,
                         int env_offset, int mode, float* logits, float* probs, float* logp, float* v,
                         float* ent, int32_t* act, float* logp_a, hipStream_t s, int hid = HID);
// The learner's n-step return recurrence (a3c.py:82-92), one step backwards in time: R = 0 at a terminal
// (dones bit 0), then R = R * gamma + r with the reward clipped to [-1, 1] iff clip_reward (a3c.py:69-70);
// f64, unfused.  returns_compute (policy.hip) and window_stats_kernel (optim.hip) both scan with it.
__device__ inline double clip_reward_f64(float r, int clip_reward) {
  const double x = (double)r;
  return clip_reward ? (x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x)) : x;
}
__device__ inline double return_step(double R, int done, float r, double gamma, int clip_reward) {
  if (done & 1) R = 0.0;
  return __dadd_rn(__dmul_rn(R, gamma), clip_reward_f64(r, clip_reward));
}
// GAE(lambda) (Schulman et al. 2016; an extension, the reference has none), one step backwards in time beside
// return_step: delta_k = (r_k + gamma v(s_k+1)) - v(s_k) with v(s_k+1) = 0 after a terminal, then
// G = delta_k + gl G with G = 0 carried across a terminal; gl = gamma * lambda, one f64 product of the host.
// f64, unfused.  vnext of step T - 1 is the bootstrap value.  The advantage of step t is (float)G after k = t.
__device__ inline double gae_step(double G, int done, float r, float vk, float vnext, double gamma, double gl,
                                  int clip_reward) {
  const double vn = (done & 1) ? 0.0 : (double)vnext;
  const double d = __dsub_rn(__dadd_rn(clip_reward_f64(r, clip_reward), __dmul_rn(gamma, vn)), (double)vk);
  if (done & 1) G = 0.0;
  return __dadd_rn(d, __dmul_rn(gl, G));
}
// lambda == 1 is not GAE: the launchers below then run the n-step kernels with the arguments they always had
inline bool gae_on(double lambda) { return lambda != 1.0; }
// Arguments of the loss-gradient launches (policy.hip describes the kernels above its device-side forms of this
// struct).  rewards / dones (T, n); v / probs / logp / act indexed (T + 1, n[, A]), row T = the bootstrap value.
// dones: bit 0 = the transition t -> t+1 ended the episode; bit 1 = step t lies past the end of this window
// (arl_truncate_window: no loss, no gradient).  pcoef = pi_loss_coef; keep_scale: keep_loss_scale_same
// (a3c.py:110-121).  loss: nullable; ctl non-null: also snapshot the step counter (CTL_STEP_SNAP).
// Callers name the fields they set (a net's window: window_returns_args below); no launcher has a default.
struct ReturnsArgs {
  const float* rewards;
  const uint8_t* dones;
  const float* v;
  const float* probs;
  const float* logp;
  const int32_t* act;
  int T, n, A;
  double gamma;
  float beta, vcoef, pcoef;
  int clip_reward, keep_scale;
  float* dlogits;
  float* dv;
  float* loss;
  int64_t* ctl;
};
// the heads' backward that rides on a loss-gradient launch: dh = dlogits Wpi + dv Wv (times mask > 0 when mask is
// given) for hidden width HID
struct HeadsBwd {
  const float *Wpi, *Wv, *mask;
  float* dh;
};
// the two from a net's workspace, parameters and loss options (net.hip); FF: mask hfc, dh = dfc; LSTM: no mask, dh
ReturnsArgs window_returns_args(const Net& net, double gamma, float beta, float vcoef, int clip_reward);
HeadsBwd window_heads_bwd(const Net& net);
// lambda: 1 = the n-step advantage, else GAE(lambda) (gae_on above)
hipError_t launch_returns(const ReturnsArgs& ra, double lambda, hipStream_t s);
// launch_returns + the heads' backward, one launch (T <= 64)
hipError_t launch_returns_heads(const ReturnsArgs& ra, double lambda, const HeadsBwd& hb, hipStream_t s);
// Clipped-surrogate (PPO) epochs on a window's rollout (arl_net_set_ppo has the definition; policy.hip).
// launch_ppo_snapshot: lpo / adv / ret (T, n) of the window, from return_step / gae_step (lambda != 1) as the
// returns launch forms them; of ra it reads rewards, dones, v, logp, act, T, n, A, gamma and clip_reward.
// launch_ppo_lossgrad: the loss gradient of one epoch from the slots' current probs / logp / v and the snapshot
// (the PPO form of launch_returns); launch_ppo_heads: + the heads' dh (the PPO form of launch_returns_heads,
// T <= 64).
hipError_t launch_ppo_snapshot(const ReturnsArgs& ra, double lambda, float* lpo, float* adv, float* ret, hipStream_t s);
struct PpoLossArgs {
  ReturnsArgs r;                  // slots, shape, coefficients, outputs, ctl (rewards, gamma, clip_reward: not read)
  const float *lpo, *adv, *ret;   // the snapshot
  float lo, hi;                   // (float)(1.0 - eps_clip), (float)(1.0 + eps_clip)
  float* ratio;                   // nullable
  // value clipping (arl_net_set_ppo_options): vold non-null picks the value-clipped form of the two launchers
  // below, ev = (float)vclip_eps
  const float* vold;
  float ev;
};
hipError_t launch_ppo_lossgrad(const PpoLossArgs& p, hipStream_t s);
hipError_t launch_ppo_heads(const PpoLossArgs& p, const HeadsBwd& hb, hipStream_t s);
// The PPO options' own launches (arl_net_set_ppo_options has the definitions; policy.hip).
// launch_ppo_vold: vold[t, e] = v[t, e] of a live sample, else 0.  launch_ppo_normalize_adv: the adv plane in
// place, moments = (n_live, mean, std); one workgroup.  launch_ppo_epoch_stats: one epoch's record from the
// arrays of p (p.r's dlogits / dv / loss and coefficients are not read, ratio is); ctl non-null: the window
// counter is read there instead of `window`; count non-null: rec is the aux block, the record goes to its ring
// and the count is advanced, else rec is the record; one workgroup.
constexpr int PPO_LOG = ARL_PPO_LOG, PPO_STAT_FIELDS = ARL_PPO_STAT_FIELDS, PPO_AUX_HEAD = 8;
static_assert(PPO_AUX_HEAD + PPO_LOG * PPO_STAT_FIELDS == ARL_PPO_AUX_DOUBLES, "aux layout");
hipError_t launch_ppo_vold(const uint8_t* dones, const float* v, float* vold, int T, int n, hipStream_t s);
hipError_t launch_ppo_normalize_adv(const uint8_t* dones, float* adv, int T, int n, double* moments, hipStream_t s);
hipError_t launch_ppo_epoch_stats(const PpoLossArgs& p, const int64_t* ctl, double window, double epoch, int64_t* count,
                                  double* rec, hipStream_t s);
// The LSTM's recurrent carry of a PPO window (ppo_state.hip): rows T of hbuf / cbuf -> carry (planes h then c,
// n * HID f32 each), or with restore the other way; one launch moves both planes.
hipError_t launch_ppo_carry(float* hbuf, float* cbuf, float* carry, int T, int n, bool restore, hipStream_t s);
// launch_policy_fc of the bootstrap slot (no draw) + launch_returns_heads for the same n envs, one launch
// (policy.hip policy_fc_returns_kernel; v(s_T) handed over in LDS); bit-identical to the two launches
hipError_t launch_policy_fc_returns(const float* slab, int n, const float* fc_bias, float* hfc, const PolicyArgs& pa,
                                    const ReturnsArgs& ra, double lambda, const HeadsBwd& hb, hipStream_t s);

}  // namespace arl
