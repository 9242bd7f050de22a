// Device-resident Catch: the environment of the closed actor-learner loop (include/asyncrl_hip.h, "device
// environment"; no reference counterpart -- the reference's envs are host emulators, ale.py / doom_env.py).
// One launch per env-step does the transition and the render: it reads the actions the policy sampled, steps
// every env's handful of integers, and writes the (frame 4, frame 3) pair, the reward and the done flag into
// the pool entry the next arl_observe reads.
//
// No workgroup reads a word another workgroup of its launch writes (the hazard optim.hip documents for the
// control block): the env state is double-buffered, every workgroup of an env recomputes the transition from
// the OLD half (a few dozen integer ops on wave-uniform values), and only band 0's thread 0 writes the new
// half, the reward and the done.
//
// The render is a pure store stream, 2 x 210 rows x 480 bytes per env as 16-byte stores; a chunk's bytes are
// decided from the two sprite rectangles, and only the 12 rows a sprite touches look at them bytewise.  No LDS,
// no loads besides the state, the action and the step counter.  Grid (CATCH_BANDS, envs): a band is 2,520
// consecutive chunks of the pair, 10 stores per lane (DESIGN.md "Device environment" has the measurements).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arl_internal.hpp"
#include "policy_rows.hpp"

namespace arl {

namespace {

constexpr int SCREEN_H = 210, SCREEN_W = 160;
constexpr int ROW_CHUNKS = SCREEN_W * 3 / 16;                  // 30 16-byte chunks a row
constexpr int PAIR_CHUNKS = 2 * SCREEN_H * ROW_CHUNKS;         // 12,600
constexpr int CATCH_BANDS = 5;                                 // workgroups per env
constexpr int BAND_CHUNKS = PAIR_CHUNKS / CATCH_BANDS;         // 2,520 = 9.84 x 256: the last pass is 84 % full
static_assert(PAIR_CHUNKS % CATCH_BANDS == 0, "bands tile the pair");
static_assert(PAIR == PAIR_CHUNKS * 16, "frame pair bytes");

// the game's constants (include/asyncrl_hip.h)
constexpr int PADDLE_W = 16, PADDLE_H = 4, PADDLE_Y = 190, PADDLE_MAX = SCREEN_W - PADDLE_W;   // px in [0, 144]
constexpr int BALL = 8, BALL_MAX = SCREEN_W - BALL;                                            // bx in [0, 152]
constexpr int BALL_Y0 = 18, PADDLE_X0 = 72, BALL_DY = 3, PADDLE_DX = 3;
constexpr uint32_t ENV_STREAM = 2;   // Philox counter word 3, beside 0 (window draws) and 1 (pi_and_v draws)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Sprites {
  int bx, by, px;
};

// bytes [16 c, 16 c + 16) of screen row r
__device__ inline u32x4 catch_chunk(int r, int c, const Sprites& s) {
  const bool ball_row = (unsigned)(r - s.by) < (unsigned)BALL;
  const bool pad_row = (unsigned)(r - PADDLE_Y) < (unsigned)PADDLE_H;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (!ball_row && !pad_row) return v;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = 16 * c + 4 * w + i, x = b / 3, ch = b - 3 * x;
      uint32_t px = 0;
      if (pad_row && (unsigned)(x - s.px) < (unsigned)PADDLE_W) px = ch == 0 ? 200u : 72u;
      if (ball_row && (unsigned)(x - s.bx) < (unsigned)BALL) px = 236u;   // the ball covers the paddle
      word |= px << (8 * i);
    }
    v[w] = word;
  }
  return v;
}

struct EnvState {
  int bx, by, vx, px, episode, steps;
};

// episode start: by = 18, px = 72, bx and vx from Philox(counter = (env id, episode, 0, 2), key = seed)
__device__ inline EnvState catch_start(uint32_t env_id, int episode, uint32_t seed_lo, uint32_t seed_hi) {
  const uint4 w = philox4x32_10(make_uint4(env_id, (uint32_t)episode, 0u, ENV_STREAM), seed_lo, seed_hi);
  return EnvState{(int)(w.x % (uint32_t)(BALL_MAX + 1)), BALL_Y0, (int)(w.y % 5u) - 2, PADDLE_X0, episode, 0};
}

__global__ void __launch_bounds__(256)
catch_kernel(CatchArgs a) {
  const int e = a.e0 + blockIdx.y;
  const bool reset = a.actions == nullptr;
  const int64_t k = (a.ctl != nullptr ? a.ctl[CTL_STEP] : 0) + a.t;   // the observation the actions answer
  const int64_t kout = reset ? k : k + 1;                             // the observation this launch produces
  const uint32_t pidx = fd_mod64(a.dpool, (uint64_t)kout);
  const uint32_t env_id = (uint32_t)(a.env_offset + e);

  EnvState st;
  Sprites cur, prev;
  float reward = 0.f;
  bool done = false;
  if (reset) {
    st = catch_start(env_id, 0, a.seed_lo, a.seed_hi);
    cur = prev = Sprites{st.bx, st.by, st.px};
  } else {
    const int4* old = reinterpret_cast<const int4*>(a.state + ((int64_t)(k & 1) * a.n + e) * CATCH_STATE_INTS);
    const int4 o0 = old[0], o1 = old[1];
    const int act = a.actions[e];
    st = EnvState{o0.x, o0.y, o0.z, o0.w, o1.x, o1.y};
    cur = prev = Sprites{st.bx, st.by, st.px};
    for (int f = 0; f < 4; ++f) {
      prev = cur;
      if (act == 2) st.px = min(st.px + PADDLE_DX, PADDLE_MAX);
      else if (act == 3) st.px = max(st.px - PADDLE_DX, 0);
      st.bx += st.vx;
      if (st.bx < 0) {
        st.bx = -st.bx;
        st.vx = -st.vx;
      } else if (st.bx > BALL_MAX) {
        st.bx = 2 * BALL_MAX - st.bx;
        st.vx = -st.vx;
      }
      st.by += BALL_DY;
      if (st.by + BALL >= PADDLE_Y) {   // the ball reached the paddle's row: the skip loop breaks (ale.py:111-139)
        done = true;
        reward = (st.bx + BALL > st.px && st.bx < st.px + PADDLE_W) ? 1.f : -1.f;
        break;
      }
      cur = Sprites{st.bx, st.by, st.px};
    }
    if (done) {   // the next episode starts at once; its first screen twice, the terminal one is never shown
      st = catch_start(env_id, st.episode + 1, a.seed_lo, a.seed_hi);
      cur = prev = Sprites{st.bx, st.by, st.px};
    } else {
      st.steps += 1;
    }
  }

  const int64_t row = (int64_t)pidx * a.n + e;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int4* out = reinterpret_cast<int4*>(a.state + ((int64_t)(kout & 1) * a.n + e) * CATCH_STATE_INTS);
    out[0] = make_int4(st.bx, st.by, st.vx, st.px);
    out[1] = make_int4(st.episode, st.steps, 0, 0);
    a.reward_pool[row] = reward;
    a.done_pool[row] = done ? 1 : 0;
  }

  u32x4* dst = reinterpret_cast<u32x4*>(a.pair_pool + row * PAIR);
  const int q0 = blockIdx.x * BAND_CHUNKS;
#pragma unroll 2
  for (int i = threadIdx.x; i < BAND_CHUNKS; i += 256) {
    const int q = q0 + i, row2 = q / ROW_CHUNKS, c = q - row2 * ROW_CHUNKS;
    const bool second = row2 >= SCREEN_H;   // pair[1]: the screen one frame earlier
    // plain stores: the observation that follows reads these bytes, and non-temporal ones measured slower
    // both here (20.1 vs 17.0 us at 512 envs) and in that observation (23.2 vs 20.5 us)
    dst[q] = catch_chunk(second ? row2 - SCREEN_H : row2, c, second ? prev : cur);
  }
}

}  // namespace

hipError_t launch_catch(const CatchArgs& a, hipStream_t s) {
  const int ne = a.ne < 0 ? a.n : a.ne;
  if (ne <= 0) return hipSuccess;
  hipLaunchKernelGGL(catch_kernel, dim3(CATCH_BANDS, (unsigned)ne), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace arl
