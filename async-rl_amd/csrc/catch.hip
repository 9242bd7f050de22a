// Device-resident Catch: the environment of the closed actor-learner loop (include/asyncrl_hip.h, "device
// environment"), as the hooks of env_kernel.hpp's skeleton.  A state of 6 integers; a chunk's bytes are decided
// from the two sprite rectangles, and only the 12 rows a sprite touches look at them bytewise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_direct.hpp"
#include "env_kernel.hpp"
#include "policy_rows.hpp"

namespace arl {

namespace {

// the game's constants (include/asyncrl_hip.h)
constexpr int PADDLE_W = 16, PADDLE_H = 4, PADDLE_Y = 190, PADDLE_MAX = SCREEN_W - PADDLE_W;   // px in [0, 144]
constexpr int BALL = 8, BALL_MAX = SCREEN_W - BALL;                                            // bx in [0, 152]
constexpr int BALL_Y0 = 18, PADDLE_X0 = 72, BALL_DY = 3, PADDLE_DX = 3;
constexpr uint32_t ENV_STREAM = 2;   // Philox counter word 3, beside 0 (window draws) and 1 (pi_and_v draws)

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

}  // namespace

struct Catch {
  static constexpr int STATE_INTS = CATCH_STATE_INTS;
  using State = EnvState;
  using Screen = Sprites;
  using Reward = float;

  __device__ static State start(uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi) {
    return catch_start(env_id, 0, seed_lo, seed_hi);
  }
  __device__ static State load(const int4* old) {
    const int4 o0 = old[0], o1 = old[1];
    return State{o0.x, o0.y, o0.z, o0.w, o1.x, o1.y};
  }
  __device__ static void store(int4* out, const State& st) {
    out[0] = make_int4(st.bx, st.by, st.vx, st.px);
    out[1] = make_int4(st.episode, st.steps, 0, 0);
  }
  __device__ static Screen screen_of(const State& st) { return Screen{st.bx, st.by, st.px}; }
  __device__ static Screen pick(bool second, const Screen& cur, const Screen& prev) { return second ? prev : cur; }
  __device__ static u32x4 chunk(int r, int c, const Screen& s) { return catch_chunk(r, c, s); }
  // env_direct.hpp's shortcut: true if every pixel of row r has one colour, rgb = R | G << 8 | B << 16
  __device__ static bool plain_row(int r, const Screen& s, uint32_t& rgb) {
    rgb = 0u;
    return (unsigned)(r - s.by) >= (unsigned)BALL && (unsigned)(r - PADDLE_Y) >= (unsigned)PADDLE_H;
  }

  __device__ static void step(State& st, int act, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi, int /*flags*/,
                              Screen& cur, Screen& prev, Reward& reward, bool& done) {
    cur = prev = screen_of(st);
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
      cur = screen_of(st);
    }
    if (done) {   // the next episode starts at once; its first screen twice, the terminal one is never shown
      st = catch_start(env_id, st.episode + 1, seed_lo, seed_hi);
      cur = prev = screen_of(st);
    } else {
      st.steps += 1;
    }
  }
};

template hipError_t launch_game<Catch>(const EnvArgs&, hipStream_t);
template hipError_t launch_game_direct<Catch>(const DirectArgs&, hipStream_t);

}  // namespace arl
