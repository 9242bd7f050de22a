// Device-resident Pong: the third device environment (include/asyncrl_hip.h, "device environment"), as the hooks
// of env_kernel.hpp's skeleton.  What the other two lack: rewards of both signs inside an episode without a
// terminal, an opponent whose paddle is part of the dynamics, games of hundreds of env-steps, a background that
// is not black, and a meaning for actions 4 and 5.  A state of 12 integers (ball, the two paddles, the counters,
// the two scores); the transition every workgroup recomputes is three int4 loads and about a hundred integer ops
// on wave-uniform values, one Philox block when a ball is served.
//
// Only chunks on the rows of the ball and the two paddles look at their pixels; every other chunk is the row's
// colour (background or wall) in the three phases a word can start in, rotated by the chunk's.  No tables in
// memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_direct.hpp"
#include "env_kernel.hpp"
#include "policy_rows.hpp"

namespace arl {

namespace {

// the game's constants (include/asyncrl_hip.h)
constexpr int WALL_H = 10, WALL_TOP = 24, WALL_BOTTOM = 194;                  // rows 24..33 and 194..203
constexpr int FIELD_Y0 = WALL_TOP + WALL_H;                                   // 34: the first row of the field
constexpr int PADDLE_W = 4, PADDLE_H = 16, PADDLE_MAX = WALL_BOTTOM - PADDLE_H, PADDLE_DY = 4, OPP_DY = 2;
constexpr int OPP_X = 16, AGENT_X = 140, PADDLE_Y0 = 106;
constexpr int BALL = 4, BALL_Y_MAX = WALL_BOTTOM - BALL, BALL_X_MAX = SCREEN_W - BALL, SERVE_X = 78, SPEED_X = 3;
constexpr int STEP_CAP = 5000;
constexpr uint32_t ENV_STREAM = 4;   // Philox counter word 3, beside 0 (window), 1 (pi_and_v), 2 (Catch), 3 (Breakout)

// a pixel's colour as 24 bits, R in the low byte: the order of its bytes in memory
__host__ __device__ inline constexpr uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return r | g << 8 | b << 16; }
constexpr uint32_t BG = rgb(144, 72, 17), WALL = rgb(236, 236, 236), OPP = rgb(213, 130, 74), AGENT = rgb(92, 186, 92);
constexpr uint32_t BALL_RGB = WALL;

struct Screen {
  int bx, by, py, oy;
};

// the 32-bit word that starts in channel p of a pixel of colour c0 and ends in the next pixel, of colour c1:
// 3 - p bytes of the first, p + 1 of the second
__host__ __device__ inline uint32_t word_of(uint32_t c0, uint32_t c1, int p) { return c0 >> (8 * p) | c1 << (24 - 8 * p); }

// bytes [16 c, 16 c + 16) of screen row r.  A word at byte b0 covers pixel x0 = b0 / 3 from its channel
// p = b0 % 3 on and pixel x0 + 1 in the rest (breakout.hip's word-wise render, on 24-bit colours: nothing here
// needs a colour's bytes twice in one value)
__host__ __device__ inline u32x4 pong_chunk(int r, int c, const Screen& s) {
  const bool wall = (unsigned)(r - WALL_TOP) < (unsigned)WALL_H || (unsigned)(r - WALL_BOTTOM) < (unsigned)WALL_H;
  const bool ball_row = (unsigned)(r - s.by) < (unsigned)BALL;
  const bool opp_row = (unsigned)(r - s.oy) < (unsigned)PADDLE_H;
  const bool pad_row = (unsigned)(r - s.py) < (unsigned)PADDLE_H;
  const uint32_t base = wall ? WALL : BG;
  u32x4 v;
  if (!ball_row && !opp_row && !pad_row) {
    // one colour: word w starts in channel (16 c + 4 w) % 3 = (c + w) % 3, the three phases rotated by c % 3
    const uint32_t s0 = word_of(base, base, 0), s1 = word_of(base, base, 1), s2 = word_of(base, base, 2);
    const int p0 = c - 3 * (c / 3);
    v[0] = v[3] = p0 == 0 ? s0 : p0 == 1 ? s1 : s2;
    v[1] = p0 == 0 ? s1 : p0 == 1 ? s2 : s0;
    v[2] = p0 == 0 ? s2 : p0 == 1 ? s0 : s1;
    return v;
  }
  // out of its rows a sprite is moved off the screen, so the per-pixel test is the column test alone
  const int bx = ball_row ? s.bx : -SCREEN_W, ox = opp_row ? OPP_X : -SCREEN_W, ax = pad_row ? AGENT_X : -SCREEN_W;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int b0 = 16 * c + 4 * w, x0 = b0 / 3, p = b0 - 3 * x0;
    uint32_t colour[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int x = x0 + i;   // (x <= 159: the row's last word starts in pixel 158)
      colour[i] = base;
      if ((unsigned)(x - ox) < (unsigned)PADDLE_W) colour[i] = OPP;
      if ((unsigned)(x - ax) < (unsigned)PADDLE_W) colour[i] = AGENT;
      if ((unsigned)(x - bx) < (unsigned)BALL) colour[i] = BALL_RGB;   // the ball over a paddle
    }
    v[w] = word_of(colour[0], colour[1], p);
  }
  return v;
}

struct EnvState {
  int bx, by, vx, vy, py, oy, serves, steps, game, game_steps, score_agent, score_opp;
};

// the ball's vy off a paddle whose top edge is y: (-3, -1, 1, 3)[clamp(by + 2 - y, 0, 15) >> 2], formed
// arithmetically.  (The clamp compiles to v_med3_i32, a vector op on a wave-uniform value: taken back to a
// scalar register at once, as in breakout.hip.)
__device__ inline int hit_vy(int by, int y) {
  return __builtin_amdgcn_readfirstlane(2 * (min(max(by + BALL / 2 - y, 0), PADDLE_H - 1) >> 2) - 3);
}

// a serve: bx = 78, by and vy from Philox(counter = (env id, serves, 0, 4), key = seed); vx = toward when it is
// +-3 (after a point: toward the side that conceded), else from the draw's third word (a new game)
__device__ inline void serve(EnvState& st, int toward, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi) {
  const uint4 w = philox4x32_10(make_uint4(env_id, (uint32_t)st.serves, 0u, ENV_STREAM), seed_lo, seed_hi);
  st.bx = SERVE_X;
  st.by = FIELD_Y0 + (int)(w.x % (uint32_t)(BALL_Y_MAX - FIELD_Y0 + 1));
  st.vy = 2 * (int)(w.y & 3u) - 3;
  st.vx = toward != 0 ? toward : (w.z & 1u) ? SPEED_X : -SPEED_X;
  st.serves += 1;
}

__device__ inline void new_game(EnvState& st, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi) {
  st.py = st.oy = PADDLE_Y0;
  st.score_agent = st.score_opp = 0;
  st.game_steps = 0;
  serve(st, 0, env_id, seed_lo, seed_hi);
}

}  // namespace

struct Pong {
  static constexpr int STATE_INTS = PONG_STATE_INTS;
  using State = EnvState;
  using Screen = arl::Screen;
  using Reward = int;   // +1, -1 or 0, cast where it is stored

  __device__ static State start(uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi) {
    State st{};
    new_game(st, env_id, seed_lo, seed_hi);
    return st;
  }
  __device__ static State load(const int4* old) {
    const int4 o0 = old[0], o1 = old[1], o2 = old[2];
    return State{o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w, o2.x, o2.y, o2.z, o2.w};
  }
  __device__ static void store(int4* out, const State& st) {
    out[0] = make_int4(st.bx, st.by, st.vx, st.vy);
    out[1] = make_int4(st.py, st.oy, st.serves, st.steps);
    out[2] = make_int4(st.game, st.game_steps, st.score_agent, st.score_opp);
  }
  __device__ static Screen screen_of(const State& st) { return Screen{st.bx, st.by, st.py, st.oy}; }
  // (field by field: a select between the two structs would put them in scratch memory)
  __device__ static Screen pick(bool second, const Screen& cur, const Screen& prev) {
    return Screen{second ? prev.bx : cur.bx, second ? prev.by : cur.by, second ? prev.py : cur.py,
                  second ? prev.oy : cur.oy};
  }
  __device__ static u32x4 chunk(int r, int c, const Screen& s) { return pong_chunk(r, c, s); }
  // env_direct.hpp's shortcut: true if every pixel of row r has one colour (the background's or the walls': no
  // ball, no paddle on it), rgb = R | G << 8 | B << 16
  __device__ static bool plain_row(int r, const Screen& s, uint32_t& rgb) {
    const bool wall = (unsigned)(r - WALL_TOP) < (unsigned)WALL_H || (unsigned)(r - WALL_BOTTOM) < (unsigned)WALL_H;
    rgb = wall ? WALL : BG;
    return (unsigned)(r - s.by) >= (unsigned)BALL && (unsigned)(r - s.oy) >= (unsigned)PADDLE_H &&
           (unsigned)(r - s.py) >= (unsigned)PADDLE_H;
  }

  // flags: the points a game is played to, 1..21 (launch_env takes them from the kind)
  __device__ static void step(State& st, int act, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi, int flags,
                              Screen& cur, Screen& prev, Reward& reward, bool& done) {
    cur = prev = screen_of(st);
    const bool up = act == 2 || act == 4, down = act == 3 || act == 5;
    for (int f = 0; f < 4; ++f) {
      prev = cur;
      if (up) st.py = max(st.py - PADDLE_DY, FIELD_Y0);
      else if (down) st.py = min(st.py + PADDLE_DY, PADDLE_MAX);
      const int c = st.by + BALL / 2 - (st.oy + PADDLE_H / 2);   // the opponent follows the ball, dead zone +-2
      if (c > 2) st.oy = min(st.oy + OPP_DY, PADDLE_MAX);
      else if (c < -2) st.oy = max(st.oy - OPP_DY, FIELD_Y0);
      st.by += st.vy;
      if (st.by < FIELD_Y0) {
        st.by = 2 * FIELD_Y0 - st.by;
        st.vy = -st.vy;
      } else if (st.by > BALL_Y_MAX) {
        st.by = 2 * BALL_Y_MAX - st.by;
        st.vy = -st.vy;
      }
      st.bx += st.vx;
      // |vx| = 3 and the three-column windows: each crossing of a paddle's face is tested exactly once
      if (st.vx > 0 && st.bx >= AGENT_X - BALL && st.bx < AGENT_X - BALL + SPEED_X) {
        if (st.by + BALL > st.py && st.by < st.py + PADDLE_H) {
          st.bx = 2 * (AGENT_X - BALL) - st.bx;
          st.vx = -SPEED_X;
          st.vy = hit_vy(st.by, st.py);
        }
      } else if (st.vx < 0 && st.bx > OPP_X + PADDLE_W - SPEED_X - 1 && st.bx <= OPP_X + PADDLE_W - 1) {
        if (st.by + BALL > st.oy && st.by < st.oy + PADDLE_H) {
          st.bx = 2 * (OPP_X + PADDLE_W) - st.bx;
          st.vx = SPEED_X;
          st.vy = hit_vy(st.by, st.oy);
        }
      }
      if (st.bx < 0) reward = 1;
      else if (st.bx > BALL_X_MAX) reward = -1;
      if (reward != 0) break;   // a point: the skip loop breaks (ale.py:111-139)
      cur = screen_of(st);
    }
    st.game_steps += 1;
    st.steps += 1;
    st.score_agent += reward > 0 ? 1 : 0;
    st.score_opp += reward < 0 ? 1 : 0;
    done = st.score_agent >= flags || st.score_opp >= flags || st.game_steps >= STEP_CAP;
    if (done) {   // the next game starts at once; its first screen twice, the last one is never shown
      st.game += 1;
      st.steps = 0;
      new_game(st, env_id, seed_lo, seed_hi);
      cur = prev = screen_of(st);
    } else if (reward != 0) {   // the paddles and the scores are kept; the ball goes toward the side that conceded
      serve(st, reward > 0 ? -SPEED_X : SPEED_X, env_id, seed_lo, seed_hi);
      cur = prev = screen_of(st);
    }
  }
};

template hipError_t launch_game<Pong>(const EnvArgs&, hipStream_t);
template hipError_t launch_game_direct<Pong>(const DirectArgs&, hipStream_t);

}  // namespace arl
