// Device-resident Breakout: the second device environment (include/asyncrl_hip.h, "device environment"), the
// game the reference's published numbers are about, as the hooks of env_kernel.hpp's skeleton.  A state of 16
// integers (ball, paddle, lives, the 120 brick bits, the counters) and the raw reward; the transition every
// workgroup recomputes is four int4 loads and a few hundred integer ops on wave-uniform values, one Philox
// block when a ball is served.
//
// Only chunks on the 36 brick rows, the ball's 4 rows and the paddle's 4 rows decide bytes; every other chunk
// is a zero store.  The two screens of a pair can differ in their bricks (a brick hit in frame 4), so each
// carries its own brick bits.  No tables in memory (the row colours are three 48-bit constants shifted by the
// brick row).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_direct.hpp"
#include "env_kernel.hpp"
#include "policy_rows.hpp"

namespace arl {

namespace {

// the game's constants (include/asyncrl_hip.h)
constexpr int BRICK_ROWS = 6, BRICK_COLS = 20, BRICK_H = 6, BRICK_Y0 = 57, BRICK_Y1 = BRICK_Y0 + BRICK_ROWS * BRICK_H;
constexpr int PADDLE_W = 16, PADDLE_H = 4, PADDLE_Y = 190, PADDLE_MAX = SCREEN_W - PADDLE_W, PADDLE_DX = 3;
constexpr int BALL = 4, BALL_MAX = SCREEN_W - BALL, CEILING = 32, SERVE_Y = 100, SPEED_Y = 4;
constexpr int LIVES = 5, PADDLE_X0 = 72, STEP_CAP = 1000;
constexpr uint32_t ENV_STREAM = 3;   // Philox counter word 3, beside 0 (window), 1 (pi_and_v) and 2 (Catch)
// byte r of each constant = that channel of brick row r: (200,72,72) (198,108,58) (180,122,48) (162,162,42)
// (72,160,72) (66,72,200)
constexpr uint64_t ROW_R = 0x4248a2b4c6c8ull, ROW_G = 0x48a0a27a6c48ull, ROW_B = 0xc8482a303a48ull;
constexpr uint64_t FULL_LO = ~0ull, FULL_HI = (1ull << 56) - 1;   // 120 bricks: words 0..2 full, 24 bits of word 3

// the 120 brick bits travel as two 64-bit halves (words b0 | b1 << 32 and b2 | b3 << 32) and are picked by
// shifts alone: a word chosen by an index would be an array in memory
struct Screen {
  int bx, by, px;
  uint64_t blo, bhi;
};

// the 20 brick bits of brick row br (bit c = column c); br may differ from lane to lane
__host__ __device__ inline uint32_t brick_row_bits(uint64_t blo, uint64_t bhi, int br) {
  const int i0 = BRICK_COLS * br;   // 0, 20, 40, 60 (row 3 straddles the halves), 80, 100
  const uint64_t v = i0 < 64 ? (blo >> i0) | ((bhi << 1) << (63 - i0)) : bhi >> (i0 - 64);
  return (uint32_t)v & ((1u << BRICK_COLS) - 1u);
}

// the colour of a pixel as a byte stream R G B R G B R G: bits [8 p, 8 p + 32) are the four bytes from channel p on
__host__ __device__ inline constexpr uint64_t rgb_stream(uint64_t r, uint64_t g, uint64_t b) {
  const uint64_t rgb = r | g << 8 | b << 16;
  return rgb | rgb << 24 | rgb << 48;
}
constexpr uint64_t BALL_STREAM = rgb_stream(236, 236, 236), PADDLE_STREAM = rgb_stream(200, 72, 72);

// bytes [16 c, 16 c + 16) of screen row r.  A 32-bit word at byte b0 covers pixel x0 = b0 / 3 from its channel
// p = b0 % 3 on (3 - p bytes) and pixel x0 + 1 in the rest, so a word is two pixel colours, shifted and masked:
// about 40 integer ops a word where a bytewise render took over 200 and made the kernel VALU-bound
__host__ __device__ inline u32x4 breakout_chunk(int r, int c, const Screen& s) {
  const bool brick_row = (unsigned)(r - BRICK_Y0) < (unsigned)(BRICK_Y1 - BRICK_Y0);
  const bool ball_row = (unsigned)(r - s.by) < (unsigned)BALL;
  const bool pad_row = (unsigned)(r - PADDLE_Y) < (unsigned)PADDLE_H;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (!brick_row && !ball_row && !pad_row) return v;
  uint32_t bits = 0;    // the brick bits of this row, bit = column
  uint64_t row = 0;     // and its colour stream
  if (brick_row) {
    const int br = (r - BRICK_Y0) / BRICK_H;
    bits = brick_row_bits(s.blo, s.bhi, br);
    row = rgb_stream((ROW_R >> (8 * br)) & 0xffu, (ROW_G >> (8 * br)) & 0xffu, (ROW_B >> (8 * br)) & 0xffu);
  }
  // out of its rows a sprite is moved off the screen, so the per-pixel test is the column test alone
  const int bx = ball_row ? s.bx : -SCREEN_W, px = pad_row ? s.px : -SCREEN_W;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int b0 = 16 * c + 4 * w, x0 = b0 / 3, p = b0 - 3 * x0;
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int x = x0 + i;   // (x <= 159: the row's last word starts in pixel 158)
      uint64_t colour = (bits >> (x >> 3)) & 1u ? row : 0ull;
      if ((unsigned)(x - px) < (unsigned)PADDLE_W) colour = PADDLE_STREAM;
      if ((unsigned)(x - bx) < (unsigned)BALL) colour = BALL_STREAM;   // a ball pixel covers anything under it
      const uint32_t first = 0x00ffffffu >> (8 * p);                   // the bytes of pixel x0
      word |= (uint32_t)(colour >> (8 * p)) & (i == 0 ? first : ~first);
    }
    v[w] = word;
  }
  return v;
}

struct EnvState {
  int bx, by, vx, vy, px, lives, serves, steps, game, game_steps, score, left;
  uint64_t blo, bhi;
};

__device__ inline int paddle_vx(int k) { return k < 2 ? k - 2 : k - 1; }   // (-2, -1, 1, 2)[k]

// a serve: by = 100, vy = +4, bx and vx from Philox(counter = (env id, serves, 0, 3), key = seed)
__device__ inline void serve(EnvState& st, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi) {
  const uint4 w = philox4x32_10(make_uint4(env_id, (uint32_t)st.serves, 0u, ENV_STREAM), seed_lo, seed_hi);
  st.bx = (int)(w.x % (uint32_t)(BALL_MAX + 1));
  st.vx = paddle_vx((int)(w.y & 3u));
  st.by = SERVE_Y;
  st.vy = SPEED_Y;
  st.serves += 1;
}

__device__ inline void new_game(EnvState& st, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi) {
  st.blo = FULL_LO;
  st.bhi = FULL_HI;
  st.left = BRICK_ROWS * BRICK_COLS;
  st.lives = LIVES;
  st.px = PADDLE_X0;
  st.game_steps = 0;
  st.score = 0;
  serve(st, env_id, seed_lo, seed_hi);
}

}  // namespace

struct Breakout {
  static constexpr int STATE_INTS = BREAKOUT_STATE_INTS;
  using State = EnvState;
  using Screen = arl::Screen;
  using Reward = int;   // the sum of brick values, cast where it is stored

  __device__ static State start(uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi) {
    State st{};
    new_game(st, env_id, seed_lo, seed_hi);
    return st;
  }
  __device__ static State load(const int4* old) {
    const int4 o0 = old[0], o1 = old[1], o2 = old[2], o3 = old[3];
    return State{o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w, o2.x, o2.y, o2.z, o2.w,
                 (uint64_t)(uint32_t)o3.x | (uint64_t)(uint32_t)o3.y << 32,
                 (uint64_t)(uint32_t)o3.z | (uint64_t)(uint32_t)o3.w << 32};
  }
  __device__ static void store(int4* out, const State& st) {
    out[0] = make_int4(st.bx, st.by, st.vx, st.vy);
    out[1] = make_int4(st.px, st.lives, st.serves, st.steps);
    out[2] = make_int4(st.game, st.game_steps, st.score, st.left);
    out[3] = make_int4((int)(uint32_t)st.blo, (int)(uint32_t)(st.blo >> 32), (int)(uint32_t)st.bhi,
                       (int)(uint32_t)(st.bhi >> 32));
  }
  __device__ static Screen screen_of(const State& st) { return Screen{st.bx, st.by, st.px, st.blo, st.bhi}; }
  // (field by field: a select between the two structs would put them in scratch memory)
  __device__ static Screen pick(bool second, const Screen& cur, const Screen& prev) {
    return Screen{second ? prev.bx : cur.bx, second ? prev.by : cur.by, second ? prev.px : cur.px,
                  second ? prev.blo : cur.blo, second ? prev.bhi : cur.bhi};
  }
  __device__ static u32x4 chunk(int r, int c, const Screen& s) { return breakout_chunk(r, c, s); }
  // env_direct.hpp's shortcut: true if every pixel of row r has one colour, rgb = R | G << 8 | B << 16: a row
  // without the ball and the paddle that is black, or a brick row with all 20 of its bricks or none
  __device__ static bool plain_row(int r, const Screen& s, uint32_t& rgb) {
    rgb = 0u;
    if ((unsigned)(r - s.by) < (unsigned)BALL || (unsigned)(r - PADDLE_Y) < (unsigned)PADDLE_H) return false;
    if ((unsigned)(r - BRICK_Y0) >= (unsigned)(BRICK_Y1 - BRICK_Y0)) return true;
    const int br = (r - BRICK_Y0) / BRICK_H;
    const uint32_t bits = brick_row_bits(s.blo, s.bhi, br);
    if (bits == (1u << BRICK_COLS) - 1u)
      rgb = (uint32_t)((ROW_R >> (8 * br)) & 0xffu) | (uint32_t)((ROW_G >> (8 * br)) & 0xffu) << 8 |
            (uint32_t)((ROW_B >> (8 * br)) & 0xffu) << 16;
    return bits == 0u || bits == (1u << BRICK_COLS) - 1u;
  }

  // flags: ARL_ENV_GAME_OVER_ONLY (a life loss is not a terminal) or 0
  __device__ static void step(State& st, int act, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi, int flags,
                              Screen& cur, Screen& prev, Reward& reward, bool& done) {
    cur = prev = screen_of(st);
    bool lost = false;
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
      st.by += st.vy;
      if (st.by < CEILING) {
        st.by = 2 * CEILING - st.by;
        st.vy = -st.vy;
      }
      const int cx = st.bx + BALL / 2, cy = st.vy < 0 ? st.by : st.by + BALL - 1;
      if (cy >= BRICK_Y0 && cy < BRICK_Y1) {
        const int r = (cy - BRICK_Y0) / BRICK_H, i = BRICK_COLS * r + (cx >> 3);
        const uint64_t bit = 1ull << (i & 63);
        if ((i < 64 ? st.blo : st.bhi) & bit) {
          st.blo &= ~(i < 64 ? bit : 0ull);
          st.bhi &= ~(i < 64 ? 0ull : bit);
          reward += r < 2 ? 7 : r < 4 ? 4 : 1;
          st.vy = -st.vy;
          st.left -= 1;
        }
      }
      if (st.vy > 0 && st.by + BALL >= PADDLE_Y) {
        if (st.bx + BALL > st.px && st.bx < st.px + PADDLE_W) {
          st.by = 2 * (PADDLE_Y - BALL) - st.by;
          st.vy = -st.vy;
          // (the clamp compiles to v_med3_i32, a vector op on a wave-uniform value: taken back to a scalar
          // register at once, or the compiler may move the rest of the transition to the vector unit after it)
          st.vx = __builtin_amdgcn_readfirstlane(paddle_vx(min(max(st.bx + BALL / 2 - st.px, 0), PADDLE_W - 1) >> 2));
        } else {
          st.lives -= 1;
          lost = true;
        }
      }
      if (lost || st.left == 0) break;   // the skip loop breaks (ale.py:111-139)
      cur = screen_of(st);
    }
    st.game_steps += 1;
    st.score += reward;
    st.steps += 1;
    const bool over = st.lives == 0 || st.left == 0 || st.game_steps >= STEP_CAP;
    if (over) {   // the next game starts at once; its first screen twice, the last one is never shown
      st.game += 1;
      new_game(st, env_id, seed_lo, seed_hi);
      cur = prev = screen_of(st);
    } else if (lost) {   // bricks, lives, score and the paddle are kept
      serve(st, env_id, seed_lo, seed_hi);
      cur = prev = screen_of(st);
    }
    done = over || (lost && !flags);
    if (done) st.steps = 0;
  }
};

template hipError_t launch_game<Breakout>(const EnvArgs&, hipStream_t);
template hipError_t launch_game_direct<Breakout>(const DirectArgs&, hipStream_t);

}  // namespace arl
