// Device-resident T-maze: the fourth device environment (include/asyncrl_hip.h, "device environment"), as the
// hooks of env_kernel.hpp's skeleton.  What the other three lack: partial observability.  A cue is shown on an
// episode's first screen only; the agent is then carried down a corridor of `length` env-steps and has to name
// the cue at the junction, after it has left the 4-observation stack (length >= 4): a task for the recurrent
// state.  A state of 8 integers; the transition every workgroup recomputes is two int4 loads and a dozen integer
// ops on wave-uniform values, one Philox block when an episode ends.
//
// Only chunks on the agent's 8 rows look at their pixels, word-wise as pong.hip's; every other chunk is one colour,
// because floor, arms and cue start on 48-byte boundaries.  No tables in memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_direct.hpp"
#include "env_kernel.hpp"
#include "policy_rows.hpp"

namespace arl {

namespace {

// the game's constants (include/asyncrl_hip.h)
constexpr int CELL = 16;                                           // a corridor cell: one env-step of 4 frames x 4 px
constexpr int FLOOR_Y0 = 96, FLOOR_H = 16;                         // rows 96..111
constexpr int ARM_Y0 = 48, ARM_H = 112;                            // rows 48..159
constexpr int AGENT = 8, AGENT_Y = 100, AGENT_X0 = 4, AGENT_DX = 4;
constexpr int CUE = 16, CUE_UP_Y = 72, CUE_DOWN_Y = 120;           // rows 72..87 / 120..135, columns 0..15
// Philox counter word 3, beside 0 (window), 1 (pi_and_v), 2 (Catch), 3 (Breakout) and 4 (Pong)
constexpr uint32_t ENV_STREAM = 5;

// a pixel's colour as 24 bits, R in the low byte: the order of its bytes in memory
__host__ __device__ inline constexpr uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return r | g << 8 | b << 16; }
constexpr uint32_t FLOOR_RGB = rgb(84, 84, 84), AGENT_RGB = rgb(92, 186, 92), CUE_UP_RGB = rgb(200, 72, 72),
                   CUE_DOWN_RGB = rgb(66, 72, 200);

struct Screen {
  int ax;     // the agent's left edge
  int xl;     // 16 * length: the arms' left edge
  int show;   // the cue drawn: 0 none, 1 "up", 2 "down"
};

// the 32-bit word that starts in channel p of a pixel of colour c0 and ends in the next pixel, of colour c1:
// 3 - p bytes of the first, p + 1 of the second (pong.hip's)
__host__ __device__ inline uint32_t word_of(uint32_t c0, uint32_t c1, int p) { return c0 >> (8 * p) | c1 << (24 - 8 * p); }

// bytes [16 c, 16 c + 16) of screen row r.  The cells are 16 pixels = 48 bytes = three chunks wide, and the floor,
// the arms and the cue start on cell boundaries: off the agent's 8 rows a chunk holds one colour -- zero, grey
// (three equal bytes) or the cue's, in the three phases a word can start in, rotated by the chunk's (pong.hip).
// On the agent's rows a word at byte b0 covers pixel x0 = b0 / 3 from its channel p = b0 % 3 on and pixel x0 + 1
// in the rest.
__host__ __device__ inline u32x4 tmaze_chunk(int r, int c, const Screen& s) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if ((unsigned)(r - ARM_Y0) >= (unsigned)ARM_H) return v;
  const bool floor_row = (unsigned)(r - FLOOR_Y0) < (unsigned)FLOOR_H;
  if ((unsigned)(r - AGENT_Y) >= (unsigned)AGENT) {
    const int arms_c = 3 * s.xl / CELL;   // the arms' first chunk; the grey chunks of the row end with theirs
    if ((unsigned)(c - (floor_row ? 0 : arms_c)) < (unsigned)(floor_row ? arms_c + 3 : 3)) {
      v[0] = v[1] = v[2] = v[3] = word_of(FLOOR_RGB, FLOOR_RGB, 0);
    } else if (c < 3 && s.show != 0 && (unsigned)(r - (s.show == 1 ? CUE_UP_Y : CUE_DOWN_Y)) < (unsigned)CUE) {
      // word w starts in channel (16 c + 4 w) % 3 = (c + w) % 3, and c is 0, 1 or 2 (no floor lies under the cue)
      const uint32_t k = s.show == 1 ? CUE_UP_RGB : CUE_DOWN_RGB;
      const uint32_t s0 = word_of(k, k, 0), s1 = word_of(k, k, 1), s2 = word_of(k, k, 2);
      v[0] = v[3] = c == 0 ? s0 : c == 1 ? s1 : s2;
      v[1] = c == 0 ? s1 : c == 1 ? s2 : s0;
      v[2] = c == 0 ? s2 : c == 1 ? s0 : s1;
    }
    return v;
  }
  // an agent row: a floor row, grey over [0, xl + 16), and no cue's
  const int gw = s.xl + CELL;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int b0 = 16 * c + 4 * w, x0 = b0 / 3, p = b0 - 3 * x0;
    uint32_t colour[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int x = x0 + i;   // (x <= 159: the row's last word starts in pixel 158)
      colour[i] = x < gw ? FLOOR_RGB : 0u;
      if ((unsigned)(x - s.ax) < (unsigned)AGENT) colour[i] = AGENT_RGB;   // the agent over the floor
    }
    v[w] = word_of(colour[0], colour[1], p);
  }
  return v;
}

struct EnvState {
  int pos, cue, length, steps, episode, hits, misses, lapses;
};

// episode start: pos = 0 (ax = 4), cue from Philox(counter = (env id, episode, 0, 5), key = seed)
__device__ inline void start_episode(EnvState& st, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi) {
  const uint4 w = philox4x32_10(make_uint4(env_id, (uint32_t)st.episode, 0u, ENV_STREAM), seed_lo, seed_hi);
  st.pos = 0;
  st.steps = 0;
  st.cue = (int)(w.x & 1u);
}

}  // namespace

struct TMaze {
  static constexpr int STATE_INTS = TMAZE_STATE_INTS;
  using State = EnvState;
  using Screen = arl::Screen;
  using Reward = int;   // +1, -1 or 0, cast where it is stored

  // flags: the corridor's length, 1..8 (launch_env takes it from the kind); it is kept in the state row
  __device__ static State start(uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi, int flags) {
    State st{};
    st.length = flags;
    start_episode(st, env_id, seed_lo, seed_hi);
    return st;
  }
  __device__ static State load(const int4* old) {
    const int4 o0 = old[0], o1 = old[1];
    return State{o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
  }
  __device__ static void store(int4* out, const State& st) {
    out[0] = make_int4(st.pos, st.cue, st.length, st.steps);
    out[1] = make_int4(st.episode, st.hits, st.misses, st.lapses);
  }
  // the screen between env-steps: the cue is on an episode's first screen alone
  __device__ static Screen screen_of(const State& st) {
    return Screen{AGENT_X0 + CELL * st.pos, CELL * st.length, st.pos == 0 ? 1 + st.cue : 0};
  }
  // (field by field: a select between the two structs would put them in scratch memory)
  __device__ static Screen pick(bool second, const Screen& cur, const Screen& prev) {
    return Screen{second ? prev.ax : cur.ax, second ? prev.xl : cur.xl, second ? prev.show : cur.show};
  }
  __device__ static u32x4 chunk(int r, int c, const Screen& s) { return tmaze_chunk(r, c, s); }
  // env_direct.hpp's shortcut: true if every pixel of row r has one colour, rgb = R | G << 8 | B << 16.  Every
  // row of 48..159 holds the arms, so only the rows outside are plain
  __device__ static bool plain_row(int r, const Screen&, uint32_t& rgb) {
    rgb = 0u;
    return (unsigned)(r - ARM_Y0) >= (unsigned)ARM_H;
  }

  // flags: the length again (the call's, as Pong's points are; a caller keeps it the reset's), kept in the row
  __device__ static void step(State& st, int act, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi, int flags,
                              Screen& cur, Screen& prev, Reward& reward, bool& done) {
    st.length = flags;
    if (st.pos < st.length) {   // the corridor: four frames of 4 px, the action ignored, no cue on either screen
      st.pos += 1;
      st.steps += 1;
      cur = Screen{AGENT_X0 + CELL * st.pos, CELL * st.length, 0};
      prev = Screen{cur.ax - AGENT_DX, cur.xl, 0};
      return;
    }
    // the junction: 2 = the upper arm, 3 = the lower one, anything else no choice
    const int choice = act == 2 ? 0 : act == 3 ? 1 : -1;
    reward = choice < 0 ? 0 : choice == st.cue ? 1 : -1;
    done = true;
    st.hits += reward > 0 ? 1 : 0;
    st.misses += reward < 0 ? 1 : 0;
    st.lapses += choice < 0 ? 1 : 0;
    st.episode += 1;
    start_episode(st, env_id, seed_lo, seed_hi);   // the next episode starts at once; its first screen twice
    cur = prev = screen_of(st);
  }
};

template hipError_t launch_game<TMaze>(const EnvArgs&, hipStream_t);
template hipError_t launch_game_direct<TMaze>(const DirectArgs&, hipStream_t);

}  // namespace arl
