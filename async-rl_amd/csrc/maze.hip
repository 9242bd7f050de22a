// Device-resident grid maze with procedurally generated levels: the fifth device environment
// (include/asyncrl_hip.h, "device environment"), as the hooks of env_kernel.hpp's skeleton.  What the other four
// lack: the layout, the start and the goal are drawn per episode from a numbered set of levels, so a policy can be
// trained on `levels` tasks and scored on all of them, and a `view` knob hides everything outside a small window
// around the agent.  A level is a handful of integers: the carving bits of a binary-tree maze over R x R rooms, a
// start room and a goal room.  A state of 8 integers; the transition every workgroup recomputes is two int4 loads
// and a few dozen integer ops on wave-uniform values, two Philox blocks when an episode ends.
//
// A tile is 16 pixels = 48 bytes = three chunks wide, so a chunk lies inside one tile: off the agent's 8 rows a
// chunk is one colour (tmaze.hip's and pong.hip's scheme); only chunks on the agent's rows look at their pixels,
// word-wise.  A tile's openness comes from the carving bits by shifts and compares.  No tables in memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env_direct.hpp"
#include "env_kernel.hpp"
#include "policy_rows.hpp"

namespace arl {

namespace {

// the game's constants (include/asyncrl_hip.h)
constexpr int TILE = 16, MAZE_Y0 = 32;                   // tile (ty, tx): rows 32 + 16 ty .. + 15, columns 16 tx .. + 15
constexpr int AGENT = 8, AGENT_OFF = 4, AGENT_DX = 4;    // 8 x 8 at (4, 4) inside its tile; a frame moves it 4 px
// Philox counter word 3, beside 0 (window), 1 (pi_and_v), 2 (Catch), 3 (Breakout), 4 (Pong) and 5 (T-maze)
constexpr uint32_t ENV_STREAM = 6;

// a pixel's colour as 24 bits, R in the low byte: the order of its bytes in memory
__host__ __device__ inline constexpr uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return r | g << 8 | b << 16; }
constexpr uint32_t OPEN_RGB = rgb(40, 40, 40), WALL_RGB = rgb(96, 96, 96), GOAL_RGB = rgb(236, 236, 120),
                   AGENT_RGB = rgb(92, 186, 92);

// the call's packed configuration, the kind's bits 16 and up with the rooms' default filled in
__host__ __device__ inline int cfg_rooms(int cfg) { return cfg & 7; }
__host__ __device__ inline int cfg_view(int cfg) { return (cfg >> 3) & 3; }
__host__ __device__ inline int cfg_levels(int cfg) { return cfg >> 5; }

struct Screen {
  int ax, ay;   // the agent's left column and top row
  int at;       // the agent's tile after the step, 16 ty + tx: the centre of the view, the same in both screens
  int goal;     // the goal's tile
  int bits;     // the carving bits
  int cfg;
};

// Is tile (ty, tx), 0 <= ty, tx <= 2 R, open?  Rooms are the odd-odd tiles; the tile north of room (i, j), i >= 1,
// is open if that room carves north (column R - 1 always does, else bit (i - 1)(R - 1) + j), the tile east of room
// (i, j), j <= R - 2, if it carves east (row 0 always does, else the bit clear).  The border and the even-even
// tiles are wall.
__host__ __device__ inline bool tile_open(int ty, int tx, uint32_t bits, int R) {
  const bool oy = ty & 1, ox = tx & 1;
  if (oy && ox) return true;
  if (oy == ox) return false;
  const int i = ty >> 1, j = oy ? (tx >> 1) - 1 : tx >> 1;   // the room the passage belongs to
  if (oy) {                                                 // east of room (i, j)
    if (j < 0 || j >= R - 1) return false;
    return i == 0 || !((bits >> ((i - 1) * (R - 1) + j)) & 1u);
  }
  if (i < 1 || i >= R) return false;                        // north of room (i, j)
  return j == R - 1 || ((bits >> ((i - 1) * (R - 1) + j)) & 1u);
}

// the 32-bit word that starts in channel p of a pixel of colour c0 and ends in the next pixel, of colour c1:
// 3 - p bytes of the first, p + 1 of the second (pong.hip's)
__host__ __device__ inline uint32_t word_of(uint32_t c0, uint32_t c1, int p) { return c0 >> (8 * p) | c1 << (24 - 8 * p); }

// the colour of tile (ty, tx) on screen s, 0 <= ty <= 2 R: background right of the maze, fog outside the view
__host__ __device__ inline uint32_t tile_rgb(int ty, int tx, const Screen& s) {
  const int R = cfg_rooms(s.cfg), V = cfg_view(s.cfg);
  if (tx > 2 * R) return 0u;
  if (V != 0) {
    const int dy = ty - (s.at >> 4), dx = tx - (s.at & 15);
    if ((dy < 0 ? -dy : dy) > V || (dx < 0 ? -dx : dx) > V) return 0u;
  }
  if ((ty << 4 | tx) == s.goal) return GOAL_RGB;
  return tile_open(ty, tx, (uint32_t)s.bits, R) ? OPEN_RGB : WALL_RGB;
}

// bytes [16 c, 16 c + 16) of screen row r.  Chunk c lies in tile column c / 3, at bytes 16 (c % 3) of the tile's
// 48: off the agent's rows it holds one colour, in the three phases a word can start in, rotated by c % 3 (greys
// read the same in every phase; the goal's colour does not).  On the agent's rows a word at byte b0 covers pixel
// x0 = b0 / 3 from its channel p = b0 % 3 on and pixel x0 + 1 in the rest, both inside the chunk's tile.
__host__ __device__ inline u32x4 maze_chunk(int r, int c, const Screen& s) {
  u32x4 v = {0u, 0u, 0u, 0u};
  const int G = 2 * cfg_rooms(s.cfg) + 1;
  if ((unsigned)(r - MAZE_Y0) >= (unsigned)(TILE * G)) return v;
  const int tx = c / 3, ph = c - 3 * tx;
  const uint32_t k = tile_rgb((r - MAZE_Y0) >> 4, tx, s);
  if ((unsigned)(r - s.ay) >= (unsigned)AGENT) {
    // word w starts in channel (16 c + 4 w) % 3 = (ph + w) % 3
    const uint32_t s0 = word_of(k, k, 0), s1 = word_of(k, k, 1), s2 = word_of(k, k, 2);
    v[0] = v[3] = ph == 0 ? s0 : ph == 1 ? s1 : s2;
    v[1] = ph == 0 ? s1 : ph == 1 ? s2 : s0;
    v[2] = ph == 0 ? s2 : ph == 1 ? s0 : s1;
    return v;
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int b0 = 16 * c + 4 * w, x0 = b0 / 3, p = b0 - 3 * x0;
    const uint32_t c0 = (unsigned)(x0 - s.ax) < (unsigned)AGENT ? AGENT_RGB : k;   // the agent over its tile
    const uint32_t c1 = (unsigned)(x0 + 1 - s.ax) < (unsigned)AGENT ? AGENT_RGB : k;
    v[w] = word_of(c0, c1, p);
  }
  return v;
}

struct EnvState {
  int posgoal;   // pos | goal << 8, both 16 ty + tx
  int bits, steps, episode, wins, timeouts, level, cfg;
};

// (uint64(a) * b) >> 32: a uniform draw from [0, b) without a division
__device__ inline uint32_t mulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }

// room index i R + j -> its tile 16 (2 i + 1) + 2 j + 1; i = idx / R by a multiply and a shift, exact for idx < 16
// and R in 2..4
__device__ inline int room_tile(int idx, int R) {
  const int i = (idx * (R == 2 ? 16 : R == 3 ? 11 : 8)) >> 5, j = idx - i * R;
  return (2 * i + 1) << 4 | (2 * j + 1);
}

// episode start: the level from Philox(counter = (env id, episode, 0, 6)), the task from Philox(counter = (level,
// 0, 1, 6)), both with key = seed; steps = 0.  R and levels are st.cfg's.
__device__ inline void start_episode(EnvState& st, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi) {
  const int R = cfg_rooms(st.cfg), levels = cfg_levels(st.cfg);
  const uint32_t w0 = philox4x32_10(make_uint4(env_id, (uint32_t)st.episode, 0u, ENV_STREAM), seed_lo, seed_hi).x;
  const uint32_t level = levels != 0 ? mulhi(w0, (uint32_t)levels) : w0;
  const uint4 t = philox4x32_10(make_uint4(level, 0u, 1u, ENV_STREAM), seed_lo, seed_hi);
  const uint32_t rooms = (uint32_t)(R * R);
  const uint32_t s = mulhi(t.y, rooms);
  uint32_t g = s + 1u + mulhi(t.z, rooms - 1u);
  g -= g >= rooms ? rooms : 0u;
  st.bits = (int)(t.x & ((1u << ((R - 1) * (R - 1))) - 1u));
  st.posgoal = room_tile((int)s, R) | room_tile((int)g, R) << 8;
  st.steps = 0;
  st.level = (int)level;
}

}  // namespace

struct Maze {
  static constexpr int STATE_INTS = MAZE_STATE_INTS;
  using State = EnvState;
  using Screen = arl::Screen;
  using Reward = int;   // 1 or 0, cast where it is stored

  // flags: the packed (rooms, view, levels) (launch_env takes it from the kind); it is kept in the state row
  __device__ static State start(uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi, int flags) {
    State st{};
    st.cfg = flags;
    start_episode(st, env_id, seed_lo, seed_hi);
    return st;
  }
  __device__ static State load(const int4* old) {
    const int4 o0 = old[0], o1 = old[1];
    return State{o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
  }
  __device__ static void store(int4* out, const State& st) {
    out[0] = make_int4(st.posgoal, st.bits, st.steps, st.episode);
    out[1] = make_int4(st.wins, st.timeouts, st.level, st.cfg);
  }
  // the screen between env-steps: the agent at rest on its tile
  __device__ static Screen screen_of(const State& st) {
    const int pos = st.posgoal & 0xff;
    return Screen{TILE * (pos & 15) + AGENT_OFF, MAZE_Y0 + TILE * (pos >> 4) + AGENT_OFF, pos, st.posgoal >> 8,
                  st.bits, st.cfg};
  }
  // (field by field: a select between the two structs would put them in scratch memory)
  __device__ static Screen pick(bool second, const Screen& cur, const Screen& prev) {
    return Screen{second ? prev.ax : cur.ax,     second ? prev.ay : cur.ay,     second ? prev.at : cur.at,
                  second ? prev.goal : cur.goal, second ? prev.bits : cur.bits, second ? prev.cfg : cur.cfg};
  }
  __device__ static u32x4 chunk(int r, int c, const Screen& s) { return maze_chunk(r, c, s); }
  // env_direct.hpp's shortcut: true if every pixel of row r has one colour, rgb = R | G << 8 | B << 16.  Every
  // row of the maze holds border wall (or, under fog, may hold the agent), so only the rows outside are plain
  __device__ static bool plain_row(int r, const Screen& s, uint32_t& rgb) {
    rgb = 0u;
    return (unsigned)(r - MAZE_Y0) >= (unsigned)(TILE * (2 * cfg_rooms(s.cfg) + 1));
  }

  // flags: the configuration again (the call's, as the T-maze's length is; a caller keeps it the reset's)
  __device__ static void step(State& st, int act, uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi, int flags,
                              Screen& cur, Screen& prev, Reward& reward, bool& done) {
    st.cfg = flags;
    const int R = cfg_rooms(flags);
    const int pos = st.posgoal & 0xff, goal = st.posgoal >> 8;
    const int d = act & 3;   // 0 up, 1 down, 2 right, 3 left
    const int dy = d == 0 ? -1 : d == 1 ? 1 : 0, dx = d == 2 ? 1 : d == 3 ? -1 : 0;
    // the agent stands inside the border, so the target is a tile of the maze
    const bool moved = tile_open((pos >> 4) + dy, (pos & 15) + dx, (uint32_t)st.bits, R);
    const int now = moved ? pos + 16 * dy + dx : pos;
    st.steps += 1;
    st.posgoal = now | goal << 8;
    if (now == goal) {
      reward = 1;
      done = true;
      st.wins += 1;
    } else if (st.steps == 8 * R) {
      done = true;
      st.timeouts += 1;
    }
    if (done) {
      st.episode += 1;
      start_episode(st, env_id, seed_lo, seed_hi);   // the next episode starts at once; its first screen twice
      cur = prev = screen_of(st);
      return;
    }
    // four frames of 4 px: pair[1] is the screen after frame 3, 4 px short of the target; a bump moves nothing
    cur = screen_of(st);
    prev = Screen{cur.ax - (moved ? AGENT_DX * dx : 0), cur.ay - (moved ? AGENT_DX * dy : 0), cur.at, cur.goal,
                  cur.bits, cur.cfg};
  }
};

template hipError_t launch_game<Maze>(const EnvArgs&, hipStream_t);
template hipError_t launch_game_direct<Maze>(const DirectArgs&, hipStream_t);

}  // namespace arl
