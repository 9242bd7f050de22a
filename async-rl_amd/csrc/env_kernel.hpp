// The device environments' kernel skeleton (include/asyncrl_hip.h, "device environment"; no reference
// counterpart -- the reference's envs are host emulators, ale.py / doom_env.py): everything of an env-step
// that is not a game rule.  One launch per env-step does the transition and the render: it reads the actions the
// policy sampled, steps every env's handful of integers, and writes the (frame 4, frame 3) pair, the reward and
// the done flag into the pool entry the next arl_observe reads (EnvArgs, arl_internal.hpp, has the indices).
//
// No workgroup reads a word another workgroup of its launch writes (the hazard optim.hip documents for the
// control block): the env state is double-buffered, every workgroup of an env recomputes the transition from
// the OLD half (integer ops on wave-uniform values), and only band 0's thread 0 writes the new half, the
// reward and the done.
//
// The render is a pure store stream, 2 x 210 rows x 480 bytes per env as 16-byte stores.  No LDS, no loads
// besides the state, the action and the step counter.  Grid (ENV_BANDS, envs): a band is 2,520 consecutive
// chunks of the pair, 10 stores per lane (DESIGN.md "Device environment" has the measurements).
//
// A game (catch.hip, breakout.hip, pong.hip, tmaze.hip) is a struct of static hooks:
//   STATE_INTS                 ints of one env's state row, a multiple of 4 (the row is read and written as int4s)
//   State, Screen, Reward      the row unpacked; what the render needs of it; int or float
//   start(env_id, seed_lo, seed_hi) -> State                   the reset; a game whose reset depends on its flags
//                              (tmaze.hip: the corridor's length) gives start(env_id, seed_lo, seed_hi, flags)
//                              instead, and game_start below calls whichever there is
//   load(const int4*) -> State, store(int4*, const State&)     the state row
//   step(State&, act, env_id, seed_lo, seed_hi, flags, Screen& cur, Screen& prev, Reward&, bool& done)
//                              up to 4 frames, then the restart / serve; cur, prev: the pair's two screens
//   screen_of(const State&) -> Screen
//   pick(second, cur, prev) -> Screen                          the screen of pair[second], by value
//   chunk(r, c, const Screen&) -> u32x4                        bytes [16 c, 16 c + 16) of screen row r
// and instantiates launch_game<Game> (arl_internal.hpp declares it; launch_env calls it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arl_internal.hpp"

namespace arl {

constexpr int SCREEN_H = 210, SCREEN_W = 160;
constexpr int ROW_CHUNKS = SCREEN_W * 3 / 16;                  // 30 16-byte chunks a row
constexpr int PAIR_CHUNKS = 2 * SCREEN_H * ROW_CHUNKS;         // 12,600
constexpr int ENV_BANDS = 5;                                   // workgroups per env
constexpr int BAND_CHUNKS = PAIR_CHUNKS / ENV_BANDS;           // 2,520 = 9.84 x 256: the last pass is 84 % full
static_assert(PAIR_CHUNKS % ENV_BANDS == 0, "bands tile the pair");
static_assert(PAIR == PAIR_CHUNKS * 16, "frame pair bytes");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Game::start with the flags if the game takes them (the int overload wins where it is well-formed), else without
template <class Game>
__device__ inline auto game_start(uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi, int flags, int)
    -> decltype(Game::start(env_id, seed_lo, seed_hi, flags)) {
  return Game::start(env_id, seed_lo, seed_hi, flags);
}
template <class Game>
__device__ inline typename Game::State game_start(uint32_t env_id, uint32_t seed_lo, uint32_t seed_hi, int, long) {
  return Game::start(env_id, seed_lo, seed_hi);
}

template <class Game>
__global__ void __launch_bounds__(256)
env_kernel(EnvArgs a) {
  const int e = a.e0 + blockIdx.y;
  const bool reset = a.actions == nullptr;
  const int64_t k = (a.ctl != nullptr ? a.ctl[CTL_STEP] : 0) + a.t;   // the observation the actions answer
  const int64_t kout = reset ? k : k + 1;                             // the observation this launch produces
  const uint32_t pidx = fd_mod64(a.dpool, (uint64_t)kout);
  const uint32_t env_id = (uint32_t)(a.env_offset + e);

  typename Game::State st;
  typename Game::Screen cur, prev;
  typename Game::Reward reward = 0;
  bool done = false;
  if (reset) {
    st = game_start<Game>(env_id, a.seed_lo, a.seed_hi, a.flags, 0);
    cur = prev = Game::screen_of(st);
  } else {
    st = Game::load(reinterpret_cast<const int4*>(a.state + ((int64_t)(k & 1) * a.n + e) * Game::STATE_INTS));
    Game::step(st, a.actions[e], env_id, a.seed_lo, a.seed_hi, a.flags, cur, prev, reward, done);
  }

  const int64_t row = (int64_t)pidx * a.n + e;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    Game::store(reinterpret_cast<int4*>(a.state + ((int64_t)(kout & 1) * a.n + e) * Game::STATE_INTS), st);
    a.reward_pool[row] = (float)reward;
    a.done_pool[row] = done ? 1 : 0;
  }

  u32x4* dst = reinterpret_cast<u32x4*>(a.pair_pool + row * PAIR);
  const int q0 = blockIdx.x * BAND_CHUNKS;
#pragma unroll 2
  for (int i = threadIdx.x; i < BAND_CHUNKS; i += 256) {
    const int q = q0 + i, row2 = q / ROW_CHUNKS, c = q - row2 * ROW_CHUNKS;
    const bool second = row2 >= SCREEN_H;   // pair[1]: the screen one frame earlier
    // plain stores: the observation that follows reads these bytes, and non-temporal ones measured slower
    // both here (20.1 vs 17.0 us at 512 envs, Catch) and in that observation (23.2 vs 20.5 us)
    dst[q] = Game::chunk(second ? row2 - SCREEN_H : row2, c, Game::pick(second, cur, prev));
  }
}

template <class Game>
hipError_t launch_game(const EnvArgs& a, hipStream_t s) {
  static_assert(Game::STATE_INTS % 4 == 0, "the state row is int4s");
  const int ne = a.ne < 0 ? a.n : a.ne;
  if (ne <= 0) return hipSuccess;
  hipLaunchKernelGGL(env_kernel<Game>, dim3(ENV_BANDS, (unsigned)ne), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace arl
