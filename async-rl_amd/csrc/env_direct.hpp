// The device environments' direct-to-ring launch (include/asyncrl_hip.h, "direct-to-ring device env"): one launch
// per env-step does the transition of env_kernel.hpp AND the observation of phi_ring_kernel (phi.hip), without the
// 210 x 160 x 3 frame pair between them.  Every screen of a game is a function of a handful of integers
// (Game::chunk), so the bytes phi_band loads from the pool are produced in registers instead: the same
// umax_bytes / luminance / resize_coeff / resize_vpass arithmetic (phi_ops.hpp) on the same bytes, hence the same
// plane, bit for bit.  Per env and step the launch writes one 84 x 84 plane (7,056 B) where the pair path writes 201,600 B
// and reads them back.
//
// Grid (envs, 7 bands) x 256 threads: one workgroup per env per band of 12 output rows, as phi_ring_kernel, with
// the env in blockIdx.x: consecutive workgroups go to consecutive XCDs, so with a multiple of 8 envs the 7 bands of
// an env run on one XCD and 6 of them find its state row and action in that XCD's L2.
// Every workgroup of an env recomputes the transition from the OLD state half (env_kernel.hpp's rule: no
// workgroup reads a word another workgroup of its launch writes); band 0's thread 0 alone writes the new half
// and the observation's bookkeeping (ring_obs_store: nvalid, reset flag, reward, done, episode statistics) from
// the reward and done it just computed.  nvalid is read at slot(k) and written at slot(k + 1).
//
// A game file (catch.hip, breakout.hip, pong.hip, tmaze.hip) instantiates launch_game_direct<Game> beside launch_game<Game>
// and gives one hook more than env_kernel.hpp lists:
//   plain_row(r, const Screen&, uint32_t& rgb) -> bool     every pixel of screen row r is the colour rgb (R low byte)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arl_internal.hpp"
#include "env_kernel.hpp"
#include "phi_ops.hpp"

namespace arl {

constexpr int DIRECT_BAND = 12;                        // output rows per workgroup
constexpr int DIRECT_NBANDS = DST / DIRECT_BAND;       // 7
static_assert(DST % DIRECT_BAND == 0, "bands tile the plane");

struct DirectShared {
  alignas(16) uint8_t gray[DIRECT_BAND][2][SRC_W];   // [output row][tap][x], written 16 bytes a stager
  uint32_t xc[DST];           // column dx: source column | weight a0 << 8 | weight a1 << 20 (weights <= 2048), one read
  uint32_t yc[DIRECT_BAND];   // output row: weight b0 | weight b1 << 16
};

// max_luminance16 (phi_ops.hpp) for rendered pixels: the same per-pixel max and the same luminance(), evaluated
// only where a pixel's (R, G, B) differs from the pixel before it.  A rendered span is a few runs of one colour,
// and the lanes of a wave change colour at few distinct positions, so most of the 16 float64 evaluations are
// skipped by the whole wave; a repeated pixel takes the value computed from the identical triple.
__device__ inline uint4 max_luminance16_runs(const u32x4& c0, const u32x4& c1, const u32x4& c2, const u32x4& p0,
                                             const u32x4& p1, const u32x4& p2) {
  const uint32_t w[12] = {umax_bytes(c0[0], p0[0]), umax_bytes(c0[1], p0[1]), umax_bytes(c0[2], p0[2]),
                          umax_bytes(c0[3], p0[3]), umax_bytes(c1[0], p1[0]), umax_bytes(c1[1], p1[1]),
                          umax_bytes(c1[2], p1[2]), umax_bytes(c1[3], p1[3]), umax_bytes(c2[0], p2[0]),
                          umax_bytes(c2[1], p2[1]), umax_bytes(c2[2], p2[2]), umax_bytes(c2[3], p2[3])};
  uint32_t g[4] = {0, 0, 0, 0};
  uint32_t last = 0xffffffffu, lum = 0;   // (no 24-bit triple equals the initial key)
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    const int b = 3 * p, k = b >> 2, sh = 8 * (b & 3);   // the pixel's 3 bytes start in word k at bit sh
    const uint32_t rgb = (sh == 0 ? w[k] : sh == 8 ? w[k] >> 8 : (w[k] >> sh) | (w[k + 1] << (32 - sh))) & 0xffffffu;
    if (rgb != last) {
      lum = luminance(rgb & 0xffu, (rgb >> 8) & 0xffu, rgb >> 16);
      last = rgb;
    }
    g[p >> 2] |= lum << (8 * (p & 3));
  }
  return make_uint4(g[0], g[1], g[2], g[3]);
}

// Output rows [dy0, dy0 + DIRECT_BAND) of the screen max(cur, prev) into `out` (row stride 84): phi_band's tasks
// with Game::chunk in place of its loads.  Stager task = (tap row r in 0..23, group c in 0..9 of 16 pixels = three
// 16-byte chunks of each screen); resize task = (local row, 4 output columns) -> one u32 store.
// Each of the four waves stages six whole tap rows (lanes 0..59; lanes 60..62 tabulate three rows' weights), so
// a wave takes the plain-row shortcut (Game::plain_row: a row of one colour in both screens needs one luminance,
// not 16 per task, and no chunk) unless one of ITS six rows holds a sprite.
template <class Game>
__device__ inline void direct_band(const typename Game::Screen& cur, const typename Game::Screen& prev,
                                   uint8_t* __restrict__ out, int dy0, int mode, DirectShared& sh) {
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  static_assert(2 * DIRECT_BAND == 4 * 6, "four waves of six tap rows");
  if (lane < 60) {
    const int r = 6 * wave + lane / 10, c = lane % 10;
    const int ly = r >> 1, tap = r & 1;
    int o, b0, b1;
    if (mode & 2) resize_coeff(dy0 + ly + CROP_TOP, SRC_H, CROP_H, o, b0, b1);
    else resize_coeff(dy0 + ly, SRC_H, DST, o, b0, b1);
    int sy = o + tap;
    if (sy > SRC_H - 1) sy = SRC_H - 1;
    uint32_t rc, rp;
    uint4 g;
    const bool plain_cur = Game::plain_row(sy, cur, rc), plain_prev = Game::plain_row(sy, prev, rp);
    if (plain_cur && plain_prev) {
      // a row without a sprite in either screen: every pixel is the same (R, G, B) pair, so one max and one
      // luminance stand for the 16 that max_luminance16 would compute from 16 equal pixels
      const uint32_t m = umax_bytes(rc, rp);
      const uint32_t w = luminance(m & 0xffu, (m >> 8) & 0xffu, (m >> 16) & 0xffu) * 0x01010101u;
      g = make_uint4(w, w, w, w);
    } else {
      g = max_luminance16_runs(Game::chunk(sy, 3 * c, cur), Game::chunk(sy, 3 * c + 1, cur),
                               Game::chunk(sy, 3 * c + 2, cur), Game::chunk(sy, 3 * c, prev),
                               Game::chunk(sy, 3 * c + 1, prev), Game::chunk(sy, 3 * c + 2, prev));
    }
    *reinterpret_cast<uint4*>(&sh.gray[ly][tap][c * 16]) = g;
  } else if (lane < 63) {   // the row weights of the wave's three output rows
    const int ly = 3 * wave + lane - 60;
    int o, b0, b1;
    if (mode & 2) resize_coeff(dy0 + ly + CROP_TOP, SRC_H, CROP_H, o, b0, b1);
    else resize_coeff(dy0 + ly, SRC_H, DST, o, b0, b1);
    sh.yc[ly] = (uint32_t)b0 | (uint32_t)b1 << 16;
  }
  if (tid < DST) {
    int o, a0, a1;
    resize_coeff(tid, SRC_W, DST, o, a0, a1);
    sh.xc[tid] = (uint32_t)o | (uint32_t)a0 << 8 | (uint32_t)a1 << 20;
  }
  __syncthreads();
  if (tid < DIRECT_BAND * (DST / 4)) {
    const int ly = tid / (DST / 4), q = tid - ly * (DST / 4);
    const uint32_t yw = sh.yc[ly];
    const int b0 = (int)(yw & 0xffffu), b1 = (int)(yw >> 16);
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int dx = q * 4 + j;
      const uint32_t xw = sh.xc[dx];
      const int sx = (int)(xw & 0xffu), a0 = (int)((xw >> 8) & 0xfffu), a1 = (int)(xw >> 20);
      const int sx1 = sx + 1 < SRC_W ? sx + 1 : SRC_W - 1;
      const int r0 = (int)sh.gray[ly][0][sx] * a0 + (int)sh.gray[ly][0][sx1] * a1;
      const int r1 = (int)sh.gray[ly][1][sx] * a0 + (int)sh.gray[ly][1][sx1] * a1;
      packed |= (uint32_t)resize_vpass(r0, r1, b0, b1, mode) << (8 * j);
    }
    // an ordinary store, as phi.hip's ring_store: the next conv launch reads it
    *reinterpret_cast<uint32_t*>(out + (size_t)(dy0 + ly) * DST + q * 4) = packed;
  }
}

template <class Game, bool EP>   // EP: with the episode statistics (launched when a.ring.episodes != null)
__global__ void __launch_bounds__(256)
env_direct_kernel(DirectArgs a) {
  __shared__ DirectShared sh;
  const EnvArgs& ea = a.env;
  const int e = ea.e0 + blockIdx.x, band = blockIdx.y;
  const bool reset = ea.actions == nullptr;
  const int64_t k = (ea.ctl != nullptr ? ea.ctl[CTL_STEP] : 0) + ea.t;   // the observation the actions answer
  const int64_t kout = reset ? k : k + 1;                                // the observation this launch produces
  const uint32_t env_id = (uint32_t)(ea.env_offset + e);

  typename Game::State st;
  typename Game::Screen cur, prev;
  typename Game::Reward reward = 0;
  bool done = false;
  if (reset) {
    st = game_start<Game>(env_id, ea.seed_lo, ea.seed_hi, ea.flags, 0);
    cur = prev = Game::screen_of(st);
  } else {
    st = Game::load(reinterpret_cast<const int4*>(ea.state + ((int64_t)(k & 1) * ea.n + e) * Game::STATE_INTS));
    Game::step(st, ea.actions[e], env_id, ea.seed_lo, ea.seed_hi, ea.flags, cur, prev, reward, done);
  }

  const int slot = (int)fd_mod64(a.ring.dR, (uint64_t)kout);
  // the one load of the bookkeeping goes out ahead of the band's work (as ring_obs_load's do in phi_ring_kernel)
  const bool keeper = band == 0 && threadIdx.x == 0;
  int pv = 0;
  if (keeper && a.ring.nvalid != nullptr)
    pv = (int)a.ring.nvalid[(int64_t)fd_wrap(slot + a.ring.R - 1, a.ring.R) * ea.n + e] + 1;
  direct_band<Game>(cur, prev, a.ring.frames + ((int64_t)slot * ea.n + e) * PLANE, band * DIRECT_BAND,
                    a.ring.mode, sh);

  if (keeper) {
    Game::store(reinterpret_cast<int4*>(ea.state + ((int64_t)(kout & 1) * ea.n + e) * Game::STATE_INTS), st);
    if (a.ring.nvalid == nullptr) {   // the granular call: the raw reward and the done, no ring
      a.reward_out[e] = (float)reward;
      a.done_out[e] = done ? 1 : 0;
    } else {
      // what ring_obs_load reads back from the pools and the slot before, from this launch's own values
      RingObs o;
      o.done = done ? 1 : 0;
      o.r = reset ? 0.f : (float)reward;
      o.nv = (a.ring.force_reset || done) ? 1 : (pv > 4 ? 4 : pv);
      ring_obs_store<EP>(a.ring, e, kout, slot, o);
    }
  }
}

template <class Game>
hipError_t launch_game_direct(const DirectArgs& a, hipStream_t s) {
  const int ne = a.env.ne < 0 ? a.env.n : a.env.ne;
  if (ne <= 0) return hipSuccess;
  const dim3 grid((unsigned)ne, DIRECT_NBANDS);
  if (a.ring.episodes != nullptr) hipLaunchKernelGGL((env_direct_kernel<Game, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((env_direct_kernel<Game, false>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace arl
