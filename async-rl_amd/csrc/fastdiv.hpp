// Exact division and remainder by a divisor the host knows (the ring length R, the env count n, the
// pool length of an observe call), for device code whose dividend is only known on the device (the step
// counter ctl[CTL_STEP], a sample index).  The host precomputes the constants once (fd_make); the device
// path is straight-line integer code: no reciprocal instruction, no float, no data-dependent branch (the
// two corrections of fd_step are selects).  Plain C++, usable from host and device; tests/test_fastdiv.py
// builds it with the system compiler and compares it with the C++ operators.
//
//   fd_div32 / fd_mod32   any 32-bit dividend: Granlund & Montgomery 1994, figure 4.1 (one multiply-high,
//                         an add, two shifts)
//   fd_mod64 / fd_divmod64  any 64-bit dividend: the dividend and the divisor are shifted left until the
//                         divisor's top bit is set, then two 2-by-1 word divisions by the normalised divisor
//                         with its precomputed reciprocal word (Moeller & Granlund 2011, algorithm 4)
//
// Divisors: 1 <= d <= 2^31 - 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ARL_FD_HD __host__ __device__
#else
#define ARL_FD_HD
#endif

namespace arl {

struct FastDiv {
  uint32_t d = 1;     // the divisor
  uint32_t mul = 1;   // floor(2^32 (2^l - d) / d) + 1, l = ceil(log2 d)
  uint32_t sh1 = 0;   // min(l, 1)
  uint32_t sh2 = 0;   // max(l - 1, 0)
  uint32_t nsh = 31;  // leading zero bits of d (1..31): dn = d << nsh has its top bit set
  uint32_t inv = 0xffffffffu;   // floor((2^64 - 1) / dn) - 2^32
};

// host: the constants of divisor d (1 <= d <= 2^31 - 1)
inline FastDiv fd_make(uint32_t d) {
  FastDiv f;
  if (d == 0 || d > 0x7fffffffu) return f;   // out of range: the constants of 1 (callers validate first)
  uint32_t l = 0;
  while (((uint64_t)1 << l) < d) ++l;
  f.d = d;
  f.mul = (uint32_t)(((((uint64_t)1 << l) - d) << 32) / d + 1);
  f.sh1 = l < 1 ? l : 1;
  f.sh2 = l > 1 ? l - 1 : 0;
  f.nsh = 0;
  while (((d << f.nsh) & 0x80000000u) == 0) ++f.nsh;
  f.inv = (uint32_t)(~(uint64_t)0 / (d << f.nsh) - ((uint64_t)1 << 32));
  return f;
}

ARL_FD_HD inline uint32_t fd_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

ARL_FD_HD inline uint32_t fd_div32(const FastDiv& f, uint32_t x) {
  const uint32_t t = fd_mulhi(f.mul, x);
  return (t + ((x - t) >> f.sh1)) >> f.sh2;
}
ARL_FD_HD inline uint32_t fd_mod32(const FastDiv& f, uint32_t x) { return x - fd_div32(f, x) * f.d; }

// (u1 2^32 + u0) / dn for u1 < dn, dn's top bit set: the remainder, the quotient word in q
ARL_FD_HD inline uint32_t fd_step(uint32_t dn, uint32_t inv, uint32_t u1, uint32_t u0, uint32_t& q) {
  const uint64_t p = (uint64_t)inv * u1 + (((uint64_t)u1 << 32) | u0);   // < 2^64 for u1 < dn
  uint32_t q1 = (uint32_t)(p >> 32) + 1u;
  const uint32_t q0 = (uint32_t)p;
  uint32_t r = u0 - q1 * dn;
  const bool up = r > q0;
  q1 -= up ? 1u : 0u;
  r += up ? dn : 0u;
  const bool over = r >= dn;
  q1 += over ? 1u : 0u;
  r -= over ? dn : 0u;
  q = q1;
  return r;
}

ARL_FD_HD inline uint32_t fd_divmod64(const FastDiv& f, uint64_t x, uint64_t& q) {
  const uint32_t dn = f.d << f.nsh, hi = (uint32_t)(x >> 32), lo = (uint32_t)x, back = 32u - f.nsh;
  // x << nsh as three words; the top one is < 2^nsh <= 2^31 <= dn
  const uint32_t u2 = hi >> back, u1 = (hi << f.nsh) | (lo >> back), u0 = lo << f.nsh;
  uint32_t qh, ql;
  uint32_t r = fd_step(dn, f.inv, u2, u1, qh);
  r = fd_step(dn, f.inv, r, u0, ql);
  q = ((uint64_t)qh << 32) | ql;
  return r >> f.nsh;
}
ARL_FD_HD inline uint32_t fd_mod64(const FastDiv& f, uint64_t x) {
  uint64_t q;
  return fd_divmod64(f, x, q);
}

// x mod d for 0 <= x < 2 d (a window-local offset added to a residue): a compare and a subtract
ARL_FD_HD inline int fd_wrap(int x, int d) { return x >= d ? x - d : x; }

}  // namespace arl
