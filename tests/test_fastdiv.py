"""csrc/fastdiv.hpp against the C++ operators, on the CPU: the header is plain C++, so a stand-alone host
program built with the system compiler runs the very functions the kernels inline.

Divisors: every value in 1..4096 and 4,000 random ones up to 2^31 - 1 (2^31 - 1 itself included).
Dividends per divisor: 0, d - 1, d, d + 1; the multiples of d on either side of 2^31, 2^32, 2^40 and 2^62,
each -2..+2; 3,000 random 62-bit values and the same values shifted down into 32 bits.  Every dividend
goes through fd_divmod64 / fd_mod64; those below 2^32 also through fd_div32 / fd_mod32.  The program
counts what it checked, and the test pins those counts, so no case can drop out unnoticed."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG

SRC = r"""
#include <stdint.h>
#include <stdio.h>
#include "fastdiv.hpp"
using namespace arl;

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static uint64_t checks64 = 0, checks32 = 0, bad = 0;

static void check(const FastDiv& f, uint64_t x) {
  const uint64_t d = f.d;
  uint64_t q;
  const uint32_t r = fd_divmod64(f, x, q);
  ++checks64;
  if (q != x / d || r != x % d || fd_mod64(f, x) != x % d) {
    if (bad++ < 10) printf("BAD64 d=%llu x=%llu q=%llu r=%u\n", (unsigned long long)d, (unsigned long long)x,
                           (unsigned long long)q, r);
  }
  if (x <= 0xffffffffull) {
    const uint32_t x32 = (uint32_t)x;
    ++checks32;
    if (fd_div32(f, x32) != x32 / f.d || fd_mod32(f, x32) != x32 % f.d) {
      if (bad++ < 10) printf("BAD32 d=%u x=%u q=%u\n", f.d, x32, fd_div32(f, x32));
    }
  }
}

static void divisor(uint32_t d) {
  const FastDiv f = fd_make(d);
  check(f, 0);
  check(f, d - 1);
  check(f, d);
  check(f, (uint64_t)d + 1);
  const int pows[4] = {31, 32, 40, 62};
  for (int i = 0; i < 4; ++i) {
    const uint64_t P = (uint64_t)1 << pows[i], below = P / d * d;
    for (int side = 0; side < 2; ++side) {
      const uint64_t m = below + (side ? d : 0);
      for (int o = -2; o <= 2; ++o)
        if (m + o < ((uint64_t)1 << 63) && !(m == 0 && o < 0)) check(f, m + o);
        else check(f, m);   // (never taken for these powers and divisors; keeps the count fixed)
    }
  }
  for (int i = 0; i < 3000; ++i) {
    const uint64_t x = rnd() >> 2;   // 62 bits
    check(f, x);
    check(f, x >> 30);               // 32 bits
  }
}

int main() {
  uint64_t divisors = 0;
  for (uint32_t d = 1; d <= 4096; ++d, ++divisors) divisor(d);
  divisor(0x7fffffffu);
  ++divisors;
  for (int i = 0; i < 3999; ++i, ++divisors) {
    // spread over every bit length up to 31
    const uint32_t bits = 13 + (uint32_t)(rnd() % 19);   // 13..31
    uint32_t d = (uint32_t)(rnd() >> (64 - bits)) | (1u << (bits - 1));
    if (d > 0x7fffffffu) d = 0x7fffffffu;
    divisor(d);
  }
  printf("divisors %llu checks64 %llu checks32 %llu bad %llu\n", (unsigned long long)divisors,
         (unsigned long long)checks64, (unsigned long long)checks32, (unsigned long long)bad);
  return bad ? 1 : 0;
}
"""

N_DIV = 4096 + 4000
PER_DIV64 = 4 + 4 * 2 * 5 + 2 * 3000


def test_fastdiv_matches_cpp_operators(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler: the fast-division helper cannot be checked"
    src = tmp_path / "fastdiv_check.cpp"
    src.write_text(SRC)
    exe = tmp_path / "fastdiv_check"
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    words = out.stdout.strip().splitlines()[-1].split()
    stats = dict(zip(words[0::2], map(int, words[1::2])))
    assert stats["divisors"] == N_DIV
    assert stats["checks64"] == N_DIV * PER_DIV64
    # below 2^32 at the least: 0, d - 1, d, d + 1; the 10 values around 2^31; two below the multiple at or
    # under 2^32; the 3,000 shifted random values
    assert stats["checks32"] >= N_DIV * (4 + 10 + 2 + 3000)
    assert stats["bad"] == 0
