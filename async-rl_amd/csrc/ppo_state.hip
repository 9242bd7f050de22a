// The recurrent carry of PPO epochs on the LSTM (arl_net_set_ppo_state): the rollout's (h_T, c_T) saved out of
// rows T of hbuf / cbuf before the re-forwards of epochs >= 2 overwrite them, and put back before the window
// advances, so the next window starts from the state the rollout reached at theta_old whatever the epoch count.
// A kernel of its own (one node of a captured window, one stamp), in a file of its own: no other object's
// device code moves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arl_internal.hpp"

namespace arl {

// One float4 of each plane per thread: both loads issued before the first store.  save: carry <- rows T;
// restore: rows T <- carry.  carry = planes h then c, count4 float4 each.
template <bool RESTORE>
__global__ void __launch_bounds__(256)
ppo_carry_kernel(float4* __restrict__ h_row, float4* __restrict__ c_row, float4* __restrict__ carry, int64_t count4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count4) return;
  float4* ch = carry + i;
  float4* cc = carry + count4 + i;
  if constexpr (RESTORE) {
    const float4 h = *ch, c = *cc;
    h_row[i] = h;
    c_row[i] = c;
  } else {
    const float4 h = h_row[i], c = c_row[i];
    *ch = h;
    *cc = c;
  }
}

hipError_t launch_ppo_carry(float* hbuf, float* cbuf, float* carry, int T, int n, bool restore, hipStream_t s) {
  static_assert(HID % 4 == 0, "a row is whole float4s");
  const int64_t count4 = (int64_t)n * (HID / 4);
  if (count4 == 0) return hipSuccess;
  float4* h_row = reinterpret_cast<float4*>(hbuf + (int64_t)T * n * HID);
  float4* c_row = reinterpret_cast<float4*>(cbuf + (int64_t)T * n * HID);
  const dim3 grid((unsigned)((count4 + 255) / 256));
  if (restore)
    hipLaunchKernelGGL(ppo_carry_kernel<true>, grid, dim3(256), 0, s, h_row, c_row, reinterpret_cast<float4*>(carry),
                       count4);
  else
    hipLaunchKernelGGL(ppo_carry_kernel<false>, grid, dim3(256), 0, s, h_row, c_row, reinterpret_cast<float4*>(carry),
                       count4);
  return hipGetLastError();
}

}  // namespace arl
