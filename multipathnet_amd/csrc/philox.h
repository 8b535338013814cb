// philox.h — the counter-based generator behind every random choice of a training run: the dropout masks (train.hip, DESIGN.md section
// 13.6) and the ROI sampler's draws (sampler.hip, section 13.11).  One definition: the two streams differ in their counters alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mpn {

// Philox4x32-10 (Salmon et al., SC'11; Random123's known answers): ten rounds of two 32 x 32 -> 64 multiplies, the key bumped between rounds
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace mpn
