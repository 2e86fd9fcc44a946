// Philox4x32-10, the counter-based generator of the kernels that draw noise (modulation.hip: OGM-GE, fbank.hip: --cav_augnois).
// Word j of philox4x32(counter, stream_id, seed) depends on nothing else, so a draw does not depend on the launch geometry.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

static __device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (uint32_t)p1;
  c[3] = (uint32_t)p0;
  c[0] = n0;
  c[2] = n2;
}
static __device__ __forceinline__ void philox4x32(uint64_t counter, uint64_t stream_id, uint64_t seed, uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}
