// The counter-based generator of the device-side batch preparation (batchprep.hip, ingest.hip): Philox4x32-10 keyed by the seed and counted by
// (element, sample id, stream), restated bit for bit by oracle/batchprep_oracle.py.  Streams in use: 0 grid mask, 1 grid-mask row shuffle, 2 token
// masking, 4 dropout, 5 DropPath, 6 horizontal flip.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

struct u4 { uint32_t x, y, z, w; };

// Philox4x32-10 (Salmon et al., SC'11; Random123 constants).  counter = (element, sample_lo, stream, sample_hi), key = seed.
__device__ __forceinline__ u4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return u4{c0, c1, c2, c3};
}
__device__ __forceinline__ u4 draws(uint64_t seed, uint64_t sample, uint32_t element, uint32_t stream) {
  return philox(element, (uint32_t)sample, stream, (uint32_t)(sample >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}
