// mi_philox.h - the counter-based random words of the cheap kernel units: render_stages.hip (the stratified jitter of
// sample_coarse) and occupancy.hip (the draws of a live grid's density update).  No MFMA kernel unit includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {

// Philox4x32-10 (Salmon et al. 2011), counter = (ray_lo, ray_hi, sample>>2, 0), key = seed.
__device__ __forceinline__ uint32_t philox_u32(uint64_t seed, uint64_t ray, uint32_t sample) {
    uint32_t c0 = (uint32_t)ray, c1 = (uint32_t)(ray >> 32), c2 = sample >> 2, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint32_t s = sample & 3;
    return s == 0 ? c0 : (s == 1 ? c1 : (s == 2 ? c2 : c3));
}

}  // namespace mi
