// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator of every
// draw the library makes on the device (sampler.hip: sample_seeded_kernel; train_step.hip: dropout_mask_kernel).  One statement
// of it: tests/test_oracle_golden.py::test_philox_known_answer holds the oracle's copy to the published vectors.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace fx3d {

// c: the 128-bit counter, replaced by the four output words; (k0, k1): the key
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

}  // namespace fx3d
