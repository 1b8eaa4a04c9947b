// cloth_philox.hpp -- the counter-based variate shared by the policy population (cloth_policy_population.hpp, which states the definition:
// THE NOISE) and the cross-entropy planner (cloth_plan.hpp): Philox4x32-10 and eps = the centred sum of four 24-bit uniforms, times
// (float)(sqrt(3) / 2^24). Integers and one float multiplication; numpy restates it bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clothhip {

__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4]) {
    for (int round = 0; round < 10; round++) {
        if (round) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// eps_k[i] for this seed (cloth_policy_population.hpp: THE NOISE)
__host__ __device__ inline float population_eps(uint64_t seed, uint32_t k, uint64_t i) {
    uint32_t r[4];
    philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), k, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const uint32_t S = (r[0] >> 8) + (r[1] >> 8) + (r[2] >> 8) + (r[3] >> 8);
    const int32_t D = (int32_t)S - ((1 << 25) - 2);
    union { uint32_t u; float f; } c = {0x33DDB3D7u};      // (float)(sqrt(3.0) / 2^24)
    return (float)D * c.f;
}

}  // namespace clothhip
