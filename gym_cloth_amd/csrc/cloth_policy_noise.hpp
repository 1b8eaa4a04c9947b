// cloth_policy_noise.hpp -- the exploration noise of the learned policy, made where the episode launch reads it (clothhip.h: EXPLORATION
// NOISE ON THE DEVICE; included by api_policy.hip alone). One thread per (t, e) of the table double [T][E][4]: the slot number
// slot_base[e] + t (slot_base NULL: t), normal_fixed(seed, e, slot) (cloth_philox.hpp), then noise[t][e][k] = sigma_k z_k, ONE double
// multiplication each. sigma_k is sigma[(rows == 1 ? 0 : e) 4 + k] of an uploaded table, or with log_sigma != NULL
// exp_fixed((double)log_sigma[k]) of the handle's float32 head read where it lies -- the bits the PPO surrogate forms. The four doubles
// leave as two 16-byte stores, so a wave writes 2 KB of contiguous memory. Workgroups of 256 over a flat grid with a tail guard; no LDS,
// no atomics, ordinary vector stores only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloth_exp_fixed.hpp"
#include "cloth_philox.hpp"

namespace clothhip {

constexpr int NOISE_THREADS = 256;

struct PolicyNoiseArgs {
    double *out;                  // [T][E][4], 16-byte aligned
    const int64_t *slot_base;     // [E] or NULL
    const double *sigma;          // [sigma_rows][4], or NULL with log_sigma
    const float *log_sigma;       // [4] or NULL
    uint64_t seed;
    int64_t n;                    // T * E
    int32_t E, sigma_rows;
};

__global__ __launch_bounds__(NOISE_THREADS) void k_policy_noise_fill(PolicyNoiseArgs a) {
    const int64_t i = (int64_t)blockIdx.x * NOISE_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const int64_t t = i / a.E;
    const int32_t e = (int32_t)(i - t * a.E);
    const uint64_t slot = (uint64_t)((a.slot_base ? a.slot_base[e] : 0) + t);
    double sg[4];
    if (a.log_sigma) {
#pragma unroll
        for (int k = 0; k < 4; k++) sg[k] = exp_fixed((double)a.log_sigma[k]);
    } else {
        const double *row = a.sigma + (a.sigma_rows == 1 ? 0 : (size_t)e * 4);
#pragma unroll
        for (int k = 0; k < 4; k++) sg[k] = row[k];
    }
    double z[4];
    normal_fixed(a.seed, (uint32_t)e, slot, z);
    double2 *o = (double2 *)(a.out + (size_t)i * 4);
    o[0] = make_double2(sg[0] * z[0], sg[1] * z[1]);
    o[1] = make_double2(sg[2] * z[2], sg[3] * z[3]);
}

}  // namespace clothhip
