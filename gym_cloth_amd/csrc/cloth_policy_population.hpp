// cloth_policy_population.hpp -- a population of policy networks made ON THE DEVICE (no reference counterpart: what a gradient-free learner --
// evolution strategies, CEM over parameters -- needs each generation): G perturbed copies theta +- sigma eps_k of one blob
// (k_population_perturb, behind clothhip_policy_population_perturb) and the weighted sum of the same perturbations, sum_k w_k eps_k
// (k_population_combine, behind clothhip_policy_population_combine). Neither draws on the host nor moves a blob over PCIe: eps is a function
// of (seed, k, i), made again wherever it is needed.
//
// THE NOISE (one exact definition; integers and one float multiplication, no transcendental function -- numpy restates it bit for bit)
//   Philox4x32-10, standard constants (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85);
//   key = (seed & 0xffffffff, seed >> 32); counter = (i & 0xffffffff, i >> 32, k, 0), i the index into the blob (weights and biases alike),
//   k the perturbation index. From the four output words
//       S = (r0 >> 8) + (r1 >> 8) + (r2 >> 8) + (r3 >> 8),   D = (int32)S - (2^25 - 2),   eps_k[i] = (float)D * c,
//   c = (float)(sqrt(3.0) / 2^24) = 1.0323827e-07 (the bits 0x33DDB3D7 below).
//   eps has zero mean, unit variance and is exactly symmetric (D and -D are equally likely and give eps and -eps). It is the centred
//   SUM OF FOUR UNIFORMS, NOT A GAUSSIAN: |eps| <= 3.47, kurtosis 2.7. Evolution strategies need the first two moments and the symmetry;
//   exactness is worth more here than the tail.
//
// THE ROWS: row stride = n_params rounded up to 64 floats (every row 256-byte aligned), pad = zeros. With CLOTHHIP_POP_ANTITHETIC rows 2k and
//   2k + 1 are theta + sigma eps_k and theta - sigma eps_k, else row g is theta + sigma eps_g; the last row (G) is theta itself.
//   A weight is (float)((double)theta[i] + (double)(+-sigma) * (double)eps): the product of two floats is exact in a double, so there is
//   one rounded addition and one rounding to float, whatever the compiler contracts.
//   One thread makes four consecutive parameters of one perturbation (both rows of an antithetic pair: eps is made once) and stores them
//   as one 16-byte vector per row; the four that straddle n_params, and the pad, go scalar.
// THE SUM: out[i] = (float) sum_{k ascending} (double)coef[k] * (double)eps_k[i], one thread per parameter, the loop over k in order -- a
//   sequential float64 loop on the host gives the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloth_philox.hpp"      // philox4x32_10 and population_eps: THE NOISE above, shared with the planner (cloth_plan.hpp)

namespace clothhip {

constexpr int POP_MAX_G = 65534;                 // perturbations of one call (the launch's second grid dimension holds G + 1 at most)
constexpr int POP_ROW_ALIGN = 64;                // floats
constexpr int POP_THREADS = 256;

__host__ __device__ inline size_t population_stride(size_t n_params) { return (n_params + POP_ROW_ALIGN - 1) / POP_ROW_ALIGN * POP_ROW_ALIGN; }

__host__ __device__ inline float population_weight(float theta, float signed_sigma, float eps) {
    return (float)((double)theta + (double)signed_sigma * (double)eps);
}

struct PopulationPerturbArgs {
    const float *center;       // [n_params] theta; 16-byte aligned
    float *rows;               // [G + 1][stride]
    uint64_t n_params, stride, seed;
    int32_t K;                 // perturbations: G / 2 with antithetic, else G
    int32_t antithetic;
    float sigma;
};

// grid (ceil(stride / 4 / POP_THREADS), K + 1): blockIdx.y = k < K makes perturbation k's row (its two rows), blockIdx.y = K the row of theta
__global__ __launch_bounds__(POP_THREADS) void k_population_perturb(PopulationPerturbArgs A) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * POP_THREADS + threadIdx.x) * 4;
    if (i0 >= A.stride) return;
    const uint32_t k = blockIdx.y;
    const bool copy = k == (uint32_t)A.K;
    const uint64_t G = A.antithetic ? 2 * (uint64_t)A.K : (uint64_t)A.K;
    float *plus = A.rows + (copy ? G : (A.antithetic ? 2 * (uint64_t)k : (uint64_t)k)) * A.stride + i0;
    float *minus = (!copy && A.antithetic) ? plus + A.stride : nullptr;
    if (i0 + 4 <= A.n_params) {
        const float4 th = *reinterpret_cast<const float4 *>(A.center + i0);
        if (copy) { *reinterpret_cast<float4 *>(plus) = th; return; }
        const float e0 = population_eps(A.seed, k, i0), e1 = population_eps(A.seed, k, i0 + 1), e2 = population_eps(A.seed, k, i0 + 2),
                    e3 = population_eps(A.seed, k, i0 + 3);
        *reinterpret_cast<float4 *>(plus) = make_float4(population_weight(th.x, A.sigma, e0), population_weight(th.y, A.sigma, e1),
                                                        population_weight(th.z, A.sigma, e2), population_weight(th.w, A.sigma, e3));
        if (minus != nullptr)
            *reinterpret_cast<float4 *>(minus) = make_float4(population_weight(th.x, -A.sigma, e0), population_weight(th.y, -A.sigma, e1),
                                                             population_weight(th.z, -A.sigma, e2), population_weight(th.w, -A.sigma, e3));
        return;
    }
    for (int j = 0; j < 4; j++) {          // the tail of the blob and the pad (i0 + 4 <= stride: the stride is a multiple of 4)
        const uint64_t i = i0 + j;
        const bool in = i < A.n_params;
        const float th = in ? A.center[i] : 0.0f;
        const float e = (in && !copy) ? population_eps(A.seed, k, i) : 0.0f;
        plus[j] = (in && !copy) ? population_weight(th, A.sigma, e) : th;
        if (minus != nullptr) minus[j] = in ? population_weight(th, -A.sigma, e) : 0.0f;
    }
}

struct PopulationCombineArgs {
    const float *coef;         // [K]
    float *out;                // [n_params]
    uint64_t n_params, seed;
    int32_t K;
};

__global__ __launch_bounds__(POP_THREADS) void k_population_combine(PopulationCombineArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * POP_THREADS + threadIdx.x;
    if (i >= A.n_params) return;
    double acc = 0.0;
    for (int32_t k = 0; k < A.K; k++) acc += (double)A.coef[k] * (double)population_eps(A.seed, (uint32_t)k, i);
    A.out[i] = (float)acc;
}

}  // namespace clothhip
