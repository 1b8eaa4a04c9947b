// cloth_plan.hpp -- the two kernels of the cross-entropy planner over forked cloths (no reference counterpart; include/clothhip.h states the
// definition, clothhip_plan_cem has the loop): k_plan_sample turns the sampling distribution of every env into the action table an episode
// launch on the scratch handle reads, k_plan_refit turns that launch's records (or a caller's score table) back into a distribution.
// All arithmetic is float64 -- action tables are doubles on both precisions --, every value has ONE order of operations and the unit is built
// without contraction, so numpy restates both kernels bit for bit (gym_cloth_amd/policies.py: plan_sample_reference, plan_refit_reference).
//
// SAMPLE   x[h][e K + k][a] = clip(fl(mean[e][h][a] + fl(std[e][h][a] * (double)eps)), act_low[a], act_high[a]),
//          eps = population_eps(seed, iter, ((e K + k) H + h) 4 + a)  (cloth_philox.hpp; cloth_policy_population.hpp defines it: Philox4x32-10, counter-based);
//          candidate k = 0 is clip(mean[e][h][a]) itself. clip(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v).
//          One thread per table element, in the table's order (consecutive threads write consecutive doubles).
// SCORE    of branch (e, k) from its record column rec[h][e K + k], h < H: its executed slots are those with ran != 0;
//          score = coverage of the last executed slot, minus penalty when any executed slot has oob or tear; -infinity without an executed slot.
// ELITES   rank_k = #{j : s_j > s_k or (s_j == s_k and j < k)} -- a counting rank: (score descending, k ascending) is one total order --,
//          candidate k is an elite when rank_k < M, the top candidate is the one of rank 0.
// REFIT    per (h, a) ONE thread loops over the elites in ascending k: mu = (sum x_k) / M, var = (sum (x_k - mu)^2) / M, sd = sqrt(var);
//          mean <- fl(fl(alpha mu) + fl(beta mean)), std <- max(min_std[a], fl(fl(alpha sd) + fl(beta std))); beta = 1 - alpha comes from the host.
// BEST     the top candidate's rows replace best_actions[e] / best_score[e] when `first` is set or its score is strictly greater.
// An env with done[e] != 0 is not planned: its mean / std stay, its best_actions / best_score become NaN, no elites, top index -1.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clothhip.h"
#include "cloth_philox.hpp"

namespace clothhip {

constexpr int PLAN_THREADS = 256;
constexpr int PLAN_MAX_H = 8;                    // horizon, in actions: 4 H <= 32 refit threads
constexpr int PLAN_MAX_K = 1024;                 // candidates per env: the scores and the elite flags of one env live in LDS

__host__ __device__ inline double plan_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct PlanSampleArgs {
    const double *mean, *std;  // [E][H][4]
    double *x;                 // [H][E K][4]
    double lo[4], hi[4];
    uint64_t seed;
    uint32_t iter;             // iter0 + it
    int32_t E, K, H;
};

__global__ __launch_bounds__(PLAN_THREADS) void k_plan_sample(PlanSampleArgs A) {
    const int64_t EK = (int64_t)A.E * A.K, n = EK * A.H * 4;
    const int64_t g = (int64_t)blockIdx.x * PLAN_THREADS + threadIdx.x;
    if (g >= n) return;
    const int a = (int)(g & 3);
    const int64_t slot = (g >> 2) % EK, h = (g >> 2) / EK;
    const int64_t e = slot / A.K, k = slot % A.K;
    const int64_t m = (e * A.H + h) * 4 + a;
    double v = A.mean[m];
    if (k != 0) {
        const double eps = (double)population_eps(A.seed, A.iter, (uint64_t)((slot * A.H + h) * 4 + a));
        const double step = A.std[m] * eps;
        v = v + step;
    }
    A.x[g] = plan_clip(v, A.lo[a], A.hi[a]);
}

struct PlanRefitArgs {
    const double *x;                 // [H][E K][4] the clipped table the launch read
    const ClothStepRecord *rec;      // [H][E K] the launch's records, or nullptr: the scores are given
    double *scores;                  // [E][K]: written from the records, else read
    const uint8_t *done;             // [E] or nullptr (= every env is planned)
    double *mean, *std;              // [E][H][4] in/out
    double *best_actions;            // [E][H][4] or nullptr
    double *best_score;              // [E] or nullptr
    uint8_t *elite;                  // [E][K] or nullptr
    int32_t *top;                    // [E] or nullptr
    double alpha, beta, penalty;
    double min_std[4];
    int32_t E, K, H, M, first;
};

// one workgroup per env
__global__ __launch_bounds__(PLAN_THREADS) void k_plan_refit(PlanRefitArgs A) {
    __shared__ double s_score[PLAN_MAX_K];
    __shared__ uint8_t s_elite[PLAN_MAX_K];
    __shared__ int s_top;
    const int e = blockIdx.x, t = threadIdx.x;
    const int64_t EK = (int64_t)A.E * A.K;
    const bool planned = A.done == nullptr || A.done[e] == 0;
    for (int k = t; k < A.K; k += PLAN_THREADS) {
        const int64_t slot = (int64_t)e * A.K + k;
        double s;
        if (A.rec != nullptr) {
            int last = -1;
            bool bad = false;
            for (int h = 0; h < A.H; h++) {
                const ClothStepRecord &r = A.rec[(int64_t)h * EK + slot];
                if (r.ran != 0) { last = h; bad = bad || r.oob != 0 || r.tear != 0; }
            }
            if (last < 0) s = -__builtin_huge_val();
            else {
                const double cov = A.rec[(int64_t)last * EK + slot].coverage;
                s = bad ? cov - A.penalty : cov;
            }
            A.scores[slot] = s;
        } else s = A.scores[slot];
        s_score[k] = s;
    }
    __syncthreads();
    if (!planned) {
        if (A.elite != nullptr) for (int k = t; k < A.K; k += PLAN_THREADS) A.elite[(int64_t)e * A.K + k] = 0;
        if (A.best_actions != nullptr && t < A.H * 4) A.best_actions[(int64_t)e * A.H * 4 + t] = __builtin_nan("");
        if (t == 0) {
            if (A.best_score != nullptr) A.best_score[e] = __builtin_nan("");
            if (A.top != nullptr) A.top[e] = -1;
        }
        return;
    }
    for (int k = t; k < A.K; k += PLAN_THREADS) {
        const double sk = s_score[k];
        int rank = 0;
        for (int j = 0; j < A.K; j++) {
            const double sj = s_score[j];
            rank += (sj > sk || (sj == sk && j < k)) ? 1 : 0;
        }
        const uint8_t el = rank < A.M ? 1 : 0;
        s_elite[k] = el;
        if (A.elite != nullptr) A.elite[(int64_t)e * A.K + k] = el;
        if (rank == 0) s_top = k;
    }
    const double old_best = (A.best_score != nullptr && !A.first) ? A.best_score[e] : 0.0;
    __syncthreads();
    const int top = s_top;
    const bool better = A.first || s_score[top] > old_best;
    if (t < A.H * 4) {
        const int h = t >> 2, a = t & 3;
        const double *col = A.x + ((int64_t)h * EK + (int64_t)e * A.K) * 4 + a;      // x[h][e K + k][a] = col[4 k]
        const double Md = (double)A.M;
        double sum = 0.0;
        for (int k = 0; k < A.K; k++) if (s_elite[k]) sum = sum + col[4 * k];
        const double mu = sum / Md;
        double sq = 0.0;
        for (int k = 0; k < A.K; k++) if (s_elite[k]) { const double d = col[4 * k] - mu; const double d2 = d * d; sq = sq + d2; }
        const double var = sq / Md;
        const double sd = __builtin_sqrt(var);
        const int64_t m = ((int64_t)e * A.H + h) * 4 + a;
        const double am = A.alpha * mu, bm = A.beta * A.mean[m];
        A.mean[m] = am + bm;
        const double as = A.alpha * sd, bs = A.beta * A.std[m];
        const double ns = as + bs;
        A.std[m] = ns < A.min_std[a] ? A.min_std[a] : ns;
        if (better && A.best_actions != nullptr) A.best_actions[m] = col[4 * top];
    }
    if (t == 0) {
        if (better && A.best_score != nullptr) A.best_score[e] = s_score[top];
        if (A.top != nullptr) A.top[e] = top;
    }
}

}  // namespace clothhip
