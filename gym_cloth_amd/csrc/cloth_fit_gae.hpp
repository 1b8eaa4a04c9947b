// cloth_fit_gae.hpp -- generalised advantage estimation over rows of the trainer's dataset (clothhip_fit_data_gae; no reference
// counterpart: the step between a fitted critic and an advantage-weighted policy fit). Included only by api_fit_rollout.hip, which has run the value
// network's forward over the range first: v [n] float32, row i of the range at v[i].
//
// A row's chain is r_0 = r, r_k+1 = next[r_k]; it stops after a row whose next is TERMINAL or whose successor is a LEAF (next == NONE).
// The host has checked every row of the range (clothhip_fit_data_set_transitions: a successor index is greater than the row's own; the
// call: it lies inside the range), so a chain is finite, acyclic and never leaves [first, first + n): no check on the device. A chain is
// one episode at most, about ten rows, so every thread walks its own (a scan over the range would be more launches than work).
//
// THE ORDER OF THE ARITHMETIC (fixed; the unit is built with -ffp-contract=off, every line below one double operation)
//   nv = (double)v[next], 0 when next is TERMINAL;  g = gamma nv;  t = (double)rew + g;  delta = t - (double)v
//   A = 0, coef = 1;  per row of the chain, ascending:  cd = coef delta;  A = A + cd;  coef = coef c      (c = gamma lambda from the host)
//   adv = (float)A;  ret = (float)(A + (double)v_r);   a leaf: adv = 0, ret = v
//   the weights: (float)((double)w_scale A), or normalised  d = A - mean;  q = d / (std + 1e-8);  (float)((double)w_scale q);  a leaf 0
//   mean = sum A / count, then std = sqrt(sum (A - mean)^2 / count), over the non-leaf rows: thread t of 256 takes rows t, t + 256, ...
//   of the range ascending, the 256 sums are added by a halving tree in LDS (k_fit_loss's order) -- one workgroup, no atomics.
// All stores are ordinary vector stores, one element per lane, contiguous over a wave.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clothhip {

constexpr int GAE_THREADS = 256;
constexpr int32_t GAE_NEXT_NONE = -2;      // = CLOTHHIP_FIT_NEXT_NONE (TERMINAL is the other negative value)

struct GaeArgs {
    const float *v;             // [n] the critic on the rows of the range
    const float *rew;           // the dataset's columns, indexed by dataset row
    const int32_t *next;
    float *ret, *w;             // ret is always written over the range; w only by k_gae_weights
    double *A;                  // [n] scratch: A of a non-leaf row, 0 of a leaf
    float *adv;                 // [n]
    double *stat;               // {mean, std} (k_gae_stats -> k_gae_weights)
    int64_t first, n;
    double gamma, c, w_scale;
    int32_t normalize;
};

// one thread per row of the range: A, adv, ret
__global__ __launch_bounds__(GAE_THREADS) void k_gae_rows(GaeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * GAE_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const int64_t r = a.first + i;
    const float vr = a.v[i];
    if (a.next[r] == GAE_NEXT_NONE) {
        a.A[i] = 0.0; a.adv[i] = 0.0f; a.ret[r] = vr;
        return;
    }
    double A = 0.0, coef = 1.0;
    for (int64_t cur = r;;) {
        const int32_t nx = a.next[cur];
        const bool terminal = nx < 0;
        const double nv = terminal ? 0.0 : (double)a.v[nx - a.first];
        const double g = a.gamma * nv;
        const double t = (double)a.rew[cur] + g;
        const double delta = t - (double)a.v[cur - a.first];
        const double cd = coef * delta;
        A = A + cd;
        coef = coef * a.c;
        if (terminal || a.next[nx] == GAE_NEXT_NONE) break;
        cur = nx;
    }
    const double target = A + (double)vr;
    a.A[i] = A; a.adv[i] = (float)A; a.ret[r] = (float)target;
}

// the sum over the non-leaf rows of f(A_i) and their count, in the house order; every thread returns the totals
template <typename F> __device__ __forceinline__ double gae_block_sum(const GaeArgs &a, F f, int32_t *count) {
    __shared__ double red[GAE_THREADS];
    __shared__ int32_t cnt[GAE_THREADS];
    const int tid = threadIdx.x;
    double s = 0.0;
    int32_t c = 0;
    for (int64_t i = tid; i < a.n; i += GAE_THREADS)
        if (a.next[a.first + i] != GAE_NEXT_NONE) { s = s + f(a.A[i]); c++; }
    red[tid] = s; cnt[tid] = c;
    __syncthreads();
    for (int o = GAE_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) { red[tid] = red[tid] + red[tid + o]; cnt[tid] += cnt[tid + o]; }
        __syncthreads();
    }
    const double total = red[0];
    *count = cnt[0];
    __syncthreads();      // (the arrays are written again by the next pass)
    return total;
}

// ONE workgroup: mean and population standard deviation of A over the non-leaf rows, two passes
__global__ __launch_bounds__(GAE_THREADS) void k_gae_stats(GaeArgs a) {
    int32_t count = 0;
    const double sum = gae_block_sum(a, [](double x) { return x; }, &count);
    const double mean = sum / (double)count;
    const double sq = gae_block_sum(a, [mean](double x) { const double d = x - mean; return d * d; }, &count);
    const double var = sq / (double)count;
    if (threadIdx.x == 0) { a.stat[0] = mean; a.stat[1] = __builtin_sqrt(var); }
}

// one thread per row of the range: the weight column
__global__ __launch_bounds__(GAE_THREADS) void k_gae_weights(GaeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * GAE_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const int64_t r = a.first + i;
    if (a.next[r] == GAE_NEXT_NONE) { a.w[r] = 0.0f; return; }
    double x = a.A[i];
    if (a.normalize) {
        const double d = x - a.stat[0];
        const double den = a.stat[1] + 1e-8;
        x = d / den;
    }
    const double wv = a.w_scale * x;
    a.w[r] = (float)wv;
}

}  // namespace clothhip
