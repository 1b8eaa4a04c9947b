// cloth_policy_mlp.hpp -- a small fully-connected policy network over the '1d' observation (no reference counterpart: the policy kind a
// learner brings), evaluated by ONE device function that the episode launch (episode_plan.inc.hpp, CLOTHHIP_POLICY_MLP) and the stand-alone
// kernel (k_policy_eval in cloth_policy_eval.hpp, behind clothhip_policy_eval) share, so the host loop and the launch compute the same bits.
// One network for all cloths, or one per env slot out of a population of blobs (MlpDesc::member; cloth_policy_population.hpp makes one).
//
//   L weight layers (1 <= L <= MLP_MAX_LAYERS), widths[0] = 3 P (the observation), widths[L] = 4 (the action), hidden widths in
//   [1, MLP_MAX_WIDTH]; ReLU after every layer but the last. Parameters: one float32 blob, for l = 0 .. L-1 W_l[out][in] row-major
//   (torch.nn.Linear.weight's layout), then b_l[out]. Input element 3 i + ax = (float)pos[ax][i], what k_write_obs emits, also on an
//   fp64 handle: the policy is float32 arithmetic in both precisions.
//
// THE ORDER OF THE ARITHMETIC (fixed: the result does not depend on the number of threads per cloth)
//   * one wave computes one neuron; neuron j goes to wave j mod n_waves -- WHICH wave computes a neuron has no influence on its value;
//   * lane l accumulates acc = fmaf(W[j][i], x[i], acc) over i = l, l + 64, l + 128, ... ascending, from acc = 0 (a lane without an
//     element keeps 0);
//   * the 64 lane sums are added by the xor butterfly, offsets 32, 16, 8, 4, 2, 1: acc += shfl_xor(acc, o) -- every lane ends with the same
//     value (IEEE addition is commutative, so both partners of a step compute the same sum);
//   * b[j] is added last; then, for a hidden layer, v < 0 ? 0 : v.
//   Hidden vectors ping-pong between two MLP_MAX_WIDTH-float arrays in LDS (layer l writes array l & 1) with a workgroup barrier after
//   every layer. No MFMA: it is one matrix-vector product per cloth, and the cloths of a launch are at different points in time.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clothhip {

constexpr int MLP_MAX_LAYERS = 4, MLP_MAX_WIDTH = 256, MLP_OUT = 4;
constexpr int MLP_SCRATCH_BYTES = 2 * MLP_MAX_WIDTH * 4;      // the two hidden arrays

struct MlpDesc {
    int32_t n_layers;                       // 0: no network
    int32_t widths[MLP_MAX_LAYERS + 1];     // widths[0 .. n_layers]
    int32_t _pad;
    const float *params;                    // device memory, owned by the handle
    // a population (clothhip_set_policy_population): env e runs the blob at params + member[e] * stride. nullptr: every env runs `params`.
    const int32_t *member;                  // device [E], values in [0, rows)
    int64_t stride;                         // floats between two blobs: n_params rounded up to 64, so every blob is 256-byte aligned
};

// floats in the blob of a network with these widths
__host__ __device__ inline size_t mlp_param_count(int n_layers, const int32_t *widths) {
    size_t n = 0;
    for (int l = 0; l < n_layers; l++) n += (size_t)widths[l + 1] * (size_t)widths[l] + (size_t)widths[l + 1];
    return n;
}
// where the action stands in `buf` after mlp_eval
__host__ __device__ constexpr int mlp_out_offset(int n_layers) { return ((n_layers - 1) & 1) ? MLP_MAX_WIDTH : 0; }

// The network on input in(i), i < widths[0], by the whole workgroup of nt threads (a multiple of 64; every thread calls, in uniform
// control flow). buf: 2 * MLP_MAX_WIDTH floats of LDS. On return -- behind a barrier -- buf[mlp_out_offset(L) + k], k < 4, is the action.
template <class In> __device__ __forceinline__ void mlp_eval(const MlpDesc &D, In in, float *buf, int tid, int nt) {
    const int lane = tid & 63, wave = tid >> 6, n_waves = nt >> 6;
    const int L = D.n_layers;
    const float *W = D.params;
    for (int l = 0; l < L; l++) {
        const int n_in = D.widths[l], n_out = D.widths[l + 1];
        const float *b = W + (size_t)n_out * n_in;
        float *dst = buf + ((l & 1) ? MLP_MAX_WIDTH : 0);
        const float *src = buf + ((l & 1) ? 0 : MLP_MAX_WIDTH);
        for (int j = wave; j < n_out; j += n_waves) {
            const float *wr = W + (size_t)j * n_in;
            float acc = 0.0f;
            if (l == 0) for (int i = lane; i < n_in; i += 64) acc = __builtin_fmaf(wr[i], in(i), acc);
            else for (int i = lane; i < n_in; i += 64) acc = __builtin_fmaf(wr[i], src[i], acc);
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            float v = acc + b[j];
            if (l + 1 < L) v = v < 0.0f ? 0.0f : v;
            if (lane == 0) dst[j] = v;
        }
        __syncthreads();
        W = b + n_out;
    }
}

// ... on particle records {x, y, z, w} in LDS (the episode launch's resident state), for env slot e: with a population the slot's own blob --
// only the base pointer moves, so a cloth under network g computes the bits a handle with g as its shared network computes. Not inlined:
// the plan's register allocation stays out of the stepper kernel's body, and nothing of it is live across the substep loop.
template <class Rec> __device__ __noinline__ void mlp_eval_records(const MlpDesc *D, int e, const Rec *cur, float *buf, int tid, int nt) {
    MlpDesc d = *D;
    if (d.member != nullptr) d.params += (size_t)d.member[e] * (size_t)d.stride;
    mlp_eval(d, [cur](int i) -> float { const int p = i / 3, ax = i - 3 * p; const Rec c = cur[p]; return (float)(ax == 0 ? c.x : (ax == 1 ? c.y : c.z)); },
             buf, tid, nt);
}

}  // namespace clothhip
