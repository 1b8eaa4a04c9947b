// cloth_policy_eval.hpp -- clothhip_policy_eval's stand-alone kernel over mlp_eval, one workgroup per row (api_policy.hip, which alone includes
// this). At global scope, as the kernel's name has always been: profiles and traces list it as k_policy_eval<T>.
#pragma once

#include "cloth_policy_mlp.hpp"

struct PolicyEvalArgs {
    clothhip::MlpDesc mlp;
    const int32_t *members;  // [n]: row r runs the blob at mlp.params + members[r] * mlp.stride; nullptr: every row runs mlp.params
    const float *rows;       // [n][3P] '1d' observations, or nullptr: the SoA state below
    const void *pos;         // [n][3][Ppad], handle precision
    int32_t P, Ppad;
    double *out;             // [n][4]
};
template <typename T> __global__ __launch_bounds__(256) void k_policy_eval(PolicyEvalArgs A) {
    __shared__ float buf[2 * clothhip::MLP_MAX_WIDTH];
    const size_t r = blockIdx.x;
    const int tid = threadIdx.x;
    clothhip::MlpDesc d = A.mlp;
    if (A.members != nullptr) d.params += (size_t)A.members[r] * (size_t)d.stride;
    if (A.rows != nullptr) {
        const float *x = A.rows + r * 3 * (size_t)A.P;
        mlp_eval(d, [x](int i) -> float { return x[i]; }, buf, tid, 256);
    } else {
        const T *p = (const T *)A.pos + r * 3 * (size_t)A.Ppad;
        const int Ppad = A.Ppad;
        mlp_eval(d, [p, Ppad](int i) -> float { const int q = i / 3, ax = i - 3 * q; return (float)p[ax * Ppad + q]; }, buf, tid, 256);
    }
    if (tid < clothhip::MLP_OUT) A.out[r * clothhip::MLP_OUT + tid] = (double)buf[clothhip::mlp_out_offset(A.mlp.n_layers) + tid];
}
