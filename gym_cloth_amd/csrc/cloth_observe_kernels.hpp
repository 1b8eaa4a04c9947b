// cloth_observe_kernels.hpp -- observation and metrics read-back of a handle's state (api_observe.hip, which alone includes this).
#pragma once

#include "cloth_common.hpp"
#include "cloth_metrics.hpp"

namespace clothhip {

// '1d' observation (cloth_env.py:196-200) as float32 [E][3P], from SoA device state
template <typename T> __global__ void k_write_obs(const T *pos, float *out, int P, int Ppad) {
    const int e = blockIdx.x;
    const T *p = pos + (size_t)e * 3 * Ppad;
    float *o = out + (size_t)e * 3 * P;
    for (int t = threadIdx.x; t < 3 * P; t += blockDim.x) {
        const int i = t / 3, ax = t - 3 * i;
        o[t] = (float)p[ax * Ppad + i];
    }
}

// ---- per-env metrics kernel: one 256-thread workgroup per env over the SoA state in HBM (metrics_block above)
template <typename T>
__global__ __launch_bounds__(256) void k_metrics(const T *pos, int P, int Ppad, int NS, int NH, double *cov, double *vinv, uint8_t *oob,
                                                 int32_t *hcnt, double half_thick) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = blockIdx.x;
    const T *px = pos + (size_t)e * 3 * Ppad, *py = px + Ppad, *pz = py + Ppad;
    auto src = [&](int i, double &x, double &y, double &z) { x = (double)px[i]; y = (double)py[i]; z = (double)pz[i]; };
    double out[4];
    metrics_block<256, T>(src, P, NS, NH, smem, (int)threadIdx.x, half_thick, out);
    if (threadIdx.x == 0) {
        cov[e] = out[0]; vinv[e] = out[1]; oob[e] = out[2] != 0.0 ? 1 : 0;
        if (hcnt) hcnt[e] = (int32_t)out[3];
    }
}

}  // namespace clothhip
