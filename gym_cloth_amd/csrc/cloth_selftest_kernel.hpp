// cloth_selftest_kernel.hpp -- clothhip_selftest_arith's kernel (api_selftest.hip, which alone includes this).
#pragma once

namespace clothhip {

__global__ void k_selftest(int op, const double *a, const double *b, double *out, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = a[i], y = b ? b[i] : 0.0, r;
    if (op == 0) r = x / y;
    else if (op == 1) r = sqrt(x);
    else if (op == 2) r = x * y + y;
    else r = floor(x / y);
    out[i] = r;
}

}  // namespace clothhip
