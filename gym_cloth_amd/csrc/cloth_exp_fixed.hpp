// cloth_exp_fixed.hpp -- the exponential of the trainer's PPO losses (cloth_policy_fit.hpp) and of the exploration noise's sigma
// (cloth_policy_noise.hpp): ONE definition, so that the sigma that acts and the sigma the surrogate differentiates are the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clothhip {

// exp(x) for x clamped to [-40, 40], made of plain double operations, each ONE rounding (no library exp, no contraction), so that numpy
// restates it bit for bit (policies.exp_fixed_reference) and the host runs the very function (clothhip_selftest_exp_fixed):
//   k = rint(x log2e);  r = (x - k ln2_hi) - k ln2_lo  (fdlibm's two constants: k ln2_hi is exact for |k| <= 58);  p = Horner over the
//   Taylor coefficients 1 / i!, i = 13 .. 0 (|r| <= 0.3466: the remainder is below 4e-18 of p);  p 2^k, the power built from its bits.
// Within 2.2e-16 relative of exp over [-40, 40]; exp_fixed(0) == 1.0 exactly (k = 0, r = 0, p = 1). x must not be NaN.
__host__ __device__ inline double exp_fixed(double x) {
    x = x < -40.0 ? -40.0 : x;
    x = x > 40.0 ? 40.0 : x;
    const double k = __builtin_rint(x * 1.44269504088896338700e+00);
    const double hi = k * 6.93147180369123816490e-01, lo = k * 1.90821492927058770002e-10;
    const double xh = x - hi, r = xh - lo;
    const double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
                          1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    double p = c[13];
#pragma unroll
    for (int i = 12; i >= 0; i--) {
        const double pr = p * r;
        p = pr + c[i];
    }
    const uint64_t bits = (uint64_t)(1023 + (int)k) << 52;      // 2^k, k in [-58, 58]
    double scale;
    __builtin_memcpy(&scale, &bits, 8);
    return p * scale;
}

}  // namespace clothhip
