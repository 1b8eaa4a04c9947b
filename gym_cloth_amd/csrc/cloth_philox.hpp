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

// ---- a standard normal: Box-Muller over Philox, made of plain double operations (clothhip.h: EXPLORATION NOISE ON THE DEVICE) -----------
// As exp_fixed (cloth_exp_fixed.hpp): no library log, sin or cos; every line ONE IEEE double operation under -ffp-contract=off (division and
// sqrt are correctly rounded on the device: cloth_fit_gae.hpp), so that numpy restates it bit for bit (references.normal_fixed_reference)
// and the host runs the very function (clothhip_selftest_normal_fixed). Every constant is a correctly rounded quotient of exact integers,
// pi / 2 or one of fdlibm's two halves of ln 2.

// log(u) for a positive normal u: u = m 2^k from the bits with m brought into [1/sqrt2, sqrt2); s = (m - 1) / (m + 1) (m - 1 is exact);
// log m = 2 s P(s^2), P = Horner over 1 / (2 j + 1), j = 13 .. 0 (s^2 <= 0.0295: the remainder is below 2e-23 of P); then + k ln2_lo,
// then + k ln2_hi (k ln2_hi is exact). Within 6.2 * 2^-53 relative of log.
__host__ __device__ inline double log_fixed(double u) {
    uint64_t bits;
    __builtin_memcpy(&bits, &u, 8);
    int k = (int)(bits >> 52) - 1023;
    const uint64_t mb = (bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
    double m;
    __builtin_memcpy(&m, &mb, 8);                            // in [1, 2)
    if (m >= 1.4142135623730951) { m = m * 0.5; k = k + 1; }
    const double f = m - 1.0, g = m + 1.0;
    const double s = f / g;
    const double z = s * s;
    const double c[14] = {1.0, 1.0 / 3.0, 1.0 / 5.0, 1.0 / 7.0, 1.0 / 9.0, 1.0 / 11.0, 1.0 / 13.0, 1.0 / 15.0, 1.0 / 17.0, 1.0 / 19.0,
                          1.0 / 21.0, 1.0 / 23.0, 1.0 / 25.0, 1.0 / 27.0};
    double p = c[13];
#pragma unroll
    for (int j = 12; j >= 0; j--) {
        const double pz = p * z;
        p = pz + c[j];
    }
    const double s2 = 2.0 * s;
    const double r = s2 * p;
    const double kd = (double)k;
    const double lo = kd * 1.90821492927058770002e-10, hi = kd * 6.93147180369123816490e-01;
    const double rl = r + lo;
    return rl + hi;
}

// (cos x, sin x) for |x| <= pi / 4: Horner in x^2 over the Taylor coefficients -+1 / i!, i up to 20 and 21 (the remainder is below 1e-23)
__host__ __device__ inline void sincos_fixed(double x, double *cs, double *sn) {
    const double x2 = x * x;
    const double ce[11] = {1.0, -1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0, -1.0 / 87178291200.0,
                           1.0 / 20922789888000.0, -1.0 / 6402373705728000.0, 1.0 / 2432902008176640000.0};
    const double so[11] = {1.0, -1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0,
                           -1.0 / 1307674368000.0, 1.0 / 355687428096000.0, -1.0 / 121645100408832000.0, 1.0 / 51090942171709440000.0};
    double c = ce[10], s = so[10];
#pragma unroll
    for (int j = 9; j >= 0; j--) {
        const double cx = c * x2, sx = s * x2;
        c = cx + ce[j];
        s = sx + so[j];
    }
    *cs = c;
    *sn = x * s;
}

// z[0..3], four independent standard normals of (seed, env, slot): pair j = 0, 1 from the Philox block at counter (slot lo, slot hi, env,
// 0x4E000000 + j) -- the tag keeps these counters apart from population_eps', whose fourth word is 0 -- as
//   u1 = (n1 + 0.5) 2^-52 in (0, 1), n1 = the top 52 bits of (r0, r1);   n2 = the top 52 bits of (r2, r3): quadrant q = n2 >> 50 and
//   t = ((n2 mod 2^50) + 0.5) 2^-50 - 0.5 in (-1/2, 1/2), both exact;   x = t (pi / 2);   rad = sqrt(-2 log_fixed(u1));
//   (c, s) = (cos, sin)(x) turned by q quarter turns with signs and swaps only;   z[2 j] = rad c, z[2 j + 1] = rad s.
// |z| reaches 8.57 (u1 = 2^-53). Within 4.1 rad 2^-52 absolute of the exact value on the same uniforms.
__host__ __device__ inline void normal_fixed(uint64_t seed, uint32_t env, uint64_t slot, double z[4]) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
        uint32_t r[4];
        philox4x32_10((uint32_t)slot, (uint32_t)(slot >> 32), env, 0x4E000000u + (uint32_t)j, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        const uint64_t n1 = ((uint64_t)r[0] << 20) | (uint64_t)(r[1] >> 12), n2 = ((uint64_t)r[2] << 20) | (uint64_t)(r[3] >> 12);
        const double a1 = (double)n1 + 0.5;
        const double u1 = a1 * 2.220446049250313e-16;                                   // 2^-52
        const int q = (int)(n2 >> 50);
        const double a2 = (double)(n2 & ((1ull << 50) - 1)) + 0.5;
        const double b2 = a2 * 8.881784197001252e-16;                                   // 2^-50
        const double t = b2 - 0.5;
        const double x = t * 1.5707963267948966;
        double c, s;
        sincos_fixed(x, &c, &s);
        const double qc = q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s)), qs = q == 0 ? s : (q == 1 ? c : (q == 2 ? -s : -c));
        const double l = log_fixed(u1);
        const double w = -2.0 * l;
        const double rad = __builtin_sqrt(w);
        z[2 * j] = rad * qc;
        z[2 * j + 1] = rad * qs;
    }
}

}  // namespace clothhip
