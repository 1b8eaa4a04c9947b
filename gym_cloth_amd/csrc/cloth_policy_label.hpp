// cloth_policy_label.hpp -- clothhip_policy_label's stand-alone kernel: the two analytic experts (examples/analytic.py's oracle corner and
// highest point) on stored '1d' observations or on the handle's present state, with the arithmetic the episode launch performs
// (episode_plan.inc.hpp: oracle_corner / highest_point) from the point where a position has become a double. api_policy.hip alone
// includes this. At global scope, as k_policy_eval is.
// One 64-lane wave per row, rows_per_block of them in a workgroup. Oracle corner: four particles' x and y are all it reads. Highest point:
// the row's heights are staged in LDS by one coalesced pass over the row (a '1d' row is read whole, lane after lane, and every third value
// kept; the state's z plane is contiguous), then k + 1 rounds of a wave arg-max over (z, -index) run on LDS.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/clothhip.h"

struct PolicyLabelArgs {
    const float *rows;       // [n][3P] '1d' observations, or nullptr: the SoA state below
    const void *pos;         // [n][3][Ppad], handle precision
    const int32_t *side;     // [n] how the row's cloth was built (FusedArgs::policy_arg row 0), or nullptr: all 0
    const int32_t *choice;   // [n] HIGHEST_POINT: which of the highest points
    double *out;             // [n][4]
    int64_t n;
    int32_t P, Ppad, N, expert, clip_act_space, rows_per_block;
    double grid_dx, grid_dy;
};

// Z: what the staged heights are held as -- float for '1d' rows, the handle's precision for the state (the launch compares heights in that precision)
template <typename T, typename Z> __global__ __launch_bounds__(256) void k_policy_label(PolicyLabelArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char label_smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t r_ = (int64_t)blockIdx.x * A.rows_per_block + w;
    const bool live = r_ < A.n;                 // (a dead wave still meets the barrier below)
    const size_t r = live ? (size_t)r_ : 0;
    const int P = A.P;
    const float *row = A.rows != nullptr ? A.rows + r * 3 * (size_t)P : nullptr;
    const T *p = (const T *)A.pos + r * 3 * (size_t)A.Ppad;
    const int Ppad = A.Ppad;
    auto xy = [&](int i, double &x, double &y) {
        if (row != nullptr) { x = (double)row[3 * i]; y = (double)row[3 * i + 1]; }
        else { x = (double)p[i]; y = (double)p[Ppad + i]; }
    };
    const int swap = A.side != nullptr ? A.side[r] : 0;
    const bool clip = A.clip_act_space != 0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (A.expert == CLOTHHIP_POLICY_ORACLE_CORNER) {
        // examples/analytic.py:105-155: the inset corner farthest from its plane corner; ur, lr, ll, ul, the first maximum wins
        const bool sw = swap == 1;
        double best = -1.0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int ci = c == 0 ? (sw ? 48 : 598) : (c == 1 ? (sw ? 26 : 576) : (c == 2 ? (sw ? 576 : 26) : (sw ? 598 : 48)));
            const double tgx = c < 2 ? 1.0 : 0.0, tgy = (c == 0 || c == 3) ? 1.0 : 0.0;
            double x, y;
            xy(ci, x, y);
            const double cx = (x - 0.5) * 2.0, cy = (y - 0.5) * 2.0;
            double dx = tgx - x, dy = tgy - y;
            const double dist = sqrt((x - tgx) * (x - tgx) + (y - tgy) * (y - tgy));
            dx = dx * 0.90; dy = dy * 0.90;
            if (dist > best) { best = dist; a0 = clip ? cx : x; a1 = clip ? cy : y; a2 = dx; a3 = dy; }
        }
    } else {
        // examples/analytic.py:792-808: the k-th highest z in stable index order, pulled to where that point sits on the flat cloth
        Z *zs = reinterpret_cast<Z *>(label_smem) + (size_t)w * P;
        if (row != nullptr) { for (int j = lane; j < 3 * P; j += 64) { const float v = row[j]; const int i = j / 3; if (j - 3 * i == 2) zs[i] = (Z)v; } }
        else { for (int i = lane; i < P; i += 64) zs[i] = (Z)p[2 * Ppad + i]; }
        __syncthreads();
        int kc = A.choice[r];
        kc = kc < 0 ? 0 : (kc > P - 1 ? P - 1 : kc);
        Z lastz = (Z)0; int lasti = -1;
        const auto better = [](Z z1, int i1, Z z0, int i0) { return i1 != 0x7fffffff && (i0 == 0x7fffffff || z1 > z0 || (z1 == z0 && i1 < i0)); };
        for (int round = 0; round <= kc; round++) {
            Z bz = (Z)0; int bi = 0x7fffffff;
            for (int i = lane; i < P; i += 64) {
                const Z z = zs[i];
                const bool ok = lasti < 0 || z < lastz || (z == lastz && i > lasti);
                if (ok && better(z, i, bz, bi)) { bz = z; bi = i; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const Z oz = __shfl_xor(bz, o); const int oi = __shfl_xor(bi, o);
                if (better(oz, oi, bz, bi)) { bz = oz; bi = oi; }
            }
            lastz = bz; lasti = bi;      // every lane holds the wave's best after the xor butterfly
        }
        lasti = lasti == 0x7fffffff ? 0 : lasti;      // (only a row of NaN heights: nothing compares as `better`; the launch has no such state)
        const int pr = lasti / A.N, pc_ = lasti - pr * A.N;
        double x, y;
        xy(lasti, x, y);
        double tgx, tgy;
        if (swap == 0) { tgx = A.grid_dx * pr; tgy = A.grid_dy * pc_; }
        else { tgx = swap == 2 ? A.grid_dy * pr : 1.0 - A.grid_dy * pr; tgy = A.grid_dx * pc_; }
        const double cx = (x - 0.5) * 2.0, cy = (y - 0.5) * 2.0;
        const double dx = (tgx - x) * 0.90, dy = (tgy - y) * 0.90;
        a0 = clip ? cx : x; a1 = clip ? cy : y; a2 = dx; a3 = dy;
    }
    if (live && lane == 0) { double *o = A.out + r * 4; o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3; }
}
