// cloth_fit_ddpg.hpp -- the five kernels DDPG adds to the trainer of cloth_policy_fit.hpp (clothhip.h: DDPG ON THE DEVICE has the
// arithmetic operation by operation; no reference counterpart): the critic's input rows, the TD loss, the gate of the deterministic
// policy gradient, that gate with a behaviour-cloning term (DDPG from demonstrations) and the soft update of the targets. Everything between them -- the forwards of four networks, the critic's backward,
// its input-gradient chain, the policy's backward, the optimizers -- is k_fit_gemm, k_fit_reduce, k_fit_colsum, k_fit_adam and k_fit_sgd,
// launched by api_fit.hip (for api_fit_ddpg.hip, which owns the order) on the critic's own scratch tables. Included only by api_fit.hip, behind cloth_policy_fit.hpp.
//
// The house rules hold: no floating-point atomics; a reduction has ONE order -- thread t of 256 takes rows t, t + 256, ... ascending, then
// fit_tree_sums --; every operation is one rounding (the unit is built with -ffp-contract=off); ordinary vector stores only. All are
// launched for the ONE shared network: there is no member index.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloth_policy_fit.hpp"

namespace clothhip {

constexpr int FIT_DDPG_THREADS = 256, FIT_CONCAT_DEPTH = 4;
constexpr int FIT_TD_STATS = 3, FIT_DPG_STATS = 3;      // = CLOTHHIP_DDPG_STATS / 2 each
constexpr int FIT_DPG_BC_STATS = 6;                     // = CLOTHHIP_DPG_BC_STATS
constexpr uint32_t FIT_NO_EXPERT = 0x7fc00000u;         // the expert column's fill: a row whose component 0 is a NaN has no expert action
constexpr int32_t FIT_NEXT_TERMINAL = -1;               // = CLOTHHIP_FIT_NEXT_TERMINAL

// X[r][0 .. L) = obs[rows[r]][.], X[r][L .. L + 4) = clamp(a_r, -bound, +bound): the critic's input rows of a minibatch, L = 3P.
// LABEL: a_r is the label column at rows[r] (the action the row executed); else row r of `act`, a scratch table [B][4] (a network's
// output). bound = +inf: no clamp (fminf / fmaxf against an infinity return the other operand); both are exact, so numpy restates the
// row bit for bit. A row of X starts at r (L + 4) 4 bytes, 16-byte aligned at a 10 x 10 grid and not at 25 x 25, and the dataset's row at
// 12 rows[r] bytes (mod 16): the copy is k_fit_gather's, DWORD accesses with the contiguous index on the lanes and FIT_CONCAT_DEPTH
// independent loads in flight before the first store -- legal at every alignment. The four action floats are one dword per lane of four.
// One workgroup per minibatch row (grid-stride).
// EXPERT (a third mode, with LABEL: the two earlier instantiations keep their code): `lab` is the dataset's EXPERT column, and a row
// without an expert action -- component 0 a NaN by its bits -- gets four 0.0f by a select on that test, never what fmaxf / fminf make of
// a NaN; the critic's value on such a row is computed and ignored (k_fit_dpg_bc).
struct FitConcatArgs {
    const float *obs;           // the dataset's observation column [n][L]
    const float *lab;           // LABEL: its label column [n][4] (EXPERT: its expert column)
    const float *act;           // !LABEL: [B][4]
    const int32_t *rows;        // [B]
    float *X;                   // [B][L + 4]
    float bound;
    int32_t B, L;
};

__device__ __forceinline__ bool fit_no_expert(float c0) { return (__float_as_uint(c0) & 0x7fffffffu) > 0x7f800000u; }

template <bool LABEL, bool EXPERT = false> __global__ __launch_bounds__(FIT_DDPG_THREADS) void k_fit_concat(FitConcatArgs a) {
    static_assert(LABEL || !EXPERT, "the expert's action is read through rows, as the label is");
    const int tid = threadIdx.x;
    for (int r = blockIdx.x; r < a.B; r += gridDim.x) {
        const int64_t row = (int64_t)a.rows[r];
        const float *s = a.obs + row * a.L;
        float *d = a.X + (int64_t)r * (a.L + 4);
        for (int i0 = tid; i0 < a.L; i0 += FIT_DDPG_THREADS * FIT_CONCAT_DEPTH) {
            float v[FIT_CONCAT_DEPTH];
#pragma unroll
            for (int k = 0; k < FIT_CONCAT_DEPTH; k++) {
                const int i = i0 + k * FIT_DDPG_THREADS;
                v[k] = i < a.L ? s[i] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < FIT_CONCAT_DEPTH; k++) {
                const int i = i0 + k * FIT_DDPG_THREADS;
                if (i < a.L) d[i] = v[k];
            }
        }
        if (tid < 4) {
            const float av = LABEL ? a.lab[row * 4 + tid] : a.act[(int64_t)r * 4 + tid];
            const float lo = fmaxf(av, -a.bound);
            if (EXPERT) {
                const float c = fminf(lo, a.bound);
                d[a.L + tid] = fit_no_expert(a.lab[row * 4]) ? 0.0f : c;
            } else {
                d[a.L + tid] = fminf(lo, a.bound);
            }
        }
    }
}

// The critic's loss, in the place of k_fit_loss<1>: one workgroup of 256, thread t owning minibatch rows t, t + 256, .... q [B] is the
// critic on [s, a], qn [B] the target critic on [s', mu'(s')]; rew and next are read through rows. Per row, each operation one double
// rounding: nv = (double)qn_r, or 0 where next == TERMINAL;  g = gamma nv;  t = (double)rew + g;  y_r = (float)t. Then in float32
// dz_r = fl(fl(q_r - y_r) / fl(B)), and the loss adds dd dd with dd = (double)q - (double)y and divides by 2 B -- the order of
// k_fit_loss<1>. stats = {loss, sum q / B, sum y / B}; y_out (may be NULL) [B] gets y.
struct FitTdArgs {
    const float *q, *qn, *rew;
    const int32_t *next, *rows;
    float *dz, *y_out;
    double *stats;
    double gamma;
    int32_t B;
};

__global__ __launch_bounds__(FIT_DDPG_THREADS) void k_fit_loss_td(FitTdArgs a) {
    __shared__ double red[FIT_TD_STATS][256];
    const int tid = threadIdx.x;
    const float den = (float)a.B;
    double s_sq = 0.0, s_q = 0.0, s_y = 0.0;
    for (int r = tid; r < a.B; r += 256) {
        const size_t row = (size_t)a.rows[r];
        const float qv = a.q[r];
        const double nv = a.next[row] == FIT_NEXT_TERMINAL ? 0.0 : (double)a.qn[r];
        const double g = a.gamma * nv;
        const double t = (double)a.rew[row] + g;
        const float yv = (float)t;
        const float d = qv - yv;
        a.dz[r] = d / den;
        if (a.y_out) a.y_out[r] = yv;
        const double dd = (double)qv - (double)yv;
        const double sq = dd * dd;
        s_sq = s_sq + sq;
        s_q = s_q + (double)qv;
        s_y = s_y + (double)yv;
    }
    red[0][tid] = s_sq; red[1][tid] = s_q; red[2][tid] = s_y;
    fit_tree_sums(red, tid);
    if (tid == 0) {
        const double Bd = (double)a.B;
        a.stats[0] = red[0][0] / (double)(2 * (int64_t)a.B); a.stats[1] = red[1][0] / Bd; a.stats[2] = red[2][0] / Bd;
    }
}

// The actor's dZ of its last layer from dA [B][4] = dL/da (the critic's input gradient at the four action columns, L = -1/B sum Q) and
// the policy's own output y [B][4]: the critic saw clamp(y), whose derivative is 0 outside the box -- but a component outside the box
// whose step would move it back INSIDE passes:  dz_rk = 0 where (y_rk >= bound and dA_rk < 0) or (y_rk <= -bound and dA_rk > 0)  (a
// descent step moves y against dA: further out), else dz_rk = dA_rk. One workgroup of 256, a thread owns whole rows; y, dA and dz lie at
// B-dependent offsets of scratch tables, so their four floats move under a 4-byte alignment promise (k_fit_loss_ppo does the same).
// stats = {-sum q / B, gated / (4 B), sum |dA| / (4 B)}, three sums in double in the house order (a row's components k ascending), q [B]
// the critic's output this pass.
struct FitDpgArgs {
    const float *dA, *y, *q;
    float *dz;
    double *stats;
    float bound;
    int32_t B;
};

__global__ __launch_bounds__(FIT_DDPG_THREADS) void k_fit_dpg_dz(FitDpgArgs a) {
    __shared__ double red[FIT_DPG_STATS][256];
    const int tid = threadIdx.x;
    double s_q = 0.0, s_gate = 0.0, s_abs = 0.0;
    for (int r = tid; r < a.B; r += 256) {
        float g[4], mu[4], out[4];
        __builtin_memcpy(g, a.dA + (size_t)4 * r, 16);
        __builtin_memcpy(mu, a.y + (size_t)4 * r, 16);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool gated = (mu[k] >= a.bound && g[k] < 0.0f) || (mu[k] <= -a.bound && g[k] > 0.0f);
            out[k] = gated ? 0.0f : g[k];
            s_gate = s_gate + (gated ? 1.0 : 0.0);
            s_abs = s_abs + (double)__builtin_fabsf(g[k]);
        }
        __builtin_memcpy(a.dz + (size_t)4 * r, out, 16);
        s_q = s_q + (double)a.q[r];
    }
    red[0][tid] = s_q; red[1][tid] = s_gate; red[2][tid] = s_abs;
    fit_tree_sums(red, tid);
    if (tid == 0) {
        const double Bd = (double)a.B, B4 = (double)(4 * (int64_t)a.B);
        a.stats[0] = -red[0][0] / Bd; a.stats[1] = red[1][0] / B4; a.stats[2] = red[2][0] / B4;
    }
}

// The actor's dZ of DDPG from demonstrations (clothhip.h: DDPG FROM DEMONSTRATIONS; Nair et al., "Overcoming Exploration in RL with
// Demonstrations"), in the place of k_fit_dpg_dz: the gated policy gradient scaled by qc, plus a behaviour-cloning term on the rows that
// carry an expert action and, under the Q-filter (qe != NULL), only where the critic rates the expert's action STRICTLY above the
// policy's own, qe_r > q_r in float32. Per row r: m = the row has an expert action (the bits of component 0 of expert[rows[r]]),
// f = m and (qe == NULL or qe_r > q_r). Per component: g = k_fit_dpg_dz's gate of dA; a = fl(qc g); where f and bc != 0:
// e = min(max(a_E, -bound), bound), d = fl(y - e), b = fl(fl(bc d) / fl(2 B)), dz = fl(a + b); ELSE dz = a and no addition is made, so
// the sign of a zero survives and with qc = 1 (an exact product) dz is k_fit_dpg_dz's by bytes. The BC loss adds dd dd,
// dd = (double)y - (double)e, over the rows with f, k ascending, and is reported over 4 B, not scaled by bc. No gradient flows through
// the filter or through e. One workgroup of 256, a thread owns whole rows; dA, y and dz move under a 4-byte alignment promise; the
// expert column's rows are 16-byte aligned (a dataset column of four floats).
// stats = {-sum q / B, gated / (4 B), sum |dA| / (4 B), bc_loss, sum m / B, sum f / B}: k_fit_dpg_dz's three, then three more.
struct FitDpgBcArgs {
    const float *dA, *y, *q;
    const float *qe;            // [B] the critic on [s, clamp(a_E)], or NULL: no filter
    const float *expert;        // the dataset's expert column [n][4]
    const int32_t *rows;        // [B]
    float *dz;
    double *stats;
    float bound, qc, bc;
    int32_t B;
};

__global__ __launch_bounds__(FIT_DDPG_THREADS) void k_fit_dpg_bc(FitDpgBcArgs a) {
    __shared__ double red[FIT_DPG_BC_STATS][256];
    const int tid = threadIdx.x;
    const float den = (float)(2 * a.B);
    double s_q = 0.0, s_gate = 0.0, s_abs = 0.0, s_bc = 0.0, s_m = 0.0, s_f = 0.0;
    for (int r = tid; r < a.B; r += 256) {
        float g[4], mu[4], out[4];
        __builtin_memcpy(g, a.dA + (size_t)4 * r, 16);
        __builtin_memcpy(mu, a.y + (size_t)4 * r, 16);
        const float4 ex = reinterpret_cast<const float4 *>(a.expert)[(size_t)a.rows[r]];
        const float ae[4] = {ex.x, ex.y, ex.z, ex.w};
        const float qv = a.q[r];
        const bool m = !fit_no_expert(ae[0]);
        const bool f = m && (a.qe == nullptr || a.qe[r] > qv);
        const bool clone = f && a.bc != 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool gated = (mu[k] >= a.bound && g[k] < 0.0f) || (mu[k] <= -a.bound && g[k] > 0.0f);
            const float gk = gated ? 0.0f : g[k];
            const float av = a.qc * gk;
            s_gate = s_gate + (gated ? 1.0 : 0.0);
            s_abs = s_abs + (double)__builtin_fabsf(g[k]);
            // (the row's expert action is finite wherever f holds; elsewhere e is not used)
            const float e = fminf(fmaxf(ae[k], -a.bound), a.bound);
            if (clone) {
                const float d = mu[k] - e;
                const float bd = a.bc * d;
                const float b = bd / den;
                out[k] = av + b;
            } else {
                out[k] = av;
            }
            if (f) {
                const double dd = (double)mu[k] - (double)e;
                const double sq = dd * dd;
                s_bc = s_bc + sq;
            }
        }
        __builtin_memcpy(a.dz + (size_t)4 * r, out, 16);
        s_q = s_q + (double)qv;
        s_m = s_m + (m ? 1.0 : 0.0);
        s_f = s_f + (f ? 1.0 : 0.0);
    }
    red[0][tid] = s_q; red[1][tid] = s_gate; red[2][tid] = s_abs; red[3][tid] = s_bc; red[4][tid] = s_m; red[5][tid] = s_f;
    fit_tree_sums(red, tid);
    if (tid == 0) {
        const double Bd = (double)a.B, B4 = (double)(4 * (int64_t)a.B);
        a.stats[0] = -red[0][0] / Bd; a.stats[1] = red[1][0] / B4; a.stats[2] = red[2][0] / B4;
        a.stats[3] = red[3][0] / B4; a.stats[4] = red[4][0] / Bd; a.stats[5] = red[5][0] / Bd;
    }
}

// The soft update of a target: target_i = fl(fl(omt target_i) + fl(t theta_i)), i < n, with t = (float)tau and omt = (float)(1 - tau)
// formed in double on the host. Over the n parameters of a one-row table; a pad behind them is not touched.
__global__ __launch_bounds__(FIT_DDPG_THREADS) void k_fit_polyak(float *target, const float *theta, int64_t n, float t, float omt) {
    const int64_t i = (int64_t)blockIdx.x * FIT_DDPG_THREADS + threadIdx.x;
    if (i >= n) return;
    const float a = omt * target[i], b = t * theta[i];
    target[i] = a + b;
}

}  // namespace clothhip
