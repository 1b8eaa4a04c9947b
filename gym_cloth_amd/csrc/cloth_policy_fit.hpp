// cloth_policy_fit.hpp -- the supervised trainer of the handle's policy networks (cloth_policy_mlp.hpp: the blobs it updates in place):
// forward, backward and one optimizer step over a minibatch of stored (observation row, action label) pairs (no reference counterpart: the
// refit half of a DAgger / behaviour-cloning iteration). ONE trainer: a call fits n_m rows of a weight table in the launches of one
// network, every row on its own minibatches; the handle's shared network is the table of one row, fitted by the call members = {0},
// n_m = 1. Included only by api_fit.hip, which owns the order of the launches.
//
//   L = 1 / (4 B) sum_r w_r sum_k (y_rk - a_rk)^2,  dL/dy_rk = w_r (y_rk - a_rk) / (2 B), w_r the stored row's weight (1.0f unless the caller
//   wrote another: any finite float, the normaliser stays B);  ReLU' = 1 where the pre-activation is > 0, else 0 (the mask is read
//   from the stored activation: relu(z) > 0 exactly when z > 0).
//
// ONE tiled matrix product, k_fit_gemm, does the three products of every layer on the f32-input matrix instruction
// v_mfma_f32_32x32x2_f32 (exact float32: per output element a k-ascending fmaf chain, one rounding per product -- the fit minimises the loss
// of the very float32 function the launch evaluates):
//   forward          H_l   = act(H_l-1 W_l^T + b_l)      A = H_l-1 [B][in]  k-contiguous, B = W_l [out][in] k-contiguous   (NT), bias (+ ReLU)
//   weight gradient  dW_l  = dZ_l^T H_l-1                A = dZ_l  [B][out] m-contiguous, B = H_l-1 [B][in] n-contiguous   (TN), none
//   input gradient   dZ_l-1 = (dZ_l W_l) * [H_l-1 > 0]   A = dZ_l  [B][out] k-contiguous, B = W_l [out][in] n-contiguous   (NN), mask
//   Layer 0's H_-1 is the dataset read through the minibatch's index table (`rows`): no gathered copy.
//
// THE MEMBER INDEX. Every kernel carries the member j of the call folded into gridDim.x (a call may name up to 65 536 members, more than
// gridDim.y / z hold): blockIdx.x = j * (blocks of one member) + the block's own x index. Member j's weights and moments lie at
// members[j] * stride of a [rows][stride] table (members: a device table), its scratch tables (activations, dZ, slabs, gradient, index
// rows, loss) at j times the table's per-member size. No element's arithmetic depends on j, n_m or the row, so member j's bits are those
// of that network fitted alone on a handle of its own.
//
// THE ORDER OF THE ARITHMETIC (fixed; no floating-point atomics anywhere)
//   * an output element is ONE accumulator: products added for k ascending from 0 within its k range, out-of-range elements of a tile are
//     zeros in LDS (a + 0 * 0 leaves a finite accumulator's bits alone), then the epilogue (+ b, ReLU / mask);
//   * the batch sum of a weight gradient is split into FIT_SPLIT_ROWS-row ranges (a function of B alone), each range one accumulator
//     written to its own slab; k_fit_reduce adds the slabs in ascending range order. B <= FIT_SPLIT_ROWS: one range, written directly;
//   * db_l[j] = sum_r dZ_l[r][j], r ascending, one thread per j (k_fit_colsum);
//   * dZ_L-1 = fl(fl(w fl(y - a)) / fl(2 B)); the loss sums (double)w * (dd * dd), dd = (double)y - (double)a, each operation one double
//     rounding: thread t of 256 takes elements t, t + 256, ... ascending, the 256 sums are added by a halving tree in LDS (k_fit_loss,
//     one workgroup per member). Multiplying by 1.0f and by 1.0 is exact: a dataset whose weights are all 1 gives the unweighted bits;
//   * the optimizer (k_fit_adam / k_fit_sgd) is elementwise, each operation one float32 rounding (the library is built with
//     -ffp-contract=off; division and sqrtf are the correctly rounded ones, no fast-math flag reaches this unit).
//   * the value network (output width 1, clothhip.h: FITTING THE CRITIC) is one more table of one row for the same kernels: N = 1 in
//     its last forward product, M = 1 in that layer's weight gradient, K = 1 in its input gradient -- each a tile whose other 63 rows,
//     columns or 15 k are the zeros in LDS above; k_fit_loss<1> sums B squares in the order k_fit_loss<4> sums 4 B;
//   * PPO's clipped surrogate (clothhip.h: PPO ON THE DEVICE) is one more loss launch of the policy's table, k_fit_loss_ppo in the place of
//     k_fit_loss<4>: per row a probability ratio against the dataset's stored old mean through exp_fixed, dZ in double with one rounding
//     to float32, three sums over ROWS in the order above; forward, backward and optimizer are the launches of the squared error.
//     Member j's constants are row j of a table the host made: one row for the shared network, a row per member for rows of a
//     population (clothhip.h: PPO FOR A POPULATION);
//   * PPO with a LEARNED sigma (clothhip.h: PPO WITH A LEARNED SIGMA) is one more loss launch again, k_fit_loss_ppo_sigma: the head
//     log_sigma[4] read from device memory, the row's old log sigma beside its old mean, nine exp_fixed per row, seven sums over ROWS;
//     the head is one more table of one row of four elements for k_fit_adam / k_fit_sgd, launched a second time per step;
//   The forward's summation order differs from mlp_eval's (64 interleaved lane sums and a butterfly there), so the trainer's y need not equal
//   clothhip_policy_eval's bits; the blob it writes is evaluated by mlp_eval as any uploaded blob is.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloth_exp_fixed.hpp"      // exp_fixed: the one exponential of the PPO losses below

namespace clothhip {

constexpr int FIT_MAX_BATCH = 4096;       // = CLOTHHIP_FIT_MAX_BATCH
constexpr int FIT_SPLIT_ROWS = 256;       // rows of the batch one accumulator of a weight gradient sums
constexpr int FIT_TILE = 64, FIT_BK = 16, FIT_THREADS = 256;      // a workgroup: 64 x 64 outputs, 4 waves of 32 x 32, k in steps of 16
constexpr int FIT_LDS_LD = FIT_TILE + 1;  // LDS images are [k][m] / [k][n], rows padded by one float

enum { FIT_EPI_NONE = 0, FIT_EPI_BIAS = 1, FIT_EPI_BIAS_RELU = 2, FIT_EPI_MASK = 3 };

// Member j: C[M][N] (+ z * c_slab) = sum_{k in the z-th range of k_chunk} A(m, k) B(k, n). The pointers are member 0's scratch tables;
// B (when b_weights) and bias are relative to row 0 of the weight table.
struct FitGemmArgs {
    const float *A, *B;         // A_KC: A(m, k) = A[row(m) * lda + k], else A[k * lda + m];  B_KC: B(k, n) = B[n * ldb + k], else B[row(k) * ldb + n]
    const int32_t *rows;        // optional indirection of the storage row of the operand that is the dataset (A when A_KC, B when !B_KC)
    const float *bias;          // [N]   FIT_EPI_BIAS*
    const float *mask;          // [M][ldc]  FIT_EPI_MASK: C = mask > 0 ? C : 0
    float *C;
    int64_t lda, ldb, ldc, c_slab;
    int32_t M, N, K, k_chunk;
    const int32_t *members;     // [n_m] rows of the weight table
    int64_t stride;             // floats between two rows of the weight table
    int64_t a_step, b_step, c_step, mask_step, rows_step;      // per-member sizes of the scratch tables (0: one table for all, the dataset)
    int32_t b_weights;          // B is the weight matrix of row members[j], else a scratch table
    int32_t tiles_n;            // blocks of one member along x
};

typedef float fit_f32x16 __attribute__((ext_vector_type(16)));

// Tile (bx, by) of the bz-th k range of the product `a` describes, its pointers already those of the member: k_fit_gemm below does the
// member's addressing, this function the tile. (It stays a function of its own although it has one caller: with its text written into
// the kernel, <false, false, 0, true> takes 37 VGPRs instead of 34.)
template <bool A_KC, bool B_KC, int EPI, bool ROWS> __device__ __forceinline__ void fit_gemm_tile(const FitGemmArgs &a, const int bx, const int by, const int bz) {
    __shared__ float As[FIT_BK][FIT_LDS_LD], Bs[FIT_BK][FIT_LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = by * FIT_TILE, n0 = bx * FIT_TILE;
    const int k_begin = bz * a.k_chunk, k_end = min(a.K, k_begin + a.k_chunk);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;      // this wave's 32 x 32 corner of the tile
    fit_f32x16 acc;
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;
    // staging: 64 x 16 of each operand, zeros outside the matrices, 4 elements per thread and operand with the contiguous index on the
    // lanes. The next tile's elements are loaded into registers while this tile's products run (the arithmetic and its order are untouched).
    int ar[4], ak[4], br[4], bk[4];      // r: the m (or n) index in the tile, k: the k index
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (A_KC) { ak[i] = tid & 15; ar[i] = (tid >> 4) + 16 * i; } else { ar[i] = tid & 63; ak[i] = (tid >> 6) + 4 * i; }
        if (B_KC) { bk[i] = tid & 15; br[i] = (tid >> 4) + 16 * i; } else { br[i] = tid & 63; bk[i] = (tid >> 6) + 4 * i; }
    }
    float va[4], vb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int m = m0 + ar[i], k = k0 + ak[i];
            va[i] = 0.0f;
            if (m < a.M && k < k_end) va[i] = A_KC ? a.A[(size_t)(ROWS ? a.rows[m] : m) * a.lda + k] : a.A[(size_t)k * a.lda + m];
            const int n = n0 + br[i], kb = k0 + bk[i];
            vb[i] = 0.0f;
            if (n < a.N && kb < k_end) vb[i] = B_KC ? a.B[(size_t)n * a.ldb + kb] : a.B[(size_t)(ROWS ? a.rows[kb] : kb) * a.ldb + n];
        }
    };
    fetch(k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += FIT_BK) {
#pragma unroll
        for (int i = 0; i < 4; i++) { As[ak[i]][ar[i]] = va[i]; Bs[bk[i]][br[i]] = vb[i]; }
        __syncthreads();
        if (k0 + FIT_BK < k_end) fetch(k0 + FIT_BK);
        // lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31] of each 32 x 32 x 2 step
#pragma unroll
        for (int ks = 0; ks < FIT_BK; ks += 2) {
            const float av = As[ks + (lane >> 5)][wm + (lane & 31)], bv = Bs[ks + (lane >> 5)][wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *C = a.C + (size_t)bz * a.c_slab;
    const int n = n0 + wn + (lane & 31);
    if (n >= a.N) return;
    float bj = 0.0f;
    if (EPI == FIT_EPI_BIAS || EPI == FIT_EPI_BIAS_RELU) bj = a.bias[n];
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
        const int m = m0 + wm + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        if (m >= a.M) continue;
        float v = acc[reg];
        if (EPI == FIT_EPI_BIAS || EPI == FIT_EPI_BIAS_RELU) v = v + bj;
        if (EPI == FIT_EPI_BIAS_RELU) v = v < 0.0f ? 0.0f : v;
        if (EPI == FIT_EPI_MASK) v = a.mask[(size_t)m * a.ldc + n] > 0.0f ? v : 0.0f;
        C[(size_t)m * a.ldc + n] = v;
    }
}

template <bool A_KC, bool B_KC, int EPI, bool ROWS> __global__ __launch_bounds__(FIT_THREADS) void k_fit_gemm(FitGemmArgs p) {
    const int j = blockIdx.x / p.tiles_n, bx = blockIdx.x - j * p.tiles_n;
    const int64_t w = (int64_t)p.members[j] * p.stride;
    FitGemmArgs a = p;
    a.A += (int64_t)j * p.a_step;
    a.B += p.b_weights ? w : (int64_t)j * p.b_step;
    a.C += (int64_t)j * p.c_step;
    if (ROWS) a.rows += (int64_t)j * p.rows_step;
    if (EPI == FIT_EPI_BIAS || EPI == FIT_EPI_BIAS_RELU) a.bias += w;
    if (EPI == FIT_EPI_MASK) a.mask += (int64_t)j * p.mask_step;
    fit_gemm_tile<A_KC, B_KC, EPI, ROWS>(a, bx, blockIdx.y, blockIdx.z);
}

// out[i] = slab_0[i] + slab_1[i] + ... in ascending order, i < n (the split batch sum of a weight gradient). Member j: part + j * part_step
// -> out + j * out_step; `blocks` blocks per member
__global__ __launch_bounds__(256) void k_fit_reduce(const float *part, int64_t slab, int32_t n_slabs, float *out, int64_t n, int64_t part_step,
                                                    int64_t out_step, int32_t blocks) {
    const int j = blockIdx.x / blocks, bx = blockIdx.x - j * blocks;
    const int64_t i = (int64_t)bx * 256 + threadIdx.x;
    if (i >= n) return;
    part += (int64_t)j * part_step;
    float s = part[i];
    for (int z = 1; z < n_slabs; z++) s = s + part[(size_t)z * slab + i];
    out[(int64_t)j * out_step + i] = s;
}

// db[c] = sum_r dz[r][c], r ascending. Member j: dz + j * dz_step -> db + j * db_step; `blocks` blocks per member
__global__ __launch_bounds__(64) void k_fit_colsum(const float *dz, int32_t B, int32_t n_out, float *db, int64_t dz_step, int64_t db_step, int32_t blocks) {
    const int j = blockIdx.x / blocks, bx = blockIdx.x - j * blocks;
    const int c = bx * 64 + threadIdx.x;
    if (c >= n_out) return;
    dz += (int64_t)j * dz_step;
    float s = 0.0f;
    for (int r = 0; r < B; r++) s = s + dz[(size_t)r * n_out + c];
    db[(int64_t)j * db_step + c] = s;
}

// The halving tree of the three loss kernels below: each of the N rows of red holds the 256 per-thread sums of one quantity, written by
// its thread; afterwards red[i][0] is row i's sum, red[i][t] + red[i][t + o] for o = 128, 64, ... 1. Every thread of the 256 calls it.
template <int N> __device__ __forceinline__ void fit_tree_sums(double (&red)[N][256], const int tid) {
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int i = 0; i < N; i++) red[i][tid] = red[i][tid] + red[i][tid + o];
        }
        __syncthreads();
    }
}

// dz[r][k] = fl(fl(w fl(y - a)) / fl(2 B)) with a = lab[rows[r]][k] and w = wgt[rows[r]]; loss = sum (double)w (double)(y - a)^2 / (4 B).
// One workgroup of 256 per member: y, dz and the index rows at j times their per-member sizes, the loss at loss[j]. The four lanes of a
// row read ONE weight (the same dword: one request); w = 1.0f leaves both products' bits alone, so an unweighted dataset keeps its bits.
// W is the network's output width: 4, the policy, as above; 1, the value network (clothhip.h: FITTING THE CRITIC) -- lab is then the
// column of value targets [n], there is no weight (wgt is not read), dz[r] = fl(fl(v - ret) / fl(B)) and loss = sum (double)(v - ret)^2 / (2 B):
// the same order over B elements.
template <int W> __global__ __launch_bounds__(256) void k_fit_loss(const float *y, const float *lab, const float *wgt, const int32_t *rows, int32_t B, float *dz,
                                                                   double *loss, int64_t y_step, int64_t dz_step, int64_t rows_step) {
    static_assert(W == 4 || W == 1, "an action or a value");
    __shared__ double red[1][256];
    const int64_t j = blockIdx.x;
    y += j * y_step; dz += j * dz_step; rows += j * rows_step;
    const int tid = threadIdx.x, n = W * B;
    const float den = (float)(W == 4 ? 2 * B : B);
    double s = 0.0;
    for (int i = tid; i < n; i += 256) {
        const size_t row = (size_t)rows[i / W];
        const float yv = y[i], av = lab[row * W + (i % W)];
        const float d = yv - av;
        const double dd = (double)yv - (double)av;
        const double sq = dd * dd;
        if (W == 4) {
            const float wv = wgt[row];
            const float wd = wv * d;
            dz[i] = wd / den;
            s = s + (double)wv * sq;
        } else {
            dz[i] = d / den;
            s = s + sq;
        }
    }
    red[0][tid] = s;
    fit_tree_sums(red, tid);
    if (tid == 0) loss[j] = red[0][0] / (double)((W == 4 ? 4 : 2) * (int64_t)B);
}

// PPO's clipped surrogate of a fixed-sigma Gaussian policy in the place of k_fit_loss<4> (clothhip.h: PPO ON THE DEVICE has the
// arithmetic operation by operation): the same launch shape, one workgroup of 256 per member, but a thread owns whole ROWS -- thread t
// takes minibatch rows t, t + 256, ... ascending -- since a row's ratio needs its four components. lab, old (16-byte rows of the
// dataset's tables) are read as one 16-byte load each; y and dz lie at B-dependent offsets of the scratch tables that need not be
// 16-byte aligned, so their four floats move under a 4-byte alignment promise and the compiler picks the widest legal access. Three
// sums (surrogate, rows not active, kl) in the house order: per thread over its rows ascending, then a halving tree each in LDS.
// stats[j] = {-sum surrogate / B, not active / B, sum kl / B}; ratio (may be NULL) [n_m][B] gets (float)rho. Ordinary stores only.
// Member j's workgroup takes ITS constants from row j of q: the shared network is a table of one row, rows of a population
// (clothhip_policy_fit_ppo*_members) have a row each. The row index is the block's, uniform over the workgroup, so the four doubles are
// scalar loads.
struct FitPpoArgs {
    const float *y, *lab, *old, *wgt;
    const int32_t *rows;
    float *dz, *ratio;
    double *stats;
    const double *q;                        // [n_m][4] {1 / sigma^2, 0.5 / sigma^2, 1 - eps, 1 + eps}: formed once in double on the host
    int64_t y_step, dz_step, rows_step;
    int32_t B;
};
constexpr int FIT_PPO_STATS = 3;            // = CLOTHHIP_PPO_STATS

__global__ __launch_bounds__(256) void k_fit_loss_ppo(FitPpoArgs a) {
    __shared__ double red[FIT_PPO_STATS][256];
    const int64_t j = blockIdx.x;
    const double *c = a.q + j * 4;
    const double inv_s2 = c[0], half_inv_s2 = c[1], lo = c[2], hi = c[3];
    const float *y = a.y + j * a.y_step;
    float *dz = a.dz + j * a.dz_step;
    const int32_t *rows = a.rows + j * a.rows_step;
    const int tid = threadIdx.x;
    const double Bd = (double)a.B;
    double s_sur = 0.0, s_clip = 0.0, s_kl = 0.0;
    for (int r = tid; r < a.B; r += 256) {
        const size_t row = (size_t)rows[r];
        float mu[4], out[4];
        __builtin_memcpy(mu, y + (size_t)4 * r, 16);
        const float4 av = reinterpret_cast<const float4 *>(a.lab)[row], ov = reinterpret_cast<const float4 *>(a.old)[row];
        const float act[4] = {av.x, av.y, av.z, av.w}, mo[4] = {ov.x, ov.y, ov.z, ov.w};
        double q = 0.0, kl = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double d_old = (double)act[k] - (double)mo[k], d_new = (double)act[k] - (double)mu[k];
            const double sq_old = d_old * d_old, sq_new = d_new * d_new;
            const double t = sq_old - sq_new;
            q = q + t;
            const double e = (double)mu[k] - (double)mo[k];
            const double ee = e * e;
            kl = kl + ee;
        }
        const double x = q * half_inv_s2;
        const double rho = exp_fixed(x);
        const double A = (double)a.wgt[row];
        const double s1 = rho * A;
        double rc = rho < lo ? lo : rho;
        rc = rc > hi ? hi : rc;
        const double s2 = rc * A;
        const bool active = s1 <= s2;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double d = (double)mu[k] - (double)act[k];
            const double g1 = s1 * d, g2 = g1 * inv_s2, g3 = g2 / Bd;
            out[k] = active ? (float)g3 : 0.0f;
        }
        __builtin_memcpy(dz + (size_t)4 * r, out, 16);
        if (a.ratio) a.ratio[j * a.B + r] = (float)rho;
        s_sur = s_sur + (active ? s1 : s2);
        s_clip = s_clip + (active ? 0.0 : 1.0);
        s_kl = s_kl + kl * half_inv_s2;
    }
    red[0][tid] = s_sur; red[1][tid] = s_clip; red[2][tid] = s_kl;
    fit_tree_sums(red, tid);
    if (tid == 0) {
        double *st = a.stats + j * FIT_PPO_STATS;
        st[0] = -red[0][0] / Bd; st[1] = red[1][0] / Bd; st[2] = red[2][0] / Bd;
    }
}

// PPO's clipped surrogate of a Gaussian policy whose log sigma is LEARNED (clothhip.h: PPO WITH A LEARNED SIGMA has the arithmetic
// operation by operation): k_fit_loss_ppo's launch shape and row ownership, with the head ls[4] read from DEVICE memory (the steps of a
// call are enqueued without a host round trip, and the optimizer moves the head between them) and the row's stored old log sigma
// beside its old mean. Nine exp_fixed per row: 1 / sigma_old^2 and sigma_old^2 per component and the ratio; 1 / sigma^2 per component
// once per thread. Seven sums in the house order: the surrogate, the rows not active, kl and the four row terms of the head's
// gradient. stats[j] = {-sum surrogate / B - ent_coef H, not active / B, sum kl / B, H}; grad_ls[j][4] = (float)(-(sum h_k) / B -
// ent_coef); ls_out (may be NULL) [n_m][4] gets the head this launch read; ratio as above. With ls == old log sigma == 0 every product
// by inv / invo / so2 is a product by 1.0 and every (lo - ls) a +0.0: rho, dz and the first three statistics (ent_coef 0) are
// k_fit_loss_ppo's bits at sigma = 1. Ordinary stores only.
struct FitPpoSigmaArgs {
    const float *y, *lab, *old, *old_ls, *wgt, *ls;
    const int32_t *rows;
    float *dz, *ratio, *grad_ls, *ls_out;
    double *stats;
    double lo, hi, ent_coef;                // 1 - eps, 1 + eps: formed once in double on the host
    int64_t y_step, dz_step, rows_step;
    int32_t B;
};
constexpr int FIT_PPO_SIGMA_STATS = 4;      // = CLOTHHIP_PPO_SIGMA_STATS
constexpr int FIT_PPO_SIGMA_SUMS = 7;
constexpr double FIT_ENTROPY_C = 5.675754132818691;      // 2 (1 + ln 2 pi): the entropy of four unit Gaussians

__global__ __launch_bounds__(256) void k_fit_loss_ppo_sigma(FitPpoSigmaArgs a) {
    __shared__ double red[FIT_PPO_SIGMA_SUMS][256];
    const int64_t j = blockIdx.x;
    const float *y = a.y + j * a.y_step;
    float *dz = a.dz + j * a.dz_step;
    const int32_t *rows = a.rows + j * a.rows_step;
    const int tid = threadIdx.x;
    const double Bd = (double)a.B;
    double ls[4], inv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        ls[k] = (double)a.ls[k];
        const double m2 = -2.0 * ls[k];
        inv[k] = exp_fixed(m2);
    }
    double s_sur = 0.0, s_clip = 0.0, s_kl = 0.0, s_h[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = tid; r < a.B; r += 256) {
        const size_t row = (size_t)rows[r];
        float mu[4], out[4];
        __builtin_memcpy(mu, y + (size_t)4 * r, 16);
        const float4 av = reinterpret_cast<const float4 *>(a.lab)[row], ov = reinterpret_cast<const float4 *>(a.old)[row];
        const float4 lv = reinterpret_cast<const float4 *>(a.old_ls)[row];
        const float act[4] = {av.x, av.y, av.z, av.w}, mo[4] = {ov.x, ov.y, ov.z, ov.w}, lo4[4] = {lv.x, lv.y, lv.z, lv.w};
        double q = 0.0, klq = 0.0, kld = 0.0, t_new[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double lo = (double)lo4[k];
            const double m2 = -2.0 * lo, p2 = 2.0 * lo;
            const double invo = exp_fixed(m2), so2 = exp_fixed(p2);
            const double d_old = (double)act[k] - (double)mo[k], d_new = (double)act[k] - (double)mu[k];
            const double sq_old = d_old * d_old, sq_new = d_new * d_new;
            const double t_old = sq_old * invo;
            t_new[k] = sq_new * inv[k];
            const double t = t_old - t_new[k];
            const double th = t * 0.5;
            const double dl = lo - ls[k];
            const double u = th + dl;
            q = q + u;
            const double e = (double)mu[k] - (double)mo[k];
            const double ee = e * e;
            const double c1 = so2 * inv[k], c2 = c1 - 1.0, c3 = ee * inv[k], c4 = c2 + c3;
            klq = klq + c4;
            const double dk = ls[k] - lo;
            kld = kld + dk;
        }
        const double klh = klq * 0.5;
        const double kl = kld + klh;
        const double rho = exp_fixed(q);
        const double A = (double)a.wgt[row];
        const double s1 = rho * A;
        double rc = rho < a.lo ? a.lo : rho;
        rc = rc > a.hi ? a.hi : rc;
        const double s2 = rc * A;
        const bool active = s1 <= s2;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double d = (double)mu[k] - (double)act[k];
            const double g1 = s1 * d, g2 = g1 * inv[k], g3 = g2 / Bd;
            out[k] = active ? (float)g3 : 0.0f;
            const double m1 = t_new[k] - 1.0, hk = s1 * m1;
            s_h[k] = s_h[k] + (active ? hk : 0.0);
        }
        __builtin_memcpy(dz + (size_t)4 * r, out, 16);
        if (a.ratio) a.ratio[j * a.B + r] = (float)rho;
        s_sur = s_sur + (active ? s1 : s2);
        s_clip = s_clip + (active ? 0.0 : 1.0);
        s_kl = s_kl + kl;
    }
    red[0][tid] = s_sur; red[1][tid] = s_clip; red[2][tid] = s_kl;
#pragma unroll
    for (int k = 0; k < 4; k++) red[3 + k][tid] = s_h[k];
    fit_tree_sums(red, tid);
    if (tid == 0) {
        double hs = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) hs = hs + ls[k];
        const double H = hs + FIT_ENTROPY_C;
        const double l0 = -red[0][0] / Bd, eh = a.ent_coef * H;
        double *st = a.stats + j * FIT_PPO_SIGMA_STATS;
        st[0] = l0 - eh; st[1] = red[1][0] / Bd; st[2] = red[2][0] / Bd; st[3] = H;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double g0 = -red[3 + k][0] / Bd, g = g0 - a.ent_coef;
            a.grad_ls[j * 4 + k] = (float)g;
            if (a.ls_out) a.ls_out[j * 4 + k] = a.ls[k];
        }
    }
}

// dst[i] = ls[i & 3], i < n4 (= 4 n): the present head into n consecutive rows of the dataset's old-log-sigma column
// (clothhip_fit_data_snapshot_policy on a handle with a head)
__global__ __launch_bounds__(256) void k_fit_fill_ls(float *dst, const float *ls, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) dst[i] = ls[i & 3];
}

// The optimizers: member j updates row members[j] of theta, m, v ([rows][stride]) from g + j * n with ITS OWN step constants
// hyper[j][FIT_HYPER], made on the host per member and step: Adam {a_t, beta1, 1 - beta1, beta2, 1 - beta2, eps} with
// a_t = (float)(lr sqrt(1 - beta2^t) / (1 - beta1^t)), SGD {lr, momentum}. Only the n parameters of a row are touched, never its pad.
constexpr int FIT_HYPER = 6;
struct FitOptArgs {
    float *theta, *m, *v;
    const float *g, *hyper;
    const int32_t *members;
    int64_t stride, n;
    int32_t blocks;             // blocks of one member
};

// Adam, every line one float32 operation
__global__ __launch_bounds__(256) void k_fit_adam(FitOptArgs a) {
    const int j = blockIdx.x / a.blocks, bx = blockIdx.x - j * a.blocks;
    const int64_t row = (int64_t)a.members[j] * a.stride, i = (int64_t)bx * 256 + threadIdx.x;
    const float *h = a.hyper + (int64_t)j * FIT_HYPER;
    const float a_t = h[0], beta1 = h[1], omb1 = h[2], beta2 = h[3], omb2 = h[4], eps = h[5];
    if (i >= a.n) return;
    float *theta = a.theta + row, *m = a.m + row, *v = a.v + row;
    const float gi = a.g[(int64_t)j * a.n + i];
    const float m1 = beta1 * m[i], m2 = omb1 * gi, mi = m1 + m2;
    const float gg = gi * gi, v1 = beta2 * v[i], v2 = omb2 * gg, vi = v1 + v2;
    const float den = __builtin_sqrtf(vi) + eps, q = mi / den, step = a_t * q;
    m[i] = mi; v[i] = vi;
    theta[i] = theta[i] - step;
}

// SGD with momentum: u = fl(fl(mu u) + g); theta = fl(theta - fl(lr u))
__global__ __launch_bounds__(256) void k_fit_sgd(FitOptArgs a) {
    const int j = blockIdx.x / a.blocks, bx = blockIdx.x - j * a.blocks;
    const int64_t row = (int64_t)a.members[j] * a.stride, i = (int64_t)bx * 256 + threadIdx.x;
    const float *h = a.hyper + (int64_t)j * FIT_HYPER;
    const float lr = h[0], mu = h[1];
    if (i >= a.n) return;
    float *theta = a.theta + row, *u = a.m + row;
    const float u1 = mu * u[i], ui = u1 + a.g[(int64_t)j * a.n + i], step = lr * ui;
    u[i] = ui;
    theta[i] = theta[i] - step;
}

}  // namespace clothhip
