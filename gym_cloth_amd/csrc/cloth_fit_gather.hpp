// cloth_fit_gather.hpp -- rows of the trainer's dataset named by where they lie on the device (clothhip_fit_hold,
// clothhip_fit_data_append_launch; no reference counterpart): ONE kernel copies observation rows of 3P floats from the last episode launch's
// tables (or the handle's held rows) to the dataset's spare capacity (or to the held rows), and converts the label alongside: the expert's
// from the label table, or the action the launch EXECUTED from its record table (clothhip_fit_data_append_launch_ex), and writes the
// destination row's loss weight. Included only by api_fit.hip.
//
// A row is 3P floats and 3P is odd for every odd grid (3 * 625 = 1875), so a row starts at 4-byte alignment only: row r of a table begins
// 12 r bytes (mod 16) into a 16-byte line, and since the source row and the destination row are unrelated numbers, the two sides are in
// different 16-byte phases for three row pairs of four. A 16-byte access can then be aligned on one side at most; the other side would need
// its data shifted across lanes or split again. The copy is DWORD accesses instead: lane i of a wave reads and writes base + 4 i, so each
// wave instruction covers 256 contiguous bytes on both sides whatever the phases are, and a thread keeps FIT_GATHER_DEPTH independent loads
// in flight before its first store. What that costs against a device-to-device copy of the same bytes is measured (profiles/dagger.txt).
// All offsets are 64-bit: a table of 2^31 rows of 7 500 bytes is far past 2^32.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clothhip {

constexpr int FIT_GATHER_THREADS = 256, FIT_GATHER_DEPTH = 4;
enum { FIT_SRC_SLOTS = 0, FIT_SRC_RESETS = 1, FIT_SRC_HELD = 2 };      // = CLOTHHIP_FIT_SRC_*

// The record table as the gather reads it, in bytes: the action is four doubles at offset 0 of a record -- dword-pair loads at 8-byte
// alignment, since a record's size is a multiple of 8 --, `ran` ONE byte near its end. api_fit.hip asserts both against ClothStepRecord.
constexpr int FIT_REC_BYTES = 72, FIT_REC_RAN = 64;

struct FitGatherArgs {
    const float *table[3];      // by source: obs [T * E][L], reset_obs [E * n_scripts][L], held [E][L] (the host has checked every index)
    const int32_t *rows;        // [n][4] = (source, row, label row or -1, destination row)
    const double *labels;       // [T * E][4] of the last armed launch, or NULL when no entry names a label or the labels are the records'
                                // (an entry that names a label row with both tables NULL gets the label (0, 0, 0, 0))
    const unsigned char *records;   // [T * E] ClothStepRecord of the last launch: the label is (float)action[0..3], or NULL
    const float *weights;       // [n] the destination rows' loss weights in entry order, or NULL: 1.0f
    float *dst_obs, *dst_lab;   // destination tables [..][L], [..][4] (dst_lab may be NULL then)
    float *dst_w;               // [..] (NULL: no weight is written -- the held rows have none)
    float *dst_exp;             // [..][4] the expert-action column, or NULL (every source but CLOTHHIP_FIT_LABEL_ACTION_EXPERT): with it `records` AND
                                // `labels` are there, the label is the record's and this gets (float)labels[label row][0..3]
    int32_t *flag;              // raised (integer atomic OR) when a copied observation value or a rounded label is not finite, or a
                                // named record did not run (its label is then stored as NaN, the label of a slot that did not run)
    int64_t n;
    int32_t L;                  // 3P
};

__device__ __forceinline__ bool fit_not_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// one workgroup per entry (grid-stride over the entries), a thread per element in passes of FIT_GATHER_THREADS * FIT_GATHER_DEPTH
__global__ __launch_bounds__(FIT_GATHER_THREADS) void k_fit_gather(FitGatherArgs a) {
    const int tid = threadIdx.x;
    bool bad = false;
    for (int64_t r = blockIdx.x; r < a.n; r += gridDim.x) {
        const int32_t *q = a.rows + 4 * r;
        const int32_t src = q[0], row = q[1], lrow = q[2], drow = q[3];
        const float *s = a.table[src] + (int64_t)row * a.L;
        float *d = a.dst_obs + (int64_t)drow * a.L;
        for (int i0 = tid; i0 < a.L; i0 += FIT_GATHER_THREADS * FIT_GATHER_DEPTH) {
            float v[FIT_GATHER_DEPTH];
#pragma unroll
            for (int k = 0; k < FIT_GATHER_DEPTH; k++) {
                const int i = i0 + k * FIT_GATHER_THREADS;
                v[k] = i < a.L ? s[i] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < FIT_GATHER_DEPTH; k++) {
                const int i = i0 + k * FIT_GATHER_THREADS;
                if (i < a.L) { d[i] = v[k]; bad |= fit_not_finite(v[k]); }
            }
        }
        if (lrow >= 0 && tid < 4) {      // the rounding of clothhip_fit_data_append: (float)label
            float lv;
            if (a.records) {
                const unsigned char *rec = a.records + (int64_t)lrow * FIT_REC_BYTES;
                lv = rec[FIT_REC_RAN] == 1 ? (float)reinterpret_cast<const double *>(rec)[tid] : __uint_as_float(0x7fc00000u);
            } else if (a.labels) {
                lv = (float)a.labels[(int64_t)lrow * 4 + tid];
            } else {
                lv = 0.0f;      // CLOTHHIP_FIT_LABEL_ZERO: a leaf, no table is read
            }
            a.dst_lab[(int64_t)drow * 4 + tid] = lv;
            bad |= fit_not_finite(lv);
        }
        if (a.dst_w && tid == 4) a.dst_w[drow] = a.weights ? a.weights[r] : 1.0f;      // (another lane than the labels': no second pass)
        if (a.dst_exp && lrow >= 0 && tid >= 8 && tid < 12) {      // (and four more lanes: the expert's action beside the executed one)
            const float ev = (float)a.labels[(int64_t)lrow * 4 + (tid - 8)];
            a.dst_exp[(int64_t)drow * 4 + (tid - 8)] = ev;
            bad |= fit_not_finite(ev);
        }
    }
    if (bad) atomicOr(a.flag, 1);
}

// the sum of (double)w (double)(y - a)^2 over a minibatch, in k_fit_loss's order and arithmetic (cloth_policy_fit.hpp: thread t of 256 takes
// elements t, t + 256, ... ascending, a halving tree over the 256 sums) and nothing else: clothhip_policy_fit_loss divides on the host
__global__ __launch_bounds__(256) void k_fit_sqsum(const float *y, const float *lab, const float *wgt, const int32_t *rows, int32_t B, double *sum) {
    __shared__ double red[256];
    const int tid = threadIdx.x, n = 4 * B;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) {
        const size_t row = (size_t)rows[i >> 2];
        const double dd = (double)y[i] - (double)lab[row * 4 + (i & 3)];
        const double sq = dd * dd;
        s = s + (double)wgt[row] * sq;
    }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    if (tid == 0) *sum = red[0];
}

// clothhip_policy_fit_predict* / clothhip_value_predict: member j's y of one chunk, n_vals = B * (output width) contiguous floats at
// y + j * y_step, to out + j * out_step, lane i at base + 4 i on both sides. One workgroup per member and 256 elements
__global__ __launch_bounds__(256) void k_fit_copy_y(const float *y, int32_t n_vals, float *out, int64_t y_step, int64_t out_step, int32_t blocks) {
    const int j = blockIdx.x / blocks, bx = blockIdx.x - j * blocks;
    const int i = bx * 256 + threadIdx.x;
    if (i < n_vals) out[(int64_t)j * out_step + i] = y[(int64_t)j * y_step + i];
}

// clothhip_fit_data_snapshot_policy_members: member j's y of one chunk, [B][4] at y + j * y_step, SCATTERED to a dataset column of
// 16-byte rows -- position r of member j goes to row rows[j * B + r] of col. A thread owns one (member, position): y lies at a
// B-dependent offset of the scratch table, so its four floats move under a 4-byte alignment promise (as k_fit_loss_ppo reads them);
// the column's row is ONE 16-byte store. Member j's index row is padded to B behind its len[j] real positions (the host repeats a valid
// row there, for the layer-0 gather): nothing is stored for a padded position, so no row of the column is written twice. One workgroup
// per member and 256 positions; ordinary vector stores only
__global__ __launch_bounds__(256) void k_fit_scatter_y(const float *y, const int32_t *rows, const int32_t *len, float *col, int32_t B, int64_t y_step, int32_t blocks) {
    const int j = blockIdx.x / blocks, bx = blockIdx.x - j * blocks;
    const int r = bx * 256 + threadIdx.x;
    if (r >= len[j]) return;      // (len[j] <= B)
    float v[4];
    __builtin_memcpy(v, y + (int64_t)j * y_step + (size_t)4 * r, 16);
    reinterpret_cast<float4 *>(col)[(size_t)rows[(int64_t)j * B + r]] = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace clothhip
