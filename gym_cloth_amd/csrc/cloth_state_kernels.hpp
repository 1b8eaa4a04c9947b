// cloth_state_kernels.hpp -- the small kernels that change a handle's state from outside the stepper (api_state.hip, which alone includes this):
// Gripper.grab_top / grab (gripper.pyx:23-53), release, flat reset, dropping parked time-slice operations, forks.
#pragma once

#include "cloth_common.hpp"

namespace clothhip {

// ---- Gripper.grab_top / grab (gripper.pyx:23-53): one wave per env ---------------------------------
template <typename T> struct GrabArgs {
    const T *pos; uint8_t *cnt;
    const double *xy;        // [E][2]
    const double *radius;    // [E] or nullptr
    const uint8_t *active;   // [E] or nullptr
    int32_t *n_grabbed;      // [E]
    const double *levels;    // [n_levels] curZ table (double; cast per use)
    int32_t n_levels, P, Ppad, top;
    double default_radius, two_thickness;
};

template <typename T> __global__ __launch_bounds__(64) void k_grab(GrabArgs<T> A) {
    const int e = blockIdx.x, lane = threadIdx.x;
    if (A.active && !A.active[e]) { if (lane == 0) A.n_grabbed[e] = 0; return; }
    const T gx = (T)A.xy[2 * e], gy = (T)A.xy[2 * e + 1];
    const T rad = (T)(A.radius ? A.radius[e] : A.default_radius);
    const T tt = (T)A.two_thickness;
    const T *px = A.pos + (size_t)e * 3 * A.Ppad, *py = px + A.Ppad, *pz = py + A.Ppad;
    uint8_t *cnt = A.cnt + (size_t)e * A.Ppad;
    int best = 0x7fffffff;
    if (A.top) {
        // first level (scanning down from `height`) at which any in-cylinder point lies in the band
#if defined(CLOTHHIP_MUTATE) && CLOTHHIP_MUTATE == 15                // MUTANT 15: the LAST level that hits, not the first
        int last = -1;
        for (int i = lane; i < A.P; i += 64) {
            const T dx = px[i] - gx, dy = py[i] - gy;
            if (dx * dx + dy * dy < rad) {
                const T z = pz[i];
                for (int l = 0; l < A.n_levels; l++) {
                    T d = z - (T)A.levels[l]; d = d < 0 ? -d : d;
                    if (d < tt && l > last) last = l;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) { int v = __shfl_xor(last, o); last = v > last ? v : last; }
        if (last >= 0) best = last;
#else
        for (int i = lane; i < A.P; i += 64) {
            const T dx = px[i] - gx, dy = py[i] - gy;
            if (GRAB_IN_CYLINDER(dx * dx + dy * dy, rad)) {             // gripper.pyx:35 (radius not squared)
                const T z = pz[i];
                for (int l = 0; l < A.n_levels && l < best; l++) {
                    T d = z - (T)A.levels[l]; d = d < 0 ? -d : d;
                    if (GRAB_IN_BAND(d, tt)) { best = l; break; }       // gripper.pyx:36
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) { int v = __shfl_xor(best, o); best = v < best ? v : best; }
#endif
        if (best == 0x7fffffff) { if (lane == 0) A.n_grabbed[e] = 0; return; }
    }
    int n = 0;
    for (int i = lane; i < A.P; i += 64) {
        const T dx = px[i] - gx, dy = py[i] - gy;
        if (GRAB_IN_CYLINDER(dx * dx + dy * dy, rad)) {
            bool hit = true;
            if (A.top) { T d = pz[i] - (T)A.levels[best]; d = d < 0 ? -d : d; hit = GRAB_IN_BAND(d, tt); }
            if (hit) {                                                  // pinned = True ; grabbed_pts.append
                uint8_t c = cnt[i];
                if ((c & CNT_GRAB_MASK) < CNT_GRAB_MASK) c = (uint8_t)(c + 1);
                cnt[i] = c; n++;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) A.n_grabbed[e] = n;
}

__global__ void k_release(uint8_t *cnt, const uint8_t *active, int Ppad) {
    const int e = blockIdx.x;
    if (active && !active[e]) return;
    uint8_t *c = cnt + (size_t)e * Ppad;
    for (int i = threadIdx.x; i < Ppad; i += blockDim.x) if (c[i] & CNT_GRAB_MASK) c[i] = 0;
}

// Cloth(...) rebuilt on reset (cloth_env.py:737-746) for the flat tiers 1/3: masked envs <- the flat grid (pos = prev),
// nothing pinned, tear flag cleared; with per-env rest tables also the flat rest lengths.
template <typename T>
__global__ void k_reset_flat(T *pos, T *prev, uint8_t *cnt, int32_t *tear, const T *flat, const uint8_t *mask, int Ppad,
                             T *rest, const T *flat_rest, int rest_stride, int Spad) {
    const int e = blockIdx.x;
    if (mask && !mask[e]) return;
    T *p = pos + (size_t)e * 3 * Ppad, *q = prev + (size_t)e * 3 * Ppad;
    for (int i = threadIdx.x; i < 3 * Ppad; i += blockDim.x) { const T v = flat[i]; p[i] = v; q[i] = v; }
    for (int i = threadIdx.x; i < Ppad; i += blockDim.x) cnt[(size_t)e * Ppad + i] = 0;
    if (rest_stride)
        for (int i = threadIdx.x; i < Spad; i += blockDim.x) rest[(size_t)e * rest_stride + i] = flat_rest[i];
    if (threadIdx.x == 0) tear[e] = 0;
}

// A state change from outside the episode launches voids the operation a time slice left in flight -- for the envs it touches only:
// mask (or the schedules' active flags) selects them, nullptr = every env.
__global__ void k_clear_resume(EpResume *r, const uint8_t *mask, const ClothSchedule *sched, int E) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    if (mask && !mask[e]) return;
    if (sched && !(sched[e].active && sched[e].n_total > 0)) return;
    r[e].valid = 0;
}

// ---- clothhip_fork: a whole cloth from env slot to env slot, device to device -------------------------------------------------------------
// nbytes from src to dst by the whole workgroup, bits untouched: 16-byte vectors while both addresses allow them (the state rows always do:
// Ppad and Spad are multiples of 64 elements and hipMalloc aligns to 256 bytes), else 4-byte words (a DevConsts<float> record is 52 bytes
// into its table), and what is left by the plain path, byte by byte.
__device__ __forceinline__ void fork_copy(void *__restrict__ dst, const void *__restrict__ src, size_t nbytes) {
    const size_t tid = threadIdx.x, nt = blockDim.x;
    const uintptr_t both = (uintptr_t)dst | (uintptr_t)src;
    size_t done = 0;
    if ((both & 15) == 0) {
        const size_t nv = nbytes / 16;
        const uint4 *__restrict__ s = (const uint4 *)src; uint4 *__restrict__ d = (uint4 *)dst;
        size_t i = tid;
        for (; i + nt < nv; i += 2 * nt) {             // two loads in flight per thread before the first store
            const uint4 a = s[i], b = s[i + nt];
            d[i] = a; d[i + nt] = b;
        }
        if (i < nv) d[i] = s[i];
        done = nv * 16;
    } else if ((both & 3) == 0) {
        const size_t nw = nbytes / 4;
        const uint32_t *__restrict__ s = (const uint32_t *)src; uint32_t *__restrict__ d = (uint32_t *)dst;
        for (size_t i = tid; i < nw; i += nt) d[i] = s[i];
        done = nw * 4;
    }
    const unsigned char *__restrict__ s = (const unsigned char *)src; unsigned char *__restrict__ d = (unsigned char *)dst;
    for (size_t i = done + tid; i < nbytes; i += nt) d[i] = s[i];
}

// All sizes in bytes, all offsets 64-bit. rest_* / mat_* nullptr: that part is not copied (shared rest tables that are equal; STATE_ONLY or
// no device material table in play). rest_src_stride 0: the source's one shared table feeds every destination row.
struct ForkArgs {
    unsigned char *pos_dst, *prev_dst, *cnt_dst, *rest_dst, *mat_dst;
    const unsigned char *pos_src, *prev_src, *cnt_src, *rest_src, *mat_src;
    int32_t *tear_dst; const int32_t *tear_src;
    EpResume *resume_dst;                 // the destination's parked time-slice operations: dropped for the envs written here
    const int32_t *dst_env, *src_env;     // [n]
    size_t pos_bytes, cnt_bytes, rest_bytes, rest_src_stride, mat_bytes;
};

// One workgroup per DESTINATION env j: the cloth of the source's env src_env[j] -- positions and previous positions [3][Ppad], the pin
// bytes (grab multiplicity and the pinned-from-outside bit as they are), the tear flag, and where asked the rest-length row and the
// material record. Many destinations may name one source (branching); no destination is a source of the same call (checked on the host).
// Nothing is computed: the kernel is a copy and runs at memory bandwidth.
__global__ __launch_bounds__(256) void k_fork(ForkArgs A) {
    const size_t j = blockIdx.x;
    const size_t d = (size_t)A.dst_env[j], s = (size_t)A.src_env[j];
    fork_copy(A.pos_dst + d * A.pos_bytes, A.pos_src + s * A.pos_bytes, A.pos_bytes);
    fork_copy(A.prev_dst + d * A.pos_bytes, A.prev_src + s * A.pos_bytes, A.pos_bytes);
    fork_copy(A.cnt_dst + d * A.cnt_bytes, A.cnt_src + s * A.cnt_bytes, A.cnt_bytes);
    if (A.rest_dst) fork_copy(A.rest_dst + d * A.rest_bytes, A.rest_src + s * A.rest_src_stride, A.rest_bytes);
    if (A.mat_dst) fork_copy(A.mat_dst + d * A.mat_bytes, A.mat_src + s * A.mat_bytes, A.mat_bytes);
    if (threadIdx.x == 0) {
        A.tear_dst[d] = A.tear_src[s];
        if (A.resume_dst) A.resume_dst[d].valid = 0;
    }
}

// A handle that leaves its one shared rest table for per-env tables: rows 1 .. E-1 <- row 0 (one workgroup per row)
__global__ __launch_bounds__(256) void k_replicate_rest(unsigned char *rest, size_t row_bytes) {
    fork_copy(rest + ((size_t)blockIdx.x + 1) * row_bytes, rest, row_bytes);
}

}  // namespace clothhip
