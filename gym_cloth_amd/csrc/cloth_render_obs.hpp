// cloth_render_obs.hpp -- image observations for MANY cloths at once: every slot of an episode launch, a table of stored '1d'
// observations, or the handle's own particles (clothhip_render_obs).
//
// The pixel rules are k_render's (cloth_render.hpp), expression for expression and in the same order: projection, per-vertex
// normals summed in face-index order, edge functions with the top-left rule, perspective-correct 1/depth, and the nearest
// fragment winning through a max over (depth key << 32 | rgb). What differs is where the z-buffer lives and where the image is
// finished:
//   * the image is cut into BANDS of rows; a band's 64-bit keys sit in LDS behind the seven per-vertex arrays, triangles are
//     culled against the band by their bounding box, and fragments merge with the LDS 64-bit max. No z-buffer in global memory
//     and no global atomic per fragment: k_render's 8 B per pixel per image of hipMalloc'ed scratch is what keeps it from
//     rendering thousands of images per call. The max is order-independent, so any band plan gives k_render's image.
//     (tests/test_gpu_render_exact.py holds this kernel to the exact reference oracle/render_exact.py -- the rules -- and byte for byte
//     to k_render -- the bits -- from every source, in every format, under one-band, one-row-band and walked plans.)
//   * the uint8 image is finished on the device: RGB [H][W][3]; DEPTH [H][W][3], the 8-bit depth replicated; RGBD [H][W][4].
//     The 8-bit depth normalises the camera-space depth over the WHOLE image (all bands), so the raw depth goes through a
//     float scratch of a fixed chunk of images and k_depth8 finishes it: depth8() below, the float32 arithmetic of
//     ClothVecEnv.image_obs (get_image_rep_279.py:390-406, cloth_env.py:301-302).
// The host picks the band height (render_plan) from the LDS budget for (Ppad, W).
#pragma once

#include <math.h>

#include "cloth_render.hpp"

namespace clothhip {

// ---- the finishing rule: one image's camera-space depth -> 8 bits -----------------------------------------------------------
// lo / hi: min / max depth of the image. rintf rounds half to even, as numpy.rint does; the division is IEEE.
__host__ __device__ inline uint8_t depth8(float d, float lo, float hi) {
    const float nz = hi > lo ? (d - lo) / (hi - lo) : 0.0f;
    const float v = rintf(nz * 255.0f) - 50.0f;
    return (uint8_t)(v > 0.0f ? v : 0.0f);
}

// ---- band plan -------------------------------------------------------------------------------------------------------------
// rows per band, bands per image, dynamic LDS bytes per workgroup (7 vertex arrays + the band's keys); fits == false: not even a
// one-row band fits the budget (lds is then what that band would need)
struct RenderPlan { int rows, bands, lds; bool fits; };
static inline RenderPlan render_plan(int Ppad, int W, int H, int budget) {
    const long long vert = 7LL * Ppad * 4;
    long long rows_max = (budget - vert) / (8LL * W);
    if (budget < vert || rows_max < 1) {
        const long long need = vert + 8LL * W;
        return {0, 0, (int)(need > INT32_MAX ? INT32_MAX : need), false};
    }
    if (rows_max > H) rows_max = H;
    const int bands = (int)((H + rows_max - 1) / rows_max);
    const int rows = (H + bands - 1) / bands;                         // balanced: the last band is short by < bands rows
    return {rows, bands, (int)(vert + 8LL * rows * W), true};
}

struct RenderObsArgs {
    RenderArgs s;              // grid, camera, colours, lamp (N, P, Ppad, W, H, cam .. energy); its E / swap / buffers are unused
    int32_t rows, bands;       // band plan
    int32_t format, C;         // CLOTHHIP_IMG_*, bytes per pixel (3 or 4)
    long long src_stride;      // elements between the sources of consecutive images: 3P (a '1d' row) or 3 * Ppad (SoA state)
    const uint8_t *valid;      // [images of this launch] or nullptr: 0 = not rasterised, bytes zero
    const uint8_t *swap;       // [images of this launch] or nullptr: != 0 swaps the two side colours
    uint8_t *out;              // [images][H][W][C]
    float *depth;              // [images][H * W] raw camera-space depth (DEPTH / RGBD), or nullptr (RGB)
};

// grid (images, workgroups per image): workgroup y renders the bands y, y + gridDim.y, ... of image x.
// AOS: src is a float32 '1d' table (x0, y0, z0, x1, ...); otherwise the handle's SoA state [3][Ppad], converted with (float).
template <typename T, bool AOS>
__global__ __launch_bounds__(256) void k_render_obs(const T *src, RenderObsArgs B) {
    const RenderArgs &A = B.s;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *vx = reinterpret_cast<float *>(smem), *vy = vx + A.Ppad, *vd = vy + A.Ppad, *vi = vd + A.Ppad;   // pixel x, y, depth, intensity
    float *wx = vi + A.Ppad, *wy = wx + A.Ppad, *wz = wy + A.Ppad;                                          // world position
    unsigned long long *zb = reinterpret_cast<unsigned long long *>(wz + A.Ppad);                          // [rows][W] keys of the band
    const int img = blockIdx.x, tid = threadIdx.x, N = A.N, P = A.P, W = A.W, H = A.H, C = B.C;
    const size_t npx = (size_t)W * H;
    uint8_t *o = B.out + (size_t)img * npx * C;
    if (B.valid != nullptr && B.valid[img] == 0) {                    // not rasterised: the image's bytes are zero
        for (int band = blockIdx.y; band < B.bands; band += gridDim.y) {
            const int r0 = band * B.rows, r1 = r0 + B.rows < H ? r0 + B.rows : H;
            for (size_t i = (size_t)r0 * W * C + tid; i < (size_t)r1 * W * C; i += 256) o[i] = 0;
        }
        return;
    }
    const T *ps = src + (size_t)img * B.src_stride;
    if (AOS) {
        for (int i = tid; i < P; i += 256) { wx[i] = (float)ps[3 * i]; wy[i] = (float)ps[3 * i + 1]; wz[i] = (float)ps[3 * i + 2]; }
    } else {
        const T *px = ps, *py = px + A.Ppad, *pz = py + A.Ppad;
        for (int i = tid; i < P; i += 256) { wx[i] = (float)px[i]; wy[i] = (float)py[i]; wz[i] = (float)pz[i]; }
    }
    const float bed_d = A.cam[2];                                    // camera-space depth of the bed plane z = 0 (top-down)
    const unsigned long long bgkey = (unsigned long long)((quant8(A.bg[0]) << 16) | (quant8(A.bg[1]) << 8) | quant8(A.bg[2]));
    __syncthreads();
    // ---- vertices: projection + smooth normal (sum of the incident faces' normals, in face index order) ----------------------
    for (int i = tid; i < P; i += 256) {
        const float X = wx[i] - A.cam[0], Y = wy[i] - A.cam[1], Z = wz[i] - A.cam[2];
        const float xc = A.R[0] * X + A.R[1] * Y + A.R[2] * Z;
        const float yc = A.R[3] * X + A.R[4] * Y + A.R[5] * Z;
        const float zc = A.R[6] * X + A.R[7] * Y + A.R[8] * Z;
        const float d = -zc;                                          // depth along the view axis
        const float ds = d > 1e-6f ? d : 1e-6f;
        vx[i] = (A.fx * xc) / ds + A.cx;
        vy[i] = A.cy - (A.fy * yc) / ds;
        vd[i] = d;
        const int r = i / N, c = i - r * N;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        for (int qr = r - 1; qr <= r; qr++)
            for (int qc = c - 1; qc <= c; qc++) {
                if (qr < 0 || qc < 0 || qr >= N - 1 || qc >= N - 1) continue;
                const int pp = qr * N + qc;
                const int f[2][3] = {{pp, pp + N, pp + 1}, {pp + 1, pp + N, pp + N + 1}};
                for (int k = 0; k < 2; k++) {
                    if (f[k][0] != i && f[k][1] != i && f[k][2] != i) continue;
                    const int a = f[k][0], b = f[k][1], cc = f[k][2];
                    const float ux = wx[b] - wx[a], uy = wy[b] - wy[a], uz = wz[b] - wz[a];
                    const float tx = wx[cc] - wx[a], ty = wy[cc] - wy[a], tz = wz[cc] - wz[a];
                    nx = nx + (uy * tz - uz * ty); ny = ny + (uz * tx - ux * tz); nz = nz + (ux * ty - uy * tx);
                }
            }
        const float nn = sqrtf(nx * nx + ny * ny + nz * nz);
        float lam = 0.0f;
        if (nn > 0.0f) {
            lam = (nx * A.light[0] + ny * A.light[1] + nz * A.light[2]) / nn;
            lam = lam < 0.0f ? -lam : lam;                            // two-sided
        }
        vi[i] = A.ambient + A.energy * lam;
    }
    const int nq = (N - 1) * (N - 1);
    const bool sw = B.swap != nullptr && B.swap[img] != 0;
    for (int band = blockIdx.y; band < B.bands; band += gridDim.y) {
        const int r0 = band * B.rows, r1 = r0 + B.rows < H ? r0 + B.rows : H, nb = (r1 - r0) * W;   // rows [r0, r1) of the image
        for (int i = tid; i < nb; i += 256) zb[i] = bgkey;
        __syncthreads();                                              // (the first pass: also the vertex arrays)
        // ---- triangles, clipped to the band ------------------------------------------------------------------------------------
        for (int t = tid; t < 2 * nq; t += 256) {
            const int q = t >> 1, qr = q / (N - 1), qc = q - qr * (N - 1), pp = qr * N + qc;
            const int a = (t & 1) ? pp + 1 : pp, b = pp + N, c = (t & 1) ? pp + N + 1 : pp + 1;
            const float x0 = vx[a], y0 = vy[a], x1 = vx[b], y1 = vy[b], x2 = vx[c], y2 = vy[c];
            if (!(vd[a] > 1e-6f && vd[b] > 1e-6f && vd[c] > 1e-6f)) continue;          // behind the camera: dropped
            const float area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
            if (!(area > 0.0f) && !(area < 0.0f)) continue;                            // degenerate (or NaN)
            const bool front = (area < 0.0f) != sw;
            const float *col = front ? A.front : A.back;
            float mnx = fminf(x0, fminf(x1, x2)), mxx = fmaxf(x0, fmaxf(x1, x2));
            float mny = fminf(y0, fminf(y1, y2)), mxy = fmaxf(y0, fmaxf(y1, y2));
            mnx = fmaxf(mnx, -1.0f); mny = fmaxf(mny, -1.0f); mxx = fminf(mxx, (float)W); mxy = fminf(mxy, (float)H);
            int ix0 = (int)floorf(mnx), ix1 = (int)floorf(mxx), iy0 = (int)floorf(mny), iy1 = (int)floorf(mxy);
            ix0 = ix0 < 0 ? 0 : ix0; iy0 = iy0 < 0 ? 0 : iy0;
            ix1 = ix1 > W - 1 ? W - 1 : ix1; iy1 = iy1 > H - 1 ? H - 1 : iy1;
            iy0 = iy0 < r0 ? r0 : iy0; iy1 = iy1 > r1 - 1 ? r1 - 1 : iy1;              // the band's share of the bounding box
            if (iy0 > iy1 || ix0 > ix1) continue;
            const float s = area > 0.0f ? 1.0f : -1.0f;               // orient the edge functions so that inside is >= 0
            const float iw0 = 1.0f / vd[a], iw1 = 1.0f / vd[b], iw2 = 1.0f / vd[c];
            for (int iy = iy0; iy <= iy1; iy++)
                for (int ix = ix0; ix <= ix1; ix++) {
#if defined(CLOTHHIP_MUTATE) && CLOTHHIP_MUTATE == 12
                    const float fxp = (float)ix + 0.0f, fyp = (float)iy + 0.0f;   // MUTANT 12 (tools/run_mutants.sh; never a product build): the pixel corner, not its centre
#else
                    const float fxp = (float)ix + 0.5f, fyp = (float)iy + 0.5f;
#endif
                    const float e0 = s * ((x2 - x1) * (fyp - y1) - (y2 - y1) * (fxp - x1));   // opposite vertex a
                    const float e1 = s * ((x0 - x2) * (fyp - y2) - (y0 - y2) * (fxp - x2));   // opposite vertex b
                    const float e2 = s * ((x1 - x0) * (fyp - y0) - (y1 - y0) * (fxp - x0));   // opposite vertex c
                    // top-left rule on exact zeros, in image coordinates (y down): an edge owns the centres on it if the face lies to its right (a left
                    // edge: e grows with x, s * (y1 - y2) > 0), or, if it is horizontal, below it (a top edge: e grows with y, s * (x2 - x1) > 0)
#if defined(CLOTHHIP_MUTATE) && CLOTHHIP_MUTATE == 10
                    const bool in0 = e0 > 0.0f || (e0 == 0.0f && ((s * (y2 - y1) > 0.0f) || (y2 == y1 && s * (x2 - x1) < 0.0f)));   // MUTANT 10 (tools/run_mutants.sh; never a product build): e0 owns its right / bottom ties
#else
                    const bool in0 = e0 > 0.0f || (e0 == 0.0f && ((s * (y2 - y1) < 0.0f) || (y2 == y1 && s * (x2 - x1) > 0.0f)));
#endif
                    const bool in1 = e1 > 0.0f || (e1 == 0.0f && ((s * (y0 - y2) < 0.0f) || (y0 == y2 && s * (x0 - x2) > 0.0f)));
                    const bool in2 = e2 > 0.0f || (e2 == 0.0f && ((s * (y1 - y0) < 0.0f) || (y1 == y0 && s * (x1 - x0) > 0.0f)));
                    if (!(in0 && in1 && in2)) continue;
                    const float sa = s * area;
                    const float b0 = e0 / sa, b1 = e1 / sa, b2 = e2 / sa;
#if defined(CLOTHHIP_MUTATE) && CLOTHHIP_MUTATE == 11
                    const float inv_d = 1.0f / (b0 * vd[a] + b1 * vd[b] + b2 * vd[c]);             // MUTANT 11 (tools/run_mutants.sh; never a product build): depth mixed affinely
#else
                    const float inv_d = b0 * iw0 + b1 * iw1 + b2 * iw2;                        // perspective-correct 1/depth
#endif
                    const float inten = b0 * vi[a] + b1 * vi[b] + b2 * vi[c];
                    const unsigned long long key = ((unsigned long long)depth_key(inv_d) << 32) | (quant8(col[0] * inten) << 16) |
                                                   (quant8(col[1] * inten) << 8) | quant8(col[2] * inten);
                    atomicMax(&zb[(iy - r0) * W + ix], key);          // LDS
                }
        }
        __syncthreads();
        // ---- resolve the band: colour bytes straight into the image, raw depth into the scratch k_depth8 finishes -----------------
        const size_t p0 = (size_t)r0 * W;
        for (int i = tid; i < nb; i += 256) {
            const unsigned long long k = zb[i];
            if (B.format != CLOTHHIP_IMG_DEPTH) {
                uint8_t *q = o + (p0 + i) * C;
                q[0] = (uint8_t)((k >> 16) & 0xFF); q[1] = (uint8_t)((k >> 8) & 0xFF); q[2] = (uint8_t)(k & 0xFF);
            }
            if (B.depth) B.depth[(size_t)img * npx + p0 + i] = (k >> 32) == 0ull ? bed_d : 1.0f / __uint_as_float((uint32_t)(k >> 32));
        }
        __syncthreads();                                              // the next band reuses zb
    }
}

// One workgroup per image: min / max of the image's raw depth, then depth8() into the depth channel(s) of the finished image.
__global__ __launch_bounds__(256) void k_depth8(RenderObsArgs B) {
    __shared__ float slo[256], shi[256];
    const int img = blockIdx.x, tid = threadIdx.x;
    if (B.valid != nullptr && B.valid[img] == 0) return;             // k_render_obs has zeroed it
    const size_t npx = (size_t)B.s.W * B.s.H;
    const float *d = B.depth + (size_t)img * npx;
    uint8_t *o = B.out + (size_t)img * npx * B.C;
    float lo = d[0], hi = d[0];
    for (size_t i = tid; i < npx; i += 256) { lo = fminf(lo, d[i]); hi = fmaxf(hi, d[i]); }
    slo[tid] = lo; shi[tid] = hi;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) { slo[tid] = fminf(slo[tid], slo[tid + st]); shi[tid] = fmaxf(shi[tid], shi[tid + st]); }
        __syncthreads();
    }
    lo = slo[0]; hi = shi[0];
    for (size_t i = tid; i < npx; i += 256) {
        const uint8_t v = depth8(d[i], lo, hi);
        if (B.format == CLOTHHIP_IMG_RGBD) o[i * 4 + 3] = v;
        else { o[i * 3] = v; o[i * 3 + 1] = v; o[i * 3 + 2] = v; }
    }
}

}  // namespace clothhip
