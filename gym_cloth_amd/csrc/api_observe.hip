// api_observe.hip -- what is read off the cloths: metrics, '1d' observations, rendered images.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <utility>

#include "api_handle.hpp"
#include "cloth_observe_kernels.hpp"
#include "cloth_render.hpp"
#include "cloth_render_obs.hpp"

// ---- metrics (host, double): cloth_env.py:1020-1098 ------------------------------------------------------
// Convex-hull area by Andrew's monotone chain + shoelace. Collinear and duplicate points (plenty after the
// clip to [0,1]^2) are dropped from the chain; they do not change the area.
extern "C" double clothhip_hull_area(const double *xy, int32_t n) {
    if (!xy || n < 3) return 0.0;
    std::vector<std::pair<double, double>> p(n);
    for (int i = 0; i < n; i++) p[i] = {xy[2 * i], xy[2 * i + 1]};
    std::sort(p.begin(), p.end());
    p.erase(std::unique(p.begin(), p.end()), p.end());
    const int m = (int)p.size();
    if (m < 3) return 0.0;
    auto cross = [](const std::pair<double, double> &o, const std::pair<double, double> &a, const std::pair<double, double> &b) {
        return (a.first - o.first) * (b.second - o.second) - (a.second - o.second) * (b.first - o.first);
    };
    std::vector<std::pair<double, double>> hull(2 * m);
    int k = 0;
    for (int i = 0; i < m; i++) { while (k >= 2 && cross(hull[k - 2], hull[k - 1], p[i]) <= 0) k--; hull[k++] = p[i]; }
    for (int i = m - 2, t = k + 1; i >= 0; i--) { while (k >= t && cross(hull[k - 2], hull[k - 1], p[i]) <= 0) k--; hull[k++] = p[i]; }
    k--;   // last point == first point
    if (k < 3) return 0.0;
    double a2 = 0.0;
    for (int i = 0; i < k; i++) {
        const auto &u = hull[i], &v = hull[(i + 1) % k];
        a2 += (u.first - hull[0].first) * (v.second - hull[0].second) - (v.first - hull[0].first) * (u.second - hull[0].second);
    }
    return 0.5 * std::fabs(a2);
}

static int launch_metrics(clothhip_handle *h) {
    const MetricsDims md = metrics_dims(h->P, h->Ppad);
    const int lds = metrics_scratch_bytes(md, (int)h->tsz, false);
    const double half_thick = h->prm.thickness / 2.0;                                   // cloth_env.py:604
    if (int rc = by_precision(h, [&](auto t) {
            using T = decltype(t);
            HIPCHECK(hipFuncSetAttribute((const void *)k_metrics<T>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            hipLaunchKernelGGL(k_metrics<T>, dim3(h->E), dim3(256), lds, h->stream, (const T *)h->d_pos, h->P, h->Ppad, md.NS, md.NH, h->d_cov, h->d_vinv, h->d_oob, h->d_hcnt, half_thick);
            return 0;
        })) return rc;
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int clothhip_metrics_ex(clothhip_handle *h, double *coverage, double *variance_inv, uint8_t *oob, uint8_t *tear,
                                   int32_t *n_below_half_thickness) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (tear) if (int rc = clothhip_get_tear(h, tear)) return rc;
    if (!coverage && !variance_inv && !oob && !n_below_half_thickness) return 0;
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = launch_metrics(h)) return rc;
    if (coverage) HIPCHECK(hipMemcpyAsync(coverage, h->d_cov, (size_t)h->E * 8, hipMemcpyDeviceToHost, h->stream));
    if (variance_inv) HIPCHECK(hipMemcpyAsync(variance_inv, h->d_vinv, (size_t)h->E * 8, hipMemcpyDeviceToHost, h->stream));
    if (oob) HIPCHECK(hipMemcpyAsync(oob, h->d_oob, (size_t)h->E, hipMemcpyDeviceToHost, h->stream));
    if (n_below_half_thickness) HIPCHECK(hipMemcpyAsync(n_below_half_thickness, h->d_hcnt, (size_t)h->E * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_metrics(clothhip_handle *h, double *coverage, double *variance_inv, uint8_t *oob, uint8_t *tear) {
    return clothhip_metrics_ex(h, coverage, variance_inv, oob, tear, nullptr);
}

extern "C" int clothhip_write_obs_f32_device(clothhip_handle *h, void *d_out) {
    if (!h || !d_out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    HIPCHECK(hipSetDevice(h->device));
    by_precision(h, [&](auto t) {
        hipLaunchKernelGGL(k_write_obs<decltype(t)>, dim3(h->E), dim3(256), 0, h->stream, (const decltype(t) *)h->d_pos, (float *)d_out, h->P, h->Ppad);
    });
    HIPCHECK(hipGetLastError());
    return 0;
}

// ---- headless rendering ------------------------------------------------------------------------------------
// the image-size and lens rules of both render entry points
static int check_render_params(const clothhip_handle *h, const ClothRenderParams *p) {
    if (!h || !p) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (p->width < 1 || p->height < 1 || p->width > 4096 || p->height > 4096) return fail(CLOTHHIP_EINVAL, "image size outside [1, 4096]");
    if (!(p->lens_mm > 0) || !(p->sensor_mm > 0)) return fail(CLOTHHIP_EINVAL, "lens / sensor must be > 0");
    return 0;
}
// ... and their scene: grid, camera, colours, lamp
static void fill_scene(RenderArgs &a, const clothhip_handle *h, const ClothRenderParams *p) {
    a.N = h->N; a.P = h->P; a.Ppad = h->Ppad; a.W = p->width; a.H = p->height; a.E = h->E;
    for (int k = 0; k < 9; k++) a.R[k] = p->world_to_cam[k];
    for (int k = 0; k < 3; k++) { a.cam[k] = p->cam_pos[k]; a.front[k] = p->front[k]; a.back[k] = p->back[k]; a.bg[k] = p->background[k]; a.light[k] = p->light_dir[k]; }
    a.fx = (p->lens_mm / p->sensor_mm) * (float)p->width; a.fy = a.fx;           // square pixels, horizontal sensor fit
    a.cx = 0.5f * (float)p->width; a.cy = 0.5f * (float)p->height;
    a.ambient = p->ambient; a.energy = p->energy;
}

extern "C" int clothhip_render(clothhip_handle *h, const ClothRenderParams *p, const uint8_t *swap_sides, uint8_t *rgb, float *depth) {
    if (int rc = check_render_params(h, p)) return rc;
    if (!rgb && !depth) return 0;
    HIPCHECK(hipSetDevice(h->device));
    const size_t npx = (size_t)p->width * p->height, E = h->E;
    Buffer<unsigned long long> d_z; Buffer<uint8_t> d_rgb, d_sw; Buffer<float> d_dep;      // per call: a handle retains no image memory
    if (int rc = d_z.reserve(E * npx * 8)) return rc;
    if (rgb) if (int rc = d_rgb.reserve(E * npx * 3)) return rc;
    if (depth) if (int rc = d_dep.reserve(E * npx * 4)) return rc;
    if (swap_sides) { if (int rc = d_sw.reserve(E)) return rc; HIPCHECK(hipMemcpyAsync(d_sw, swap_sides, E, hipMemcpyHostToDevice, h->stream)); }
    RenderArgs a;
    fill_scene(a, h, p);
    a.swap = d_sw; a.zbuf = d_z; a.rgb = d_rgb; a.depth = d_dep;
    const int lds = 7 * h->Ppad * 4;
    if (int rc = by_precision(h, [&](auto t) {
            using T = decltype(t);
            HIPCHECK(hipFuncSetAttribute((const void *)k_render<T>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            hipLaunchKernelGGL(k_render<T>, dim3(h->E), dim3(256), lds, h->stream, (const T *)h->d_pos, a);
            return 0;
        })) return rc;
    HIPCHECK(hipGetLastError());
    if (rgb) HIPCHECK(hipMemcpyAsync(rgb, d_rgb, E * npx * 3, hipMemcpyDeviceToHost, h->stream));
    if (depth) HIPCHECK(hipMemcpyAsync(depth, d_dep, E * npx * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- image observations for many cloths (cloth_render_obs.hpp) -------------------------------------------------------------
// images per chunk: the scratch (finished images, raw depth, uploaded rows) is sized for one chunk, whatever n is
static int render_obs_chunk(size_t npx) {
    const size_t per_image = npx * 4, budget = (size_t)64 << 20;      // the largest scratch: 4 B per pixel (RGBD bytes, float depth)
    const size_t c = budget / per_image;
    return c < 1 ? 1 : (c > 256 ? 256 : (int)c);
}

extern "C" int clothhip_render_obs(clothhip_handle *h, const ClothRenderParams *p, int32_t source, const float *obs_host, int64_t n,
                                   const uint8_t *valid, const uint8_t *swap, int32_t format, uint8_t *out, void *d_out) {
    if (int rc = check_render_params(h, p)) return rc;
    if (format != CLOTHHIP_IMG_RGB && format != CLOTHHIP_IMG_DEPTH && format != CLOTHHIP_IMG_RGBD) return fail(CLOTHHIP_EINVAL, "unknown image format %d", format);
    if (source < CLOTHHIP_OBS_STATE || source > CLOTHHIP_OBS_HOST) return fail(CLOTHHIP_EINVAL, "unknown observation source %d", source);
    if (n < 0) return fail(CLOTHHIP_EINVAL, "n < 0");
    if (source == CLOTHHIP_OBS_HOST && !obs_host && n > 0) return fail(CLOTHHIP_EINVAL, "CLOTHHIP_OBS_HOST needs obs_host[n][3P]");
    int64_t n_src = source == CLOTHHIP_OBS_STATE ? (int64_t)h->E : n;
    const void *d_table = nullptr;      // a table of the last launch, where it lies
    if (source == CLOTHHIP_OBS_SLOTS || source == CLOTHHIP_OBS_RESETS) {
        if (int rc = check_idle(h)) return rc;
        if (int rc = launch_table(h, source == CLOTHHIP_OBS_SLOTS ? LaunchTable::obs : LaunchTable::reset_obs, &d_table, &n_src)) return rc;
    }
    if (n != n_src) return fail(CLOTHHIP_EINVAL, "n = %lld, the source holds %lld cloths", (long long)n, (long long)n_src);
    const RenderPlan plan = render_plan(h->Ppad, p->width, p->height, h->dbg.render_lds_kib * 1024);
    if (!plan.fits) return fail(CLOTHHIP_EINVAL, "a one-row band of width %d needs %d B of LDS beside the %d-point grid", p->width, plan.lds, h->P);
    if (n == 0 || (!out && !d_out)) return 0;
    HIPCHECK(hipSetDevice(h->device));
    const size_t npx = (size_t)p->width * p->height, C = format == CLOTHHIP_IMG_RGBD ? 4 : 3, img_bytes = npx * C;
    const size_t chunk = (size_t)render_obs_chunk(npx), cmax = (size_t)n < chunk ? (size_t)n : chunk;
    const bool need_depth = format != CLOTHHIP_IMG_RGB, have_flags = valid || swap;
    if (!d_out) if (int rc = h->ro.d_ro_img.reserve(cmax * img_bytes)) return rc;
    if (need_depth) if (int rc = h->ro.d_ro_depth.reserve(cmax * npx * 4)) return rc;
    if (source == CLOTHHIP_OBS_HOST) if (int rc = h->ro.d_ro_src.reserve(cmax * 3 * h->P * 4)) return rc;
    if (have_flags) if (int rc = h->ro.d_ro_flags.reserve(2 * chunk)) return rc;
    RenderObsArgs a;
    memset(&a, 0, sizeof(a));
    fill_scene(a.s, h, p);
    a.rows = plan.rows; a.bands = plan.bands; a.format = format; a.C = (int)C;
    const bool soa = source == CLOTHHIP_OBS_STATE;
    a.src_stride = soa ? 3LL * h->Ppad : 3LL * h->P;
    a.depth = need_depth ? (float *)h->ro.d_ro_depth : nullptr;
    const unsigned wg_per_image = h->dbg.render_walk ? 1 : plan.bands;      // one workgroup per band, or one that walks them all
    HIPCHECK(hipFuncSetAttribute((const void *)k_render_obs<float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHECK(hipFuncSetAttribute((const void *)k_render_obs<float, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHECK(hipFuncSetAttribute((const void *)k_render_obs<double, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        const size_t m = (size_t)n - i0 < chunk ? (size_t)n - i0 : chunk;
        if (have_flags) {
            uint8_t *fl = (uint8_t *)h->ro.d_ro_flags;
            if (valid) HIPCHECK(hipMemcpyAsync(fl, valid + i0, m, hipMemcpyHostToDevice, h->stream));
            if (swap) HIPCHECK(hipMemcpyAsync(fl + chunk, swap + i0, m, hipMemcpyHostToDevice, h->stream));
            a.valid = valid ? fl : nullptr; a.swap = swap ? fl + chunk : nullptr;
        }
        a.out = d_out ? (uint8_t *)d_out + i0 * img_bytes : (uint8_t *)h->ro.d_ro_img;
        const dim3 grid((unsigned)m, wg_per_image);
        if (soa) {
            by_precision(h, [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL((k_render_obs<T, false>), grid, dim3(256), plan.lds, h->stream, (const T *)h->d_pos + i0 * 3 * h->Ppad, a);
            });
        } else {
            const float *rows = d_table ? (const float *)d_table + i0 * 3 * h->P : (const float *)h->ro.d_ro_src;
            if (!d_table) HIPCHECK(hipMemcpyAsync(h->ro.d_ro_src, obs_host + i0 * 3 * h->P, m * 3 * h->P * 4, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL((k_render_obs<float, true>), grid, dim3(256), plan.lds, h->stream, rows, a);
        }
        HIPCHECK(hipGetLastError());
        if (need_depth) {
            hipLaunchKernelGGL(k_depth8, dim3((unsigned)m), dim3(256), 0, h->stream, a);
            HIPCHECK(hipGetLastError());
        }
        if (out && !d_out) HIPCHECK(hipMemcpyAsync(out + i0 * img_bytes, h->ro.d_ro_img, m * img_bytes, hipMemcpyDeviceToHost, h->stream));
    }
    if (out && d_out) HIPCHECK(hipMemcpyAsync(out, d_out, (size_t)n * img_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_selftest_depth8(const float *depth, int32_t n_images, int64_t npx, uint8_t *out) {
    if (n_images < 0 || npx < 0 || ((!depth || !out) && n_images > 0 && npx > 0)) return fail(CLOTHHIP_EINVAL, "bad argument");
    for (int64_t e = 0; e < n_images; e++) {
        const float *d = depth + e * npx;
        if (npx == 0) break;
        float lo = d[0], hi = d[0];
        for (int64_t i = 1; i < npx; i++) { lo = fminf(lo, d[i]); hi = fmaxf(hi, d[i]); }
        for (int64_t i = 0; i < npx; i++) out[e * npx + i] = depth8(d[i], lo, hi);
    }
    return 0;
}

extern "C" int clothhip_selftest_render_plan(const ClothParams *p, int32_t width, int32_t height, int32_t out[4]) {
    if (int rc = check_params(p)) return rc;
    if (!out || width < 1 || height < 1) return fail(CLOTHHIP_EINVAL, "bad argument");
    const int P = p->n_side * p->n_side, Ppad = (P + 63) / 64 * 64;           // as init_host_fields pads the grid
    const RenderPlan plan = render_plan(Ppad, width, height, read_debug_knobs().render_lds_kib * 1024);
    out[0] = plan.rows; out[1] = plan.bands; out[2] = plan.lds; out[3] = plan.fits ? 1 : 0;
    return 0;
}
