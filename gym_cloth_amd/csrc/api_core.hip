// api_core.hip -- libclothhip.so's C ABI (include/clothhip.h), first of six units around api_handle.hpp: the library and a handle's life --
// errors and versions, the reference's grid on the host, create / destroy / getters, raw device buffers. Host side only orchestrates:
// tables, uploads, launches; api_state.hip, api_run.hip, api_observe.hip, api_policy.hip and api_selftest.hip hold the rest.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <new>

#include "api_handle.hpp"

extern "C" const char *clothhip_last_error(void) { return g_err.c_str(); }
extern "C" int clothhip_abi_version(void) { return CLOTHHIP_ABI_VERSION; }

extern "C" int clothhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int clothhip::check_params(const ClothParams *p) {
    if (!p) return fail(CLOTHHIP_EINVAL, "params is NULL");
    if (p->n_side < 3 || p->n_side > MAX_SIDE) return fail(CLOTHHIP_EINVAL, "n_side %d outside [3,%d]", p->n_side, MAX_SIDE);
    if (!(p->width > 0) || !(p->height > 0)) return fail(CLOTHHIP_EINVAL, "width/height must be > 0");
    if (p->height != p->width) return fail(CLOTHHIP_EINVAL, "height must equal width (cloth.pyx:91)");
    if (p->frames_per_sec <= 0 || p->simulation_steps <= 0) return fail(CLOTHHIP_EINVAL, "frames_per_sec/simulation_steps must be > 0");
    if (!(p->density > 0) || !(p->thickness > 0)) return fail(CLOTHHIP_EINVAL, "density/thickness must be > 0");
    return 0;
}

// ---- host restatement of Cloth.__init__ grid + rest lengths (cloth.pyx:92-146, :411-417) -----------
extern "C" int clothhip_init_grid(const ClothParams *p, int32_t tier, int32_t init_side,
                                  const double *rand_draws, double *pos, double *rest) {
    if (int rc = check_params(p)) return rc;
    if (tier < 1 || tier > 3) return fail(CLOTHHIP_EINVAL, "init tier %d (ValueError, cloth.pyx:131-132)", tier);
    if (tier == 2 && !rand_draws) return fail(CLOTHHIP_EINVAL, "tier 2 needs the P rand() draws");
    if (!pos) return fail(CLOTHHIP_EINVAL, "pos is NULL");
    const int N = p->n_side;
    const double dx = p->width * 1.0 / (N - 1), dy = p->height * 1.0 / (N - 1);   // cloth.pyx:55-56
    for (int r = 0; r < N; r++)
        for (int c = 0; c < N; c++) {
            const int i = r * N + c;
            double x, y, z;
            if (tier == 2) {
                double noise = rand_draws[i] * 0.01 - 0.005;           // cloth.pyx:101
                if (r == 0) noise = 0;                                 // :102-103
                x = init_side ? 0.0 + std::fabs(noise) : 1.0 - std::fabs(noise);   // :104-107
                y = dx * c; z = dy * r;                                // :109-110
            } else {
                x = dx * r; y = dy * c; z = 0.0;                       // :122-124
            }
            pos[3 * i] = x; pos[3 * i + 1] = y; pos[3 * i + 2] = z;
        }
    if (rest) {
        Topology t = build_topology(N);
        for (int s = 0; s < t.S; s++) {
            const double *A = pos + 3 * t.a[s], *B = pos + 3 * t.b[s];
            const double ux = A[0] - B[0], uy = A[1] - B[1], uz = A[2] - B[2];
            rest[s] = std::sqrt(ux * ux + uy * uy + uz * uz);         // cloth.pyx:417 via :17-18
        }
    }
    return 0;
}

extern "C" int clothhip_spring_topology(const ClothParams *p, int32_t *a, int32_t *b, uint8_t *type) {
    if (int rc = check_params(p)) return rc;
    Topology t = build_topology(p->n_side);
    if (a) memcpy(a, t.a.data(), sizeof(int32_t) * t.S);
    if (b) memcpy(b, t.b.data(), sizeof(int32_t) * t.S);
    if (type) memcpy(type, t.type.data(), t.S);
    return 0;
}

extern "C" int clothhip_create(const ClothParams *params, int32_t n_envs, int32_t device, int32_t precision,
                               clothhip_handle **out) {
    if (!out) return fail(CLOTHHIP_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = check_params(params)) return rc;
    if (n_envs < 1) return fail(CLOTHHIP_EINVAL, "n_envs must be >= 1");
    if (precision != CLOTHHIP_F64 && precision != CLOTHHIP_F32) return fail(CLOTHHIP_EINVAL, "precision must be 0 (f64) or 1 (f32)");
    int ndev = clothhip_device_count();
    if (ndev <= 0) return fail(CLOTHHIP_ENODEV, "no HIP device visible: libclothhip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(CLOTHHIP_EINVAL, "device %d outside [0,%d)", device, ndev);
    HIPCHECK(hipSetDevice(device));
    std::unique_ptr<clothhip_handle> owner(new (std::nothrow) clothhip_handle());      // (destroyed, with all it holds, by every early return)
    clothhip_handle *const h = owner.get();
    if (!h) return fail(CLOTHHIP_ENOMEM, "out of host memory");
    h->device = device;
    init_host_fields(h, *params, n_envs, precision);
    h->mat.assign((size_t)n_envs, material_of(*params));
    std::vector<double> levels = build_grab_levels(params->height, params->thickness);
    h->n_grab_levels = (int)levels.size();
    HIPCHECK(hipStreamCreateWithFlags(&h->stream.v, hipStreamNonBlocking));
    HIPCHECK(hipEventCreate(&h->ev0.v));
    HIPCHECK(hipEventCreate(&h->ev1.v));
    const size_t E = h->E;
    int rc = 0;      // (the first allocation that fails ends them)
    auto take = [&rc](auto &buf, size_t bytes) { if (!rc) rc = buf.reserve(bytes); };
    take(h->d_pos, E * 3 * h->Ppad * h->tsz); take(h->d_prev, E * 3 * h->Ppad * h->tsz); take(h->d_rest, E * h->Spad * h->tsz);
    take(h->d_cnt, E * h->Ppad); take(h->d_active, E); take(h->d_tear, E * 4); take(h->d_exec, E * 4); take(h->d_ngrab, E * 4); take(h->d_stats, E * 64);
    take(h->d_sched, E * sizeof(ClothSchedule)); take(h->h_sched, E * sizeof(ClothSchedule));
    take(h->d_gather, h->gather.size() * 4); take(h->d_wt_ent, (size_t)h->Spad * 4); take(h->d_wt_dep, (size_t)h->Spad * 8); take(h->launch.d_lstc, (size_t)h->Ppad * 16);
    take(h->d_levels, (levels.size() + 1) * 8); take(h->d_xy, E * 2 * 8); take(h->d_radius, E * 8); take(h->d_cov, E * 8); take(h->d_vinv, E * 8);
    take(h->d_oob, E); take(h->d_hcnt, E * 4); take(h->epi.d_resume, E * sizeof(EpResume));
    take(h->d_flat, (size_t)3 * h->Ppad * h->tsz); take(h->d_flat_rest, (size_t)h->Spad * h->tsz);
    if (rc) return rc;
    HIPCHECK(hipMemset(h->d_stats, 0, E * 64));
    HIPCHECK(hipMemset(h->launch.d_lstc, 0, (size_t)h->Ppad * 16));
    HIPCHECK(hipMemset(h->epi.d_resume, 0, E * sizeof(EpResume)));
    HIPCHECK(hipMemcpy(h->d_gather, h->gather.data(), h->gather.size() * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(h->d_wt_ent, h->wt.ent.data(), (size_t)h->Spad * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(h->d_wt_dep, h->wt.dep.data(), (size_t)h->Spad * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(h->d_rest, 0, E * h->Spad * h->tsz));
    if (!levels.empty()) HIPCHECK(hipMemcpy(h->d_levels, levels.data(), levels.size() * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(h->d_exec, 0, E * 4));
    if ((rc = plan_steppers(h))) return rc;
    // initial state: flat tier-1 grid for every env, shared rest table
    std::vector<double> pos((size_t)h->P * 3), rest(h->S);
    if ((rc = clothhip_init_grid(params, 1, 0, nullptr, pos.data(), rest.data()))) return rc;
    h->flat_rest = rest;
    std::vector<double> all((size_t)h->E * h->P * 3);
    for (int e = 0; e < h->E; e++) memcpy(all.data() + (size_t)e * h->P * 3, pos.data(), sizeof(double) * h->P * 3);
    std::vector<uint8_t> pin((size_t)h->E * h->P, 0);
    if ((rc = clothhip_set_state(h, 0, h->E, all.data(), all.data(), pin.data(), rest.data(), CLOTHHIP_REST_SHARED))) return rc;
    // the flat grid and its rest table stay on the device for clothhip_reset_flat / the in-kernel episode reset
    if (hipMemcpy(h->d_flat, h->d_pos, (size_t)3 * h->Ppad * h->tsz, hipMemcpyDeviceToDevice) != hipSuccess ||
        hipMemcpy(h->d_flat_rest, h->d_rest, (size_t)h->Spad * h->tsz, hipMemcpyDeviceToDevice) != hipSuccess)
        return fail(CLOTHHIP_EHIP, "copying the flat-grid template failed");
    *out = owner.release();
    return 0;
}

extern "C" int clothhip_destroy(clothhip_handle *h) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
    return 0;
}

extern "C" int clothhip_num_points(const clothhip_handle *h) { return h ? h->P : fail(CLOTHHIP_EINVAL, "handle is NULL"); }
extern "C" int clothhip_num_springs(const clothhip_handle *h) { return h ? h->S : fail(CLOTHHIP_EINVAL, "handle is NULL"); }
extern "C" int clothhip_num_envs(const clothhip_handle *h) { return h ? h->E : fail(CLOTHHIP_EINVAL, "handle is NULL"); }
extern "C" int clothhip_precision(const clothhip_handle *h) { return h ? h->precision : fail(CLOTHHIP_EINVAL, "handle is NULL"); }
extern "C" void *clothhip_stream(clothhip_handle *h) { return h ? (void *)h->stream : nullptr; }

// no call that touches what an episode launch reads or writes between clothhip_run_actions_begin and _end
int clothhip::check_idle(const clothhip_handle *h) { return h->epi.last.pending ? fail(CLOTHHIP_ESTATE, "clothhip_run_actions_begin still in flight: call clothhip_run_actions_end first") : 0; }

extern "C" int clothhip_fused_supported(const clothhip_handle *h) { return h ? (fused_supported(*h) ? 1 : 0) : fail(CLOTHHIP_EINVAL, "handle is NULL"); }

// ---- raw device buffers on the handle's device (collective staging of the multi-GPU driver) ------------------
extern "C" int clothhip_device_alloc(clothhip_handle *h, uint64_t nbytes, void **d_out) {
    if (!h || !d_out || nbytes == 0) return fail(CLOTHHIP_EINVAL, "bad argument");
    HIPCHECK(hipSetDevice(h->device));
    hipError_t err = hipMalloc(d_out, (size_t)nbytes);
    if (err != hipSuccess) return fail(hip_status(err), "hipMalloc(%llu) failed: %s",
                                       (unsigned long long)nbytes, hipGetErrorString(err));
    return 0;
}
extern "C" int clothhip_device_free(clothhip_handle *h, void *d) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (d) HIPCHECK(hipFree(d));
    return 0;
}
extern "C" int clothhip_device_upload(clothhip_handle *h, void *d_dst, const void *src, uint64_t nbytes) {
    if (!h || !d_dst || !src) return fail(CLOTHHIP_EINVAL, "NULL argument");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(d_dst, src, (size_t)nbytes, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // the host buffer is never retained
    return 0;
}
extern "C" int clothhip_device_download(clothhip_handle *h, void *dst, const void *d_src, uint64_t nbytes) {
    if (!h || !dst || !d_src) return fail(CLOTHHIP_EINVAL, "NULL argument");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(dst, d_src, (size_t)nbytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_debug_stats(clothhip_handle *h, int32_t *stats) {
    if (!h || !stats) return fail(CLOTHHIP_EINVAL, "NULL argument");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipMemcpy(stats, h->d_stats, (size_t)h->E * 64, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" double clothhip_last_kernel_ms(clothhip_handle *h) {
    if (!h || !h->have_timing) return -1.0;
    if (hipSetDevice(h->device) != hipSuccess) return -1.0;
    if (hipEventSynchronize(h->ev1) != hipSuccess) return -1.0;
    float ms = -1.f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) return -1.0;
    return (double)ms;
}
