// api_state.hip -- the cloths of a handle, changed and read from outside the stepper: state up- and download, resets, tear flags, gripper,
// pins, per-env materials, forks; and dropping what a time slice left in flight, which every such change does.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "api_handle.hpp"
#include "cloth_state_kernels.hpp"

// Any state change from outside the episode launches (uploads, resets, grabs, raw schedules) voids the operation a time slice
// left in flight -- for the envs that call touches, and only for them: the parked operations of the others continue in the next
// episode launch. d_mask: device mask [E] (nullptr = all); d_sched: device schedules whose active flag selects (or nullptr).
int clothhip::drop_in_flight(clothhip_handle *h, const uint8_t *d_mask, const ClothSchedule *d_sched) {
    if (!h->epi.d_resume) return 0;
    hipLaunchKernelGGL(k_clear_resume, dim3((h->E + 255) / 256), dim3(256), 0, h->stream, h->epi.d_resume, d_mask, d_sched, h->E);
    HIPCHECK(hipGetLastError());
    return 0;
}
static int drop_in_flight_range(clothhip_handle *h, int env0, int n) {
    if (h->epi.d_resume && n > 0) HIPCHECK(hipMemsetAsync(h->epi.d_resume + env0, 0, (size_t)n * sizeof(EpResume), h->stream));
    return 0;
}

static int check_range(const clothhip_handle *h, int env0, int n) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (env0 < 0 || n < 0 || env0 + n > h->E) return fail(CLOTHHIP_EINVAL, "env range [%d,%d) outside [0,%d)", env0, env0 + n, h->E);
    return 0;
}

// [n][P][3] double  ->  [n][3][Ppad] T
template <typename T> static void aos_to_soa(const double *src, T *dst, int n, int P, int Ppad) {
    for (int e = 0; e < n; e++) {
        const double *s = src + (size_t)e * P * 3;
        T *d = dst + (size_t)e * 3 * Ppad;
        for (int i = 0; i < P; i++) { d[i] = (T)s[3 * i]; d[Ppad + i] = (T)s[3 * i + 1]; d[2 * Ppad + i] = (T)s[3 * i + 2]; }
        for (int i = P; i < Ppad; i++) { d[i] = 0; d[Ppad + i] = 0; d[2 * Ppad + i] = 0; }
    }
}
template <typename T> static void soa_to_aos(const T *src, double *dst, int n, int P, int Ppad) {
    for (int e = 0; e < n; e++) {
        const T *s = src + (size_t)e * 3 * Ppad;
        double *d = dst + (size_t)e * P * 3;
        for (int i = 0; i < P; i++) { d[3 * i] = (double)s[i]; d[3 * i + 1] = (double)s[Ppad + i]; d[3 * i + 2] = (double)s[2 * Ppad + i]; }
    }
}

extern "C" int clothhip_set_state(clothhip_handle *h, int32_t env0, int32_t n, const double *pos, const double *prev,
                                  const uint8_t *pinned, const double *rest, int32_t flags) {
    if (int rc = check_range(h, env0, n)) return rc;
    if (int rc = drop_in_flight_range(h, env0, n)) return rc;
    const bool rest_shared = (flags & CLOTHHIP_REST_SHARED) != 0;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    const size_t per = (size_t)3 * h->Ppad * h->tsz;
    for (int pass = 0; pass < 2; pass++) {
        const double *src = pass == 0 ? pos : prev;
        if (!src) continue;
        h->stage.resize(per * n);
        by_precision(h, [&](auto t) { aos_to_soa(src, (decltype(t) *)h->stage.data(), n, h->P, h->Ppad); });
        char *dst = (char *)(pass == 0 ? h->d_pos : h->d_prev) + per * env0;
        HIPCHECK(hipMemcpy(dst, h->stage.data(), per * n, hipMemcpyHostToDevice));
    }
    if (pos && !(flags & CLOTHHIP_KEEP_TEAR)) HIPCHECK(hipMemset(h->d_tear + env0, 0, (size_t)n * 4));
    if (pinned) {
        std::vector<uint8_t> c((size_t)n * h->Ppad, 0);
        for (int e = 0; e < n; e++)
            for (int i = 0; i < h->P; i++) c[(size_t)e * h->Ppad + i] = pinned[(size_t)e * h->P + i] ? 1 : 0;
        HIPCHECK(hipMemcpy(h->d_cnt + (size_t)env0 * h->Ppad, c.data(), c.size(), hipMemcpyHostToDevice));
    }
    if (rest) {
        if (!rest_shared && h->rest_stride == 0 && !(env0 == 0 && n == h->E)) {
            // switching from the shared table to per-env tables: replicate the shared one first
            std::vector<unsigned char> one((size_t)h->Spad * h->tsz);
            HIPCHECK(hipMemcpy(one.data(), h->d_rest, one.size(), hipMemcpyDeviceToHost));
            for (int e = 1; e < h->E; e++)
                HIPCHECK(hipMemcpy((char *)h->d_rest + (size_t)e * one.size(), one.data(), one.size(), hipMemcpyHostToDevice));
        }
        const int nt = rest_shared ? 1 : n;
        std::vector<unsigned char> buf((size_t)nt * h->Spad * h->tsz, 0);
        for (int e = 0; e < nt; e++)
            for (int p = 0; p < h->S; p++) {
                const int i = h->wt.slot_of[p];                               // list order -> table slot (empty slots stay 0)
                const double v = rest[(size_t)e * h->S + p];
                by_precision(h, [&](auto t) { ((decltype(t) *)buf.data())[(size_t)e * h->Spad + i] = (decltype(t))v; });
            }
        char *dst = (char *)h->d_rest + (rest_shared ? 0 : (size_t)env0 * h->Spad * h->tsz);
        HIPCHECK(hipMemcpy(dst, buf.data(), buf.size(), hipMemcpyHostToDevice));
        h->rest_stride = rest_shared ? 0 : h->Spad;
        h->launch.lean_dirty = true;
        if (rest_shared) h->fork.shared_rest.swap(buf);       // (clothhip_fork compares shared tables by this mirror)
    }
    return 0;
}

extern "C" int clothhip_get_state(clothhip_handle *h, int32_t env0, int32_t n, double *pos, double *prev, uint8_t *pinned) {
    if (int rc = check_range(h, env0, n)) return rc;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    const size_t per = (size_t)3 * h->Ppad * h->tsz;
    for (int pass = 0; pass < 2; pass++) {
        double *dst = pass == 0 ? pos : prev;
        if (!dst) continue;
        h->stage.resize(per * n);
        const char *src = (const char *)(pass == 0 ? h->d_pos : h->d_prev) + per * env0;
        HIPCHECK(hipMemcpy(h->stage.data(), src, per * n, hipMemcpyDeviceToHost));
        by_precision(h, [&](auto t) { soa_to_aos((const decltype(t) *)h->stage.data(), dst, n, h->P, h->Ppad); });
    }
    if (pinned) {
        std::vector<uint8_t> c((size_t)n * h->Ppad);
        HIPCHECK(hipMemcpy(c.data(), h->d_cnt + (size_t)env0 * h->Ppad, c.size(), hipMemcpyDeviceToHost));
        for (int e = 0; e < n; e++)
            for (int i = 0; i < h->P; i++) pinned[(size_t)e * h->P + i] = c[(size_t)e * h->Ppad + i] ? 1 : 0;
    }
    return 0;
}

extern "C" int clothhip_get_rest(clothhip_handle *h, int32_t env0, int32_t n, double *rest) {
    if (int rc = check_range(h, env0, n)) return rc;
    if (!rest) return fail(CLOTHHIP_EINVAL, "rest is NULL");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    std::vector<unsigned char> buf((size_t)h->Spad * h->tsz);
    for (int e = 0; e < n; e++) {
        const char *src = (const char *)h->d_rest + (size_t)(env0 + e) * h->rest_stride * h->tsz;   // stride 0: the shared table
        if (e == 0 || h->rest_stride) HIPCHECK(hipMemcpy(buf.data(), src, buf.size(), hipMemcpyDeviceToHost));
        for (int p = 0; p < h->S; p++) {        // table slot -> list order (Spring.rest_length of cloth.springs[p])
            const int i = h->wt.slot_of[p];
            rest[(size_t)e * h->S + p] = h->precision == CLOTHHIP_F64 ? ((const double *)buf.data())[i] : (double)((const float *)buf.data())[i];
        }
    }
    return 0;
}

extern "C" int clothhip_reset_flat(clothhip_handle *h, const uint8_t *mask) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    HIPCHECK(hipSetDevice(h->device));
    if (mask) HIPCHECK(hipMemcpyAsync(h->d_active, mask, (size_t)h->E, hipMemcpyHostToDevice, h->stream));
    if (int rc = drop_in_flight(h, mask ? h->d_active : nullptr, nullptr)) return rc;
    by_precision(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_reset_flat<T>, dim3(h->E), dim3(256), 0, h->stream, (T *)h->d_pos, (T *)h->d_prev, h->d_cnt,
                           h->d_tear, (const T *)h->d_flat, mask ? h->d_active : nullptr, h->Ppad, (T *)h->d_rest,
                           (const T *)h->d_flat_rest, h->rest_stride, h->Spad);
    });
    // (the LEAN palette verdict stands: a shared rest table is not touched here, and per-env tables rule the variant out anyway)
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_get_tear(clothhip_handle *h, uint8_t *tear) {
    if (!h || !tear) return fail(CLOTHHIP_EINVAL, "NULL argument");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    std::vector<int32_t> t(h->E);
    HIPCHECK(hipMemcpy(t.data(), h->d_tear, (size_t)h->E * 4, hipMemcpyDeviceToHost));
    for (int e = 0; e < h->E; e++) tear[e] = t[e] ? 1 : 0;
    return 0;
}

extern "C" int clothhip_set_tear(clothhip_handle *h, const uint8_t *tear) {
    if (!h || !tear) return fail(CLOTHHIP_EINVAL, "NULL argument");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    std::vector<int32_t> t(h->E);
    for (int e = 0; e < h->E; e++) t[e] = tear[e] ? 1 : 0;
    HIPCHECK(hipMemcpy(h->d_tear, t.data(), (size_t)h->E * 4, hipMemcpyHostToDevice));
    return 0;
}

static int do_grab(clothhip_handle *h, const double *xy, const double *radius, const uint8_t *active,
                   int32_t *n_grabbed, int top) {
    if (!h || !xy) return fail(CLOTHHIP_EINVAL, "NULL argument");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(h->d_xy, xy, (size_t)h->E * 16, hipMemcpyHostToDevice, h->stream));
    if (radius) HIPCHECK(hipMemcpyAsync(h->d_radius, radius, (size_t)h->E * 8, hipMemcpyHostToDevice, h->stream));
    if (active) HIPCHECK(hipMemcpyAsync(h->d_active, active, (size_t)h->E, hipMemcpyHostToDevice, h->stream));
    if (int rc = drop_in_flight(h, active ? h->d_active : nullptr, nullptr)) return rc;
    by_precision(h, [&](auto t) {
        using T = decltype(t);
        GrabArgs<T> a{(const T *)h->d_pos, h->d_cnt, h->d_xy, radius ? h->d_radius : nullptr,
                      active ? h->d_active : nullptr, h->d_ngrab, h->d_levels, h->n_grab_levels, h->P, h->Ppad, top,
                      h->prm.grip_radius, 2 * h->prm.thickness};
        hipLaunchKernelGGL(k_grab<T>, dim3(h->E), dim3(64), 0, h->stream, a);
    });
    HIPCHECK(hipGetLastError());
    if (n_grabbed) HIPCHECK(hipMemcpyAsync(n_grabbed, h->d_ngrab, (size_t)h->E * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_grab_top(clothhip_handle *h, const double *xy, const double *radius, const uint8_t *active, int32_t *n_grabbed) {
    return do_grab(h, xy, radius, active, n_grabbed, 1);
}
extern "C" int clothhip_grab(clothhip_handle *h, const double *xy, const double *radius, const uint8_t *active, int32_t *n_grabbed) {
    return do_grab(h, xy, radius, active, n_grabbed, 0);
}

extern "C" int clothhip_release(clothhip_handle *h, const uint8_t *active) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    HIPCHECK(hipSetDevice(h->device));
    if (active) HIPCHECK(hipMemcpyAsync(h->d_active, active, (size_t)h->E, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_release, dim3(h->E), dim3(64), 0, h->stream, h->d_cnt, active ? h->d_active : nullptr, h->Ppad);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_pin_points(clothhip_handle *h, int32_t env, const int32_t *idx, int32_t n) {
    if (int rc = check_range(h, env, 1)) return rc;
    if (n < 0 || (n > 0 && !idx)) return fail(CLOTHHIP_EINVAL, "bad idx/n");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    std::vector<uint8_t> c(h->Ppad);
    HIPCHECK(hipMemcpy(c.data(), h->d_cnt + (size_t)env * h->Ppad, c.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; k++) {
        if (idx[k] < 0 || idx[k] >= h->P) return fail(CLOTHHIP_EINVAL, "point index %d outside [0,%d)", idx[k], h->P);
        c[idx[k]] |= CNT_EXT_PIN;
    }
    HIPCHECK(hipMemcpy(h->d_cnt + (size_t)env * h->Ppad, c.data(), c.size(), hipMemcpyHostToDevice));
    return 0;
}

// the rules check_params applies to the fields a material overrides: the material put into the handle's parameters must pass them
int clothhip::check_material(const ClothParams &prm, const ClothMaterial &m, int idx) {
    ClothParams p = prm;
    p.density = m.density; p.ks = m.ks; p.damping = m.damping; p.plane_friction = m.plane_friction; p.tear_thresh = m.tear_thresh; p.gravity = m.gravity;
    if (check_params(&p)) return fail(CLOTHHIP_EINVAL, "material %d: %s", idx, std::string(g_err).c_str());
    return 0;
}

// the physics parameters of a handle in the form the one derivation of the stepper's constants takes (cloth_common.hpp: make_consts)
SpecPhys clothhip::phys_of(const ClothParams &p) {
    return SpecPhys{p.width, p.height, p.density, p.ks, p.damping, p.thickness, p.plane_friction, p.tear_thresh, p.gravity, p.minimum_z, p.frames_per_sec, p.simulation_steps};
}
// ... and of one env of it that holds material m: the material's six fields over the handle's (cloth.pyx:175-186)
SpecPhys clothhip::phys_of(const ClothParams &p, const ClothMaterial &m) {
    SpecPhys s = phys_of(p);
    s.density = m.density; s.ks = m.ks; s.damping = m.damping; s.plane_friction = m.plane_friction; s.tear_thresh = m.tear_thresh; s.gravity = m.gravity;
    return s;
}
ClothMaterial clothhip::material_of(const ClothParams &p) { return ClothMaterial{p.density, p.ks, p.damping, p.plane_friction, p.tear_thresh, p.gravity}; }

// ---- per-env materials -------------------------------------------------------------------------------------------------------------------
// The one path by which a handle's materials change (clothhip_set_material, clothhip_fork): `next` becomes the host vector, n_mixed follows, and
// while any env differs from the handle's parameters the device's table is (created and) rebuilt whole -- unless `upload` is false: the
// caller has the device copy the records it changes (a fork between two handles whose tables are both live).
static size_t mat_record_bytes(const clothhip_handle *h) { return h->precision == CLOTHHIP_F64 ? sizeof(DevConsts<double>) : sizeof(DevConsts<float>); }
static int apply_materials(clothhip_handle *h, std::vector<ClothMaterial> &next, bool upload) {
    const ClothMaterial own = material_of(h->prm);
    int mixed = 0;
    for (const ClothMaterial &v : next) mixed += memcmp(&v, &own, sizeof(own)) != 0 ? 1 : 0;
    HIPCHECK(hipSetDevice(h->device));
    if (mixed && upload) {
        // the device's table, rebuilt whole: every env's record by the ONE derivation (make_consts), in the handle's precision
        const size_t bytes = (size_t)h->E * mat_record_bytes(h);
        if (int rc = h->d_mat.reserve(bytes)) return rc;
        std::vector<unsigned char> buf(bytes);
        by_precision(h, [&](auto t) {
            using T = decltype(t);
            DevConsts<T> *d = (DevConsts<T> *)buf.data();
            for (int e = 0; e < h->E; e++) d[e] = make_consts<T>(phys_of(h->prm, next[e]), h->N);
        });
        HIPCHECK(hipStreamSynchronize(h->stream));     // (a launch of clothhip_run_async may still be reading the table)
        HIPCHECK(hipMemcpy(h->d_mat, buf.data(), bytes, hipMemcpyHostToDevice));
    }
    h->mat.swap(next);
    h->n_mixed = mixed;
    return 0;
}

extern "C" int clothhip_set_material(clothhip_handle *h, int32_t env0, int32_t n, const ClothMaterial *m) {
    if (int rc = check_range(h, env0, n)) return rc;
    if (int rc = check_idle(h)) return rc;
    const ClothMaterial own = material_of(h->prm);
    for (int e = 0; m && e < n; e++)
        if (int rc = check_material(h->prm, m[e], e)) return rc;
    std::vector<ClothMaterial> next = h->mat;
    for (int e = 0; e < n; e++) next[(size_t)env0 + e] = m ? m[e] : own;
    return apply_materials(h, next, true);
}

extern "C" int clothhip_get_material(clothhip_handle *h, int32_t env0, int32_t n, ClothMaterial *m) {
    if (int rc = check_range(h, env0, n)) return rc;
    if (!m) return fail(CLOTHHIP_EINVAL, "m is NULL");
    for (int e = 0; e < n; e++) m[e] = h->mat[(size_t)env0 + e];
    return 0;
}

// ---- clothhip_fork: whole cloths between env slots and handles, on the device ---------------------------------------------------------------
// the fields of ClothParams a material does not override, bit for bit: two handles that agree in them derive the same DevConsts record from
// the same material, so a fork may copy the record on the device instead of deriving it again
static bool same_non_material_params(const ClothParams &a, const ClothParams &b) {
    ClothParams x = a, y = b;
    for (ClothParams *p : {&x, &y}) { p->density = 1; p->ks = 0; p->damping = 0; p->plane_friction = 0; p->tear_thresh = 0; p->gravity = 0; p->_pad = 0; }
    return memcmp(&x, &y, sizeof(x)) == 0;
}

extern "C" int clothhip_fork(clothhip_handle *dst, const int32_t *dst_env, clothhip_handle *src, const int32_t *src_env, int32_t n, int32_t flags) {
    if (!dst || !src) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (n < 0 || (n > 0 && (!dst_env || !src_env))) return fail(CLOTHHIP_EINVAL, "bad index lists");
    if (flags & ~CLOTHHIP_FORK_STATE_ONLY) return fail(CLOTHHIP_EINVAL, "unknown flags %d", flags);
    if (dst->device != src->device) return fail(CLOTHHIP_EINVAL, "fork across devices (%d <- %d)", dst->device, src->device);
    if (dst->precision != src->precision) return fail(CLOTHHIP_EINVAL, "fork between handles of different precision");
    if (dst->N != src->N) return fail(CLOTHHIP_EINVAL, "fork between grids of %d and %d points a side", dst->N, src->N);
    if (int rc = check_idle(dst)) return rc;
    if (int rc = check_idle(src)) return rc;
    {
        std::vector<uint8_t> seen((size_t)dst->E, 0);
        for (int j = 0; j < n; j++) {
            if (dst_env[j] < 0 || dst_env[j] >= dst->E) return fail(CLOTHHIP_EINVAL, "dst_env[%d] = %d outside [0,%d)", j, dst_env[j], dst->E);
            if (src_env[j] < 0 || src_env[j] >= src->E) return fail(CLOTHHIP_EINVAL, "src_env[%d] = %d outside [0,%d)", j, src_env[j], src->E);
            if (seen[dst_env[j]]) return fail(CLOTHHIP_EINVAL, "env %d occurs twice in dst_env", dst_env[j]);
            seen[dst_env[j]] = 1;
        }
        for (int j = 0; dst == src && j < n; j++)
            if (seen[src_env[j]]) return fail(CLOTHHIP_EINVAL, "env %d is both a source and a destination of one fork", src_env[j]);
    }
    if (n == 0) return 0;
    // (two uniform handles of one material: every destination env already holds what its source holds -- nothing to do for the materials)
    const ClothMaterial own_dst = material_of(dst->prm), own_src = material_of(src->prm);
    const bool with_mat = !(flags & CLOTHHIP_FORK_STATE_ONLY) &&
                          !(dst->n_mixed == 0 && src->n_mixed == 0 && memcmp(&own_dst, &own_src, sizeof(own_dst)) == 0);
    std::vector<ClothMaterial> next;
    if (with_mat) {
        next = dst->mat;
        for (int j = 0; j < n; j++) {
            if (int rc = check_material(dst->prm, src->mat[src_env[j]], j)) return rc;
            next[dst_env[j]] = src->mat[src_env[j]];
        }
    }
    HIPCHECK(hipSetDevice(dst->device));
    if (int rc = dst->fork.d_fork_idx.reserve((size_t)2 * n * 4)) return rc;
    if (int rc = dst->fork.h_fork_idx.reserve((size_t)2 * n * 4)) return rc;
    if (dst->stream != src->stream) {                  // the copy reads what the source's stream has enqueued so far
        if (!dst->fork.ev_fork) HIPCHECK(hipEventCreateWithFlags(&dst->fork.ev_fork.v, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(dst->fork.ev_fork, src->stream));
        HIPCHECK(hipStreamWaitEvent(dst->stream, dst->fork.ev_fork, 0));
    }
    // materials: the host vector, n_mixed and so spec_ns by clothhip_set_material's path; the records themselves on the device when both
    // tables are live and derived under the same parameters, else the destination's table is rebuilt whole as set_material does
    bool mat_on_device = false;
    if (with_mat) {
        mat_on_device = dst->n_mixed > 0 && src->n_mixed > 0 && dst->d_mat && src->d_mat && same_non_material_params(dst->prm, src->prm);
        if (int rc = apply_materials(dst, next, !mat_on_device)) return rc;
        if (dst->n_mixed == 0) mat_on_device = false;
    }
    // rest lengths: two handles that each share ONE table keep doing so when the tables are bitwise equal (the mirrors of what set_state
    // uploaded); in every other case the destination takes per-env tables, as set_state does when it is given per-env rest
    const size_t rest_bytes = (size_t)dst->Spad * dst->tsz;
    const bool rest_equal_shared = dst == src ? dst->rest_stride == 0
                                              : dst->rest_stride == 0 && src->rest_stride == 0 && !dst->fork.shared_rest.empty() &&
                                                    dst->fork.shared_rest.size() == src->fork.shared_rest.size() &&
                                                    memcmp(dst->fork.shared_rest.data(), src->fork.shared_rest.data(), dst->fork.shared_rest.size()) == 0;
    const bool copy_rest = !rest_equal_shared;
    if (copy_rest && dst->rest_stride == 0) {
        if (dst->E > 1) hipLaunchKernelGGL(k_replicate_rest, dim3(dst->E - 1), dim3(256), 0, dst->stream, (unsigned char *)dst->d_rest, rest_bytes);
        HIPCHECK(hipGetLastError());
        dst->rest_stride = dst->Spad;
        dst->launch.lean_dirty = true;
    }
    memcpy(dst->fork.h_fork_idx, dst_env, (size_t)n * 4); memcpy(dst->fork.h_fork_idx + n, src_env, (size_t)n * 4);   // (free again: every fork ends synchronised)
    HIPCHECK(hipMemcpyAsync(dst->fork.d_fork_idx, dst->fork.h_fork_idx, (size_t)2 * n * 4, hipMemcpyHostToDevice, dst->stream));
    ForkArgs a;
    a.pos_dst = (unsigned char *)dst->d_pos; a.prev_dst = (unsigned char *)dst->d_prev; a.cnt_dst = dst->d_cnt;
    a.pos_src = (const unsigned char *)src->d_pos; a.prev_src = (const unsigned char *)src->d_prev; a.cnt_src = src->d_cnt;
    a.rest_dst = copy_rest ? (unsigned char *)dst->d_rest : nullptr; a.rest_src = (const unsigned char *)src->d_rest;
    a.mat_dst = mat_on_device ? (unsigned char *)dst->d_mat : nullptr; a.mat_src = (const unsigned char *)src->d_mat;
    a.tear_dst = dst->d_tear; a.tear_src = src->d_tear;
    a.resume_dst = dst->epi.d_resume;
    a.dst_env = dst->fork.d_fork_idx; a.src_env = dst->fork.d_fork_idx + n;
    a.pos_bytes = (size_t)3 * dst->Ppad * dst->tsz; a.cnt_bytes = (size_t)dst->Ppad;
    a.rest_bytes = rest_bytes; a.rest_src_stride = (size_t)src->rest_stride * src->tsz;
    a.mat_bytes = mat_record_bytes(dst);
    hipLaunchKernelGGL(k_fork, dim3(n), dim3(256), 0, dst->stream, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(dst->stream));
    return 0;
}

extern "C" int clothhip_in_flight(clothhip_handle *h, uint8_t *parked) {
    if (!h || !parked) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = check_idle(h)) return rc;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    std::vector<int32_t> v((size_t)h->E);
    static_assert(offsetof(EpResume, valid) == 0, "the valid flag leads the record");
    HIPCHECK(hipMemcpy2D(v.data(), 4, h->epi.d_resume, sizeof(EpResume), 4, (size_t)h->E, hipMemcpyDeviceToHost));
    for (int e = 0; e < h->E; e++) parked[e] = v[e] ? 1 : 0;
    return 0;
}

extern "C" int clothhip_get_pin_counts(clothhip_handle *h, int32_t env0, int32_t n, uint8_t *cnt) {
    if (int rc = check_range(h, env0, n)) return rc;
    if (!cnt) return fail(CLOTHHIP_EINVAL, "cnt is NULL");
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    std::vector<uint8_t> c((size_t)n * h->Ppad);
    HIPCHECK(hipMemcpy(c.data(), h->d_cnt + (size_t)env0 * h->Ppad, c.size(), hipMemcpyDeviceToHost));
    for (int e = 0; e < n; e++) memcpy(cnt + (size_t)e * h->P, c.data() + (size_t)e * h->Ppad, (size_t)h->P);
    return 0;
}
