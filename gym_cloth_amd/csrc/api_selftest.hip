// api_selftest.hip -- clothhip_selftest_*: host and device pieces exposed to the test suite. (The two that test cloth_render_obs.hpp are
// beside its kernels in api_observe.hip: a header with a non-template kernel has one includer.)
#include <hip/hip_runtime.h>

#include "api_handle.hpp"
#include "cloth_exp_fixed.hpp"
#include "cloth_philox.hpp"
#include "cloth_selftest_kernel.hpp"

extern "C" int clothhip_selftest_windows(const ClothParams *p, int32_t *n_windows, int32_t *n_slots, int32_t *reach_shift,
                                         int32_t *spring_at, uint32_t *ent, uint64_t *dep, int32_t capacity) {
    if (int rc = check_params(p)) return rc;
    const Topology t = build_topology(p->n_side);
    const WindowTable W = build_windows(t, build_levels(t));
    if (n_windows) *n_windows = W.nW;
    if (n_slots) *n_slots = W.n_slots;
    if (reach_shift) *reach_shift = W.reach_shift;
    if ((spring_at || ent || dep) && capacity < W.n_slots) return fail(CLOTHHIP_EINVAL, "capacity below the table's slot count");
    if (spring_at) memcpy(spring_at, W.spring_at.data(), sizeof(int32_t) * W.n_slots);
    if (ent) memcpy(ent, W.ent.data(), sizeof(uint32_t) * W.n_slots);
    if (dep) memcpy(dep, W.dep.data(), sizeof(uint64_t) * W.n_slots);
    return 0;
}

extern "C" int clothhip_selftest_material(const ClothParams *p, const ClothMaterial *m, int32_t precision, double out[7]) {
    if (int rc = check_params(p)) return rc;
    if (!out) return fail(CLOTHHIP_EINVAL, "out is NULL");
    if (precision != CLOTHHIP_F64 && precision != CLOTHHIP_F32) return fail(CLOTHHIP_EINVAL, "precision must be 0 (f64) or 1 (f32)");
    if (m) if (int rc = check_material(*p, *m, 0)) return rc;
    const SpecPhys s = m ? phys_of(*p, *m) : phys_of(*p);
    auto fill = [&](auto k) {
        const double v[7] = {(double)k.mg, (double)k.ks_str, (double)k.ks_bend, (double)k.dsm, (double)k.damp, (double)k.one_m_fric, (double)k.tear_thresh};
        memcpy(out, v, sizeof(v));
    };
    if (precision == CLOTHHIP_F64) fill(make_consts<double>(s, p->n_side)); else fill(make_consts<float>(s, p->n_side));
    return 0;
}

extern "C" int clothhip_selftest_layout(const ClothParams *p, int32_t precision, int32_t n_envs, int32_t n_cus, int32_t *out, int32_t capacity) {
    if (int rc = check_params(p)) return rc;
    if (!out || capacity < 24) return fail(CLOTHHIP_EINVAL, "out needs 24 entries");
    if (precision != CLOTHHIP_F64 && precision != CLOTHHIP_F32) return fail(CLOTHHIP_EINVAL, "precision must be 0 (f64) or 1 (f32)");
    if (n_envs < 1 || n_cus < 1) return fail(CLOTHHIP_EINVAL, "n_envs and n_cus must be >= 1");
    HostPlan h;                                              // host fields only: nothing here touches a device
    init_host_fields(&h, *p, n_envs, precision);
    plan_layouts(&h, n_cus);
    auto put = [&](int o, const Layout &L) {
        out[o] = L.v.nt; out[o + 1] = L.v.ppt; out[o + 2] = L.v.tab; out[o + 3] = L.v.rest_reg ? 1 : 0; out[o + 4] = L.cell_copy;
        out[o + 5] = L.lds_bytes; out[o + 6] = L.HT; out[o + 7] = L.scratch_have; out[o + 8] = L.scratch_need;
        out[o + 9] = L.scratch_have >= L.scratch_need ? 1 : 0;
    };
    put(0, h.lay_std);
    out[10] = h.lean ? 1 : 0; out[11] = h.lean_r;
    put(12, h.lay_lean);
    out[22] = fused_supported(h) ? 1 : 0; out[23] = h.lay_std.lds_bytes <= 160 * 1024 ? 1 : 0;
    return 0;
}

extern "C" int clothhip_selftest_rng(uint32_t *state, int32_t kind, int32_t n, double a, double b, double c, double *out) {
    if (!state || n < 0 || (n > 0 && !out && kind != 5)) return fail(CLOTHHIP_EINVAL, "bad argument");
    for (int i = 0; i < n; i++) {
        switch (kind) {
        case 0: out[i] = (double)mt_next32(state); break;
        case 1: out[i] = mt_double(state); break;
        case 2: out[i] = mt_uniform(state, a, b); break;
        case 3: out[i] = (double)mt_randint(state, (uint32_t)a); break;
        case 4: out[i] = mt_randval_minabs(state, a, b, c); break;
        default: break;
        }
    }
    if (kind == 5) mt_skip_serial(state, (uint64_t)a);
    return 0;
}

extern "C" int clothhip_selftest_normal_fixed(uint64_t seed, const uint32_t *env, const uint64_t *slot, int64_t n, double *out) {
    if (n < 0 || (n > 0 && (!env || !slot || !out))) return fail(CLOTHHIP_EINVAL, "bad argument");
    for (int64_t i = 0; i < n; i++) normal_fixed(seed, env[i], slot[i], out + 4 * i);
    return 0;
}

extern "C" int clothhip_selftest_arith(int32_t device, int32_t op, const double *a, const double *b, double *out, int64_t n) {
    if (!a || !out || n <= 0) return fail(CLOTHHIP_EINVAL, "bad argument");
    if (clothhip_device_count() <= 0) return fail(CLOTHHIP_ENODEV, "no HIP device visible");
    HIPCHECK(hipSetDevice(device));
    Buffer<double> da, db, dout;
    if (int rc = da.reserve(n * 8)) return rc;
    if (int rc = dout.reserve(n * 8)) return rc;
    if (b) { if (int rc = db.reserve(n * 8)) return rc; HIPCHECK(hipMemcpy(db, b, n * 8, hipMemcpyHostToDevice)); }
    HIPCHECK(hipMemcpy(da, a, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, da, db, dout, (long long)n);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

// the host runs the very function of the PPO losses and of the exploration noise (cloth_exp_fixed.hpp)
extern "C" int clothhip_selftest_exp_fixed(const double *x, int64_t n, double *out) {
    if (n < 0 || (n > 0 && (!x || !out))) return fail(CLOTHHIP_EINVAL, "bad argument");
    for (int64_t i = 0; i < n; i++) {
        if (x[i] != x[i]) return fail(CLOTHHIP_EINVAL, "x[%lld] is NaN", (long long)i);
        out[i] = exp_fixed(x[i]);
    }
    return 0;
}
