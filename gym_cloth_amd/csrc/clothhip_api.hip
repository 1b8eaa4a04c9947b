// clothhip_api.hip -- C-ABI implementation of libclothhip.so (see include/clothhip.h).
// Host side only orchestrates: tables, uploads, launches. All physics runs in cloth_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "cloth_kernels.hpp"
#include "device_buffer.hpp"
#include "layout_plan.hpp"
#include "cloth_render.hpp"
#include "cloth_render_obs.hpp"
#include "cloth_policy_population.hpp"

using namespace clothhip;

// The host fields (HostPlan: layout_plan.hpp) and everything the handle holds on its device. Each buffer frees itself; the stream and the
// events are declared in front of the buffers, so they go after them.
struct clothhip_handle : HostPlan {
    int device = 0;
    Stream stream;
    Event ev0, ev1, ev_fork;   // ev_fork (clothhip_fork): orders a fork after the source handle's stream
    ~clothhip_handle() { (void)hipSetDevice(device); }
    bool have_timing = false, pending_exec = false;
    Buffer<void> d_pos, d_prev, d_rest;
    Buffer<void> d_flat, d_flat_rest;   // flat tier-1 grid [3][Ppad] and its rest table [Spad] (window-table slot order), handle precision
    Buffer<uint8_t> d_cnt, d_active;
    int rest_stride = 0;
    Buffer<int32_t> d_tear, d_exec, d_ngrab, d_stats;
    Buffer<ClothSchedule> d_sched;
    PinnedBuffer<ClothSchedule> h_sched;   // pinned staging
    Buffer<uint32_t> d_gather, d_wt_ent;
    Buffer<unsigned long long> d_wt_dep;
    bool lean_dirty = true, lean_ok = false;   // (HostPlan::lean: the shared rest table is checked whenever it may have changed)
    bool relaxed = false;   // clothhip_set_relaxed_order(h, 1): THIS handle's episode launches run the relaxed-order companion kernel (bench only, no parity)
    int last_dispatches = 0; // kernel dispatches the last stepper launch was issued as (clothhip_last_dispatches)
    int spec_now = 0;        // 25 / 50: the layout in use runs that grid-specialised build (decided by lean_refresh per launch: spec_ns); 0: the generic build
    int last_spec = 0;       // what the last launch ran (clothhip_last_specialised)
    float pal[3] = {0, 0, 0};
    double pal64[3] = {0, 0, 0};     // fp64 LEAN build: the smallest rest length of each spring type (the others are it + a few ulps: StepArgs::lstc)
    Buffer<uint4> d_lstc;            // [Ppad] fp64 LEAN build: per particle {stencil mask, 12 offset bytes}
    // per-env materials (clothhip_set_material): every env's effective values; how many differ bitwise from the handle's parameters (0: a uniform
    // handle -- no table goes to the kernel, the grid-specialised builds stay eligible); the device's [E] DevConsts<T> table, allocated by the first set
    std::vector<ClothMaterial> mat;
    int n_mixed = 0;
    Buffer<void> d_mat;
    int32_t last_variant[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // what the last launch ran (clothhip_last_variant)
    bool have_variant = false;
    bool on_lean = false;            // which of the two layouts runs now (lean_refresh)
    const Layout &lay() const { return on_lean ? lay_lean : lay_std; }
    struct OccKey { const void *fn; int lds; int occ; } occ_cache[8] = {};   // hipOccupancyMaxActiveBlocksPerMultiprocessor per (kernel, LDS bytes)
    Buffer<double> d_levels, d_xy, d_radius, d_cov, d_vinv;
    Buffer<uint8_t> d_oob;
    Buffer<int32_t> d_hcnt;         // per env: #points with z < thickness/2 (height reward, cloth_env.py:1047-1073)
    int n_grab_levels = 0;
    // clothhip_run_actions staging (device), sized on demand
    Buffer<void> d_fz, d_fact, d_fscr, d_frec, d_frst, d_fobs, d_frobs;
    Buffer<int32_t> d_fsteps, d_fparg;
    Buffer<EpResume> d_resume;      // [E] operations cut by a time slice (clothhip_run_actions), continued by the next launch
    Buffer<uint32_t> d_fmt;         // [E][MT_WORDS] numpy RandomState of every env (device-drawn resets)
    Buffer<uint8_t> d_fdone;
    Buffer<double> d_fsum;          // [E][4] per-env summary of the last episode launch (what the multi-GPU driver all-gathers)
    Buffer<uint64_t> d_fticks;      // [E][8] per-operation-class ticks and update() counts of the last episode launch
    int f_T = 0; size_t f_nscr = 0; bool f_pending = false, f_resets = false, f_obs = false, f_robs = false, f_mt = false;
    // clothhip_render_obs scratch for ONE chunk of images, sized on demand: finished images (when the caller gives no device buffer),
    // raw depth, uploaded '1d' rows, valid + swap flags
    Buffer<void> d_ro_img, d_ro_depth, d_ro_src, d_ro_flags;
    std::vector<unsigned char> stage;   // host staging for layout conversion
    std::vector<double> flat_rest;
    // clothhip_fork: the bytes of the ONE shared rest table as clothhip_set_state last uploaded them (handle precision, slot order) -- the only
    // writer of a shared table, so two shared tables are equal exactly when these mirrors are; the device index lists of a fork
    std::vector<unsigned char> shared_rest;
    Buffer<int32_t> d_fork_idx;
    PinnedBuffer<int32_t> h_fork_idx;   // (pinned staging, so that the upload is a plain DMA)
    // clothhip_set_policy_mlp: the handle's network (n_layers 0: none; mlp.params = d_mlp) and clothhip_policy_eval's scratch for ONE chunk of rows
    MlpDesc mlp = {};
    Buffer<float> d_mlp, d_pe_rows;
    Buffer<double> d_pe_out;
    // clothhip_set_policy_population / clothhip_policy_population_perturb: pop_rows blobs at mlp.stride floats in d_pop (mlp.params = d_pop) and
    // the env slots' map d_member (mlp.member; its host mirror pop_member). pop_rows 0: no population (a shared network counts as ONE row for
    // clothhip_policy_eval_members and clothhip_get_policy_mlp). pop_generated: the rows were made from (pop_seed, pop_sigma, pop_flags) around row
    // pop_rows - 1 = theta, so clothhip_policy_population_combine can make the same eps again
    Buffer<float> d_pop, d_pop_center, d_pop_coef, d_pop_out;
    Buffer<int32_t> d_member, d_pe_mem;
    int64_t pop_rows = 0;
    size_t mlp_n_params = 0;
    bool pop_generated = false;
    uint64_t pop_seed = 0;
    float pop_sigma = 0.0f;
    int32_t pop_flags = 0;
};

// f(float{}) or f(double{}) by the handle's precision: a launch that exists in both precisions is written once, as a generic lambda
template <typename F> static auto by_precision(const clothhip_handle *h, F &&f) { return h->precision == CLOTHHIP_F64 ? f(double{}) : f(float{}); }

extern "C" const char *clothhip_last_error(void) { return g_err.c_str(); }
extern "C" int clothhip_abi_version(void) { return CLOTHHIP_ABI_VERSION; }

extern "C" int clothhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

static int check_params(const ClothParams *p) {
    if (!p) return fail(CLOTHHIP_EINVAL, "params is NULL");
    if (p->n_side < 3 || p->n_side > MAX_SIDE) return fail(CLOTHHIP_EINVAL, "n_side %d outside [3,%d]", p->n_side, MAX_SIDE);
    if (!(p->width > 0) || !(p->height > 0)) return fail(CLOTHHIP_EINVAL, "width/height must be > 0");
    if (p->height != p->width) return fail(CLOTHHIP_EINVAL, "height must equal width (cloth.pyx:91)");
    if (p->frames_per_sec <= 0 || p->simulation_steps <= 0) return fail(CLOTHHIP_EINVAL, "frames_per_sec/simulation_steps must be > 0");
    if (!(p->density > 0) || !(p->thickness > 0)) return fail(CLOTHHIP_EINVAL, "density/thickness must be > 0");
    return 0;
}
// the rules check_params applies to the fields a material overrides: the material put into the handle's parameters must pass them
static int check_material(const ClothParams &prm, const ClothMaterial &m, int idx) {
    ClothParams p = prm;
    p.density = m.density; p.ks = m.ks; p.damping = m.damping; p.plane_friction = m.plane_friction; p.tear_thresh = m.tear_thresh; p.gravity = m.gravity;
    if (check_params(&p)) return fail(CLOTHHIP_EINVAL, "material %d: %s", idx, std::string(g_err).c_str());
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

// the physics parameters of a handle in the form the one derivation of the stepper's constants takes (cloth_common.hpp: make_consts)
static SpecPhys phys_of(const ClothParams &p) {
    return SpecPhys{p.width, p.height, p.density, p.ks, p.damping, p.thickness, p.plane_friction, p.tear_thresh, p.gravity, p.minimum_z, p.frames_per_sec, p.simulation_steps};
}
// ... and of one env of it that holds material m: the material's six fields over the handle's (cloth.pyx:175-186)
static SpecPhys phys_of(const ClothParams &p, const ClothMaterial &m) {
    SpecPhys s = phys_of(p);
    s.density = m.density; s.ks = m.ks; s.damping = m.damping; s.plane_friction = m.plane_friction; s.tear_thresh = m.tear_thresh; s.gravity = m.gravity;
    return s;
}
static ClothMaterial material_of(const ClothParams &p) { return ClothMaterial{p.density, p.ks, p.damping, p.plane_friction, p.tear_thresh, p.gravity}; }

static int spec_ns(const clothhip_handle *h, const Layout &L, bool with_palette = true);

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
    take(h->d_gather, h->gather.size() * 4); take(h->d_wt_ent, (size_t)h->Spad * 4); take(h->d_wt_dep, (size_t)h->Spad * 8); take(h->d_lstc, (size_t)h->Ppad * 16);
    take(h->d_levels, (levels.size() + 1) * 8); take(h->d_xy, E * 2 * 8); take(h->d_radius, E * 8); take(h->d_cov, E * 8); take(h->d_vinv, E * 8);
    take(h->d_oob, E); take(h->d_hcnt, E * 4); take(h->d_resume, E * sizeof(EpResume));
    take(h->d_flat, (size_t)3 * h->Ppad * h->tsz); take(h->d_flat_rest, (size_t)h->Spad * h->tsz);
    if (rc) return rc;
    HIPCHECK(hipMemset(h->d_stats, 0, E * 64));
    HIPCHECK(hipMemset(h->d_lstc, 0, (size_t)h->Ppad * 16));
    HIPCHECK(hipMemset(h->d_resume, 0, E * sizeof(EpResume)));
    HIPCHECK(hipMemcpy(h->d_gather, h->gather.data(), h->gather.size() * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(h->d_wt_ent, h->wt.ent.data(), (size_t)h->Spad * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(h->d_wt_dep, h->wt.dep.data(), (size_t)h->Spad * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(h->d_rest, 0, E * h->Spad * h->tsz));
    if (!levels.empty()) HIPCHECK(hipMemcpy(h->d_levels, levels.data(), levels.size() * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(h->d_exec, 0, E * 4));
    // large dynamic LDS (up to the CU's 160 KiB) for the stepper kernels: which variant, which layout (plan_layouts)
    {
        hipDeviceProp_t dp;
        int cus = 256;
        if (hipGetDeviceProperties(&dp, device) == hipSuccess && dp.multiProcessorCount > 0) cus = dp.multiProcessorCount;
        plan_layouts(h, cus);
        // the pick assumed lean_r resident cloths per CU: ask the device (registers, LDS granules, what else it counts) and fall back to the
        // best residency it does grant -- a build planned for r that runs at r - 1 would be slower than the build meant for r - 1
        for (int guard = 0; guard < 5 && h->lean && h->lean_r >= 3 && !h->dbg.lean_set; guard++) {
            const void *fl = find_stepper(h->lay_lean.v, 0, 1);
            int occ = 0;
            if (!fl || hipFuncSetAttribute(fl, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fl, h->lay_lean.v.nt, (size_t)h->lay_lean.lds_bytes) != hipSuccess) { (void)hipGetLastError(); break; }
            if (occ >= h->lean_r) break;
            plan_layouts(h, cus, std::max(2, occ));
        }
        if (h->lay_std.lds_bytes > 160 * 1024) return fail(CLOTHHIP_EINVAL, "n_side %d needs %d B of LDS (> 160 KiB)", h->N, h->lay_std.lds_bytes);
        // every kernel the handle may launch: the generic build of the standard layout, of the lean one (which of the two runs is decided
        // per launch) and, where one exists for a layout, its grid-specialised build (tier 2 at 25x25, the LEAN builds). The attribute is
        // per kernel function and process-global: always the CU's full 160 KiB, so that a later handle with a smaller footprint can never
        // lower it under an earlier one
        for (const Layout *L : {&h->lay_std, &h->lay_lean}) {
            if (L == &h->lay_lean && !h->lean) continue;
            const int ns = spec_ns(h, *L, false);
            for (int f = 0; f < 3; f++) {
                const void *fn = find_stepper(L->v, 0, f);
                if (!fn) return fail(CLOTHHIP_EINVAL, "no %sstepper variant for n_side %d", L == &h->lay_lean ? "lean " : "", h->N);
                HIPCHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                if (ns) HIPCHECK(hipFuncSetAttribute(find_stepper(L->v, ns, f), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            }
        }
    }
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

// Any state change from outside the episode launches (uploads, resets, grabs, raw schedules) voids the operation a time slice
// left in flight -- for the envs that call touches, and only for them: the parked operations of the others continue in the next
// episode launch. d_mask: device mask [E] (nullptr = all); d_sched: device schedules whose active flag selects (or nullptr).
static int drop_in_flight(clothhip_handle *h, const uint8_t *d_mask, const ClothSchedule *d_sched) {
    if (!h->d_resume) return 0;
    hipLaunchKernelGGL(k_clear_resume, dim3((h->E + 255) / 256), dim3(256), 0, h->stream, h->d_resume, d_mask, d_sched, h->E);
    HIPCHECK(hipGetLastError());
    return 0;
}
static int drop_in_flight_range(clothhip_handle *h, int env0, int n) {
    if (h->d_resume && n > 0) HIPCHECK(hipMemsetAsync(h->d_resume + env0, 0, (size_t)n * sizeof(EpResume), h->stream));
    return 0;
}

// no call that touches what an episode launch reads or writes between clothhip_run_actions_begin and _end
static int check_idle(const clothhip_handle *h) { return h->f_pending ? fail(CLOTHHIP_ESTATE, "clothhip_run_actions_begin still in flight: call clothhip_run_actions_end first") : 0; }

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
        h->lean_dirty = true;
        if (rest_shared) h->shared_rest.swap(buf);       // (clothhip_fork compares shared tables by this mirror)
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

template <typename T> static StepArgs<T> make_args(clothhip_handle *h, const ClothSchedule *d_sched) {
    StepArgs<T> a;
    a.e0 = 0;
    a.pos = (T *)h->d_pos; a.prev = (T *)h->d_prev; a.cnt = h->d_cnt; a.rest = (const T *)h->d_rest;
    a.tear = h->d_tear; a.executed = h->d_exec; a.stats = h->d_stats; a.sched = d_sched;
    a.gather = h->d_gather; a.wt_ent = h->d_wt_ent; a.wt_dep = h->d_wt_dep; a.nW = h->wt.nW; a.wt_rshift = h->wt.reach_shift; a.cell_copy = h->lay().cell_copy;
    a.N = h->N; a.P = h->P; a.Ppad = h->Ppad; a.S = h->S; a.Spad = h->Spad;
    a.HT = h->lay().HT; a.ht_bits = h->lay().ht_bits;
    a.rest_stride = h->rest_stride; a.phase_mask = h->dbg.phase_mask;
    a.k = make_consts<T>(phys_of(h->prm), h->N);
    if (sizeof(T) == 8) { a.pal_struct = (T)h->pal64[SPRING_STRUCTURAL]; a.pal_shear = (T)h->pal64[SPRING_SHEARING]; a.pal_bend = (T)h->pal64[SPRING_BENDING]; }
    else { a.pal_struct = (T)h->pal[SPRING_STRUCTURAL]; a.pal_shear = (T)h->pal[SPRING_SHEARING]; a.pal_bend = (T)h->pal[SPRING_BENDING]; }
    a.lstc = h->d_lstc;
    a.mat = h->n_mixed ? (const DevConsts<T> *)h->d_mat : nullptr;
    a.fz = nullptr;
    return a;
}

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
    if (int rc = dst->d_fork_idx.reserve((size_t)2 * n * 4)) return rc;
    if (int rc = dst->h_fork_idx.reserve((size_t)2 * n * 4)) return rc;
    if (dst->stream != src->stream) {                  // the copy reads what the source's stream has enqueued so far
        if (!dst->ev_fork) HIPCHECK(hipEventCreateWithFlags(&dst->ev_fork.v, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(dst->ev_fork, src->stream));
        HIPCHECK(hipStreamWaitEvent(dst->stream, dst->ev_fork, 0));
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
                                              : dst->rest_stride == 0 && src->rest_stride == 0 && !dst->shared_rest.empty() &&
                                                    dst->shared_rest.size() == src->shared_rest.size() &&
                                                    memcmp(dst->shared_rest.data(), src->shared_rest.data(), dst->shared_rest.size()) == 0;
    const bool copy_rest = !rest_equal_shared;
    if (copy_rest && dst->rest_stride == 0) {
        if (dst->E > 1) hipLaunchKernelGGL(k_replicate_rest, dim3(dst->E - 1), dim3(256), 0, dst->stream, (unsigned char *)dst->d_rest, rest_bytes);
        HIPCHECK(hipGetLastError());
        dst->rest_stride = dst->Spad;
        dst->lean_dirty = true;
    }
    memcpy(dst->h_fork_idx, dst_env, (size_t)n * 4); memcpy(dst->h_fork_idx + n, src_env, (size_t)n * 4);   // (free again: every fork ends synchronised)
    HIPCHECK(hipMemcpyAsync(dst->d_fork_idx, dst->h_fork_idx, (size_t)2 * n * 4, hipMemcpyHostToDevice, dst->stream));
    ForkArgs a;
    a.pos_dst = (unsigned char *)dst->d_pos; a.prev_dst = (unsigned char *)dst->d_prev; a.cnt_dst = dst->d_cnt;
    a.pos_src = (const unsigned char *)src->d_pos; a.prev_src = (const unsigned char *)src->d_prev; a.cnt_src = src->d_cnt;
    a.rest_dst = copy_rest ? (unsigned char *)dst->d_rest : nullptr; a.rest_src = (const unsigned char *)src->d_rest;
    a.mat_dst = mat_on_device ? (unsigned char *)dst->d_mat : nullptr; a.mat_src = (const unsigned char *)src->d_mat;
    a.tear_dst = dst->d_tear; a.tear_src = src->d_tear;
    a.resume_dst = dst->d_resume;
    a.dst_env = dst->d_fork_idx; a.src_env = dst->d_fork_idx + n;
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
    HIPCHECK(hipMemcpy2D(v.data(), 4, h->d_resume, sizeof(EpResume), 4, (size_t)h->E, hipMemcpyDeviceToHost));
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

// Which grid-specialised kernel (k_run_schedule<..., NS>, NS = 25 or 50) may run layout L -- 0: none, the generic build. Only if the
// variant is one of the specialised ones (stepper_variants.hpp: CLOTH_SPEC_*) AND every constant that build has compiled in
// (cloth_common.hpp: spec_*) is what this handle computed: grid, window table, hash-table size, whether the cell-ordered copy exists, all phases
// on (debug masks take the generic build, as does CLOTHHIP_DEBUG_NOSPEC=1 -- the A/B and the bit-identity test of the two; read at every call).
// (with_palette false: clothhip_create, which prepares every kernel the handle may launch before any rest table has been read back)
static int spec_ns(const clothhip_handle *h, const Layout &L, bool with_palette) {
    if (read_debug_knobs().nospec) return 0;
    if (h->dbg.phase_mask != 15 || (h->N != 25 && h->N != 50)) return 0;
    if (h->n_mixed) return 0;       // per-env materials: the specialised builds hold ONE material as literals and never read the table
    const int ns = h->N;
    // the physics constants the build has compiled in (cloth_common.hpp: spec_phys) must be this handle's
    if (!(phys_of(h->prm) == spec_phys(ns))) return 0;
    // (belt and braces: the literals the kernel holds, evaluated at compile time, are what the generic build is given at run time, bit for bit)
    const bool same_consts = by_precision(h, [&](auto t) {
        using T = decltype(t);
        static constexpr DevConsts<T> c25 = spec_consts<T>(25), c50 = spec_consts<T>(50);
        const DevConsts<T> a = make_consts<T>(phys_of(h->prm), h->N);
        return memcmp(&a, ns == 25 ? &c25 : &c50, sizeof(a)) == 0;
    });
    if (!same_consts) return 0;
    if (!find_stepper(L.v, ns, 0)) return 0;
    const bool same = h->P == spec_p(ns) && h->Ppad == spec_ppad(ns) && L.HT == spec_ht(ns, L.v) && L.ht_bits == spec_htbits(ns, L.v) &&
                      h->Spad == spec_spad(ns) && h->wt.nW == spec_nw(ns) && h->wt.reach_shift == spec_rshift(ns) && L.cell_copy == spec_cell_copy(ns, L.v);
    if (!same) return 0;
    // the LEAN fp32 builds hold the rest-length palette as literals: it must be what lean_refresh read back from the device's table
    if (with_palette && h->precision == CLOTHHIP_F32 && L.v.lean()) {
        for (int t = 0; t < 3; t++) { const float v = spec_pal(ns, t); if (memcmp(&v, &h->pal[t], 4) != 0) return 0; }
    }
    return ns;
}

// fp64 LEAN: every spring's rest length in the device's shared table must be its type's smallest value + at most 255 ulps (the flat tiers: <= 46
// at 50x50). Fills pal64 and the per-particle stencil table d_lstc: slot k of particle i = the offset of its k-th stencil position (lean_off).
static int check_palette_f64(clothhip_handle *h) {
    std::vector<double> r((size_t)h->Spad);
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipMemcpy(r.data(), h->d_rest, r.size() * 8, hipMemcpyDeviceToHost));
    long long base[3] = {0, 0, 0}; bool have[3] = {false, false, false}, ok = true;
    auto bits = [](double v) { long long b; memcpy(&b, &v, 8); return b; };
    for (int sp = 0; sp < h->S; sp++) {
        const int ty = h->topo.type[sp];
        const double v = r[h->wt.slot_of[sp]];
        if (!(v > 0.0) || !std::isfinite(v)) { ok = false; break; }
        if (!have[ty] || bits(v) < base[ty]) { base[ty] = bits(v); have[ty] = true; }
    }
    ok = ok && have[0] && have[1] && have[2];
    std::vector<uint32_t> tab((size_t)h->Ppad * 4, 0u);
    for (int i = 0; i < h->P && ok; i++) {
        tab[(size_t)4 * i] = lean_valid_mask(i / h->N, i % h->N, h->N);
        ok = walk_stencil(h, i, [&](int k, uint32_t g) {
            const int pos = (int)((g >> HK_POS_SHIFT) & HK_POS_MASK);
            const int sp = h->wt.spring_at[pos];
            const long long off = sp >= 0 ? bits(r[pos]) - base[h->topo.type[sp]] : -1;
            if (off < 0 || off > 255) return false;
            tab[(size_t)4 * i + 1 + (k >> 2)] |= (uint32_t)off << (8 * (k & 3));
            return true;
        }) >= 0;
    }
    if (ok) {
        for (int t = 0; t < 3; t++) memcpy(&h->pal64[t], &base[t], 8);
        HIPCHECK(hipMemcpy(h->d_lstc, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    }
    h->lean_ok = ok;
    return 0;
}
// fp32 LEAN: the device's shared rest table must hold ONE value per spring type, bit for bit (pal)
static int check_palette_f32(clothhip_handle *h) {
    std::vector<float> r((size_t)h->Spad);
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipMemcpy(r.data(), h->d_rest, r.size() * 4, hipMemcpyDeviceToHost));
    bool have[3] = {false, false, false}, ok = true;
    for (int sp = 0; sp < h->S && ok; sp++) {
        const int ty = h->topo.type[sp];
        const float v = r[h->wt.slot_of[sp]];
        if (!have[ty]) { h->pal[ty] = v; have[ty] = true; }
        else if (memcmp(&h->pal[ty], &v, 4) != 0) ok = false;
    }
    h->lean_ok = ok && have[0] && have[1] && have[2];
    return 0;
}

// Which of the handle's two layouts the next launch runs: the LEAN one when this handle has one and the device's shared rest table is
// its palette (re-checked whenever the table may have changed: per-env tables, i.e. tier 2, or odd rest lengths uploaded by the
// caller switch back), else the standard one. LDS is rebuilt by every launch, so the layout may change from one launch to the next.
static int lean_refresh(clothhip_handle *h) {
    if (h->lean && h->lean_dirty) {
        h->lean_dirty = false; h->lean_ok = false;
        if (h->rest_stride == 0)
            if (int rc = h->precision == CLOTHHIP_F64 ? check_palette_f64(h) : check_palette_f32(h)) return rc;
    }
    if (h->lean) h->on_lean = h->lean_ok && h->rest_stride == 0;
    h->spec_now = spec_ns(h, h->lay());
    return 0;
}

// resident workgroups per CU of a stepper kernel at the active layout's LDS footprint (for clothhip_last_variant): asked once per (kernel,
// LDS bytes), not on every launch -- the step mode launches once per env step
static int cached_occupancy(clothhip_handle *h, const void *fn) {
    const Layout &L = h->lay();
    for (auto &c : h->occ_cache) if (c.fn == fn && c.lds == L.lds_bytes) return c.occ;
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, L.v.nt, (size_t)L.lds_bytes) != hipSuccess) { (void)hipGetLastError(); occ = 0; }
    for (auto &c : h->occ_cache) if (c.fn == nullptr) { c = {fn, L.lds_bytes, occ}; return occ; }
    h->occ_cache[0] = {fn, L.lds_bytes, occ};
    return occ;
}

template <typename T> static int launch_generations(clothhip_handle *h, const void *fn, int cap, const ClothSchedule *d_sched, const void *d_fz) {
    StepArgs<T> a = make_args<T>(h, d_sched);
    a.fz = (const FusedArgs<T> *)d_fz;
    void *args[] = {&a};
    h->last_dispatches = 0;
    for (int e0 = 0; e0 < h->E; e0 += cap) {
        a.e0 = e0; h->last_dispatches++;
        HIPCHECK(hipLaunchKernel(fn, dim3(std::min(cap, h->E - e0)), dim3(h->lay().v.nt), args, (size_t)h->lay().lds_bytes, h->stream));
    }
    return 0;
}

// One stepper launch of the active layout (the caller has run lean_refresh(h) -- which of the handle's two layouts may run now -- BEFORE
// recording its start event). fused: 0 one external schedule, 1 episodes, 2 episodes incl. tier-2 resets and the cold policies, 3 the
// relaxed-order companion (Jacobi self-collision, coloured strain limit; the headline variant's layout only): its results differ from the
// reference's by construction -- a labelled measurement of what the exact order costs (bench.py's companion record "exact_order": false),
// never a product path.
// `by_generation` (the time-sliced episode launches): every workgroup runs for the same time slice, counted from its own start, so a batch of
// more cloths than are resident runs in generations -- which go out as ONE LAUNCH EACH, in stream order. Left to the hardware's
// dispatcher the generations of a single launch change hands on every CU within a few dozen microseconds, and now and then a CU
// that has just lost both of its workgroups takes only one new one for the whole slice (measured on 1 024 cloths of 50x50, two per
// CU at 79.9 KB of LDS and 4 x 128 VGPRs per SIMD: in 3 launches of 8 one workgroup of the 1 024 started only when the second
// generation had ended, 2 400 instead of 1 600 ms -- tools/placement.py, profiles/r05_placement.txt). A fresh launch finds every CU empty.
static int launch_run(clothhip_handle *h, int fused, const ClothSchedule *d_sched, const void *d_fz, bool by_generation) {
    const Layout &L = h->lay();
    const Variant &V = L.v;
    const int ns = fused == 3 ? 0 : h->spec_now;
    const void *fn = find_stepper(V, ns, fused);
    if (!fn) return fail(CLOTHHIP_ESTATE, "no stepper variant for this layout (fused mode %d)", fused);
    const int occ = cached_occupancy(h, fn);
    const int cap = by_generation && occ > 0 && h->n_cus > 0 && !read_debug_knobs().one_launch ? occ * h->n_cus : h->E;
    if (int rc = by_precision(h, [&](auto t) { return launch_generations<decltype(t)>(h, fn, cap, d_sched, d_fz); })) return rc;
    const int32_t v[10] = {V.nt, V.ppt, V.tab, V.rest_reg ? 1 : 0, V.lean() ? 1 : 0, fused, L.lds_bytes, occ, h->n_cus, V.tsz == 4 ? 1 : 0};
    memcpy(h->last_variant, v, sizeof(v)); h->have_variant = true; h->last_spec = ns;
    return 0;
}

static int run_common(clothhip_handle *h, const ClothSchedule *d_sched) {
    if (int rc = drop_in_flight(h, nullptr, d_sched)) return rc;
    if (int rc = lean_refresh(h)) return rc;         // (may synchronise and read the rest table back: outside the timed events)
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    if (int rc = launch_run(h, 0, d_sched, nullptr, false)) return rc;
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    h->pending_exec = true;
    return 0;
}

extern "C" int clothhip_run_async(clothhip_handle *h, const ClothSchedule *sched) {
    if (!h || !sched) return fail(CLOTHHIP_EINVAL, "NULL argument");
    for (int e = 0; e < h->E; e++) {
        const ClothSchedule &s = sched[e];
        if (s.n_total < 0 || s.n_up_end < 0 || s.n_uprest_end < s.n_up_end || s.n_pull_end < s.n_uprest_end ||
            s.n_griprest_end < s.n_pull_end || s.n_total < s.n_griprest_end)
            return fail(CLOTHHIP_EINVAL, "env %d: phase boundaries must be non-decreasing and <= n_total", e);
    }
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));      // h_sched may still be in flight from a previous _async call
    memcpy(h->h_sched, sched, (size_t)h->E * sizeof(ClothSchedule));
    HIPCHECK(hipMemcpyAsync(h->d_sched, h->h_sched, (size_t)h->E * sizeof(ClothSchedule), hipMemcpyHostToDevice, h->stream));
    return run_common(h, h->d_sched);
}

extern "C" int clothhip_run_device_sched_async(clothhip_handle *h, const void *d_sched) {
    if (!h || !d_sched) return fail(CLOTHHIP_EINVAL, "NULL argument");
    HIPCHECK(hipSetDevice(h->device));
    return run_common(h, (const ClothSchedule *)d_sched);
}

extern "C" int clothhip_sync(clothhip_handle *h, int32_t *executed) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    HIPCHECK(hipSetDevice(h->device));
    if (executed && h->pending_exec)
        HIPCHECK(hipMemcpyAsync(executed, h->d_exec, (size_t)h->E * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_run(clothhip_handle *h, const ClothSchedule *sched, int32_t *executed) {
    if (int rc = clothhip_run_async(h, sched)) return rc;
    return clothhip_sync(h, executed);
}

// ---- whole episodes on the device ---------------------------------------------------------------------------------
template <typename T> static void fill_fused(clothhip_handle *h, FusedArgs<T> &f, const ClothEpisodeParams *ep, int T_, int policy,
                                             const double *d_actions, bool have_parg, bool have_scripts, bool have_resets, bool have_obs,
                                             bool have_robs, int n_scripts, uint64_t budget_ticks, bool have_mt, int rng_tier,
                                             uint64_t domrand_words, int NS, int NH) {
    memset(&f, 0, sizeof(f));
    f.nT = T_; f.policy = policy; f.NS = NS; f.NH = NH;
    f.actions = d_actions;
    f.policy_arg = have_parg ? h->d_fparg : nullptr;
    f.scripts = have_scripts ? (const ClothResetScript *)h->d_fscr : nullptr;
    f.num_steps = h->d_fsteps; f.done = h->d_fdone;
    f.records = (ClothStepRecord *)h->d_frec;
    f.resets = have_resets ? (ClothResetRecord *)h->d_frst : nullptr;
    f.obs = have_obs ? (float *)h->d_fobs : nullptr;
    f.reset_obs = have_robs ? (float *)h->d_frobs : nullptr;
    f.flat = (const T *)h->d_flat;
    f.wt_ent = h->d_wt_ent;
    f.rest = (const T *)h->d_rest; f.rest_rw = (T *)h->d_rest; f.rest_stride = h->rest_stride;
    f.grid_dx = h->prm.width * 1.0 / (h->N - 1); f.grid_dy = h->prm.height * 1.0 / (h->N - 1);
    f.levels = h->d_levels; f.n_glevels = h->n_grab_levels; f.E = h->E; f.n_scripts = n_scripts; f.budget_ticks = budget_ticks;
    f.resume = h->d_resume;
    f.op_ticks = h->d_fticks;
    f.summary = h->d_fsum;
    f.mt = have_mt ? h->d_fmt : nullptr; f.rng_tier = rng_tier; f.domrand_words = domrand_words;
    f.two_thickness = 2 * h->prm.thickness; f.half_thickness = h->prm.thickness / 2.0;
    f.ep = *ep;
    f.mlp = h->mlp;
}

extern "C" int clothhip_fused_supported(const clothhip_handle *h) { return h ? (fused_supported(*h) ? 1 : 0) : fail(CLOTHHIP_EINVAL, "handle is NULL"); }

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

extern "C" int clothhip_run_actions_begin(clothhip_handle *h, const ClothEpisodeParams *ep, int32_t T_, int32_t policy,
                                          const double *actions, int32_t actions_on_device, const int32_t *policy_arg,
                                          const ClothResetScript *scripts, int32_t n_scripts, const int32_t *num_steps,
                                          const uint8_t *done, const uint32_t *rng_states, int32_t rng_tier, uint64_t domrand_words,
                                          int32_t want_resets, int32_t want_obs, int32_t want_reset_obs,
                                          double time_budget_ms) {
    if (!h || !ep || !num_steps || !done) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (h->f_pending) return fail(CLOTHHIP_ESTATE, "a clothhip_run_actions_begin is already in flight");
    const bool resets = want_resets != 0, obs = want_obs != 0, reset_obs = want_reset_obs != 0;
    if (T_ < 1 || T_ > 4096) return fail(CLOTHHIP_EINVAL, "T must be in [1, 4096]");
    if (policy != CLOTHHIP_POLICY_TABLE && policy != CLOTHHIP_POLICY_ORACLE_CORNER && policy != CLOTHHIP_POLICY_HIGHEST_POINT && policy != CLOTHHIP_POLICY_MLP)
        return fail(CLOTHHIP_EINVAL, "unknown policy %d", policy);
    if (policy == CLOTHHIP_POLICY_MLP && h->mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "the MLP policy needs a network: call clothhip_set_policy_mlp or clothhip_set_policy_population first");
    if (policy == CLOTHHIP_POLICY_MLP && h->relaxed)
        return fail(CLOTHHIP_ESTATE, "clothhip_set_relaxed_order: the relaxed-order companion is a bench-only kernel without the MLP policy");
    if (policy == CLOTHHIP_POLICY_HIGHEST_POINT && !policy_arg)
        return fail(CLOTHHIP_EINVAL, "the highest-point policy needs policy_arg[1 + T][E] (construction codes + which of the highest points per slot)");
    if (policy == CLOTHHIP_POLICY_TABLE && !actions) return fail(CLOTHHIP_EINVAL, "the table policy needs actions[T][E][4]");
    if (policy == CLOTHHIP_POLICY_ORACLE_CORNER && h->N != 25)
        return fail(CLOTHHIP_ESTATE, "the oracle-corner policy is defined for 25x25 cloths only (analytic.py:106)");
    if ((scripts || rng_states) && (n_scripts < 1 || n_scripts > 255)) return fail(CLOTHHIP_EINVAL, "n_scripts must be in [1, 255]");
    if (scripts && rng_states) return fail(CLOTHHIP_EINVAL, "resets come either from scripts or from the device-side RNG streams, not both");
    if (rng_states && (rng_tier < 1 || rng_tier > 3)) return fail(CLOTHHIP_EINVAL, "rng_tier must be 1, 2 or 3");
    if (!scripts && !rng_states) n_scripts = 0;
    const bool tier2 = rng_states && rng_tier == 2;
    if ((scripts || rng_states) && !tier2 && h->rest_stride != 0)
        return fail(CLOTHHIP_ESTATE, "in-kernel resets of the flat tiers need the shared flat rest table; this handle has per-env rest lengths");
    if (tier2 && h->rest_stride == 0)
        return fail(CLOTHHIP_ESTATE, "in-kernel tier-2 resets rebuild per-env rest lengths; upload per-env rest tables first (clothhip_set_state without CLOTHHIP_REST_SHARED)");
    if (tier2 && (size_t)3 * h->P * 8 > (size_t)160 * 1024) return fail(CLOTHHIP_ESTATE, "grid too large for the tier-2 reset scratch");
    if (!(ep->reduce_factor > 0) || ep->max_actions < 1) return fail(CLOTHHIP_EINVAL, "bad episode parameters");
    if (h->relaxed && h->n_mixed)
        return fail(CLOTHHIP_ESTATE, "clothhip_set_relaxed_order: the relaxed-order companion is a bench-only kernel; this handle holds per-env materials (clothhip_set_material)");
    HIPCHECK(hipSetDevice(h->device));
    // which of the handle's two layouts runs now (may synchronise and read the rest table back: long before the timed events) -- the
    // scratch check below is against THAT layout, not the previous launch's
    if (int rc = lean_refresh(h)) return rc;
    if (h->lay().scratch_have < h->lay().scratch_need)
        return fail(CLOTHHIP_ESTATE, "n_side %d: the in-kernel metrics need %d B of LDS scratch, this variant has %d", h->N, h->lay().scratch_need, h->lay().scratch_have);
    if (policy == CLOTHHIP_POLICY_MLP && h->lay().scratch_have < MLP_SCRATCH_BYTES)
        return fail(CLOTHHIP_ESTATE, "n_side %d: the MLP policy's hidden vectors need %d B of LDS scratch, this variant has %d", h->N, MLP_SCRATCH_BYTES, h->lay().scratch_have);
    HIPCHECK(hipStreamSynchronize(h->stream));
    const size_t E = h->E, nrec = (size_t)T_ * E;
    if (int rc = h->d_fz.reserve(1024)) return rc;
    if (int rc = h->d_fsteps.reserve(E * 4)) return rc;
    if (int rc = h->d_fdone.reserve(E)) return rc;
    if (int rc = h->d_fticks.reserve(E * 64)) return rc;
    if (int rc = h->d_fsum.reserve(E * 32)) return rc;
    HIPCHECK(hipMemsetAsync(h->d_fticks, 0, E * 64, h->stream));
    if (int rc = h->d_frec.reserve(nrec * sizeof(ClothStepRecord))) return rc;
    const size_t nscr = E * (size_t)(n_scripts > 0 ? n_scripts : 1);
    if (int rc = h->d_fscr.reserve(nscr * sizeof(ClothResetScript))) return rc;
    if (int rc = h->d_frst.reserve(nscr * sizeof(ClothResetRecord))) return rc;
    const double *d_actions = nullptr;
    if (policy == CLOTHHIP_POLICY_TABLE || (policy == CLOTHHIP_POLICY_MLP && actions)) {      // (MLP: the optional noise table)
        if (actions_on_device) d_actions = actions;
        else {
            if (int rc = h->d_fact.reserve(nrec * 4 * 8)) return rc;
            HIPCHECK(hipMemcpyAsync(h->d_fact, actions, nrec * 4 * 8, hipMemcpyHostToDevice, h->stream));
            d_actions = (const double *)h->d_fact;
        }
    }
    if (obs) if (int rc = h->d_fobs.reserve(nrec * 3 * h->P * 4)) return rc;
    if ((reset_obs || resets) && !scripts && !rng_states) return fail(CLOTHHIP_EINVAL, "reset outputs without a reset source");
    if (reset_obs) {
        if (int rc = h->d_frobs.reserve(nscr * 3 * h->P * 4)) return rc;
        HIPCHECK(hipMemsetAsync(h->d_frobs, 0, nscr * 3 * h->P * 4, h->stream));
    }
    if (rng_states) {
        if (int rc = h->d_fmt.reserve(E * MT_WORDS * 4)) return rc;
        HIPCHECK(hipMemcpyAsync(h->d_fmt, rng_states, E * MT_WORDS * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (policy_arg) {
        const size_t nb = (policy == CLOTHHIP_POLICY_HIGHEST_POINT ? (size_t)(1 + T_) : (size_t)1) * E * 4;
        if (int rc = h->d_fparg.reserve(nb)) return rc;
        HIPCHECK(hipMemcpyAsync(h->d_fparg, policy_arg, nb, hipMemcpyHostToDevice, h->stream));
    }
    if (scripts) HIPCHECK(hipMemcpyAsync(h->d_fscr, scripts, nscr * sizeof(ClothResetScript), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->d_fsteps, num_steps, E * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->d_fdone, done, E, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemsetAsync(h->d_frec, 0, nrec * sizeof(ClothStepRecord), h->stream));
    if (resets) HIPCHECK(hipMemsetAsync(h->d_frst, 0, nscr * sizeof(ClothResetRecord), h->stream));
    const uint64_t budget_ticks = time_budget_ms > 0 ? (uint64_t)(time_budget_ms * 1e5) : 0;      // s_memrealtime: 100 MHz
    static_assert(sizeof(FusedArgs<double>) <= 1024 && sizeof(FusedArgs<float>) <= 1024, "fused argument block");
    unsigned char fzbuf[1024];
    const MetricsDims md = metrics_dims(h->P, h->Ppad);
    by_precision(h, [&](auto t) {
        fill_fused(h, *reinterpret_cast<FusedArgs<decltype(t)> *>(fzbuf), ep, T_, policy, d_actions, policy_arg != nullptr, scripts != nullptr, resets, obs, reset_obs, n_scripts,
                   budget_ticks, rng_states != nullptr, rng_tier, domrand_words, md.NS, md.NH);
    });
    HIPCHECK(hipMemcpyAsync(h->d_fz, fzbuf, 1024, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));          // fzbuf is on this stack frame
    if (h->relaxed && !(find_stepper(h->lay().v, 0, 3) && h->lay().cell_copy && !tier2 && policy != CLOTHHIP_POLICY_HIGHEST_POINT))
        return fail(CLOTHHIP_ESTATE, "clothhip_set_relaxed_order: the relaxed-order companion exists for the eight-wave LEAN layout only (fp32, flat tiers, 25x25 class, <= 512 cloths)");
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    // (FUSED 2: the variant that also carries the tier-2 reset code and the cold policies; the relaxed-order companion is one launch)
    const int fused = h->relaxed ? 3 : (tier2 || policy == CLOTHHIP_POLICY_HIGHEST_POINT || policy == CLOTHHIP_POLICY_MLP || read_debug_knobs().cold_build) ? 2 : 1;
    if (int rc = launch_run(h, fused, h->d_sched, h->d_fz, !h->relaxed && budget_ticks != 0)) return rc;
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    h->pending_exec = true;
    h->f_T = T_; h->f_nscr = nscr; h->f_resets = resets; h->f_obs = obs; h->f_robs = reset_obs; h->f_mt = rng_states != nullptr;
    h->f_pending = true;
    return 0;
}

extern "C" int clothhip_run_actions_end(clothhip_handle *h, int32_t *num_steps, uint8_t *done, ClothStepRecord *records,
                                        ClothResetRecord *resets, float *obs, float *reset_obs, uint32_t *rng_states) {
    if (!h || !num_steps || !done || !records) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!h->f_pending) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions_begin in flight");
    if ((resets != nullptr) != h->f_resets || (obs != nullptr) != h->f_obs || (reset_obs != nullptr) != h->f_robs)
        return fail(CLOTHHIP_EINVAL, "the output buffers must match the ones announced to clothhip_run_actions_begin");
    if ((rng_states != nullptr) != h->f_mt) return fail(CLOTHHIP_EINVAL, "rng_states must be given to both halves or to neither");
    HIPCHECK(hipSetDevice(h->device));
    const size_t E = h->E, nrec = (size_t)h->f_T * E, nscr = h->f_nscr;
    HIPCHECK(hipMemcpyAsync(records, h->d_frec, nrec * sizeof(ClothStepRecord), hipMemcpyDeviceToHost, h->stream));
    if (resets) HIPCHECK(hipMemcpyAsync(resets, h->d_frst, nscr * sizeof(ClothResetRecord), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(num_steps, h->d_fsteps, E * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(done, h->d_fdone, E, hipMemcpyDeviceToHost, h->stream));
    if (obs) HIPCHECK(hipMemcpyAsync(obs, h->d_fobs, nrec * 3 * h->P * 4, hipMemcpyDeviceToHost, h->stream));
    if (reset_obs) HIPCHECK(hipMemcpyAsync(reset_obs, h->d_frobs, nscr * 3 * h->P * 4, hipMemcpyDeviceToHost, h->stream));
    if (rng_states) HIPCHECK(hipMemcpyAsync(rng_states, h->d_fmt, E * MT_WORDS * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->f_pending = false;
    return 0;
}

extern "C" int clothhip_run_actions_summary(clothhip_handle *h, double *summary, void **d_summary) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!h->d_fsum) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions launch yet");
    if (d_summary) *d_summary = h->d_fsum;
    if (summary) {
        HIPCHECK(hipSetDevice(h->device));
        HIPCHECK(hipMemcpyAsync(summary, h->d_fsum, (size_t)h->E * 32, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

extern "C" int clothhip_run_actions_op_ticks(clothhip_handle *h, uint64_t *ticks) {
    if (!h || !ticks) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!h->d_fticks) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions launch yet");
    if (int rc = check_idle(h)) return rc;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(ticks, h->d_fticks, (size_t)h->E * 64, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_run_actions(clothhip_handle *h, const ClothEpisodeParams *ep, int32_t T_, int32_t policy,
                                    const double *actions, int32_t actions_on_device, const int32_t *policy_arg,
                                    const ClothResetScript *scripts, int32_t n_scripts, int32_t *num_steps, uint8_t *done,
                                    ClothStepRecord *records, ClothResetRecord *resets, float *obs, float *reset_obs,
                                    double time_budget_ms) {
    if (!records) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (int rc = clothhip_run_actions_begin(h, ep, T_, policy, actions, actions_on_device, policy_arg, scripts, n_scripts,
                                            num_steps, done, nullptr, 0, 0, resets != nullptr, obs != nullptr,
                                            reset_obs != nullptr, time_budget_ms))
        return rc;
    return clothhip_run_actions_end(h, num_steps, done, records, resets, obs, reset_obs, nullptr);
}

extern "C" int clothhip_update(clothhip_handle *h, int32_t n_sub, const double *delta) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (n_sub < 0) return fail(CLOTHHIP_EINVAL, "n_sub < 0");
    std::vector<ClothSchedule> s(h->E);
    for (auto &x : s) {
        memset(&x, 0, sizeof(x));
        x.active = 1; x.break_on_tear = 0; x.n_total = n_sub; x.n_griprest_end = n_sub;
        if (delta) {   // n x { adjust(delta) ; update }: the whole run is one "pull" phase
            x.n_pull_end = n_sub;
            x.dx_pull = delta[0]; x.dy_pull = delta[1]; x.dz_pull = delta[2];
        }
    }
    return clothhip_run(h, s.data(), nullptr);
}

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

// ---- a learned policy: the handle's network (cloth_policy_mlp.hpp) ----------------------------------------------------------------------
// the shape rules of every entry that takes a network
static int check_mlp_shape(const clothhip_handle *h, int32_t n_layers, const int32_t *widths) {
    if (n_layers < 1 || n_layers > MLP_MAX_LAYERS) return fail(CLOTHHIP_EINVAL, "n_layers %d outside [0, %d]", n_layers, MLP_MAX_LAYERS);
    if (!widths) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (widths[0] != 3 * h->P) return fail(CLOTHHIP_EINVAL, "the network's input width is %d, the '1d' observation has %d values", widths[0], 3 * h->P);
    if (widths[n_layers] != MLP_OUT) return fail(CLOTHHIP_EINVAL, "the network's output width is %d, an action has %d values", widths[n_layers], MLP_OUT);
    for (int l = 1; l < n_layers; l++)
        if (widths[l] < 1 || widths[l] > MLP_MAX_WIDTH) return fail(CLOTHHIP_EINVAL, "hidden width %d (layer %d) outside [1, %d]", widths[l], l, MLP_MAX_WIDTH);
    return 0;
}
static int check_members(const int32_t *member, int64_t n, int64_t rows, const char *what) {
    if (!member) return fail(CLOTHHIP_EINVAL, "%s is NULL", what);
    for (int64_t e = 0; e < n; e++)
        if (member[e] < 0 || member[e] >= rows) return fail(CLOTHHIP_EINVAL, "%s[%lld] = %d outside [0, %lld)", what, (long long)e, member[e], (long long)rows);
    return 0;
}
// the handle without a network of either kind (the memory stays with the handle for the next one)
static void drop_network(clothhip_handle *h) { h->mlp = MlpDesc{}; h->pop_rows = 0; h->mlp_n_params = 0; h->pop_generated = false; }
static MlpDesc mlp_desc(int32_t n_layers, const int32_t *widths, const float *params, const int32_t *member, size_t stride) {
    MlpDesc d = {};
    d.n_layers = n_layers;
    for (int l = 0; l <= n_layers; l++) d.widths[l] = widths[l];
    d.params = params; d.member = member; d.stride = (int64_t)stride;
    return d;
}

extern "C" int clothhip_set_policy_mlp(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, size_t n_params) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (n_layers == 0) { drop_network(h); return 0; }
    if (int rc = check_mlp_shape(h, n_layers, widths)) return rc;
    if (!params) return fail(CLOTHHIP_EINVAL, "NULL argument");
    const size_t need = mlp_param_count(n_layers, widths);
    if (n_params != need) return fail(CLOTHHIP_EINVAL, "n_params = %zu, these widths hold %zu parameters", n_params, need);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));      // nothing in flight reads the blob reserve() may free
    drop_network(h);                                // from here on the old network is gone: a failure below leaves the handle without one
    if (int rc = h->d_mlp.reserve(need * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->d_mlp, params, need * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));      // the host blob is never retained
    h->mlp = mlp_desc(n_layers, widths, h->d_mlp, nullptr, 0);
    h->mlp_n_params = need;
    return 0;
}

// ---- a population: one network per env slot (cloth_policy_mlp.hpp MlpDesc::member, cloth_policy_population.hpp) ----------------------------------
static int upload_members(clothhip_handle *h, const int32_t *member) {
    if (int rc = h->d_member.reserve((size_t)h->E * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->d_member, member, (size_t)h->E * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_set_policy_population(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *params, int32_t G,
                                              const int32_t *member) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (n_layers == 0) { drop_network(h); return 0; }
    if (int rc = check_mlp_shape(h, n_layers, widths)) return rc;
    if (!params) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (G < 1) return fail(CLOTHHIP_EINVAL, "G = %d: a population has at least one network", G);
    if (int rc = check_members(member, h->E, G, "member")) return rc;
    const size_t n = mlp_param_count(n_layers, widths), stride = population_stride(n);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    drop_network(h);                                // as clothhip_set_policy_mlp: a failure below leaves the handle without a network
    if (int rc = h->d_pop.reserve((size_t)G * stride * 4)) return rc;
    HIPCHECK(hipMemsetAsync(h->d_pop, 0, (size_t)G * stride * 4, h->stream));      // the pad is zeros
    HIPCHECK(hipMemcpy2DAsync(h->d_pop, stride * 4, params, n * 4, n * 4, (size_t)G, hipMemcpyHostToDevice, h->stream));
    if (int rc = upload_members(h, member)) return rc;
    h->mlp = mlp_desc(n_layers, widths, h->d_pop, h->d_member, stride);
    h->mlp_n_params = n; h->pop_rows = G;
    return 0;
}

extern "C" int clothhip_set_policy_members(clothhip_handle *h, const int32_t *member) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pop_rows < 1) return fail(CLOTHHIP_ESTATE, "no population on this handle: call clothhip_set_policy_population or clothhip_policy_population_perturb first");
    if (int rc = check_members(member, h->E, h->pop_rows, "member")) return rc;
    HIPCHECK(hipSetDevice(h->device));
    return upload_members(h, member);
}

extern "C" int clothhip_get_policy_mlp(clothhip_handle *h, int64_t g, float *out, size_t n_params) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle");
    const int64_t rows = h->pop_rows ? h->pop_rows : 1;
    if (g < 0 || g >= rows) return fail(CLOTHHIP_EINVAL, "g = %lld outside [0, %lld)", (long long)g, (long long)rows);
    if (!out) return fail(CLOTHHIP_EINVAL, "out is NULL");
    if (n_params != h->mlp_n_params && !(h->pop_rows && n_params == (size_t)h->mlp.stride))
        return fail(CLOTHHIP_EINVAL, "n_params = %zu, the network holds %zu parameters", n_params, h->mlp_n_params);
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(out, h->mlp.params + (size_t)g * (size_t)h->mlp.stride, n_params * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_policy_population_perturb(clothhip_handle *h, int32_t n_layers, const int32_t *widths, const float *center, int32_t G,
                                                  float sigma, uint64_t seed, int32_t flags, const int32_t *member) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (int rc = check_mlp_shape(h, n_layers, widths)) return rc;
    if (!center) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (flags & ~CLOTHHIP_POP_ANTITHETIC) return fail(CLOTHHIP_EINVAL, "unknown flags 0x%x", flags);
    const bool anti = (flags & CLOTHHIP_POP_ANTITHETIC) != 0;
    if (G < 1 || G > POP_MAX_G) return fail(CLOTHHIP_EINVAL, "G = %d outside [1, %d]", G, POP_MAX_G);
    if (anti && (G & 1)) return fail(CLOTHHIP_EINVAL, "G = %d: antithetic perturbations come in pairs, G must be even", G);
    if (!std::isfinite(sigma)) return fail(CLOTHHIP_EINVAL, "sigma is not finite");
    if (int rc = check_members(member, h->E, (int64_t)G + 1, "member")) return rc;
    const size_t n = mlp_param_count(n_layers, widths), stride = population_stride(n), rows = (size_t)G + 1;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    drop_network(h);
    if (int rc = h->d_pop.reserve(rows * stride * 4)) return rc;
    if (int rc = h->d_pop_center.reserve(n * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->d_pop_center, center, n * 4, hipMemcpyHostToDevice, h->stream));
    PopulationPerturbArgs a;
    memset(&a, 0, sizeof(a));
    a.center = h->d_pop_center; a.rows = h->d_pop; a.n_params = n; a.stride = stride; a.seed = seed;
    a.K = anti ? G / 2 : G; a.antithetic = anti ? 1 : 0; a.sigma = sigma;
    const size_t per_row = (stride / 4 + POP_THREADS - 1) / POP_THREADS;
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_population_perturb, dim3((unsigned)per_row, (unsigned)(a.K + 1)), dim3(POP_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;                                  // clothhip_last_kernel_ms: this kernel
    if (int rc = upload_members(h, member)) return rc;      // (synchronises: the host centre is never retained)
    h->mlp = mlp_desc(n_layers, widths, h->d_pop, h->d_member, stride);
    h->mlp_n_params = n; h->pop_rows = (int64_t)rows;
    h->pop_generated = true; h->pop_seed = seed; h->pop_sigma = sigma; h->pop_flags = flags;
    return 0;
}

extern "C" int clothhip_policy_population_combine(clothhip_handle *h, const float *coef, int32_t K, float *out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->pop_rows < 1) return fail(CLOTHHIP_ESTATE, "no population on this handle: call clothhip_policy_population_perturb first");
    if (!h->pop_generated) return fail(CLOTHHIP_ESTATE, "this population was uploaded (clothhip_set_policy_population), not generated: there are no perturbations to sum");
    if (!coef || !out) return fail(CLOTHHIP_EINVAL, "NULL argument");
    const int64_t G = h->pop_rows - 1, want = (h->pop_flags & CLOTHHIP_POP_ANTITHETIC) ? G / 2 : G;
    if (K != want) return fail(CLOTHHIP_EINVAL, "K = %d, this population has %lld perturbations", K, (long long)want);
    const size_t n = h->mlp_n_params;
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = h->d_pop_coef.reserve((size_t)K * 4)) return rc;
    if (int rc = h->d_pop_out.reserve(n * 4)) return rc;
    HIPCHECK(hipMemcpyAsync(h->d_pop_coef, coef, (size_t)K * 4, hipMemcpyHostToDevice, h->stream));
    PopulationCombineArgs a;
    memset(&a, 0, sizeof(a));
    a.coef = h->d_pop_coef; a.out = h->d_pop_out; a.n_params = n; a.seed = h->pop_seed; a.K = K;
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_population_combine, dim3((unsigned)((n + POP_THREADS - 1) / POP_THREADS)), dim3(POP_THREADS), 0, h->stream, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    HIPCHECK(hipMemcpyAsync(out, h->d_pop_out, n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- clothhip_policy_eval: one workgroup per row --------------------------------------------------------------------------------
struct PolicyEvalArgs {
    MlpDesc mlp;
    const int32_t *members;  // [n]: row r runs the blob at mlp.params + members[r] * mlp.stride; nullptr: every row runs mlp.params
    const float *rows;       // [n][3P] '1d' observations, or nullptr: the SoA state below
    const void *pos;         // [n][3][Ppad], handle precision
    int32_t P, Ppad;
    double *out;             // [n][4]
};
template <typename T> __global__ __launch_bounds__(256) void k_policy_eval(PolicyEvalArgs A) {
    __shared__ float buf[2 * MLP_MAX_WIDTH];
    const size_t r = blockIdx.x;
    const int tid = threadIdx.x;
    MlpDesc d = A.mlp;
    if (A.members != nullptr) d.params += (size_t)A.members[r] * (size_t)d.stride;
    if (A.rows != nullptr) {
        const float *x = A.rows + r * 3 * (size_t)A.P;
        mlp_eval(d, [x](int i) -> float { return x[i]; }, buf, tid, 256);
    } else {
        const T *p = (const T *)A.pos + r * 3 * (size_t)A.Ppad;
        const int Ppad = A.Ppad;
        mlp_eval(d, [p, Ppad](int i) -> float { const int q = i / 3, ax = i - 3 * q; return (float)p[ax * Ppad + q]; }, buf, tid, 256);
    }
    if (tid < MLP_OUT) A.out[r * MLP_OUT + tid] = (double)buf[mlp_out_offset(A.mlp.n_layers) + tid];
}

// rows per chunk: the uploaded rows of one chunk take at most 32 MB, whatever n is
static size_t policy_eval_chunk(int P) {
    const size_t c = ((size_t)32 << 20) / ((size_t)3 * P * 4);
    return c < 1 ? 1 : (c > 65536 ? 65536 : c);
}

// both evaluation entries; members == nullptr: every row under the shared network
static int policy_eval_rows(clothhip_handle *h, const float *obs_rows, int64_t n, const int32_t *members, double *actions_out) {
    if (n < 0) return fail(CLOTHHIP_EINVAL, "n < 0");
    if (!obs_rows && n != h->E) return fail(CLOTHHIP_EINVAL, "n = %lld, the handle's state holds %d cloths", (long long)n, h->E);
    if (!actions_out && n > 0) return fail(CLOTHHIP_EINVAL, "actions_out is NULL");
    if (int rc = check_idle(h)) return rc;
    if (h->mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "no network on this handle: call clothhip_set_policy_mlp first");
    if (!members && h->pop_rows)
        return fail(CLOTHHIP_ESTATE, "this handle holds a population of networks: clothhip_policy_eval_members says which one evaluates a row");
    if (n == 0) return 0;
    if (members) if (int rc = check_members(members, n, h->pop_rows ? h->pop_rows : 1, "members")) return rc;
    HIPCHECK(hipSetDevice(h->device));
    const size_t row = (size_t)3 * h->P, chunk = policy_eval_chunk(h->P), cmax = (size_t)n < chunk ? (size_t)n : chunk;
    if (obs_rows) if (int rc = h->d_pe_rows.reserve(cmax * row * 4)) return rc;
    if (int rc = h->d_pe_out.reserve(cmax * MLP_OUT * 8)) return rc;
    if (members) if (int rc = h->d_pe_mem.reserve(cmax * 4)) return rc;
    PolicyEvalArgs a;
    memset(&a, 0, sizeof(a));
    a.mlp = h->mlp; a.P = h->P; a.Ppad = h->Ppad; a.out = h->d_pe_out;
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        const size_t m = (size_t)n - i0 < chunk ? (size_t)n - i0 : chunk;
        if (members) {
            HIPCHECK(hipMemcpyAsync(h->d_pe_mem, members + i0, m * 4, hipMemcpyHostToDevice, h->stream));
            a.members = h->d_pe_mem;
        }
        if (obs_rows) {
            HIPCHECK(hipMemcpyAsync(h->d_pe_rows, obs_rows + i0 * row, m * row * 4, hipMemcpyHostToDevice, h->stream));
            a.rows = h->d_pe_rows;
            hipLaunchKernelGGL(k_policy_eval<float>, dim3((unsigned)m), dim3(256), 0, h->stream, a);
        } else {
            by_precision(h, [&](auto t) {
                using T = decltype(t);
                a.pos = (const T *)h->d_pos + i0 * 3 * h->Ppad;
                hipLaunchKernelGGL(k_policy_eval<T>, dim3((unsigned)m), dim3(256), 0, h->stream, a);
            });
        }
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(actions_out + i0 * MLP_OUT, h->d_pe_out, m * MLP_OUT * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_policy_eval(clothhip_handle *h, const float *obs_rows, int64_t n, double *actions_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    return policy_eval_rows(h, obs_rows, n, nullptr, actions_out);
}
extern "C" int clothhip_policy_eval_members(clothhip_handle *h, const float *obs_rows, int64_t n, const int32_t *members, double *actions_out) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!members && n > 0) return fail(CLOTHHIP_EINVAL, "members is NULL");
    return policy_eval_rows(h, obs_rows, n, members, actions_out);
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
    if (source == CLOTHHIP_OBS_SLOTS || source == CLOTHHIP_OBS_RESETS) {
        if (int rc = check_idle(h)) return rc;
        if (h->f_T < 1) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions launch yet");
        if (source == CLOTHHIP_OBS_SLOTS && !h->f_obs) return fail(CLOTHHIP_ESTATE, "the last clothhip_run_actions launch was not given want_obs");
        if (source == CLOTHHIP_OBS_RESETS && !h->f_robs) return fail(CLOTHHIP_ESTATE, "the last clothhip_run_actions launch was not given want_reset_obs");
    }
    const int64_t n_src = source == CLOTHHIP_OBS_STATE ? (int64_t)h->E : source == CLOTHHIP_OBS_SLOTS ? (int64_t)h->f_T * h->E
                        : source == CLOTHHIP_OBS_RESETS ? (int64_t)h->f_nscr : n;
    if (n != n_src) return fail(CLOTHHIP_EINVAL, "n = %lld, the source holds %lld cloths", (long long)n, (long long)n_src);
    const RenderPlan plan = render_plan(h->Ppad, p->width, p->height, h->dbg.render_lds_kib * 1024);
    if (!plan.fits) return fail(CLOTHHIP_EINVAL, "a one-row band of width %d needs %d B of LDS beside the %d-point grid", p->width, plan.lds, h->P);
    if (n == 0 || (!out && !d_out)) return 0;
    HIPCHECK(hipSetDevice(h->device));
    const size_t npx = (size_t)p->width * p->height, C = format == CLOTHHIP_IMG_RGBD ? 4 : 3, img_bytes = npx * C;
    const size_t chunk = (size_t)render_obs_chunk(npx), cmax = (size_t)n < chunk ? (size_t)n : chunk;
    const bool need_depth = format != CLOTHHIP_IMG_RGB, have_flags = valid || swap;
    if (!d_out) if (int rc = h->d_ro_img.reserve(cmax * img_bytes)) return rc;
    if (need_depth) if (int rc = h->d_ro_depth.reserve(cmax * npx * 4)) return rc;
    if (source == CLOTHHIP_OBS_HOST) if (int rc = h->d_ro_src.reserve(cmax * 3 * h->P * 4)) return rc;
    if (have_flags) if (int rc = h->d_ro_flags.reserve(2 * chunk)) return rc;
    RenderObsArgs a;
    memset(&a, 0, sizeof(a));
    fill_scene(a.s, h, p);
    a.rows = plan.rows; a.bands = plan.bands; a.format = format; a.C = (int)C;
    const bool soa = source == CLOTHHIP_OBS_STATE;
    a.src_stride = soa ? 3LL * h->Ppad : 3LL * h->P;
    a.depth = need_depth ? (float *)h->d_ro_depth : nullptr;
    const unsigned wg_per_image = h->dbg.render_walk ? 1 : plan.bands;      // one workgroup per band, or one that walks them all
    const float *d_table = source == CLOTHHIP_OBS_SLOTS ? (const float *)h->d_fobs : source == CLOTHHIP_OBS_RESETS ? (const float *)h->d_frobs : nullptr;
    HIPCHECK(hipFuncSetAttribute((const void *)k_render_obs<float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHECK(hipFuncSetAttribute((const void *)k_render_obs<float, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHECK(hipFuncSetAttribute((const void *)k_render_obs<double, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        const size_t m = (size_t)n - i0 < chunk ? (size_t)n - i0 : chunk;
        if (have_flags) {
            uint8_t *fl = (uint8_t *)h->d_ro_flags;
            if (valid) HIPCHECK(hipMemcpyAsync(fl, valid + i0, m, hipMemcpyHostToDevice, h->stream));
            if (swap) HIPCHECK(hipMemcpyAsync(fl + chunk, swap + i0, m, hipMemcpyHostToDevice, h->stream));
            a.valid = valid ? fl : nullptr; a.swap = swap ? fl + chunk : nullptr;
        }
        a.out = d_out ? (uint8_t *)d_out + i0 * img_bytes : (uint8_t *)h->d_ro_img;
        const dim3 grid((unsigned)m, wg_per_image);
        if (soa) {
            by_precision(h, [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL((k_render_obs<T, false>), grid, dim3(256), plan.lds, h->stream, (const T *)h->d_pos + i0 * 3 * h->Ppad, a);
            });
        } else {
            const float *rows = d_table ? d_table + i0 * 3 * h->P : (const float *)h->d_ro_src;
            if (!d_table) HIPCHECK(hipMemcpyAsync(h->d_ro_src, obs_host + i0 * 3 * h->P, m * 3 * h->P * 4, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL((k_render_obs<float, true>), grid, dim3(256), plan.lds, h->stream, rows, a);
        }
        HIPCHECK(hipGetLastError());
        if (need_depth) {
            hipLaunchKernelGGL(k_depth8, dim3((unsigned)m), dim3(256), 0, h->stream, a);
            HIPCHECK(hipGetLastError());
        }
        if (out && !d_out) HIPCHECK(hipMemcpyAsync(out + i0 * img_bytes, h->d_ro_img, m * img_bytes, hipMemcpyDeviceToHost, h->stream));
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

extern "C" int clothhip_set_relaxed_order(clothhip_handle *h, int32_t on) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (on) {
        HIPCHECK(hipSetDevice(h->device));
        HIPCHECK(hipFuncSetAttribute(find_stepper(Variant{4, 512, 2, TAB_LDS_SLOTS, true}, 0, 3), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    h->relaxed = on != 0;
    return 0;
}

extern "C" int clothhip_last_specialised(clothhip_handle *h, int32_t *n_side) {
    if (!h || !n_side) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!h->have_variant) return fail(CLOTHHIP_ESTATE, "no stepper launch on this handle yet");
    *n_side = h->last_spec;
    return 0;
}

extern "C" int clothhip_last_dispatches(clothhip_handle *h, int32_t *n) {
    if (!h || !n) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!h->have_variant) return fail(CLOTHHIP_ESTATE, "no stepper launch on this handle yet");
    *n = h->last_dispatches;
    return 0;
}

extern "C" int clothhip_last_variant(clothhip_handle *h, int32_t v[10]) {
    if (!h || !v) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!h->have_variant) return fail(CLOTHHIP_ESTATE, "no stepper launch on this handle yet");
    memcpy(v, h->last_variant, sizeof(h->last_variant));
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
