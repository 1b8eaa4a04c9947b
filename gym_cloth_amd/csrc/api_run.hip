// api_run.hip -- everything that selects or launches a stepper kernel, and the only unit that sees them (stepper_variants.hpp): which layout
// and which build run now, the launches, clothhip_run* / clothhip_run_actions* and what they report afterwards.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "api_handle.hpp"
#include "stepper_variants.hpp"

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
    if (sizeof(T) == 8) { a.pal_struct = (T)h->launch.pal64[SPRING_STRUCTURAL]; a.pal_shear = (T)h->launch.pal64[SPRING_SHEARING]; a.pal_bend = (T)h->launch.pal64[SPRING_BENDING]; }
    else { a.pal_struct = (T)h->launch.pal[SPRING_STRUCTURAL]; a.pal_shear = (T)h->launch.pal[SPRING_SHEARING]; a.pal_bend = (T)h->launch.pal[SPRING_BENDING]; }
    a.lstc = h->launch.d_lstc;
    a.mat = h->n_mixed ? (const DevConsts<T> *)h->d_mat : nullptr;
    a.fz = nullptr;
    return a;
}

// Which grid-specialised kernel (k_run_schedule<..., NS>, NS = 25 or 50) may run layout L -- 0: none, the generic build. Only if the
// variant is one of the specialised ones (stepper_variants.hpp: CLOTH_SPEC_*) AND every constant that build has compiled in
// (cloth_common.hpp: spec_*) is what this handle computed: grid, window table, hash-table size, whether the cell-ordered copy exists, all phases
// on (debug masks take the generic build, as does CLOTHHIP_DEBUG_NOSPEC=1 -- the A/B and the bit-identity test of the two; read at every call).
// (with_palette false: clothhip_create, which prepares every kernel the handle may launch before any rest table has been read back)
static int spec_ns(const clothhip_handle *h, const Layout &L, bool with_palette = true) {
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
        for (int t = 0; t < 3; t++) { const float v = spec_pal(ns, t); if (memcmp(&v, &h->launch.pal[t], 4) != 0) return 0; }
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
        for (int t = 0; t < 3; t++) memcpy(&h->launch.pal64[t], &base[t], 8);
        HIPCHECK(hipMemcpy(h->launch.d_lstc, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    }
    h->launch.lean_ok = ok;
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
        if (!have[ty]) { h->launch.pal[ty] = v; have[ty] = true; }
        else if (memcmp(&h->launch.pal[ty], &v, 4) != 0) ok = false;
    }
    h->launch.lean_ok = ok && have[0] && have[1] && have[2];
    return 0;
}

// Which of the handle's two layouts the next launch runs: the LEAN one when this handle has one and the device's shared rest table is
// its palette (re-checked whenever the table may have changed: per-env tables, i.e. tier 2, or odd rest lengths uploaded by the
// caller switch back), else the standard one. LDS is rebuilt by every launch, so the layout may change from one launch to the next.
static int lean_refresh(clothhip_handle *h) {
    if (h->lean && h->launch.lean_dirty) {
        h->launch.lean_dirty = false; h->launch.lean_ok = false;
        if (h->rest_stride == 0)
            if (int rc = h->precision == CLOTHHIP_F64 ? check_palette_f64(h) : check_palette_f32(h)) return rc;
    }
    if (h->lean) h->launch.on_lean = h->launch.lean_ok && h->rest_stride == 0;
    h->launch.spec_now = spec_ns(h, h->lay());
    return 0;
}

// resident workgroups per CU of a stepper kernel at the active layout's LDS footprint (for clothhip_last_variant): asked once per (kernel,
// LDS bytes), not on every launch -- the step mode launches once per env step
static int cached_occupancy(clothhip_handle *h, const void *fn) {
    const Layout &L = h->lay();
    for (auto &c : h->launch.occ_cache) if (c.fn == fn && c.lds == L.lds_bytes) return c.occ;
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, L.v.nt, (size_t)L.lds_bytes) != hipSuccess) { (void)hipGetLastError(); occ = 0; }
    for (auto &c : h->launch.occ_cache) if (c.fn == nullptr) { c = {fn, L.lds_bytes, occ}; return occ; }
    h->launch.occ_cache[0] = {fn, L.lds_bytes, occ};
    return occ;
}

// For clothhip_create. Large dynamic LDS (up to the CU's 160 KiB) for the stepper kernels: which variant, which layout (plan_layouts)
int clothhip::plan_steppers(clothhip_handle *h) {
    hipDeviceProp_t dp;
    int cus = 256;
    if (hipGetDeviceProperties(&dp, h->device) == hipSuccess && dp.multiProcessorCount > 0) cus = dp.multiProcessorCount;
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
    return 0;
}

template <typename T> static int launch_generations(clothhip_handle *h, const void *fn, int cap, const ClothSchedule *d_sched, const void *d_fz) {
    StepArgs<T> a = make_args<T>(h, d_sched);
    a.fz = (const FusedArgs<T> *)d_fz;
    void *args[] = {&a};
    h->launch.last_dispatches = 0;
    for (int e0 = 0; e0 < h->E; e0 += cap) {
        a.e0 = e0; h->launch.last_dispatches++;
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
    const int ns = fused == 3 ? 0 : h->launch.spec_now;
    const void *fn = find_stepper(V, ns, fused);
    if (!fn) return fail(CLOTHHIP_ESTATE, "no stepper variant for this layout (fused mode %d)", fused);
    const int occ = cached_occupancy(h, fn);
    const int cap = by_generation && occ > 0 && h->n_cus > 0 && !read_debug_knobs().one_launch ? occ * h->n_cus : h->E;
    if (int rc = by_precision(h, [&](auto t) { return launch_generations<decltype(t)>(h, fn, cap, d_sched, d_fz); })) return rc;
    const int32_t v[10] = {V.nt, V.ppt, V.tab, V.rest_reg ? 1 : 0, V.lean() ? 1 : 0, fused, L.lds_bytes, occ, h->n_cus, V.tsz == 4 ? 1 : 0};
    memcpy(h->launch.last_variant, v, sizeof(v)); h->launch.have_variant = true; h->launch.last_spec = ns;
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
static size_t reset_rows(const clothhip_handle *h, const LaunchRequest &req) { return (size_t)h->E * (size_t)(req.n_scripts > 0 ? req.n_scripts : 1); }

// the kernel's argument block of a request that stage_launch has staged: every table the request names, where it lies on the device
template <typename T> static void fill_fused(clothhip_handle *h, const LaunchRequest &req, FusedArgs<T> &f) {
    const MetricsDims md = metrics_dims(h->P, h->Ppad);
    memset(&f, 0, sizeof(f));
    f.nT = req.T; f.policy = req.policy; f.NS = md.NS; f.NH = md.NH;
    f.actions = !req.action_table() ? nullptr : req.actions_on_device ? req.actions : (const double *)h->epi.d_fact;
    f.policy_arg = req.policy_arg ? h->epi.d_fparg : nullptr;
    f.scripts = req.reset_source == ResetSource::scripts ? (const ClothResetScript *)h->epi.d_fscr : nullptr;
    f.num_steps = h->epi.d_fsteps; f.done = h->epi.d_fdone;
    f.records = (ClothStepRecord *)h->epi.d_frec;
    f.resets = req.resets != TableMode::Absent ? (ClothResetRecord *)h->epi.d_frst : nullptr;
    f.obs = req.obs != TableMode::Absent ? (float *)h->epi.d_fobs : nullptr;
    f.reset_obs = req.reset_obs != TableMode::Absent ? (float *)h->epi.d_frobs : nullptr;
    f.flat = (const T *)h->d_flat;
    f.wt_ent = h->d_wt_ent;
    f.rest = (const T *)h->d_rest; f.rest_rw = (T *)h->d_rest; f.rest_stride = h->rest_stride;
    f.grid_dx = h->prm.width * 1.0 / (h->N - 1); f.grid_dy = h->prm.height * 1.0 / (h->N - 1);
    f.levels = h->d_levels; f.n_glevels = h->n_grab_levels; f.E = h->E; f.n_scripts = req.n_scripts; f.budget_ticks = req.budget_ticks;
    f.resume = h->epi.d_resume;
    f.op_ticks = h->epi.d_fticks;
    f.summary = h->epi.d_fsum;
    f.mt = req.reset_source == ResetSource::rng ? h->epi.d_fmt : nullptr; f.rng_tier = req.rng_tier; f.domrand_words = req.domrand_words;
    f.two_thickness = 2 * h->prm.thickness; f.half_thickness = h->prm.thickness / 2.0;
    f.ep = *req.ep;
    f.mlp = h->pol.mlp;
    if (req.expert) {
        f.expert = req.expert; f.resume_labelled = req.resume_labelled ? 1 : 0;
        f.labels = h->epi.d_flab;
        f.expert_mix = req.expert_mix ? (const uint8_t *)h->epi.d_fmix : nullptr;
        f.expert_choice = req.expert == CLOTHHIP_POLICY_HIGHEST_POINT ? (const int32_t *)h->epi.d_fchoice : nullptr;
    }
}

// ---- an expert beside the acting policy (clothhip.h: clothhip_run_actions_expert) ----------------------------------------------------
static bool known_expert(int32_t x) { return x == CLOTHHIP_POLICY_ORACLE_CORNER || x == CLOTHHIP_POLICY_HIGHEST_POINT; }

extern "C" int clothhip_run_actions_expert(clothhip_handle *h, int32_t expert, int32_t T_, const uint8_t *mix, const int32_t *choice) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    h->epi.arm_expert = 0;                              // whatever happens below, an earlier arming is gone
    if (h->epi.last.pending) return fail(CLOTHHIP_ESTATE, "a clothhip_run_actions_begin is in flight: arm the expert before the launch");
    if (!known_expert(expert)) return fail(CLOTHHIP_EINVAL, "unknown expert %d (CLOTHHIP_POLICY_ORACLE_CORNER or CLOTHHIP_POLICY_HIGHEST_POINT)", expert);
    if (T_ < 1 || T_ > 4096) return fail(CLOTHHIP_EINVAL, "T must be in [1, 4096]");
    if (expert == CLOTHHIP_POLICY_HIGHEST_POINT && !choice) return fail(CLOTHHIP_EINVAL, "the highest-point expert needs choice[T][E]: which of the highest points per slot");
    if (h->relaxed) return fail(CLOTHHIP_ESTATE, "clothhip_set_relaxed_order: the relaxed-order companion is a bench-only kernel without an expert");
    for (const Layout *L : {&h->lay_std, &h->lay_lean})
        if ((L == &h->lay_std || h->lean) && !find_stepper(L->v, 0, 2)) return fail(CLOTHHIP_ESTATE, "this handle's stepper variant has no build with the cold policies");
    if (expert == CLOTHHIP_POLICY_ORACLE_CORNER && h->N != 25)
        return fail(CLOTHHIP_ESTATE, "the oracle-corner policy is defined for 25x25 cloths only (analytic.py:106)");
    const size_t n = (size_t)T_ * h->E;
    h->epi.arm_mix = mix != nullptr;
    if (mix) h->epi.h_arm_mix.assign(mix, mix + n);
    if (expert == CLOTHHIP_POLICY_HIGHEST_POINT) h->epi.h_arm_choice.assign(choice, choice + n);
    h->epi.arm_T = T_; h->epi.arm_expert = expert;
    return 0;
}

extern "C" int clothhip_run_actions_labels(clothhip_handle *h, double *labels, void **d_labels) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (h->epi.last.pending) return fail(CLOTHHIP_ESTATE, "a clothhip_run_actions_begin is in flight: call clothhip_run_actions_end first");
    const void *d_lab = nullptr;
    int64_t rows = 0;
    if (int rc = launch_table(h, LaunchTable::labels, &d_lab, &rows)) return rc;
    if (d_labels) *d_labels = const_cast<void *>(d_lab);
    if (labels) {
        HIPCHECK(hipSetDevice(h->device));
        HIPCHECK(hipMemcpyAsync(labels, d_lab, (size_t)rows * 4 * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

// ---- one episode launch: a request (api_handle.hpp), its refusals, its staging, the launch and its record ---------------------------------
// an arming (clothhip_run_actions_expert) is for the next request alone, whatever becomes of it
LaunchRequest clothhip::next_request(clothhip_handle *h) {
    LaunchRequest req;
    req.expert = h->epi.arm_expert; req.expert_mix = h->epi.arm_mix;
    req.resume_labelled = h->epi.last.armed;
    h->epi.arm_expert = 0;
    return req;
}
static TableMode table_mode(int32_t want) { return want == 0 ? TableMode::Absent : want == 2 ? TableMode::Keep : TableMode::Download; }
static uint64_t budget_ticks(double time_budget_ms) { return time_budget_ms > 0 ? (uint64_t)(time_budget_ms * 1e5) : 0; }      // s_memrealtime: 100 MHz

// What a request is refused for before any table on the device is touched, in the order these refusals always had (two more come later,
// each where it always stood: one in stage_launch, one in begin_launch).
static int check_launch(clothhip_handle *h, const LaunchRequest &req) {
    const int T_ = req.T, policy = req.policy, expert = req.expert;
    const bool have_src = req.reset_source != ResetSource::none, tier2 = req.tier2();
    if (!req.ep || !req.num_steps || !req.done) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (h->epi.last.pending) return fail(CLOTHHIP_ESTATE, "a clothhip_run_actions_begin is already in flight");
    if (expert && T_ != h->epi.arm_T) return fail(CLOTHHIP_EINVAL, "T = %d, the expert was armed for %d slots", T_, h->epi.arm_T);
    if (expert && policy != CLOTHHIP_POLICY_TABLE && policy != CLOTHHIP_POLICY_MLP)
        return fail(CLOTHHIP_EINVAL, "only CLOTHHIP_POLICY_TABLE and CLOTHHIP_POLICY_MLP may act beside an expert (policy %d)", policy);
    if (expert && h->relaxed) return fail(CLOTHHIP_ESTATE, "clothhip_set_relaxed_order: the relaxed-order companion is a bench-only kernel without an expert");
    if (T_ < 1 || T_ > 4096) return fail(CLOTHHIP_EINVAL, "T must be in [1, 4096]");
    if (policy != CLOTHHIP_POLICY_TABLE && policy != CLOTHHIP_POLICY_ORACLE_CORNER && policy != CLOTHHIP_POLICY_HIGHEST_POINT && policy != CLOTHHIP_POLICY_MLP)
        return fail(CLOTHHIP_EINVAL, "unknown policy %d", policy);
    if (policy == CLOTHHIP_POLICY_MLP && h->pol.mlp.n_layers < 1) return fail(CLOTHHIP_ESTATE, "the MLP policy needs a network: call clothhip_set_policy_mlp or clothhip_set_policy_population first");
    if (policy == CLOTHHIP_POLICY_MLP && h->relaxed)
        return fail(CLOTHHIP_ESTATE, "clothhip_set_relaxed_order: the relaxed-order companion is a bench-only kernel without the MLP policy");
    if (policy == CLOTHHIP_POLICY_HIGHEST_POINT && !req.policy_arg)
        return fail(CLOTHHIP_EINVAL, "the highest-point policy needs policy_arg[1 + T][E] (construction codes + which of the highest points per slot)");
    if (policy == CLOTHHIP_POLICY_TABLE && !req.actions) return fail(CLOTHHIP_EINVAL, "the table policy needs actions[T][E][4]");
    if (policy == CLOTHHIP_POLICY_ORACLE_CORNER && h->N != 25)
        return fail(CLOTHHIP_ESTATE, "the oracle-corner policy is defined for 25x25 cloths only (analytic.py:106)");
    if (have_src && (req.n_scripts < 1 || req.n_scripts > 255)) return fail(CLOTHHIP_EINVAL, "n_scripts must be in [1, 255]");
    if (req.two_reset_sources) return fail(CLOTHHIP_EINVAL, "resets come either from scripts or from the device-side RNG streams, not both");
    if (req.reset_source == ResetSource::rng && (req.rng_tier < 1 || req.rng_tier > 3)) return fail(CLOTHHIP_EINVAL, "rng_tier must be 1, 2 or 3");
    if (have_src && !tier2 && h->rest_stride != 0)
        return fail(CLOTHHIP_ESTATE, "in-kernel resets of the flat tiers need the shared flat rest table; this handle has per-env rest lengths");
    if (tier2 && h->rest_stride == 0)
        return fail(CLOTHHIP_ESTATE, "in-kernel tier-2 resets rebuild per-env rest lengths; upload per-env rest tables first (clothhip_set_state without CLOTHHIP_REST_SHARED)");
    if (tier2 && (size_t)3 * h->P * 8 > (size_t)160 * 1024) return fail(CLOTHHIP_ESTATE, "grid too large for the tier-2 reset scratch");
    if (!(req.ep->reduce_factor > 0) || req.ep->max_actions < 1) return fail(CLOTHHIP_EINVAL, "bad episode parameters");
    if (h->relaxed && h->n_mixed)
        return fail(CLOTHHIP_ESTATE, "clothhip_set_relaxed_order: the relaxed-order companion is a bench-only kernel; this handle holds per-env materials (clothhip_set_material)");
    HIPCHECK(hipSetDevice(h->device));
    // which of the handle's two layouts runs now (may synchronise and read the rest table back: long before the timed events). A side
    // effect among the checks, and it stays here: the scratch checks below are against THAT layout, not the previous launch's
    if (int rc = lean_refresh(h)) return rc;
    if (h->lay().scratch_have < h->lay().scratch_need)
        return fail(CLOTHHIP_ESTATE, "n_side %d: the in-kernel metrics need %d B of LDS scratch, this variant has %d", h->N, h->lay().scratch_need, h->lay().scratch_have);
    if (policy == CLOTHHIP_POLICY_MLP && h->lay().scratch_have < MLP_SCRATCH_BYTES)
        return fail(CLOTHHIP_ESTATE, "n_side %d: the MLP policy's hidden vectors need %d B of LDS scratch, this variant has %d", h->N, MLP_SCRATCH_BYTES, h->lay().scratch_have);
    return 0;
}

// Reserve, upload and clear every table the request names, and the kernel's argument block. Two things happen on the way, each in the
// place it always had: the previous launch's observation tables stop being readable, and the one refusal that comes after that.
static int stage_launch(clothhip_handle *h, const LaunchRequest &req) {
    const int expert = req.expert;
    HIPCHECK(hipStreamSynchronize(h->stream));
    const size_t E = h->E, nrec = (size_t)req.T * E, nscr = reset_rows(h, req);
    if (int rc = h->epi.d_fz.reserve(1024)) return rc;
    if (int rc = h->epi.d_fsteps.reserve(E * 4)) return rc;
    if (int rc = h->epi.d_fdone.reserve(E)) return rc;
    if (int rc = h->epi.d_fticks.reserve(E * 64)) return rc;
    if (int rc = h->epi.d_fsum.reserve(E * 32)) return rc;
    HIPCHECK(hipMemsetAsync(h->epi.d_fticks, 0, E * 64, h->stream));
    h->epi.last.records = false;                       // (the record table may be reallocated now, and is cleared below: the previous launch's is gone)
    if (int rc = h->epi.d_frec.reserve(nrec * sizeof(ClothStepRecord))) return rc;
    if (int rc = h->epi.d_fscr.reserve(nscr * sizeof(ClothResetScript))) return rc;
    if (int rc = h->epi.d_frst.reserve(nscr * sizeof(ClothResetRecord))) return rc;
    if (req.action_table() && !req.actions_on_device) {
        if (int rc = h->epi.d_fact.reserve(nrec * 4 * 8)) return rc;
        HIPCHECK(hipMemcpyAsync(h->epi.d_fact, req.actions, nrec * 4 * 8, hipMemcpyHostToDevice, h->stream));
    }
    // from here on the previous launch's observation tables may be reallocated or overwritten: they stop being readable now, also if this
    // call fails further down (launch_table then refuses them)
    h->epi.last.invalidate_obs_tables();
    if (req.obs != TableMode::Absent) if (int rc = h->epi.d_fobs.reserve(nrec * 3 * h->P * 4)) return rc;
    // (a refusal behind the invalidation, and it stays there: a launch refused here has taken the tables with it, as clothhip.h says)
    if ((req.reset_obs != TableMode::Absent || req.resets != TableMode::Absent) && req.reset_source == ResetSource::none)
        return fail(CLOTHHIP_EINVAL, "reset outputs without a reset source");
    if (req.reset_obs != TableMode::Absent) {
        if (int rc = h->epi.d_frobs.reserve(nscr * 3 * h->P * 4)) return rc;
        HIPCHECK(hipMemsetAsync(h->epi.d_frobs, 0, nscr * 3 * h->P * 4, h->stream));
    }
    if (req.reset_source == ResetSource::rng) {
        if (int rc = h->epi.d_fmt.reserve(E * MT_WORDS * 4)) return rc;
        HIPCHECK(hipMemcpyAsync(h->epi.d_fmt, req.reset_data, E * MT_WORDS * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (req.policy_arg) {
        const size_t nb = (req.policy == CLOTHHIP_POLICY_HIGHEST_POINT ? (size_t)(1 + req.T) : (size_t)1) * E * 4;
        if (int rc = h->epi.d_fparg.reserve(nb)) return rc;
        HIPCHECK(hipMemcpyAsync(h->epi.d_fparg, req.policy_arg, nb, hipMemcpyHostToDevice, h->stream));
    }
    if (expert) {                                       // labels start as all-ones NaNs: a slot without an action keeps them
        if (int rc = h->epi.d_flab.reserve(nrec * 4 * 8)) return rc;
        HIPCHECK(hipMemsetAsync(h->epi.d_flab, 0xFF, nrec * 4 * 8, h->stream));
        if (req.expert_mix) {
            if (int rc = h->epi.d_fmix.reserve(nrec)) return rc;
            HIPCHECK(hipMemcpyAsync(h->epi.d_fmix, h->epi.h_arm_mix.data(), nrec, hipMemcpyHostToDevice, h->stream));
        }
        if (expert == CLOTHHIP_POLICY_HIGHEST_POINT) {
            if (int rc = h->epi.d_fchoice.reserve(nrec * 4)) return rc;
            HIPCHECK(hipMemcpyAsync(h->epi.d_fchoice, h->epi.h_arm_choice.data(), nrec * 4, hipMemcpyHostToDevice, h->stream));
        }
    }
    if (req.reset_source == ResetSource::scripts) HIPCHECK(hipMemcpyAsync(h->epi.d_fscr, req.reset_data, nscr * sizeof(ClothResetScript), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->epi.d_fsteps, req.num_steps, E * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->epi.d_fdone, req.done, E, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemsetAsync(h->epi.d_frec, 0, nrec * sizeof(ClothStepRecord), h->stream));
    if (req.resets != TableMode::Absent) HIPCHECK(hipMemsetAsync(h->epi.d_frst, 0, nscr * sizeof(ClothResetRecord), h->stream));
    static_assert(sizeof(FusedArgs<double>) <= 1024 && sizeof(FusedArgs<float>) <= 1024, "fused argument block");
    unsigned char fzbuf[1024];
    by_precision(h, [&](auto t) { fill_fused(h, req, *reinterpret_cast<FusedArgs<decltype(t)> *>(fzbuf)); });
    HIPCHECK(hipMemcpyAsync(h->epi.d_fz, fzbuf, 1024, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));          // fzbuf is on this stack frame
    return 0;
}

int clothhip::begin_launch(clothhip_handle *h, const LaunchRequest &req) {
    if (int rc = check_launch(h, req)) return rc;
    if (int rc = stage_launch(h, req)) return rc;
    // (the last refusal, behind the staging, and it stays there: it asks about the layout lean_refresh chose, after every other refusal)
    if (h->relaxed && !(find_stepper(h->lay().v, 0, 3) && h->lay().cell_copy && !req.tier2() && req.policy != CLOTHHIP_POLICY_HIGHEST_POINT))
        return fail(CLOTHHIP_ESTATE, "clothhip_set_relaxed_order: the relaxed-order companion exists for the eight-wave LEAN layout only (fp32, flat tiers, 25x25 class, <= 512 cloths)");
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    // (FUSED 2: the variant that also carries the tier-2 reset code and the cold policies; the relaxed-order companion is one launch)
    const bool cold = req.tier2() || req.policy == CLOTHHIP_POLICY_HIGHEST_POINT || req.policy == CLOTHHIP_POLICY_MLP || req.expert != 0 || read_debug_knobs().cold_build;
    if (int rc = launch_run(h, h->relaxed ? 3 : cold ? 2 : 1, h->d_sched, h->epi.d_fz, !h->relaxed && req.budget_ticks != 0)) return rc;
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    h->have_timing = true;
    h->pending_exec = true;
    LaunchRecord &r = h->epi.last;
    r.T = req.T; r.reset_rows = reset_rows(h, req); r.pending = true;
    r.resets = req.resets != TableMode::Absent; r.rng = req.reset_source == ResetSource::rng;
    r.obs = req.obs; r.reset_obs = req.reset_obs; r.armed = req.expert != 0; r.records = true;
    return 0;
}

extern "C" int clothhip_run_actions_begin(clothhip_handle *h, const ClothEpisodeParams *ep, int32_t T_, int32_t policy,
                                          const double *actions, int32_t actions_on_device, const int32_t *policy_arg,
                                          const ClothResetScript *scripts, int32_t n_scripts, const int32_t *num_steps,
                                          const uint8_t *done, const uint32_t *rng_states, int32_t rng_tier, uint64_t domrand_words,
                                          int32_t want_resets, int32_t want_obs, int32_t want_reset_obs,
                                          double time_budget_ms) {
    if (!h) return fail(CLOTHHIP_EINVAL, "NULL argument");
    LaunchRequest req = next_request(h);                // (takes the arming here, before any refusal: also a call that fails consumes it)
    req.ep = ep; req.T = T_; req.policy = policy;
    req.actions = actions; req.actions_on_device = actions_on_device != 0; req.policy_arg = policy_arg;
    req.reset_source = scripts ? ResetSource::scripts : rng_states ? ResetSource::rng : ResetSource::none;
    req.reset_data = scripts ? (const void *)scripts : (const void *)rng_states;
    req.two_reset_sources = scripts && rng_states;
    req.n_scripts = scripts || rng_states ? n_scripts : 0; req.rng_tier = rng_tier; req.domrand_words = domrand_words;
    req.num_steps = num_steps; req.done = done;
    req.resets = want_resets ? TableMode::Download : TableMode::Absent; req.obs = table_mode(want_obs); req.reset_obs = table_mode(want_reset_obs);
    req.budget_ticks = budget_ticks(time_budget_ms);
    return begin_launch(h, req);
}

// Where a table of the last launch lies, or why it is not there: the one place that knows the record's rule and the tables' row counts.
int clothhip::launch_table(const clothhip_handle *h, LaunchTable which, const void **d_ptr, int64_t *rows) {
    const LaunchRecord &r = h->epi.last;
    const void *p = nullptr;
    int64_t n = (int64_t)r.T * h->E;
    if (which == LaunchTable::labels) {
        if (!r.armed) return fail(CLOTHHIP_ESTATE, "the last episode launch on this handle was not armed with an expert (clothhip_run_actions_expert)");
        p = h->epi.d_flab;
    } else if (which == LaunchTable::records) {
        if (r.T < 1 || !r.records) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions launch whose record table is still on the device");
        p = h->epi.d_frec;
    } else {
        if (r.T < 1) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions launch yet");
        if (which == LaunchTable::obs) {
            if (r.obs == TableMode::Absent) return fail(CLOTHHIP_ESTATE, "the last clothhip_run_actions launch was not given want_obs");
            p = h->epi.d_fobs;
        } else {
            if (r.reset_obs == TableMode::Absent) return fail(CLOTHHIP_ESTATE, "the last clothhip_run_actions launch was not given want_reset_obs");
            p = h->epi.d_frobs; n = (int64_t)r.reset_rows;
        }
    }
    if (d_ptr) *d_ptr = p;
    if (rows) *rows = n;
    return 0;
}

extern "C" int clothhip_run_actions_end(clothhip_handle *h, int32_t *num_steps, uint8_t *done, ClothStepRecord *records,
                                        ClothResetRecord *resets, float *obs, float *reset_obs, uint32_t *rng_states) {
    if (!h || !num_steps || !done || !records) return fail(CLOTHHIP_EINVAL, "NULL argument");
    const LaunchRecord &r = h->epi.last;
    if (!r.pending) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions_begin in flight");
    // (a table announced with 2 stays on the device: no buffer for it)
    if ((resets != nullptr) != r.resets || (obs != nullptr) != (r.obs == TableMode::Download) || (reset_obs != nullptr) != (r.reset_obs == TableMode::Download))
        return fail(CLOTHHIP_EINVAL, "the output buffers must match the ones announced to clothhip_run_actions_begin");
    if ((rng_states != nullptr) != r.rng) return fail(CLOTHHIP_EINVAL, "rng_states must be given to both halves or to neither");
    HIPCHECK(hipSetDevice(h->device));
    const size_t E = h->E, nrec = (size_t)r.T * E, nscr = r.reset_rows;
    HIPCHECK(hipMemcpyAsync(records, h->epi.d_frec, nrec * sizeof(ClothStepRecord), hipMemcpyDeviceToHost, h->stream));
    if (resets) HIPCHECK(hipMemcpyAsync(resets, h->epi.d_frst, nscr * sizeof(ClothResetRecord), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(num_steps, h->epi.d_fsteps, E * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(done, h->epi.d_fdone, E, hipMemcpyDeviceToHost, h->stream));
    if (obs) HIPCHECK(hipMemcpyAsync(obs, h->epi.d_fobs, nrec * 3 * h->P * 4, hipMemcpyDeviceToHost, h->stream));
    if (reset_obs) HIPCHECK(hipMemcpyAsync(reset_obs, h->epi.d_frobs, nscr * 3 * h->P * 4, hipMemcpyDeviceToHost, h->stream));
    if (rng_states) HIPCHECK(hipMemcpyAsync(rng_states, h->epi.d_fmt, E * MT_WORDS * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->epi.last.pending = false;
    return 0;
}

// clothhip_run_actions_end without its downloads, for a caller inside the library that reads the launch's tables where they lie
// (clothhip_plan_cem scores epi.d_frec on the device): the launch is no longer in flight as far as the handle's state goes; its work is
// still on the handle's stream, and whatever reads its tables is enqueued there after it. No wait, nothing crosses PCIe.
int clothhip::run_actions_end_on_device(clothhip_handle *h) {
    if (!h->epi.last.pending) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions_begin in flight");
    h->epi.last.pending = false;
    return 0;
}

extern "C" int clothhip_run_actions_summary(clothhip_handle *h, double *summary, void **d_summary) {
    if (!h) return fail(CLOTHHIP_EINVAL, "handle is NULL");
    if (!h->epi.d_fsum) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions launch yet");
    if (d_summary) *d_summary = h->epi.d_fsum;
    if (summary) {
        HIPCHECK(hipSetDevice(h->device));
        HIPCHECK(hipMemcpyAsync(summary, h->epi.d_fsum, (size_t)h->E * 32, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

extern "C" int clothhip_run_actions_op_ticks(clothhip_handle *h, uint64_t *ticks) {
    if (!h || !ticks) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!h->epi.d_fticks) return fail(CLOTHHIP_ESTATE, "no clothhip_run_actions launch yet");
    if (int rc = check_idle(h)) return rc;
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipMemcpyAsync(ticks, h->epi.d_fticks, (size_t)h->E * 64, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int clothhip_run_actions(clothhip_handle *h, const ClothEpisodeParams *ep, int32_t T_, int32_t policy,
                                    const double *actions, int32_t actions_on_device, const int32_t *policy_arg,
                                    const ClothResetScript *scripts, int32_t n_scripts, int32_t *num_steps, uint8_t *done,
                                    ClothStepRecord *records, ClothResetRecord *resets, float *obs, float *reset_obs,
                                    double time_budget_ms) {
    if (!h) return fail(CLOTHHIP_EINVAL, "NULL argument");
    LaunchRequest req = next_request(h);                // (also a call that fails below consumes an arming)
    if (!records) return fail(CLOTHHIP_EINVAL, "NULL argument");
    req.ep = ep; req.T = T_; req.policy = policy;
    req.actions = actions; req.actions_on_device = actions_on_device != 0; req.policy_arg = policy_arg;
    if (scripts) { req.reset_source = ResetSource::scripts; req.reset_data = scripts; req.n_scripts = n_scripts; }
    req.num_steps = num_steps; req.done = done;
    req.resets = resets ? TableMode::Download : TableMode::Absent; req.obs = obs ? TableMode::Download : TableMode::Absent;
    req.reset_obs = reset_obs ? TableMode::Download : TableMode::Absent;
    req.budget_ticks = budget_ticks(time_budget_ms);
    if (int rc = begin_launch(h, req)) return rc;
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
    if (!h->launch.have_variant) return fail(CLOTHHIP_ESTATE, "no stepper launch on this handle yet");
    *n_side = h->launch.last_spec;
    return 0;
}

extern "C" int clothhip_last_dispatches(clothhip_handle *h, int32_t *n) {
    if (!h || !n) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!h->launch.have_variant) return fail(CLOTHHIP_ESTATE, "no stepper launch on this handle yet");
    *n = h->launch.last_dispatches;
    return 0;
}

extern "C" int clothhip_last_variant(clothhip_handle *h, int32_t v[10]) {
    if (!h || !v) return fail(CLOTHHIP_EINVAL, "NULL argument");
    if (!h->launch.have_variant) return fail(CLOTHHIP_ESTATE, "no stepper launch on this handle yet");
    memcpy(v, h->launch.last_variant, sizeof(h->launch.last_variant));
    return 0;
}
