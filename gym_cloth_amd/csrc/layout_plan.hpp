// layout_plan.hpp -- which stepper variants and which LDS layouts a handle runs, planned on the host fields of a handle alone (HostPlan).
// Pure host logic: nothing here calls the HIP runtime, so the CPU test suite sweeps it without a device (clothhip_selftest_layout).
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "cloth_common.hpp"
#include "cloth_tables.hpp"
#include "lean_rates.hpp"

namespace clothhip {
// What a stepper launch runs: the variant (stepper_traits.hpp) and its LDS
// carve-up (plan_layouts). scratch_have / scratch_need: the LDS behind the hash table that the in-kernel metrics of
// the episode launches borrow, and what they need.
struct Layout { Variant v; int cell_copy, lds_bytes, HT, ht_bits, scratch_have, scratch_need; };

// metrics_block (cloth_metrics.hpp) for a grid of P points: it sorts NS values (the next power of two >= P) and its hull's monotone chain holds
// at most m + 1 <= P + 1 points (NH)
struct MetricsDims { int NS, NH; };
static inline MetricsDims metrics_dims(int P, int Ppad) { int n = 1; while (n < P) n <<= 1; return {n, Ppad + 8}; }
// ... and its LDS scratch: two sort buffers of NS values in the handle's precision, 64 doubles, the hull stack (NH points, or NH u16 indices)
static inline int metrics_scratch_bytes(MetricsDims d, int tsz, bool hull_idx) {
    return hull_idx ? 2 * d.NS * tsz + 64 * 8 + ((2 * d.NH + 15) / 16) * 16 : 2 * d.NS * tsz + (2 * d.NH + 64) * 8;
}

// Every CLOTHHIP_DEBUG_* switch, read here and nowhere else. The planning switches are read when a handle is created
// (clothhip_create, clothhip_selftest_layout) and kept on it; NOSPEC, ONE_LAUNCH and COLD are read again at every launch.
struct DebugKnobs {
    bool w8_off = false;         // W8=0: the four-wave standard builds of the 25x25 class (only the value 0 switches)
    bool nt1024 = false;         // NT1024 (set at all): 1024 x 3 instead of 512 x 5 for the grids of 769 .. 2 560 points
    int tab_lds = INT_MAX;       // TAB_LDS: caps the standard layout's TAB code (TAB_STREAM < TAB_LDS)
    bool rest_reg = true;        // REST_REG=0: no rest lengths in registers
    bool cell_copy = true;       // CELL_COPY=0: no cell-ordered record copy (the switch can only turn it off)
    bool lean_set = false;       // LEAN: 0 never the LEAN arithmetic, 8 (or 2) its eight-wave build, 3 (or 1) / 4 / 5 / 6 its build for that
    int lean = 0;                //   many cloths per CU; any value also keeps clothhip_create from lowering the residency after its occupancy query
    bool large2_set = false, large2 = false;   // LARGE2: 0 / 1 one / two large-grid cloths per CU
    int phase_mask = 15;         // PHASES: phase ablation mask
    bool nospec = false;         // NOSPEC (nonzero): the generic build instead of the grid-specialised one
    bool one_launch = false;     // ONE_LAUNCH (set at all): a time-sliced episode launch as one dispatch, not one per generation
    int render_lds_kib = 160;    // RENDER_LDS: LDS budget in KiB of a clothhip_render_obs workgroup (smaller: shorter bands, more workgroups per CU)
    bool render_walk = false;    // RENDER_WALK (nonzero): one workgroup walks all bands of an image instead of one workgroup per band
    bool cold_build = false;     // COLD (nonzero): every episode launch takes the build that carries the tier-2 resets and the cold policies (tools/policy_bench.py)
};
static DebugKnobs read_debug_knobs() {
    DebugKnobs k;
    if (const char *t = getenv("CLOTHHIP_DEBUG_W8")) k.w8_off = atoi(t) == 0;
    k.nt1024 = getenv("CLOTHHIP_DEBUG_NT1024") != nullptr;
    if (const char *t = getenv("CLOTHHIP_DEBUG_TAB_LDS")) k.tab_lds = atoi(t);
    if (const char *t = getenv("CLOTHHIP_DEBUG_REST_REG")) k.rest_reg = atoi(t) != 0;
    if (const char *t = getenv("CLOTHHIP_DEBUG_CELL_COPY")) k.cell_copy = atoi(t) != 0;
    if (const char *t = getenv("CLOTHHIP_DEBUG_LEAN")) { k.lean_set = true; k.lean = atoi(t); }
    if (const char *t = getenv("CLOTHHIP_DEBUG_LARGE2")) { k.large2_set = true; k.large2 = atoi(t) != 0; }
    if (const char *t = getenv("CLOTHHIP_DEBUG_PHASES")) k.phase_mask = atoi(t);
    if (const char *t = getenv("CLOTHHIP_DEBUG_NOSPEC")) k.nospec = atoi(t) != 0;
    k.one_launch = getenv("CLOTHHIP_DEBUG_ONE_LAUNCH") != nullptr;
    if (const char *t = getenv("CLOTHHIP_DEBUG_RENDER_LDS")) { const int v = atoi(t); if (v >= 1 && v <= 160) k.render_lds_kib = v; }
    if (const char *t = getenv("CLOTHHIP_DEBUG_RENDER_WALK")) k.render_walk = atoi(t) != 0;
    if (const char *t = getenv("CLOTHHIP_DEBUG_COLD")) k.cold_build = atoi(t) != 0;
    return k;
}

// The host fields of a handle, all that init_host_fields and plan_layouts read and write: clothhip_handle adds what lives on a device
struct HostPlan {
    ClothParams prm{};
    int E = 0, N = 0, P = 0, Ppad = 0, S = 0, Spad = 0, precision = 0;
    size_t tsz = 8;
    Topology topo;
    WindowTable wt;
    std::vector<uint32_t> gather;       // the gather table (host copy of d_gather): the LEAN stencil checks read it
    DebugKnobs dbg;
    int n_cus = 0;
    // LEAN stepper (fp32, n_side <= 27, batches of >= 1024 cloths): 168 VGPRs and 33 KB of LDS per cloth -> three cloths per CU.
    // It needs ONE shared rest table whose fp32 values are one per spring type (checked on the device's table whenever that table
    // may have changed) and the regular gather stencil (checked once); otherwise the (0, false) variant runs on the same layout.
    bool lean = false, lean_stencil_ok = false;
    int lean_r = 3;         // cloths per CU the chosen LEAN build is compiled for (3: 168 VGPRs, 4: 128 VGPRs; 2: eight waves per cloth, table in LDS; 1: the large grids)
    // the two layouts a handle may run (plan_layouts); which one runs now is the handle's (lean_refresh)
    Layout lay_std = {Variant{8, 256, 3, TAB_STREAM, false}, 0, 0, 0, 0, 0, 0}, lay_lean = {Variant{8, 256, 3, TAB_STREAM, true}, 0, 0, 0, 0, 0, 0};
};

// The LDS a layout leaves the in-kernel metrics (from the hash table to the end of the allocation) against what they need; the
// allocation is padded behind the layout's end when that fits the budget (the kernel addresses LDS by the layout's offsets: bytes
// behind `total` are free). False: the episode launches cannot run on this layout.
static bool fit_scratch(const HostPlan *h, Layout &L, int budget) {
    const LdsLayout lay = lds_layout(L.v, h->Ppad, h->Spad, L.HT, L.cell_copy);
    L.scratch_need = metrics_scratch_bytes(metrics_dims(h->P, h->Ppad), L.v.tsz, L.v.hull_as_indices());
    if (L.lds_bytes < lay.total) L.lds_bytes = lay.total;
    if (L.lds_bytes - lay.hkey < L.scratch_need && lay.hkey + L.scratch_need <= budget) L.lds_bytes = (lay.hkey + L.scratch_need + 15) / 16 * 16;
    L.scratch_have = L.lds_bytes - lay.hkey;
    return L.scratch_have >= L.scratch_need;
}

// LDS a workgroup may use when r workgroups are to share a CU: LDS is allocated in granules of 1 280 bytes on gfx950 (128 granules = the CU's
// 160 KiB), so r cloths fit when each takes at most floor(128 / r) granules -- 160 KiB / r overstates that for r = 3, 5, 6.
static constexpr int LDS_GRANULE = 1280;
static constexpr int lds_budget(int r) { return (128 / (r < 1 ? 1 : r)) * LDS_GRANULE; }
static_assert(lds_budget(1) == 160 * 1024 && lds_budget(2) == 80 * 1024 && lds_budget(4) == 40 * 1024, "granule arithmetic");

// A layout of variant v with a hash table of HT (a power of two) slots: the cell-ordered record copy for the collision
// pre-check is taken only if the layout with it fits `budget` (and CLOTHHIP_DEBUG_CELL_COPY allows it). The scratch of the in-kernel
// metrics is the caller's (fit_scratch).
static Layout make_layout(const HostPlan *h, Variant v, int HT, int budget) {
    const int cc = h->dbg.cell_copy && lds_layout(v, h->Ppad, h->Spad, HT, 1).total <= budget ? 1 : 0;
    int ht_bits = 0;
    while ((1 << ht_bits) < HT) ht_bits++;
    return {v, cc, lds_layout(v, h->Ppad, h->Spad, HT, cc).total, HT, ht_bits, 0, 0};
}

// For particle i: body(k, g) for each stencil position k that exists (lean_valid_mask), g = the particle's slot-th gather entry, slot = how
// many positions below k exist (the gather table is compacted). Stops when body returns false (-1); else the number of entries visited.
template <typename F> static int walk_stencil(const HostPlan *h, int i, F &&body) {
    const uint32_t vm = lean_valid_mask(i / h->N, i % h->N, h->N);
    int slot = 0;
    for (int k = 0; k < HK_SLOTS; k++) {
        if (!((vm >> k) & 1u)) continue;
        if (!body(k, h->gather[(size_t)slot * h->Ppad + i])) return -1;
        slot++;
    }
    return slot;
}

// Which stepper variants and which LDS layouts a handle runs: pure host logic (no HIP call), so that the CPU test suite can sweep it
// over grid sizes and precisions (clothhip_selftest_layout). Fills the standard layout lay_std and, where the LEAN arithmetic applies,
// lay_lean, lean and lean_r.
// max_r: the highest residency the pick may choose (clothhip_create lowers it when the device's occupancy query grants the chosen LEAN
// build fewer workgroups per CU than it was planned for).
static inline void plan_layouts(HostPlan *h, int cus, int max_r = 6) {
    const DebugKnobs &dbg = h->dbg;
    const int tsz = (int)h->tsz, precision = h->precision;
    // threads per cloth x particles per thread (compile-time variants of the stepper)
    // P <= 768 (the 25x25 class, two cloths per CU): EIGHT waves per cloth -- 512 threads x 2 particles, compiled for 128 VGPRs: the cell
    // sweeps have eight ticket takers and the parallel phases two waves per SIMD to hide their LDS latency (+4 % fp32 standard
    // arithmetic, +9 % fp64, +13 % tier 2 over the four-wave 256 x 3 variants, bit-identical; CLOTHHIP_DEBUG_W8=0 selects those)
    const bool small_grid = h->P <= 768;
    int nt, ppt;
    if (small_grid) { nt = dbg.w8_off ? 256 : 512; ppt = dbg.w8_off ? 3 : 2; }
    else if (h->P <= 2560 && !dbg.nt1024) { nt = 512; ppt = 5; }
    else if (h->P <= 3072) { nt = 1024; ppt = 3; } else { nt = 1024; ppt = 4; }
    int HT = 64;
    while (HT <= h->P + h->P / 2) HT <<= 1;
    // large dynamic LDS (up to the CU's 160 KiB) for the stepper kernels. The static tables ride in LDS too
    // as long as TWO cloths still fit per CU (512 cloths = 2 per CU on the 256 CUs of an MI355X).
    // 256-thread variants: two cloths per CU (<= 80 KiB each); the larger ones own the CU (<= 160 KiB)
    const int budget = small_grid ? lds_budget(2) : lds_budget(1);
    Variant vstd{tsz, nt, ppt, TAB_LDS, false};
    vstd.tab = std::min((nt <= 512 && lds_layout(vstd, h->Ppad, h->Spad, HT, 0).total <= budget) ? TAB_LDS : TAB_STREAM, dbg.tab_lds);
    vstd.rest_reg = nt == 256 && precision == CLOTHHIP_F32 && vstd.table_in_lds() && dbg.rest_reg;
    // LEAN variants: three to six cloths per CU instead of two, each stepping at a lower rate (lean_rates.hpp, measured by
    // tools/measure_pick_table.py). A launch runs its cloths in generations of what is resident, so the batch size decides:
    // the largest rate_r / ceil(E / (r * CUs)) wins.
    {
        h->n_cus = cus;
        // substeps/s of ONE resident cloth at 2 (standard), 3 and 4 cloths per CU, relative to the standard variant's: measured
        // by tools/measure_pick_table.py on the bench workload and written to lean_rates.hpp (its output: profiles/)
        // r = 2: the EIGHT-WAVE LEAN build (512 threads x 2 particles, window table in LDS) when the flat palette holds, else the
        // standard variant; r = 3 .. 6: the four-wave LEAN builds with the table streamed from L2 (168 / 128 / 96 / 80 VGPRs; from
        // five per CU on without the cell-ordered record copy: 22.6 KB of LDS per cloth)
        const bool lean_able = small_grid && precision == CLOTHHIP_F32;
        const double rate[5] = {lean_able ? LEAN_RATE_2_PER_CU_8W : 1.0, LEAN_RATE_3_PER_CU, LEAN_RATE_4_PER_CU, LEAN_RATE_5_PER_CU, LEAN_RATE_6_PER_CU};
        double best = 0.0; int best_r = 2;
        for (int r = 2; r <= std::max(2, std::min(6, max_r)); r++) {
            // (r >= 3: the four-wave LEAN layout, table streamed, must fit r times in the CU's LDS -- 27x27 does not at five per CU)
            if (r >= 3 && (!lean_able || lds_layout(lean_four_wave(r), h->Ppad, h->Spad, HT, 0).total > lds_budget(r))) continue;
            const double v = rate[r - 2] / (double)((h->E + r * cus - 1) / (r * cus));
            if (v > best * 1.02) { best = v; best_r = r; }
        }
        h->lean = lean_able;
        h->lean_r = best_r;
        // the large grids (one cloth per CU): the LEAN arithmetic frees the registers of the gather entries and takes the rest lengths
        // off the L2 path, which lets SIXTEEN waves step a cloth at 128 VGPRs (1024 threads x 3 or 4 particles; 50x50: 2.90 M/s
        // standard 512 x 5 -> 3.05 LEAN 512 x 5 -> 3.26 LEAN 1024 x 3); the standard variant stays as the fallback (per-env rest tables)
        if (!small_grid && precision == CLOTHHIP_F32) { h->lean = true; h->lean_r = 1; }
        // fp64, 25x25 class, eight waves per cloth (round 6): the LEAN arithmetic with per-spring ulp offsets (StepArgs::lstc) -- no gather-table and no
        // rest-length loads from L2 in the Hooke gather and the strain pre-pass; same layout class as the standard fp64 variant (two cloths per CU)
        if (small_grid && precision == CLOTHHIP_F64 && nt == 512) { h->lean = true; h->lean_r = 2; }
    }
    if (dbg.lean_set) {      // 0: never; 8 (or 2): the eight-wave build; 3 (or 1) / 4 / 5 / 6: the LEAN build for that many cloths per CU, whatever the batch size
        if (dbg.lean == 0) h->lean = false;
        else if (small_grid && precision == CLOTHHIP_F32) { h->lean = true; h->lean_r = (dbg.lean == 8 || dbg.lean == 2) ? 2 : ((dbg.lean >= 4 && dbg.lean <= 6) ? dbg.lean : 3); }
    }
    if (h->lean) {
        // the arithmetic stencil of the LEAN kernel against the gather table built from the reference's spring list
        h->lean_stencil_ok = true;
        for (int i = 0; i < h->P && h->lean_stencil_ok; i++) {
            const int n = walk_stencil(h, i, [&](int k, uint32_t g) {
                const uint32_t want = (uint32_t)(i + lean_off(k, h->N)) | HK_VALID | (k < HK_SLOTS / 2 ? HK_ASB : 0u) | (lean_bend(k) ? HK_BEND : 0u);
                const uint32_t have = g & (HK_NBR_MASK | HK_VALID | HK_ASB | HK_BEND);
                const int sp = h->wt.spring_at[(g >> HK_POS_SHIFT) & HK_POS_MASK];
                const int ty = sp >= 0 ? h->topo.type[sp] : -1;
                const int want_ty = lean_bend(k) ? SPRING_BENDING : (lean_shear(k) ? SPRING_SHEARING : SPRING_STRUCTURAL);
                return have == want && ty == want_ty;
            });
            // (and the entry behind the last one the stencil has must be empty)
            if (n < 0 || (n < HK_SLOTS && (h->gather[(size_t)n * h->Ppad + i] & HK_VALID))) h->lean_stencil_ok = false;
        }
        if (!h->lean_stencil_ok) h->lean = false;
    }
    // the cell-ordered record copy for the collision pre-check is taken only if it does not cost the table its place
    h->lay_std = make_layout(h, vstd, HT, budget);
    // the in-kernel metrics of the episode launches borrow the LDS from the hash table on (the window table in front of it stays
    // resident). With the table in LDS but no room for the cell-ordered copy that region can be too small (fp64 21, 22, 30-32;
    // fp32 41-43): the allocation is then padded behind the layout's end, or, if the budget forbids that, the table leaves LDS
    if (!fit_scratch(h, h->lay_std, budget) && vstd.table_in_lds()) {
        h->lay_std = make_layout(h, Variant{tsz, nt, ppt, TAB_STREAM, false}, HT, budget);
        fit_scratch(h, h->lay_std, budget);
    }
    if (!h->lean) return;
    if (precision == CLOTHHIP_F64) {                     // fp64 LEAN: table streamed, the stencil constants in LDS
        h->lay_lean = make_layout(h, Variant{tsz, 512, 2, TAB_STREAM, true}, HT, lds_budget(2));
        if (h->lay_lean.lds_bytes > lds_budget(2)) h->lean = false;
    } else if (h->lean_r == 2 && small_grid) {           // eight waves per cloth, two cloths per CU: the standard variant's LDS budget
        h->lay_lean = make_layout(h, Variant{tsz, 512, 2, TAB_LDS_SLOTS, true}, HT, 80 * 1024);
        if (h->lay_lean.lds_bytes > 80 * 1024 || h->P > 1024) h->lean = false;      // (the table must fit beside a second cloth)
    } else if (h->lean_r == 1) {                         // the whole CU: same LDS budget as the standard variant of these grids
        h->lay_lean = make_layout(h, Variant{tsz, 1024, h->P <= 3072 ? 3 : 4, TAB_LARGE_1, true}, HT, 160 * 1024);
        // TWO large-grid cloths per CU (eight waves each, 128 VGPRs) when the batch has more cloths than the device has CUs and it
        // pays by the measured rates: <= 80 KB of LDS per cloth -- no cell-ordered copy, and a hash table of just enough slots
        // (not a power of two: > P, so that a free slot always exists, and large enough that the in-kernel metrics' scratch fits)
        const Variant v2{tsz, 512, 5, TAB_LARGE_2, true};
        const int need2 = metrics_scratch_bytes(metrics_dims(h->P, h->Ppad), tsz, v2.hull_as_indices());
        int ht2 = (h->P / 64 + 2) * 64;
        auto lay2 = [&]() { return lds_layout(v2, h->Ppad, h->Spad, ht2, 0); };
        while (lay2().total - lay2().hkey < need2) ht2 += 64;
        const int lds2 = lay2().total;
        const int gens1 = (h->E + h->n_cus - 1) / h->n_cus, gens2 = (h->E + 2 * h->n_cus - 1) / (2 * h->n_cus);
        const bool fits2 = h->P <= 2560 && lds2 <= 80 * 1024;
        if (dbg.large2_set ? dbg.large2 && fits2 : fits2 && LEAN_RATE_LARGE_2_PER_CU / gens2 > 1.02 / gens1) {
            h->lay_lean = {v2, 0, lds2, ht2, 0, 0, 0}; h->lean_r = 2;
        }
    } else {                                             // the four-wave LEAN builds, window table streamed from L2, 33 KB of LDS
        h->lay_lean = make_layout(h, lean_four_wave(h->lean_r), HT, lds_budget(h->lean_r));
    }
    // the in-kernel metrics borrow the region behind the hash table (clothhip_fused_supported): it must hold them here too
    if (!fit_scratch(h, h->lay_lean, lds_budget(h->lean_r))) h->lean = false;
}

// The host fields of a handle -- grid, topology, window and gather tables, debug switches: nothing here touches a device (clothhip_create,
// and clothhip_selftest_layout, which plans on a HostPlan that is no handle)
static inline void init_host_fields(HostPlan *h, const ClothParams &p, int n_envs, int precision) {
    h->prm = p; h->E = n_envs; h->precision = precision;
    h->N = p.n_side; h->P = h->N * h->N; h->Ppad = (h->P + 63) / 64 * 64;
    h->tsz = precision == CLOTHHIP_F64 ? 8 : 4;
    h->topo = build_topology(h->N);
    h->wt = build_windows(h->topo, build_levels(h->topo));
    h->S = h->topo.S; h->Spad = h->wt.n_slots;               // rest-length arrays are kept in window-table slot order
    h->dbg = read_debug_knobs();
    h->gather = build_gather(h->topo, h->wt, h->Ppad);
}

// Every layout the handle may run (the standard one always; the LEAN one while its palette holds) holds the in-kernel metrics' scratch
static inline bool fused_supported(const HostPlan &h) {
    return h.lay_std.scratch_have >= h.lay_std.scratch_need && (!h.lean || h.lay_lean.scratch_have >= h.lay_lean.scratch_need);
}
}  // namespace clothhip
