// stepper_traits.hpp -- what ONE compile-time variant of the stepper kernel (episode_loop.hpp: k_run_schedule<T, NT, PPT, TAB, REST_REG, ...>) is:
// the names of the TAB codes and the questions kernel and host ask about a variant, each answered in one place. The kernel forms
// `static constexpr Variant V{sizeof(T), NT, PPT, TAB, REST_REG}` once; the host keeps the same value in Layout (layout_plan.hpp) / StepperRow (stepper_variants.hpp).
#pragma once

namespace clothhip {

// The TAB template argument ("table mode"). The numbers are part of the mangled kernel names (tools/, profiles/) and of what
// clothhip_last_variant / clothhip_selftest_layout report: they never change. Code 0 is three kernels, told apart by the rest of the Variant.
constexpr int
    TAB_LEAN_6 = -3,    // fp32 LEAN, four waves per cloth, built for six cloths per CU (80 VGPRs), window table streamed from L2
    TAB_LEAN_5 = -2,    //   ... five per CU (96 VGPRs)
    TAB_LEAN_4 = -1,    //   ... four per CU (128 VGPRs)
    TAB_STREAM = 0,     // window table + rest lengths streamed from L2. Without REST_REG: standard arithmetic. With it: the fp32 four-wave LEAN
                        //   build for three cloths per CU (256 threads, 168 VGPRs), or the fp64 eight-wave LEAN build (512 x 2, two per CU)
    TAB_LDS = 1,        // standard arithmetic, window table + rest lengths resident in LDS (REST_REG: the owner's rest lengths in registers)
    TAB_LDS_SLOTS = 2,  // fp32 LEAN, table in LDS plus the per-point slot table; 512 x 2: eight waves per cloth at 128 VGPRs, two per CU (the headline)
    TAB_LARGE_1 = 3,    // fp32 LEAN, the large grids: the whole CU for one cloth (1024 threads, sixteen waves), table streamed
    TAB_LARGE_2 = 4;    // fp32 LEAN, the large grids: two 512 x 5 cloths per CU, table streamed
// what LdsLayout (cloth_common.hpp) reserves for the window table
constexpr int LDS_TABLE_NONE = 0, LDS_TABLE = 1, LDS_TABLE_SLOTS = 2;

struct Variant {
    int tsz, nt, ppt, tab;      // sizeof(T), threads per cloth, particles per thread, TAB code
    bool rest_reg;              // REST_REG: rest lengths in registers (TAB_LDS) / the LEAN arithmetic (every other code)

    constexpr bool operator==(const Variant &o) const { return tsz == o.tsz && nt == o.nt && ppt == o.ppt && tab == o.tab && rest_reg == o.rest_reg; }
    // LEAN arithmetic: the 12-slot gather stencil recomputed from the grid position instead of held in 36 registers, rest lengths from a
    // three-value palette (fp32) or palette + per-spring ulp offset (fp64, TAB_STREAM only) instead of 36 more (episode_loop.hpp)
    constexpr bool lean() const { return rest_reg && (tsz == 4 ? tab != TAB_LDS : tab == TAB_STREAM); }
    constexpr bool lean64() const { return lean() && tsz == 8; }      // ... its stencil table (Ppad x 16 bytes) rides in LDS in front of the hash table
    // REST_REG proper: the owned particles' rest lengths in registers (the LEAN arithmetic has its palette instead)
    constexpr bool rest_in_registers() const { return rest_reg && !lean(); }
    constexpr bool table_in_lds() const { return tab == TAB_LDS || tab == TAB_LDS_SLOTS; }
    constexpr int lds_table_mode() const { return tab == TAB_LDS_SLOTS ? LDS_TABLE_SLOTS : (table_in_lds() ? LDS_TABLE : LDS_TABLE_NONE); }
    // the table slots of every particle's six own springs in LDS: the LEAN strain pre-pass reads them there, not from the L2-resident gather table
    constexpr bool has_point_slots() const { return tab == TAB_LDS_SLOTS; }
    // the strain sweep's lean walk with its read-ahead: not below TAB_LDS (the four-wave builds for three to six cloths per CU do better
    // without: 768 cloths 24.9 -> 25.2 M/s, 1 024: 31.4 -> 31.7, 1 280: +-0, 1 536: 33.8 -> 34.2); the eight-wave headline build loses 2.8 % without it
    constexpr bool sweep_read_ahead() const { return tab >= TAB_LDS; }
    // Cloths per CU the build is compiled for, i.e. its VGPR cap. fp32 LEAN: by the code (three .. six per CU: 168 / 128 / 96 / 80 VGPRs).
    // Everything else: two per CU for the 25x25 class (up to 1 024 particle slots per cloth), the whole CU for the larger grids.
    constexpr int built_for_cloths_per_cu() const {
        if (lean() && tsz == 4) return tab == TAB_LARGE_1 ? 1 : ((tab == TAB_LDS_SLOTS || tab == TAB_LARGE_2) ? 2 : 3 + (TAB_STREAM - tab));
        return nt * ppt <= 1024 ? 2 : 1;
    }
    // __launch_bounds__' second argument, waves per SIMD: that many cloths of nt / 64 waves over the CU's four SIMDs
    constexpr int waves_per_eu() const { return built_for_cloths_per_cu() * (nt / 64) / 4; }
    // The in-kernel metrics' hull stack as u16 indices (same arithmetic, an eighth of the LDS): the variants whose LDS is tight -- two large-grid
    // cloths per CU, five / six 25x25 cloths per CU, the fp64 instantiation of the large grids (50x50: 71 KB of scratch instead of 107 KB,
    // which is what lets its episode launches exist at all) and the 1024 x 4 variants (64x64)
    constexpr bool hull_as_indices() const { return tab == TAB_LARGE_2 || tab <= TAB_LEAN_5 || (tsz == 8 && nt * ppt > 1024) || nt * ppt >= 4096; }
    // self-collision, register-lean form: a thread's owned particles one per trip of the member loop; two per trip where the register cap
    // is 80 (six per CU): 23 fewer spill reloads, +1.6 % at 1 536 cloths
    constexpr bool collide_two_visits_per_trip() const { return tab <= TAB_LEAN_6; }
    // The eight-wave fp32 LEAN build (the headline): waves 0 and 1 own two particles per lane, so every parallel phase lasts as long as their
    // instruction stream (profiles/seed_gather_ab.txt).
    // Its Hooke gather and strain pre-pass: the neighbour of stencil position k is read at the owner's LDS address plus the position's offset (a
    // compile-time constant, the DS instruction's immediate, in the grid-specialised builds), its validity is bit k of the particle's mask -- no
    // table-format gather entry is built and taken apart per slot.
    // An absent position's read (value discarded) must stay inside the cloth's LDS: `cur` gets that many unused records in front of it
    // (2 N <= 54 for the 25x25 class this build exists for; behind `cur` the layout's own regions follow)
    constexpr bool lean_native_gather() const { return tsz == 4 && tab == TAB_LDS_SLOTS; }
    constexpr int cur_front_pad_records() const { return lean_native_gather() ? 64 : 0; }
    // The same build's strain phase: wave 0 enters the walk at window 0 right behind the plane barrier while waves 1-7 run the pre-pass over ALL
    // particles (lanes take t and t + 448, t = tid - 64), and learns the pre-pass's bounds only where its own reach is used up (DESIGN.md 4.1,
    // phase_strain.hpp). Production walk only (strain_sweep_lean, tear_thresh >= 1.1); the profiling builds keep pre-pass, barrier, sweep.
    constexpr bool sweep_starts_early() const { return lean_native_gather() && nt == 512 && ppt == 2; }
    constexpr int early_prepass_threads() const { return nt - 64; }
    // the grid-specialised builds (cloth_common.hpp: spec_*): 50x50 at two cloths per CU has a hash table sized to the LDS left (not a power of
    // two); every specialised 25x25 layout but the builds for five / six per CU has the cell-ordered record copy
    constexpr bool spec_ht_fitted() const { return tab == TAB_LARGE_2; }
    constexpr bool spec_has_cell_copy() const { return tab > TAB_LEAN_5; }
};

// the four-wave fp32 LEAN build for r cloths per CU (three .. six)
constexpr Variant lean_four_wave(int r) { return Variant{4, 256, 3, r >= 4 ? TAB_STREAM - (r - 3) : TAB_STREAM, true}; }

}  // namespace clothhip
