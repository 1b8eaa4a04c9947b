// stepper_variants.hpp -- the compile-time variants of k_run_schedule (episode_loop.hpp), the translation unit each one is compiled in, and
// the table the host picks them from.
//
// The library has 100 instantiations of one kernel template; compiled in one translation unit they took three minutes. They are split into
// GROUPS, one object file each (stepper_inst.hip compiled with -DCLOTHHIP_INST_GROUP=g, in parallel by make); api_run.hip sees them as
// `extern template` declarations and only takes their addresses, through STEPPER_ROWS / find_stepper below (a kernel launch across
// translation units needs no relocatable device code: the host stub is an ordinary symbol, the device code is registered by the object that
// defines it).
//   X(T, NT, PPT, TAB, REST_REG): threads per cloth, particles per thread, table mode, rest lengths in registers / LEAN palette. TAB stays a number here,
//   as a table reads best: stepper_traits.hpp names the codes (-3 .. -1 TAB_LEAN_6 / _5 / _4, 0 TAB_STREAM, 1 TAB_LDS, 2 TAB_LDS_SLOTS, 3 / 4 TAB_LARGE_1 / _2)
#pragma once

#include "episode_loop.hpp"

// standard arithmetic: the 25x25 class, then the large grids. Rest lengths in registers and the 1024 x 4 variant are fp32 only: the plan
// (layout_plan.hpp: plan_layouts) keeps REST_REG to fp32, and fp64 grids of more than 3 072 points exceed the CU's LDS.
#define CLOTH_VARIANTS_SMALL_F32(X) X(float, 512, 2, 1, false) X(float, 512, 2, 0, false) X(float, 256, 3, 1, true) X(float, 256, 3, 1, false) X(float, 256, 3, 0, false)
#define CLOTH_VARIANTS_SMALL_F64(X) X(double, 512, 2, 1, false) X(double, 512, 2, 0, false) X(double, 256, 3, 1, false) X(double, 256, 3, 0, false)
#ifdef CLOTHHIP_FAST_BUILD           // development builds: the 25x25-class variants only (make fast)
#define CLOTH_VARIANTS_LARGE_F32(X)
#define CLOTH_VARIANTS_LARGE_F64(X)
#else
#define CLOTH_VARIANTS_LARGE_F32(X) X(float, 512, 5, 0, false) X(float, 512, 5, 1, false) X(float, 1024, 3, 0, false) X(float, 1024, 4, 0, false)
#define CLOTH_VARIANTS_LARGE_F64(X) X(double, 512, 5, 0, false) X(double, 512, 5, 1, false) X(double, 1024, 3, 0, false)
#endif
// the LEAN builds (fp32 only; 25x25 class: three to six cloths per CU, and eight waves per cloth at two per CU; the large grids: the whole CU
// for a cloth, or two 512 x 5 cloths per CU)
#define CLOTH_VARIANTS_LEAN_SMALL(X, T) X(T, 256, 3, 0, true) X(T, 256, 3, -1, true) X(T, 256, 3, -2, true) X(T, 256, 3, -3, true) X(T, 512, 2, 2, true)
#ifdef CLOTHHIP_FAST_BUILD
#define CLOTH_VARIANTS_LEAN_LARGE(X, T)
#else
#define CLOTH_VARIANTS_LEAN_LARGE(X, T) X(T, 1024, 3, 3, true) X(T, 1024, 4, 3, true) X(T, 512, 5, 4, true)
#endif
// the fp64 LEAN build (25x25 class, eight waves per cloth; rest lengths = palette value + per-spring ulp offset)
#define CLOTH_VARIANTS_LEAN64(X, T) X(T, 512, 2, 0, true)

// the grid-specialised builds (NS = 25 / 50: a BASELINE grid at compile time, cloth_common.hpp spec_*); XS(T, NT, PPT, TAB, RR, NS)
//   A, B: the fp32 LEAN variants of the 25x25 class (the headline; three to six cloths per CU)
//   C: tier 2 at 25x25 (configs[3]'s per-GPU shape: standard arithmetic, per-env rest tables), the fp64 LEAN build at 25x25, 50x50 at two cloths per CU (configs[4])
#define CLOTH_SPEC_A(XS) XS(float, 512, 2, 2, true, 25) XS(float, 256, 3, 0, true, 25) XS(float, 256, 3, -1, true, 25)
#define CLOTH_SPEC_B(XS) XS(float, 256, 3, -2, true, 25) XS(float, 256, 3, -3, true, 25)
#define CLOTH_SPEC_C_F32(XS) XS(float, 512, 2, 1, false, 25) XS(float, 512, 5, 4, true, 50)
#define CLOTH_SPEC_C_F64(XS) XS(double, 512, 2, 0, true, 25)
#ifdef CLOTHHIP_FAST_BUILD
#define CLOTH_SPEC_F32(XS) CLOTH_SPEC_A(XS) CLOTH_SPEC_B(XS)
#define CLOTH_SPEC_F64(XS)
#else
#define CLOTH_SPEC_F32(XS) CLOTH_SPEC_A(XS) CLOTH_SPEC_B(XS) CLOTH_SPEC_C_F32(XS)
#define CLOTH_SPEC_F64(XS) CLOTH_SPEC_C_F64(XS)
#endif

// every variant exists for FUSED = 0 (one external schedule), 1 (episodes, flat tiers), 2 (episodes incl. tier-2 resets and the cold policies)
#define CLOTH_FUSED3(KW, T, NT, PPT, TAB, RR)                                                        \
    KW template __global__ void clothhip::k_run_schedule<T, NT, PPT, TAB, RR, 0>(clothhip::StepArgs<T>);  \
    KW template __global__ void clothhip::k_run_schedule<T, NT, PPT, TAB, RR, 1>(clothhip::StepArgs<T>);  \
    KW template __global__ void clothhip::k_run_schedule<T, NT, PPT, TAB, RR, 2>(clothhip::StepArgs<T>);
#define CLOTH_DECL(T, NT, PPT, TAB, RR) CLOTH_FUSED3(extern, T, NT, PPT, TAB, RR)
#define CLOTH_DEFN(T, NT, PPT, TAB, RR) CLOTH_FUSED3(, T, NT, PPT, TAB, RR)
#define CLOTH_FUSED3_S(KW, T, NT, PPT, TAB, RR, NS_)                                                        \
    KW template __global__ void clothhip::k_run_schedule<T, NT, PPT, TAB, RR, 0, NS_>(clothhip::StepArgs<T>);  \
    KW template __global__ void clothhip::k_run_schedule<T, NT, PPT, TAB, RR, 1, NS_>(clothhip::StepArgs<T>);  \
    KW template __global__ void clothhip::k_run_schedule<T, NT, PPT, TAB, RR, 2, NS_>(clothhip::StepArgs<T>);
#define CLOTH_DECL_S(T, NT, PPT, TAB, RR, NS_) CLOTH_FUSED3_S(extern, T, NT, PPT, TAB, RR, NS_)
#define CLOTH_DEFN_S(T, NT, PPT, TAB, RR, NS_) CLOTH_FUSED3_S(, T, NT, PPT, TAB, RR, NS_)

// The groups (object files). CLOTHHIP_INST_GROUPS of them; stepper_inst.hip defines group CLOTHHIP_INST_GROUP, everybody else declares.
//   0 fp32 standard small   1 fp64 standard small   2 fp32 standard large   3 fp64 standard large   4 LEAN small (+ the relaxed-order companion)   5 LEAN large + fp64 LEAN   6, 7, 8 the grid-specialised builds (CLOTH_SPEC_A / _B / _C)
#define CLOTHHIP_INST_GROUPS 9
#define CLOTH_GROUP_0(M) CLOTH_VARIANTS_SMALL_F32(M)
#define CLOTH_GROUP_1(M) CLOTH_VARIANTS_SMALL_F64(M)
#define CLOTH_GROUP_2(M) CLOTH_VARIANTS_LARGE_F32(M)
#define CLOTH_GROUP_3(M) CLOTH_VARIANTS_LARGE_F64(M)
#define CLOTH_GROUP_4(M) CLOTH_VARIANTS_LEAN_SMALL(M, float)
#define CLOTH_GROUP_5(M) CLOTH_VARIANTS_LEAN_LARGE(M, float) CLOTH_VARIANTS_LEAN64(M, double)
#define CLOTH_RELAXED(KW) KW template __global__ void clothhip::k_run_schedule<float, 512, 2, 2, true, 3>(clothhip::StepArgs<float>);

#ifndef CLOTHHIP_INST_GROUP          // the user of the kernels (api_run.hip): nothing is instantiated here
CLOTH_GROUP_0(CLOTH_DECL) CLOTH_GROUP_1(CLOTH_DECL) CLOTH_GROUP_2(CLOTH_DECL) CLOTH_GROUP_3(CLOTH_DECL) CLOTH_GROUP_4(CLOTH_DECL) CLOTH_GROUP_5(CLOTH_DECL)
CLOTH_SPEC_F32(CLOTH_DECL_S) CLOTH_SPEC_F64(CLOTH_DECL_S)
CLOTH_RELAXED(extern)

namespace clothhip {
// Every instantiation above as one row {Variant{sizeof(T), NT, PPT, TAB, REST_REG}, NS, FUSED, kernel}: the only place the host names a kernel.
struct StepperRow { Variant v; int ns, fused; const void *fn; };
#define CLOTH_ROW(T, NT, PPT, TAB, RR, NS_, F) {{(int)sizeof(T), NT, PPT, TAB, RR}, NS_, F, (const void *)k_run_schedule<T, NT, PPT, TAB, RR, F, NS_>},
#define CLOTH_ROWS_S(T, NT, PPT, TAB, RR, NS_) CLOTH_ROW(T, NT, PPT, TAB, RR, NS_, 0) CLOTH_ROW(T, NT, PPT, TAB, RR, NS_, 1) CLOTH_ROW(T, NT, PPT, TAB, RR, NS_, 2)
#define CLOTH_ROWS(T, NT, PPT, TAB, RR) CLOTH_ROWS_S(T, NT, PPT, TAB, RR, 0)
static const StepperRow STEPPER_ROWS[] = {
    CLOTH_GROUP_0(CLOTH_ROWS) CLOTH_GROUP_1(CLOTH_ROWS) CLOTH_GROUP_2(CLOTH_ROWS) CLOTH_GROUP_3(CLOTH_ROWS) CLOTH_GROUP_4(CLOTH_ROWS) CLOTH_GROUP_5(CLOTH_ROWS)
    CLOTH_SPEC_F32(CLOTH_ROWS_S) CLOTH_SPEC_F64(CLOTH_ROWS_S)
    CLOTH_ROW(float, 512, 2, 2, true, 0, 3)    // the relaxed-order companion (CLOTH_RELAXED)
};
#undef CLOTH_ROWS
#undef CLOTH_ROWS_S
#undef CLOTH_ROW

// The kernel that runs variant v as the grid-specialised build NS = ns (0: the generic one) for FUSED = fused;
// nullptr: not compiled.
inline const void *find_stepper(const Variant &v, int ns, int fused) {
    for (const StepperRow &r : STEPPER_ROWS)
        if (r.v == v && r.ns == ns && r.fused == fused) return r.fn;
    return nullptr;
}
}  // namespace clothhip
#endif
