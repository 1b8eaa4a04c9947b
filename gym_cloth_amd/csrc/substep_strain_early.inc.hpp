// substep_strain_early.inc.hpp -- strain limit + tear of the eight-wave fp32 LEAN build (Variant::sweep_starts_early): the walk starts while the other
// waves run the pre-pass. A FRAGMENT of substep_strain.inc.hpp (the SWEEP_EARLY branch of its `if constexpr`), textual for the reason given there;
// production builds only (SWEEP_LEAN, no stamps, no census), so none of their instrumentation appears here. Names it uses beyond that file's: e, A.
            // early_ (wave-uniform): wave 0 enters the walk at window 0 right here, behind the plane barrier; waves 1-7 test the springs of ALL
            // particles -- thread t = tid - 64 takes t and t + 448 -- from LDS positions alone (the stencil mask of a particle the thread does not
            // own: lean_valid_mask), publish as ever (any flag, first / last flagged slot) and then count themselves done in misc[17]. No barrier
            // in front of the walk: strain_sweep_lean learns the pre-pass's bounds where its own reach is used up (phase_strain.hpp; DESIGN.md 4.1
            // has the argument that the result is the sequential loop's although the pre-pass reads records the walk is correcting).
            // Not with PH_NOSKIP (walk everything), tear_thresh < 1.1 (strain_sweep) or more particles than 2 x 448: those keep the barriered order.
            constexpr int EARLY_NT = V.early_prepass_threads();
            const bool tic = __builtin_amdgcn_readfirstlane(!(k.tear_thresh < k.c11) ? 1 : 0) != 0;
            const bool early_ = tic && __builtin_amdgcn_readfirstlane((!(pm & PH_NOSKIP) && P <= 2 * EARLY_NT) ? 1 : 0) != 0;
            if (!(early_ && tid < 64)) {
                int nact = 0, pmin = 0x7fffffff, pmax = -1;     // flagged springs; the first / last of them in table order
#define PP_IDX_(q_) (early_ ? (tid - 64) + (q_) * EARLY_NT : tid + (q_) * NT)
#define PP_MASK_(q_) if (early_) { const int r_ = iq_ / KA_N(Ak_); vq_ = lean_valid_mask(r_, iq_ - r_ * KA_N(Ak_), KA_N(Ak_)); }
#include "substep_strain_prepass.inc.hpp"
#undef PP_IDX_
#undef PP_MASK_
                if (__any(nact)) {
                    const int min_ = __builtin_amdgcn_readlane(wave_incl_min(pmin), 63);         // DPP: no LDS round trips
                    const int max_ = -__builtin_amdgcn_readlane(wave_incl_min(-pmax), 63);
                    if (lane == 0) { misc[1] = 1; atomicMin(&misc[10], min_); atomicMax(&misc[11], max_); }
                }
                // (release: the wave's flag and bounds are in LDS before its count is)
                if (early_ && lane == 0) __hip_atomic_fetch_add(&misc[17], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (!early_) __syncthreads();
            if (tid < 64 && (early_ || misc[1] || (pm & PH_NOSKIP))) {
                __builtin_amdgcn_s_setprio(3);            // the serial sweep is the critical path of the whole cloth
                const bool all_ = (pm & PH_NOSKIP) != 0;
                // (the early walk: from window 0, no end of its own)
                const int w0 = early_ ? 0 : __builtin_amdgcn_readfirstlane(all_ ? 0 : (misc[10] >> 6));
                const int w1 = early_ ? -1 : __builtin_amdgcn_readfirstlane(all_ ? KA_NW(Ak_) - 1 : (misc[11] >> 6));
                int tear = tic ? strain_sweep_lean<T, V.table_in_lds(), SWEEP_STATS, SWEEP_AHEAD, true>(cur, wtab, Ak_->wt_ent, g_rest, Ak_->wt_dep, w0, w1, KA_RSHIFT(Ak_), k,
                                                                                                  lane, st_windows, st_passes, st_commits, early_, misc, KA_NW(Ak_))
                               : strain_sweep<T, V.table_in_lds(), SWEEP_TIMED, SWEEP_STATS, false>(cur, wtab, Ak_->wt_ent, g_rest, Ak_->wt_dep, w0, w1, Ak_->nW, KA_RSHIFT(Ak_), k,
                                                                                                    lane, st_windows, st_passes, st_commits, tph, 0ull);
                // bit 1: the walk gave up waiting for the pre-pass (exact, every window walked -- but something is broken): stats[4] of the env
                if (tear & 2) { if (lane == 0 && A.stats) atomicAdd(&A.stats[16 * e + 4], 1); }
                tear &= 1;
                if (__any(tear) && lane == 0) misc[0] = 1;
                // sweeps run (clothhip_debug_stats): counted where a spring was flagged, as in the barriered order (a cloth at rest: the walk only
                // waited for the count). The published words are reset behind the barrier below: a wave of the pre-pass may still be on its way
                // to them if the walk gave up waiting.
                if (early_) { if (lane == 0 && __hip_atomic_load(&misc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0) misc[15]++; }
                else if (lane == 0) { misc[15]++; misc[1] = 0; misc[10] = 0x7fffffff; misc[11] = -1; }
                __builtin_amdgcn_s_setprio(0);
            }
            __syncthreads();
            // (the early walk's resets: no publisher of this substep is ahead of this barrier, and the next pre-pass is barriers away; by the
            //  last thread of wave 7, which owns one particle and is never a phase's longest stream)
            if (early_ && tid == NT - 1) { misc[1] = 0; misc[10] = 0x7fffffff; misc[11] = -1; misc[17] = 0; }
