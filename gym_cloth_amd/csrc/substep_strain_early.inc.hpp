// substep_strain_early.inc.hpp -- strain limit + tear of the eight-wave fp32 LEAN build (Variant::sweep_starts_early): the walk starts while the other
// waves run the pre-pass. A FRAGMENT of substep_strain.inc.hpp (the SWEEP_EARLY branch of its `if constexpr`), textual for the reason given there;
// production builds only (SWEEP_LEAN, no stamps, no census), so none of their instrumentation appears here. Names it uses beyond that file's: e, A,
// hkey, hco, olist (the hash-table reset of substep_collision.inc.hpp, done here in the early order).
            // early_ (wave-uniform, EARLY_ORDER_: episode_loop.hpp): wave 0 enters the walk at window 0 right here, behind the plane barrier; waves
            // 1-7 test whole WINDOWS from LDS positions alone -- wave j takes windows j-1, j-1+7, ... ascending, one spring per lane, with the
            // walk's own quiet-window test (strain_sweep_lean::step) -- and publish per window its bit in the flag mask F (if a spring of it is
            // over-stretched) and then, with release order, its bit in the tested mask D. No barrier in front of the walk, no count, no first /
            // last slot: strain_sweep_lean reads D and F where its own reach is used up (phase_strain.hpp; DESIGN.md 4.1 has the argument that the
            // result is the sequential loop's although the pre-pass reads records the walk is correcting). Behind their last window the seven
            // waves reset the collision phase's hash table (substep_collision.inc.hpp leaves it to them in this order): they idle there anyway.
            // Not with PH_NOSKIP (walk everything), tear_thresh < 1.1 (strain_sweep) or more windows than the masks hold: those keep the barriered order.
            const bool tic = __builtin_amdgcn_readfirstlane(!(k.tear_thresh < k.c11) ? 1 : 0) != 0;
            const bool early_ = __builtin_amdgcn_readfirstlane(EARLY_ORDER_(k) ? 1 : 0) != 0;
            if (early_) {
                if (tid >= 64) {
                    constexpr int NPRE = NT / 64 - 1;                                   // waves 1-7
                    const int nW_ = KA_NW(Ak_);
                    const int nocc_ = __builtin_amdgcn_readfirstlane(misc[3]);          // (reset behind the end-of-substep barrier, below)
                    int w_ = __builtin_amdgcn_readfirstlane(tid >> 6) - 1;
                    T c11_ = k.c11;
                    // entry: from LDS or, the generic build's large tables, L2 -- as the walk's `load`; an index past the wave's last window reads that window again
                    auto entry_ = [&](int wi, uint32_t &ab_, T &r_) {
                        const uint32_t ix = (uint32_t)((wi < nW_ ? wi : w_) * 64 + lane);
                        if (V.table_in_lds()) { const WEnt<T> e_ = wtab[ix]; ab_ = e_.ab; r_ = e_.rest; }
                        else { ab_ = Ak_->wt_ent[ix]; r_ = g_rest[ix]; }
                    };
                    if (w_ < nW_) {
                        uint32_t ab0, ab1; T r0, r1;
                        entry_(w_, ab0, r0);
                        Pt<T> A0 = cur[ab0 & WT_IDX_MASK], B0 = cur[__builtin_amdgcn_ubfe(ab0, WT_IDX_BITS, WT_IDX_BITS)];
                        entry_(w_ + NPRE, ab1, r1);
                        do {
                            // the next window's records and the entry behind it are in flight while this one is evaluated
                            const Pt<T> A1 = cur[ab1 & WT_IDX_MASK], B1 = cur[__builtin_amdgcn_ubfe(ab1, WT_IDX_BITS, WT_IDX_BITS)];
                            uint32_t ab2; T r2;
                            entry_(w_ + 2 * NPRE, ab2, r2);
                            const T dx = A0.x - B0.x, dy = A0.y - B0.y, dz = A0.z - B0.z;
                            const T len = dev_sqrt<T>(sumsq<T>(dx, dy, dz));                // :270, the walk's expression
                            const bool trig = (len > r0 * c11_) & !((w_cnt(A0.w) != 0) & (w_cnt(B0.w) != 0));   // :275; both ends pinned: skipped (:268)
                            const bool any_ = ballot64(trig) != 0ull;
                            if (lane == 0) {
                                if (any_) __hip_atomic_fetch_or(&misc[EARLY_F_WORD + (w_ >> 5)], 1 << (w_ & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                // (release: the window's flag is in LDS before its tested bit is)
                                __hip_atomic_fetch_or(&misc[EARLY_D_WORD + (w_ >> 5)], 1 << (w_ & 31), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                            A0 = A1; B0 = B1; r0 = r1; ab1 = ab2; r1 = r2;
                            w_ += NPRE;
                        } while (w_ < nW_);
                    }
                    // the hash table of the collision phase, ready for the next substep: its next reader is the next substep's hash insert,
                    // barriers away; nothing in the plane or strain phase reads it (PH_COLLIDE off: nocc_ == 0)
                    for (int t = tid - 64; t < nocc_; t += NT - 64) { const int h = (int)olist[t]; hkey[h] = KEY_EMPTY; hco[h] = 0; }
                }
            } else {
                int nact = 0, pmin = 0x7fffffff, pmax = -1;     // flagged springs; the first / last of them in table order
#define PP_IDX_(q_) tid + (q_) * NT
#define PP_MASK_(q_)
#include "substep_strain_prepass.inc.hpp"
#undef PP_IDX_
#undef PP_MASK_
                if (__any(nact)) {
                    const int min_ = __builtin_amdgcn_readlane(wave_incl_min(pmin), 63);         // DPP: no LDS round trips
                    const int max_ = -__builtin_amdgcn_readlane(wave_incl_min(-pmax), 63);
                    if (lane == 0) { misc[1] = 1; atomicMin(&misc[10], min_); atomicMax(&misc[11], max_); }
                }
                __syncthreads();
            }
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
                // sweeps run (clothhip_debug_stats), as the barriered order counts them -- where a spring was flagged: a flag bit is set or the walk
                // corrected something (bit 2 of its result; a walk that reached the table's end may be ahead of the flags). The masks are reset
                // behind the barrier below: a wave of the pre-pass may still be on its way to them.
                if (early_) {
                    int any_ = tear & 4;
#pragma unroll
                    for (int j = 0; j < EARLY_MASK_WORDS; j++) any_ |= __hip_atomic_load(&misc[EARLY_F_WORD + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (lane == 0 && any_ != 0) misc[15]++;
                }
                else if (lane == 0) { misc[15]++; misc[1] = 0; misc[10] = 0x7fffffff; misc[11] = -1; }
                tear &= 1;
                if (__any(tear) && lane == 0) misc[0] = 1;
                __builtin_amdgcn_s_setprio(0);
            }
            __syncthreads();
            // (the early order's resets: no publisher of this substep is ahead of this barrier, and the next pre-pass is barriers away -- as is the
            //  next reader of the collision phase's counters, the hash insert; by the last thread of wave 7, which owns one particle and is never a
            //  phase's longest stream)
            if (early_ && tid == NT - 1) {
#pragma unroll
                for (int j = 0; j < EARLY_MASK_WORDS; j++) { misc[EARLY_F_WORD + j] = 0; misc[EARLY_D_WORD + j] = 0; }
                misc[2] = 0; misc[3] = 0; misc[4] = 0; misc[5] = 0; misc[6] = 0;
            }
