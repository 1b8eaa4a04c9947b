// substep_strain_prepass.inc.hpp -- the strain pre-pass's test of a thread's particles: a FRAGMENT of substep_strain.inc.hpp / substep_strain_early.inc.hpp
// (textual for the reason given there). The includer defines PP_IDX_(q), the particle the thread tests in trip q, and PP_MASK_(q), a statement that may
// replace that particle's stencil mask vq_ (empty where the thread owns the particle), and declares nact, pmin, pmax.
#pragma unroll
                for (int q = 0; q < PPT; q++) {
                    if (PP_IDX_(q) < P) {
                        const Pt<T> me = cur[PP_IDX_(q)];
                        const uint32_t cme_ = w_cnt(me.w);
                        uint32_t gl[HK_SLOTS / 2];
                        int iq_ = PP_IDX_(q); uint4 lw_ = uint4{0u, 0u, 0u, 0u}; if constexpr (LEAN64) lw_ = lstc[iq_]; uint32_t vq_ = LEAN64 ? lw_.x : vm[(LEAN && !LEAN64) ? q : 0];
                        PP_MASK_(q)
                        if (LEAN) asm volatile("" : "+v"(iq_), "+v"(vq_));
                        // LEAN_NATIVE, as in the Hooke phase: the owner's address + the position's offset, valid = bit sl of the mask
#pragma unroll
                        for (int sl = 0; sl < HK_SLOTS / 2; sl++)
                            gl[sl] = LEAN_NATIVE ? 0u : LEAN ? lean_entry(iq_, vq_, sl) : (GT_REG ? gt[GT_REG ? q : 0][sl] : Ak_->gather[sl * Ppad + PP_IDX_(q)]);
                        // software pipeline, as in the Hooke phase: two neighbour reads in flight ahead of the test
                        constexpr int PP_AHEAD = 2;
                        Pt<T> nbq[PP_AHEAD];
#pragma unroll
                        for (int sl = 0; sl < PP_AHEAD; sl++) {
                            if constexpr (LEAN_NATIVE) nbq[sl] = cur[iq_ + lean_off(sl, KA_N(Ak_))];
                            else {
                            uint32_t g = gl[sl];
                            asm volatile("" : "+v"(g));
                            gl[sl] = g;
                            nbq[sl] = cur[g & HK_NBR_MASK];
                            }
                        }
                        // (a) branch-free: which of the six springs come within the slack band of their limit at all?
                        uint32_t cand = 0u;
                        T l2s[HK_SLOTS / 2];
#pragma unroll
                        for (int sl = 0; sl < HK_SLOTS / 2; sl++) {       // own springs come first in ascending list order
                            const uint32_t g = gl[sl];
                            const Pt<T> nb = nbq[sl % PP_AHEAD];
                            if (sl + PP_AHEAD < HK_SLOTS / 2) {
                                if constexpr (LEAN_NATIVE) nbq[sl % PP_AHEAD] = cur[iq_ + lean_off(sl + PP_AHEAD, KA_N(Ak_))];
                                else {
                                uint32_t gn = gl[sl + PP_AHEAD];
                                asm volatile("" : "+v"(gn));
                                gl[sl + PP_AHEAD] = gn;
                                nbq[sl % PP_AHEAD] = cur[gn & HK_NBR_MASK];
                                }
                            }
                            __builtin_amdgcn_sched_barrier(0);
                            T r = LEAN64 ? lean_rest64(sl, lw_) : LEAN ? lean_rest(sl) : (REST_R ? rr[REST_R ? q : 0][sl] : rest_at((g >> HK_POS_SHIFT) & HK_POS_MASK));
                            asm volatile("" : "+v"(r));     // or the thresholds below are hoisted out of the substep loop
                                                            // for all 18 springs and live in scratch
                            const T dx = nb.x - me.x, dy = nb.y - me.y, dz = nb.z - me.z;   // (ptA - ptB), as :270
                            const T len2 = sumsq<T>(dx, dy, dz);
                            l2s[sl] = len2;
                            const T t11 = r * k.c11, tt = r * k.tear_thresh;
                            const T tmin = t11 < tt ? t11 : tt;
#if defined(CLOTHHIP_MUTATE) && CLOTHHIP_MUTATE == 4       // MUTANT 4 (see strain_sweep_lean): the pre-pass flags both-pinned springs too
                            const bool pre = (LEAN_NATIVE ? (vq_ & (1u << sl)) != 0u : (g & (HK_VALID | HK_ASB)) == (HK_VALID | HK_ASB)) &
                                             (len2 > tmin * tmin * ((T)1 - filt_slack<T>()));
#else
                            const bool pre = (LEAN_NATIVE ? (vq_ & (1u << sl)) != 0u : (g & (HK_VALID | HK_ASB)) == (HK_VALID | HK_ASB)) &
                                             !((cme_ != 0) & (w_cnt(nb.w) != 0)) &
                                             (len2 > tmin * tmin * ((T)1 - filt_slack<T>()));
#endif
                            cand |= pre ? (1u << sl) : 0u;
                        }
                        // (b) those few: inside the slack band around the limit the sweep's exact test (:270-275) decides: a
                        // spring that sits exactly ON its limit (left there by an earlier substep's correction) is then not
                        // flagged, and a cloth at rest skips the sweep altogether
                        if (cand) {
#pragma unroll
                            for (int sl = 0; sl < HK_SLOTS / 2; sl++) {
                                if (cand & (1u << sl)) {
                                    // (LEAN: the spring's table slot is read from the gather table only now that it is needed: the table
                                    //  is compacted, the sl-th stencil position is the particle's popcount(valid below sl)-th entry)
                                    const uint32_t pos_ = V.has_point_slots() ? (uint32_t)pslot[sl * Ppad + iq_] : ((LEAN ? Ak_->gather[__popc(vq_ & ((1u << sl) - 1u)) * Ppad + iq_] : gl[sl])      // (the opaque copies: nothing of this is hoisted out of the substep loop and held)
                                                           >> HK_POS_SHIFT) & HK_POS_MASK;
                                    T r = LEAN64 ? lean_rest64(sl, lw_) : LEAN ? lean_rest(sl) : (REST_R ? rr[REST_R ? q : 0][sl] : rest_at(pos_));
                                    asm volatile("" : "+v"(r));
                                    const T len2 = l2s[sl];
                                    const T t11 = r * k.c11, tt = r * k.tear_thresh;
                                    const T tmin = t11 < tt ? t11 : tt;
                                    bool flag = len2 > tmin * tmin * ((T)1 + filt_slack<T>());
                                    if (!flag) { const T len = dev_sqrt<T>(len2); flag = len > t11 || len > tt; }
                                    if (flag) { nact++; pmin = (int)pos_ < pmin ? (int)pos_ : pmin; pmax = (int)pos_ > pmax ? (int)pos_ : pmax; }
#ifdef CLOTHHIP_CELL_COUNTERS
                                    if (flag) atomicOr(&misc[13 + (((int)pos_ >> 6) >> 5 & 1)], 1 << (((int)pos_ >> 6) & 31));
#endif
                                }
                            }
                        }
                    }
                }
