#!/usr/bin/env python3
"""Counters of the self-collision phase over the bench workload (dev tool, GPU box). Needs the counter build:
    make -C gym_cloth_amd/csrc cnt      (-DCLOTHHIP_CELL_COUNTERS: the api_*.hip units and the stepper objects -> libclothhip_cnt.so)
    CLOTHHIP_LIB=$PWD/gym_cloth_amd/libclothhip_cnt.so python tools/cell_counters.py
Wave 0 of every cloth counts what IT did (about a quarter of the cells): big cells (> 16 members) swept, their members and
visits, small-cell tickets (up to four cells each), the pre-check's trip bound, active / occupied cells. Also the strain sweep's census,
with mean and histogram of the FIRST FLAGGED WINDOW (where the barriered walk starts, i.e. how many quiet windows a walk from window 0
has in front of it: profiles/early_walk_ab.txt)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv  # noqa: E402

E = 512
env = ClothVecEnv(bench.bench_cfg(25, 0.02), n_envs=E, precision="f32")
env.seed(1000); env.reset()
rs = [np.random.RandomState(2000 + e) for e in range(E)]
tot = np.zeros(16); nsub = 0.0
first = np.zeros(64); first_sweeps = np.zeros(64)      # by window: sweeps that started there, all sweeps of the envs that counted it
for it in range(6):
    acts = np.stack([np.stack([r.uniform(-1, 1, 4) for r in rs]) for _ in range(40)])
    out = env.step_many(actions=acts, time_budget_ms=800.0)
    if it >= 1:
        st = env.batch.debug_stats()
        # counter 0 shares its word: low half = substeps without an active cell, high half = this env's sweeps whose first flagged
        # window was (env mod 64) -- sixteen words per env hold no histogram, so every env counts one window
        w4 = st[:, 4].astype(np.int64) & 0xFFFFFFFF
        np.add.at(first, np.arange(E) % 64, w4 >> 16)
        np.add.at(first_sweeps, np.arange(E) % 64, st[:, 0])
        st = st.astype(np.float64); st[:, 4] = w4 & 0xFFFF
        tot += st.sum(0)
        nsub += float(out["executed"].sum() + out["reset_substeps"].sum())
# stats[4 + q] = counter q of the kernel's tph[] array
big, nmem, vis, trips, smt, na, nocc = (tot[4 + q] for q in (4, 5, 6, 7, 8, 9, 10))
noseed, frozen, fixed, skipw, hits = (tot[4 + q] for q in (0, 1, 2, 3, 11))
print("census, fraction of all cloth-substeps: no active collision cell %.3f | no strain sweep %.3f | frozen (no adjust, every "
      "unpinned particle restored by the plane, no over-stretched spring) %.3f | no particle changed its collision cell since "
      "the substep before %.3f" % (noseed / nsub, 1.0 - tot[0] / nsub, frozen / nsub, fixed / nsub))
print("strain sweep per cloth-substep: windows walked %.1f, passes %.1f, correcting %.1f | windows without a flagged spring and beyond "
      "every correction's reach (skippable) %.1f" % (tot[1] / nsub, tot[2] / nsub, tot[3] / nsub, skipw / nsub))
# first flagged window = where the walk starts: window w is counted by the envs with env mod 64 == w, as a share of THEIR sweeps
share = first / np.maximum(first_sweeps, 1.0)
wn = np.arange(64)
cdf = np.cumsum(share)
print("first flagged window over %.0f sweeps: mean %.2f (shares sum to %.3f) | median %d | P(first <= 0, 3, 7, 15, 31) = %s" %
      (tot[0], float((share * wn).sum() / max(share.sum(), 1e-30)), share.sum(), int(np.searchsorted(cdf, 0.5 * cdf[-1])),
       " ".join("%.3f" % (cdf[q] / max(cdf[-1], 1e-30)) for q in (0, 3, 7, 15, 31))))
print("first flagged window, histogram (window: share of sweeps in percent):")
for w_ in range(0, 64, 8):
    print("  " + "  ".join("%2d: %5.2f" % (q, 100.0 * share[q]) for q in range(w_, w_ + 8)))
print("big cells: hits per visit %.2f" % (hits / max(vis, 1)))
print("substeps %.0f | per cloth-substep: strain sweeps %.3f" % (nsub, tot[0] / nsub))
print("wave 0, per cloth-substep: big cells %.2f (mean %.1f members, %.1f visits each) | small-cell tickets %.2f | "
      "pre-check member bound %.1f | active cells %.1f of %.1f occupied" %
      (big / nsub, nmem / max(big, 1), vis / max(big, 1), smt / nsub, trips / nsub, na / nsub, nocc / nsub))
