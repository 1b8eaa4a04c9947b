"""Dev tool (GPU box): mechanism counts of the early walk on the bench workload's cloths (512 x 25x25, tier 1, the bench's seeds): one untimed episode launch of
10 action slots per env with the counting build (make -C gym_cloth_amd/csrc earlycnt; CLOTHHIP_LIB=gym_cloth_amd/libclothhip_earlycnt.so), then the
per-env stats summed: sweeps, windows walked, passes, correcting passes, jumps, windows jumped over (profiles/window_flags_ab.txt 1).
  python tools/early_walk_counts.py [tier1|tier3]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from gym_cloth_amd.envs import ClothVecEnv

E, T = 512, 10
env = ClothVecEnv(bench.bench_cfg(25, 0.02, sys.argv[1] if len(sys.argv) > 1 else "tier1"), n_envs=E, precision="f32", consume_domrand_draws=False)
for e in range(E):
    env.np_randoms[e] = np.random.RandomState(1000 + e)
env.reset()
acts = np.ascontiguousarray(np.stack([np.random.RandomState(2000 + e).uniform(-1, 1, size=(T, 4)) for e in range(E)], axis=1))
out = env.step_many(acts, auto_reset=True, max_resets=T)
v = env.batch.last_variant()
st = env.batch.debug_stats().astype(np.int64)
s = st.sum(axis=0)
sub = int(out["executed"].sum())
print(os.environ.get("CLOTHHIP_LIB"), v["name"], "spec", v.get("spec_n_side"))
print("action substeps %d | sweeps %d | windows walked %d (%.2f per sweep) | passes %d (%.2f) | correcting passes %d (%.2f) | jumps %d (%.2f per sweep) | windows jumped over %d (%.2f per sweep) | stats[4] %d"
      % (sub, s[0], s[1], s[1] / s[0], s[2], s[2] / s[0], s[3], s[3] / s[0], s[5], s[5] / s[0], s[6], s[6] / s[0], s[4]))
print("state checksum", float(np.abs(env.batch.positions()).sum()))
env.close()
