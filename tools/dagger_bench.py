#!/usr/bin/env python3
"""What the expert beside the acting policy costs, and what the stand-alone labelling kernel gives, measured. It prints its figures (and
with --out FILE also appends them there); a run of it is quoted, with the command, in profiles/dagger.txt and in DESIGN 4.3.3.

Workload: tools/policy_bench.py's -- 512 cloths of 25x25, fp32, tier 1 (bench.bench_cfg, with force_grab), a [64, 64] network with seeded
random weights, 12 action slots per launch, episode resets in the kernel.
  (a) step_many(policy='mlp'): the un-armed launch.
  (b) the same launch armed with the oracle-corner expert, which never acts: the same actions on the same states (reported: rewards
      equal to (a)'s), on the same stepper build -- (b) - (a) is what the labels cost.
  Two envs from the same seeds, launched alternately: one warm-up launch each, then --launches timed ones, then one more of each that is not
  timed (the armed one writes the observations part (c) relabels). Kernel time is the launch's
  (clothhip_last_kernel_ms), rate = Cloth.update() calls of the actions / that time.
  (c) clothhip_policy_label (ClothVecEnv.expert_actions) on --rows stored float32 observations -- the rows (b) wrote, repeated -- against
      policies.OracleCornerPolicy on the first --numpy-rows of them (numpy, row by row as the policy is written). Labels/s, wall time
      incl. the upload; the kernel's own time for its last chunk beside it.
    python3 tools/dagger_bench.py [--envs 512] [--slots 12] [--launches 3] [--rows 196608] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv, slot_start_obs            # noqa: E402
from gym_cloth_amd.policies import MLPPolicy, OracleCornerPolicy     # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def make_env(E, layers):
    cfg = bench.bench_cfg(25, 0.02, "tier1")
    cfg["env"]["force_grab"] = True
    env = ClothVecEnv(cfg, n_envs=E, precision="f32", consume_domrand_draws=False)
    for e in range(E):
        env.np_randoms[e] = np.random.RandomState(1000 + e)
    obs = env.reset()
    env.set_policy(MLPPolicy(env, layers))
    return env, obs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rows", type=int, default=196608)
    ap.add_argument("--numpy-rows", type=int, default=4096)
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    E, T, n_l = args.envs, args.slots, args.launches
    r = np.random.RandomState(7)
    widths = [1875, 64, 64, 4]
    layers = [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32),
               (r.normal(size=widths[l + 1]) / np.sqrt(widths[l])).astype(np.float32)) for l in range(3)]
    env_a, _ = make_env(E, layers)
    env_b, obs_b = make_env(E, layers)
    ms_a, ms_b, sub_a, sub_b, same = [], [], [], [], True
    rows = labels = None
    for k in range(n_l + 2):
        out_a = env_a.step_many(policy="mlp", n_actions=T)
        ka = env_a.batch.last_kernel_ms
        want_obs = k == n_l + 1
        before = env_b.state if want_obs else None
        out_b = env_b.step_many(policy="mlp", n_actions=T, expert="oracle_corner", want_obs=want_obs)
        kb = env_b.batch.last_kernel_ms
        same = same and np.array_equal(out_a["rew"], out_b["rew"]) and np.array_equal(out_a["actions"], out_b["actions"])
        if want_obs:
            ran = out_b["ran"]
            rows, labels = slot_start_obs(out_b, before)[ran], out_b["expert_actions"][ran]
        elif k:
            ms_a.append(ka); ms_b.append(kb)
            sub_a.append(int(out_a["executed"].sum())); sub_b.append(int(out_b["executed"].sum()))
    if not ms_a:
        raise SystemExit("--launches must be at least 1")
    var_a, var_b = env_a.batch.last_variant(), env_b.batch.last_variant()
    assert var_a["name"] == var_b["name"], (var_a["name"], var_b["name"])
    ra, rb = np.asarray(sub_a) / (np.asarray(ms_a) * 1e-3), np.asarray(sub_b) / (np.asarray(ms_b) * 1e-3)
    fmt = lambda v: "median %.3f M substeps/s (min %.3f .. max %.3f, n = %d)" % (np.median(v) / 1e6, v.min() / 1e6, v.max() / 1e6, len(v))
    say("the expert beside the MLP policy: %d cloths 25x25 fp32 tier 1 (force_grab), network %r, %d slots per launch, %d timed launches each, alternated" % (E, widths, T, len(ms_a)))
    say("variant: %s" % var_a["name"])
    say("action substeps per launch: %s (a), %s (b); actions and rewards of (b) equal to (a)'s: %s" % (sub_a, sub_b, same))
    say("(a) step_many(policy='mlp')                          %s; kernel ms %s" % (fmt(ra), ["%.1f" % m for m in ms_a]))
    say("(b) ... armed, expert='oracle_corner', never acting  %s; kernel ms %s" % (fmt(rb), ["%.1f" % m for m in ms_b]))
    say("armed / un-armed = %.4f (kernel time (b) - (a): %+.2f ms per launch of %d labels)" % (
        np.median(rb) / np.median(ra), float(np.median(ms_b) - np.median(ms_a)), E * T))
    env_a.close()

    # (c) relabelling stored rows
    same_lab = np.array_equal(env_b.expert_actions("oracle_corner", obs=rows), labels)
    n = int(args.rows)
    big = np.ascontiguousarray(np.tile(rows, ((n + len(rows) - 1) // len(rows), 1))[:n])
    env_b.expert_actions("oracle_corner", obs=big[:E])                       # warm-up (buffers)
    t0 = time.perf_counter()
    got = env_b.expert_actions("oracle_corner", obs=big)
    dt = time.perf_counter() - t0
    k_ms = env_b.batch.last_kernel_ms
    m = (min(int(args.numpy_rows), n) // E) * E
    pol = OracleCornerPolicy(env_b)
    t0 = time.perf_counter()
    ref = np.concatenate([pol.get_action(big[i:i + E]) for i in range(0, m, E)])
    dn = time.perf_counter() - t0
    say("labels of the armed launch == expert_actions(obs=slot_start_obs(...)): %s; device labels == numpy policy on %d rows: %s" % (
        same_lab, m, np.array_equal(got[:m], ref)))
    say("(c) clothhip_policy_label: %d rows in %.1f ms wall incl. upload = %.3f M labels/s (kernel, last chunk: %.3f ms); "
        "numpy OracleCornerPolicy: %d rows in %.1f ms = %.4f M labels/s; ratio %.1f" % (
            n, dt * 1e3, n / dt / 1e6, k_ms, m, dn * 1e3, m / dn / 1e6, (n / dt) / (m / dn)))
    env_b.close()
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
