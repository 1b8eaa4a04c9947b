#!/usr/bin/env python3
"""What the MLP policy inside the episode launch buys, measured. It prints its figures (and with --out FILE also writes them there); a run
of it is quoted, with the command, in profiles/mlp_policy.txt section 3 and in DESIGN 4.3.1.

Workload: 512 cloths of 25x25, fp32, tier 1 (bench.bench_cfg, with force_grab so that every action of a random network moves the
cloth), a [64, 64] network with seeded random weights, 12 action slots per launch, episode resets in the kernel.
  (a) step_many(policy='mlp'): the network evaluated inside the launch.
  (b) the actions (a) recorded, replayed through step_many(actions=...) from the same start state with CLOTHHIP_DEBUG_COLD=1, i.e. on
      the very stepper build (a) runs (the one that carries the cold policies): (a) - (b) is what the policy costs inside the launch.
  (c) the host loop step(policy.get_action(obs), auto_reset=True): download the observation, evaluate (on the device, one call),
      upload the actions, one launch sequence per action -- the path a learner takes without (a).
All three execute the same actions on the same states (reported: rewards equal to (a)'s), so the substeps are the same and only the time differs.
Rate = Cloth.update() calls of the actions / wall time of the calls. One warm-up launch, then --launches timed ones.
    python3 tools/policy_bench.py [--envs 512] [--slots 12] [--launches 3] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv            # noqa: E402
from gym_cloth_amd.policies import MLPPolicy          # noqa: E402

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
    return env, MLPPolicy(env, layers), obs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()
    E, T, n_l = args.envs, args.slots, args.launches
    r = np.random.RandomState(7)
    widths = [1875, 64, 64, 4]
    layers = [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32),
               (r.normal(size=widths[l + 1]) / np.sqrt(widths[l])).astype(np.float32)) for l in range(3)]
    os.environ.pop("CLOTHHIP_DEBUG_COLD", None)

    # (a) the policy in the launch
    env, pol, _ = make_env(E, layers)
    recorded, rew_a, t_a, sub_a, ms_a = [], [], [], [], []
    for k in range(n_l + 1):
        t0 = time.perf_counter()
        out = env.step_many(policy="mlp", n_actions=T)
        dt = time.perf_counter() - t0
        recorded.append(out["actions"].copy()); rew_a.append(out["rew"].copy())
        if k:
            t_a.append(dt); sub_a.append(int(out["executed"].sum())); ms_a.append(env.batch.last_kernel_ms)
    var_a = env.batch.last_variant()
    env.close()

    # (b) the same actions from a table, on the same stepper build
    os.environ["CLOTHHIP_DEBUG_COLD"] = "1"
    env, _, _ = make_env(E, layers)
    t_b, sub_b, ms_b, same_b = [], [], [], True
    for k in range(n_l + 1):
        t0 = time.perf_counter()
        out = env.step_many(recorded[k])
        dt = time.perf_counter() - t0
        same_b = same_b and np.array_equal(out["rew"], rew_a[k])
        if k:
            t_b.append(dt); sub_b.append(int(out["executed"].sum())); ms_b.append(env.batch.last_kernel_ms)
    var_b = env.batch.last_variant()
    env.close()
    os.environ.pop("CLOTHHIP_DEBUG_COLD", None)
    assert var_a["name"] == var_b["name"], (var_a["name"], var_b["name"])

    # (c) the host loop
    env, pol, obs = make_env(E, layers)
    t_c, sub_c, same_c = [], [], True
    for k in range(n_l + 1):
        t0 = time.perf_counter()
        n_sub = 0
        for t in range(T):
            act = pol.get_action(obs)
            obs, rew, done, info = env.step(act, auto_reset=True)
            same_c = same_c and np.array_equal(rew, rew_a[k][t])
            n_sub += int(np.asarray(info["executed"]).sum())
        dt = time.perf_counter() - t0
        if k:
            t_c.append(dt); sub_c.append(n_sub)
    env.close()

    rate = lambda sub, t: np.asarray(sub, dtype=np.float64) / np.asarray(t)
    ra, rb, rc = rate(sub_a, t_a), rate(sub_b, t_b), rate(sub_c, t_c)
    fmt = lambda v: "median %.3f M substeps/s (min %.3f .. max %.3f, n = %d)" % (np.median(v) / 1e6, v.min() / 1e6, v.max() / 1e6, len(v))
    say("MLP policy in the episode launch: %d cloths 25x25 fp32 tier 1 (force_grab), network %r, %d slots per launch, %d timed launches" % (E, widths, T, n_l))
    say("variant: %s" % var_a["name"])
    say("action substeps per launch: %s (a), %s (b), %s (c); rewards equal to (a)'s: (b) %s, (c) %s" % (sub_a, sub_b, sub_c, same_b, same_c))
    say("(a) step_many(policy='mlp')                 %s; kernel ms %s" % (fmt(ra), ["%.1f" % m for m in ms_a]))
    say("(b) step_many(actions=recorded), same build %s; kernel ms %s" % (fmt(rb), ["%.1f" % m for m in ms_b]))
    say("(c) host loop step(get_action(obs))         %s" % fmt(rc))
    say("(a) / (b) = %.4f (kernel time (a) - (b): %.2f ms per launch of %d network evaluations)   (a) / (c) = %.3f   (b) / (c) = %.3f" % (
        np.median(ra) / np.median(rb), float(np.median(ms_a) - np.median(ms_b)), E * T, np.median(ra) / np.median(rc), np.median(rb) / np.median(rc)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
