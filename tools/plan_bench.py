#!/usr/bin/env python3
"""What the cross-entropy planner over forked cloths costs, measured: stated figures for DESIGN 4.3.6, written to profiles/plan_cem.txt.

  1. ClothVecEnv.plan on tier 1, fp32, 25x25: 64 envs x K = 16 (1 024 branches) and 48 envs x K = 32 (1 536), H = 1 and H = 3, 3
     iterations each. The whole call (host clock), then the same loop iteration by iteration (one call per iteration, the same bits):
     host clock and the episode launch's own time (HIP events around the stepper kernel: ClothBatch.last_kernel_ms); the difference is
     sample + fork + refit + host. Measured alone: the fork (host clock around the same fork; it synchronises) and the two planner
     kernels (host clock around the stand-alone entries on tables of the same shape, which also move their tables over PCIe: upper
     bounds). Beside it the floor: one bare launch of the last iteration's table on the scratch batch (run_actions on a host table).
  2. The host route as the alternative, same (mean, std, seed): H = 1 numpy sampling + ClothVecEnv.lookahead + numpy refit; H = 3
     policies.cem_reference (numpy sampling + fork_from + host-table run_actions + numpy refit).
  3. Model-predictive control from tier-3 starts: mean coverage after 10 actions for CEMPolicy warm-started by the corner oracle, beside the
     oracle alone, same seeds. A recorded result.
    python3 tools/plan_bench.py [--out profiles/plan_cem.txt] [--skip-mpc | --skip-cost]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv            # noqa: E402
from gym_cloth_amd.policies import (CEMPolicy, OracleCornerPolicy, cem_reference, plan_refit_reference, plan_sample_reference)  # noqa: E402

LINES = []
N_ITERS = 3


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def med(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), min(out), max(out)


def planner_cost(E, K, H):
    cfg = bench.bench_cfg(25, 0.02, "tier1")
    env = ClothVecEnv(cfg, n_envs=E, precision="f32", consume_domrand_draws=False)
    env.seed(1000)
    env.reset()
    M = max(2, K // 4)
    mean = np.zeros((E, H, 4))
    std = np.full((E, H, 4), 0.4)
    kw = dict(min_std=0.02, alpha=1.0, penalty=1.0, seed=1)
    call = lambda: env.plan(H, K, M, N_ITERS, mean=mean, std=std, want_scores=True, want_candidates=True, **kw)
    out = call()                                                             # creates the scratch batch, warms every kernel
    plain = lambda: env.plan(H, K, M, N_ITERS, mean=mean, std=std, **kw)
    total = med(plain)
    scratch = env._plan_scratch
    v = scratch.last_variant()
    # iteration by iteration: the same loop as n_iters calls of one iteration each (mean, std and iter0 handed on; the same bits), so that
    # every iteration's launch has its own HIP-event time -- the iterations differ: the distribution narrows, the pulls get shorter
    walls, kernels = [], []
    for _ in range(3):
        m, s, w, k = mean, std, [], []
        for it in range(N_ITERS):
            t0 = time.perf_counter()
            o = env.plan(H, K, M, 1, mean=m, std=s, iter0=it, **kw)
            w.append((time.perf_counter() - t0) * 1e3)
            k.append(scratch.last_kernel_ms)
            m, s = o["mean"], o["std"]
        assert np.array_equal(m, out["mean"]) and np.array_equal(s, out["std"])
        walls.append(w); kernels.append(k)
    walls, kernels = np.median(walls, axis=0), np.median(kernels, axis=0)
    other = walls - kernels
    rep = np.repeat(np.arange(E), K)
    fork = med(lambda: scratch.fork_from(env.batch, rep))
    sp = env.action_space
    x = out["candidates"][-1]
    sample = med(lambda: scratch.plan_sample(mean, std, sp.low, sp.high, it=0, horizon=H, n_candidates=K, seed=1))
    refit = med(lambda: scratch.plan_refit(x, out["scores"][-1], mean, std, horizon=H, n_elite=M, min_std=0.02))
    # the floor: the last iteration's table, one launch through the host-table entry
    ep = env._episode_params()
    ns = np.ascontiguousarray(env.num_steps[rep], dtype=np.int32)
    floor_k = []

    def bare():
        scratch.fork_from(env.batch, rep)
        t0 = time.perf_counter()
        scratch.run_actions(ep, H, ns.copy(), np.zeros(E * K, dtype=np.uint8), actions=x)
        floor_k.append((scratch.last_kernel_ms, (time.perf_counter() - t0) * 1e3))
    for _ in range(3):
        bare()
    fk, fw = np.median([a for a, _ in floor_k]), np.median([b for _, b in floor_k])
    f3 = lambda a: ", ".join("%.2f" % t for t in a)
    share = float(other.sum() / kernels.sum())
    say("  E = %d, K = %d (%d branches), H = %d, %d iterations, M = %d; scratch batch ran %s" % (E, K, E * K, H, N_ITERS, M, v["name"]))
    say("    plan(), all iterations in one call: %.2f ms (min %.2f .. max %.2f) = %.2f ms per iteration" % (total[0], total[1], total[2], total[0] / N_ITERS))
    say("    iteration by iteration (one call each, medians of 3): host clock %s ms; launch (kernel, HIP events) %s ms; everything else %s ms" %
        (f3(walls), f3(kernels), f3(other)))
    say("    -> sample + fork + refit + host = %.2f ms per iteration = %.2f %% of the launch; the one call of %d iterations takes %.2f ms less than the %d calls" %
        (other.mean(), 100.0 * share, N_ITERS, walls.sum() - total[0], N_ITERS))
    say("    measured alone: fork %.3f ms (host clock, synchronises); sample <= %.3f ms, refit <= %.3f ms (stand-alone entries incl. their table transfers)" %
        (fork[0], sample[0], refit[0]))
    say("    floor: one bare launch of the last iteration's table on the scratch batch: kernel %.2f ms, host clock around run_actions %.2f ms "
        "(the planner's own last iteration: kernel %.2f ms, host clock %.2f ms)" % (fk, fw, kernels[-1], walls[-1]))
    # the host route
    if H == 1:
        def host_route():
            m, s = mean.copy(), std.copy()
            for it in range(N_ITERS):
                xx = plan_sample_reference(m, s, sp.low, sp.high, K, seed=1, iteration=it)
                look = env.lookahead(np.ascontiguousarray(xx[0].reshape(E, K, 4)))
                sc = np.where(look["out_of_bounds"] | look["have_tear"], look["actual_coverage"] - 1.0, look["actual_coverage"])
                m, s, _, _ = plan_refit_reference(xx, sc, m, s, M, min_std=0.02)
        name = "numpy sampling + lookahead (the step path) + numpy refit"
    else:
        def host_route():
            cem_reference(env, scratch, H, K, M, N_ITERS, mean, std, **kw)
        name = "cem_reference (numpy sampling + fork_from + host-table run_actions + numpy refit)"
    host_route()
    hr = med(host_route, reps=2)
    say("    host route, %s: %.2f ms per call = %.2f ms per iteration -> host route / plan() = %.2f" %
        (name, hr[0], hr[0] / N_ITERS, hr[0] / total[0]))
    env.close()
    return share


def mpc(E=32, K=16, n_actions=10):
    cfg = bench.bench_cfg(25, 0.02, "tier3")
    cfg["env"]["max_actions"] = n_actions
    res = {}
    for name in ("oracle", "cem+oracle"):
        env = ClothVecEnv(cfg, n_envs=E, precision="f32", consume_domrand_draws=False)
        env.seed(4000)
        obs = env.reset()
        start = env._start_coverage.copy()
        oracle = OracleCornerPolicy(env)
        pol = oracle if name == "oracle" else CEMPolicy(env, horizon=1, n_candidates=K, n_elite=4, n_iters=2, init_std=[0.1, 0.1, 0.2, 0.2],
                                                       min_std=0.01, seed=3, warm_start=oracle)
        alive = np.ones(E, dtype=bool)
        cov = start.copy()
        t0 = time.perf_counter()
        for t in range(n_actions):
            if not alive.any():
                break
            act = np.nan_to_num(np.asarray(pol.get_action(obs, t), dtype=np.float64))
            obs, _, done, info = env.step(act, active=alive)
            cov = np.where(alive, info["actual_coverage"], cov)
            alive &= ~np.asarray(done, dtype=bool)
        res[name] = (float(start.mean()), float(cov.mean()), time.perf_counter() - t0, int((~alive).sum()), float(env.num_steps.mean()))
        env.close()
    for name, (s, c, sec, ended, steps) in res.items():
        say("  %-11s start coverage %.4f -> mean coverage after up to %d actions %.4f (%d of %d episodes ended, %.2f actions per env on average; %.1f s)" %
            (name, s, n_actions, c, ended, E, steps, sec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_cem.txt"))
    ap.add_argument("--skip-mpc", action="store_true")
    ap.add_argument("--skip-cost", action="store_true")
    a = ap.parse_args()
    say("tools/plan_bench.py -- the cross-entropy planner over forked cloths (ClothVecEnv.plan / clothhip_plan_cem), measured on %s" % time.strftime("%Y-%m-%d"))
    say("1. + 2. tier 1, 25x25, fp32, one MI355X")
    shares = []
    for E, K in (() if a.skip_cost else ((64, 16), (48, 32))):
        for H in (1, 3):
            shares.append(planner_cost(E, K, H))
    say("  sample + fork + refit + host per iteration as a share of the launch: %s" % ", ".join("%.1f %%" % (100 * s) for s in shares))
    if not a.skip_mpc:
        say("3. MPC from tier-3 starts, 32 envs, 25x25, fp32, seeds 4000 + e; CEM: H = 1, K = 16, M = 4, 2 iterations, warm start = the corner oracle")
        mpc()
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
