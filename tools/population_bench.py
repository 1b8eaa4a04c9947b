#!/usr/bin/env python3
"""What a population of MLP policies in ONE episode launch costs and what making it on the device saves, measured. It prints its figures
(and with --out FILE also writes them there); a run of it is quoted, with the command, in profiles/mlp_population.txt and DESIGN 4.3.2.

Workload of (a) and (b): tools/policy_bench.py's -- 512 cloths of 25x25, fp32, tier 1 (bench.bench_cfg, force_grab), a [64, 64] network
(124 484 parameters) with seeded random weights, 12 action slots per launch, episode resets in the kernel.
  (a) step_many(policy='mlp') with 512 DISTINCT networks (an MLPPopulation of 512 members, env e under row e) against the same launch
      with ONE shared network (the centre), on the same stepper build, launches alternated. The networks differ, so the actions and
      the substeps differ: the figure is substeps per second of each, and the kernel time per launch. Between them: 512 COPIES of the centre
      at 512 addresses (population_perturb with sigma = 0), which executes the shared network's very actions and differs from it only in
      where the weights come from. Report only.
  (b) population_perturb (512 antithetic members + the centre, on the device) against numpy drawing 256 x n_params normal variates,
      building the same 513 rows and uploading them (set_policy_population); population_combine (256 coefficients) against numpy summing
      its own variates (float32 BLAS, coef @ eps). Wall time of the calls; for the device also the kernel's time by HIP events
      (clothhip_last_kernel_ms) and, for perturb, the bytes it stored per second.
  (c) ten evolution-strategies generations on tier 1 (448 members + 64 envs under the centre, episodes of max_actions slots without
      resets, centred ranks): the mean return of the centre's row and of the members per generation. A record, not a claim.
    python3 tools/population_bench.py [--envs 512] [--slots 12] [--launches 3] [--generations 10] [--skip a,b,c] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                                    # noqa: E402
from gym_cloth_amd import _lib                                  # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv                      # noqa: E402
from gym_cloth_amd.policies import MLPPolicy, MLPPopulation, pack_mlp, population_stride    # noqa: E402

LINES = []
WIDTHS = [1875, 64, 64, 4]


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def make_env(E):
    cfg = bench.bench_cfg(25, 0.02, "tier1")
    cfg["env"]["force_grab"] = True
    env = ClothVecEnv(cfg, n_envs=E, precision="f32", consume_domrand_draws=False)
    for e in range(E):
        env.np_randoms[e] = np.random.RandomState(1000 + e)
    env.reset()
    return env


def centre_layers(seed=7):
    r = np.random.RandomState(seed)
    return [((r.normal(size=(WIDTHS[l + 1], WIDTHS[l])) / np.sqrt(WIDTHS[l])).astype(np.float32),
             (r.normal(size=WIDTHS[l + 1]) / np.sqrt(WIDTHS[l])).astype(np.float32)) for l in range(3)]


def med(v):
    v = np.asarray(v, dtype=np.float64)
    return "median %.3f (min %.3f .. max %.3f, n = %d)" % (np.median(v), v.min(), v.max(), len(v))


def part_a(E, T, n_l):
    layers = centre_layers()
    G = E if E % 2 == 0 else E - 1
    env_p, env_c, env_s = make_env(E), make_env(E), make_env(E)
    MLPPopulation(env_p, layers, G, 0.02, 11, member=np.arange(E) % G)
    MLPPopulation(env_c, layers, G, 0.02, 11, member=np.arange(E) % G)
    env_c.batch.population_perturb(layers, G, 0.0, 11, antithetic=True, member=np.arange(E) % G)     # sigma = 0: every row IS the centre, at its own address
    MLPPolicy(env_s, layers)
    res = {"pop": ([], [], []), "copies": ([], [], []), "shared": ([], [], [])}
    same = True
    for k in range(n_l + 1):
        acts = {}
        for name, env in (("pop", env_p), ("copies", env_c), ("shared", env_s)):
            t0 = time.perf_counter()
            out = env.step_many(policy="mlp", n_actions=T)
            dt = time.perf_counter() - t0
            acts[name] = out["actions"]
            if k:
                res[name][0].append(dt); res[name][1].append(int(out["executed"].sum())); res[name][2].append(env.batch.last_kernel_ms)
        same = same and np.array_equal(acts["copies"], acts["shared"])
    var_p, var_s = env_p.batch.last_variant(), env_s.batch.last_variant()
    env_p.close(); env_c.close(); env_s.close()
    assert var_p["name"] == var_s["name"]
    say("(a) %d cloths 25x25 fp32 tier 1 (force_grab), network %r, %d slots per launch, %d timed launches each, alternated; variant %s" % (
        E, WIDTHS, T, n_l, var_p["name"]))
    for name, label in (("pop", "%d distinct networks" % G), ("copies", "%d copies of one network" % G), ("shared", "one shared network")):
        t, sub, ms = res[name]
        rate = np.asarray(sub, dtype=np.float64) / np.asarray(t) / 1e6
        krate = np.asarray(sub, dtype=np.float64) / (np.asarray(ms) * 1e-3) / 1e6
        say("    %-24s M substeps/s by wall time %s; by kernel time %s; substeps %s, kernel ms %s" % (
            label, med(rate), med(krate), sub, ["%.1f" % m for m in ms]))
    kp = np.asarray(res["pop"][1]) / np.asarray(res["pop"][2])
    ks = np.asarray(res["shared"][1]) / np.asarray(res["shared"][2])
    kc = np.asarray(res["copies"][1]) / np.asarray(res["copies"][2])
    say("    substeps per kernel ms: distinct / shared = %.4f; copies / shared = %.4f (the copies' actions equal the shared network's: %s -- the same work, "
        "the weights streamed from %d rows instead of one)" % (np.median(kp) / np.median(ks), np.median(kc) / np.median(ks), same, G))


def part_b(E, reps):
    layers = centre_layers()
    widths, theta = pack_mlp(layers)
    n, G, K, sigma = theta.size, 512, 256, np.float32(0.02)
    stride = population_stride(n)
    env = make_env(E)
    b = env.batch
    member = np.arange(E) % (G + 1)
    t_dev, ms_dev, t_cmb, ms_cmb, t_draw, t_build, t_up, t_sum = [], [], [], [], [], [], [], []
    coef = np.random.RandomState(3).normal(size=K).astype(np.float32)
    for k in range(reps + 1):
        t0 = time.perf_counter()
        b.population_perturb(layers, G, sigma, 100 + k, antithetic=True, member=member)
        t1 = time.perf_counter()
        ms_p = b.last_kernel_ms
        t2 = time.perf_counter()
        b.population_combine(coef)
        t3 = time.perf_counter()
        ms_c = b.last_kernel_ms
        # the host's way (the rows go up as one packed array, straight through the C entry)
        rng = np.random.default_rng(100 + k)
        t4 = time.perf_counter()
        eps = rng.standard_normal((K, n), dtype=np.float32)
        t5 = time.perf_counter()
        rows = np.empty((G + 1, n), dtype=np.float32)
        rows[0:G:2] = theta + sigma * eps
        rows[1:G:2] = theta - sigma * eps
        rows[G] = theta
        t6 = time.perf_counter()
        _lib.check(b._L.clothhip_set_policy_population(b._h, len(widths) - 1, _lib.i32p(widths), rows.ctypes.data_as(C.POINTER(C.c_float)),
                                                       G + 1, _lib.i32p(member.astype(np.int32))))
        t7 = time.perf_counter()
        coef @ eps
        t8 = time.perf_counter()
        if k:
            t_dev.append((t1 - t0) * 1e3); ms_dev.append(ms_p); t_cmb.append((t3 - t2) * 1e3); ms_cmb.append(ms_c)
            t_draw.append((t5 - t4) * 1e3); t_build.append((t6 - t5) * 1e3); t_up.append((t7 - t6) * 1e3); t_sum.append((t8 - t7) * 1e3)
    env.close()
    stored = (G + 1) * stride * 4
    say("(b) %d antithetic members + the centre of %r (%d parameters, row stride %d floats, %.1f MB of rows), %d timed repetitions" % (
        G, WIDTHS, n, stride, stored / 1e6, reps))
    say("    population_perturb   wall ms %s; kernel ms %s = %.2f TB/s stored" % (med(t_dev), med(ms_dev), stored / (np.median(ms_dev) * 1e-3) / 1e12))
    say("    numpy                draw %d x %d normals ms %s; build the rows ms %s; upload (set_policy_population) ms %s" % (
        K, n, med(t_draw), med(t_build), med(t_up)))
    say("    host total / device wall = %.1f" % ((np.median(t_draw) + np.median(t_build) + np.median(t_up)) / np.median(t_dev)))
    say("    population_combine   wall ms %s; kernel ms %s (%d Philox calls per parameter)" % (med(t_cmb), med(ms_cmb), K))
    say("    numpy coef @ eps     ms %s (float32 BLAS on variates the host kept, %.0f MB)" % (med(t_sum), K * n * 4 / 1e6))


def part_c(E, generations):
    cfg = bench.bench_cfg(25, 0.02, "tier1")
    env = ClothVecEnv(cfg, n_envs=E, precision="f32", consume_domrand_draws=False)
    T = int(cfg["env"]["max_actions"])
    G = (E * 7 // 8) // 2 * 2
    member = np.where(np.arange(E) < G, np.arange(E), G).astype(np.int32)
    layers = centre_layers(seed=12)
    layers[-1] = (layers[-1][0] * np.float32(0.1), layers[-1][1] * np.float32(0.1))
    sigma, lr = 0.02, 0.05
    env.seed(4000)
    env.reset()
    pop = MLPPopulation(env, layers, G, sigma, 77, member=member)
    say("(c) evolution strategies on tier 1 (reward %s): %d members + %d envs under the centre, sigma %.3g, step %.3g x gradient, centred ranks, "
        "episodes of up to %d actions, every generation from the same seeds" % (cfg["env"]["reward_type"], G, E - G, sigma, lr, T))
    for gen in range(generations):
        env.seed(4000)
        env.reset()
        t0 = time.perf_counter()
        out = env.step_many(policy="mlp", n_actions=T, auto_reset=False)
        t1 = time.perf_counter()
        fit = pop.fitness(out)
        grad = pop.gradient(fit, "centered_rank")
        pop.apply(np.float32(lr) * grad)
        t2 = time.perf_counter()
        say("    generation %2d (seed %d): centre's mean return %+.4f, members' mean %+.4f (best %+.4f); launch %.0f ms, fitness + gradient + "
            "next generation %.1f ms" % (gen, pop.generation_seed(gen), fit[G], fit[:G].mean(), fit[:G].max(), (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: a, b, c")
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()
    skip = set(args.skip.split(",")) if args.skip else set()
    os.environ.pop("CLOTHHIP_DEBUG_COLD", None)
    if "a" not in skip:
        part_a(args.envs, args.slots, args.launches)
    if "b" not in skip:
        part_b(args.envs, args.launches)
    if "c" not in skip:
        part_c(args.envs, args.generations)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
