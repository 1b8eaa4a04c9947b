#!/usr/bin/env python3
"""Actor-critic from reward, end to end and small: tools/reward_fit_demo.py's loop with a critic. Per iteration: collect
under the present network plus Gaussian exploration noise (demos.actor_critic_collect: rows appended where they lie, labelled with the
action the slot EXECUTED, the state behind an env's last open slot appended as a leaf, the transitions written in one call) -> ONE
clothhip_fit_data_gae call writes the value targets and the advantage weights on the device -> Adam steps of the critic on the non-leaf
rows, then of the policy under the weights (demos.actor_critic_fit). Beside it, from the same seeds and the same noise, a
demos.reward_collect / reward_fit run on an env of its own. It prints, per iteration, the mean return of the episodes that completed in
both runs and where the time went; with --out FILE it also appends the lines there. profiles/actor_critic.txt holds a run. The tool
claims nothing about learning curves: it says what came out. The policy takes FEW steps per iteration (--policy-steps, 10): a normalised
advantage is negative for about half of the rows, and a squared error under a negative weight has no minimum -- it is a policy-gradient
step, not a regression to run to convergence (200 steps drive the network's output off to infinity; so they do under reward_weights'
'advantage').
With --bench it measures instead (profiles/actor_critic.txt): clothhip_fit_data_gae over the rows of one --envs x --slots collection,
kernels and call, beside the host route it replaces in the same run (value_predict download, policies.gae_reference, set_weights +
set_returns); and a critic Adam step at hidden [64, 64], B = 256 and 4096, beside the policy's on the same rows.
    python3 tools/actor_critic_demo.py [--envs 64] [--slots 12] [--iters 4] [--sigma 0.1] [--gamma 0.99] [--lam 0.95] [--hidden 64,64]
                                       [--value-steps 200] [--policy-steps 10] [--batch 256] [--lr 1e-3] [--out FILE]
    python3 tools/actor_critic_demo.py --bench [--envs 512] [--slots 12] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd.demos import actor_critic_collect, actor_critic_fit, reward_collect, reward_fit      # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv            # noqa: E402
from gym_cloth_amd.policies import MLPPolicy, MLPTrainer, ValueTrainer, gae_reference                   # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def make_env(E):
    cfg = bench.bench_cfg(25, 0.02, "tier1")
    cfg["env"]["force_grab"] = True
    return ClothVecEnv(cfg, n_envs=E, precision="f32", consume_domrand_draws=False)


def make_layers(widths, seed=0):
    r = np.random.RandomState(seed)
    return [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32), np.zeros(widths[l + 1], dtype=np.float32))
            for l in range(len(widths) - 1)]


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return "%.3f ms (min %.3f, max %.3f)" % (np.median(xs), xs.min(), xs.max())


def mean(x):
    return float(np.mean(x)) if len(x) else float("nan")


def run(args):
    E, T = args.envs, args.slots
    hidden = [int(w) for w in args.hidden.split(",") if w]
    ac_env, rf_env = make_env(E), make_env(E)
    widths = [3 * ac_env.P] + hidden
    ac = MLPTrainer(ac_env, MLPPolicy(ac_env, make_layers(widths + [4])), optimizer="adam", lr=args.lr)
    critic = ValueTrainer(ac_env, make_layers(widths + [1], seed=1), optimizer="adam", lr=args.lr)
    rf = MLPTrainer(rf_env, MLPPolicy(rf_env, make_layers(widths + [4])), optimizer="adam", lr=args.lr)
    say("actor-critic demo: %d cloths 25x25 fp32 tier 1 (force_grab), MLP policy and critic hidden %r, %d slots per iteration in one launch, "
        "Gaussian exploration noise sigma %g; actor-critic: GAE gamma %g lambda %g, normalised advantages as weights, Adam lr %g, %d critic + "
        "%d policy steps of %d rows per iteration; beside it reward_collect / reward_fit (scheme 'advantage', gamma 1, %d steps) from the "
        "same seeds and noise" % (E, hidden, T, args.sigma, args.gamma, args.lam, args.lr, args.value_steps, args.policy_steps, args.batch,
                                  args.policy_steps))
    for i in range(args.iters):
        noise = np.random.RandomState(100 + i).normal(size=(T, E, 4)) * args.sigma
        for env in (ac_env, rf_env):
            env.seed([2000 + e for e in range(E)])                            # every iteration from the same start states
            env.reset()
        t0 = time.perf_counter()
        col = actor_critic_collect(ac_env, ac, n_actions=T, policy_noise=noise, slots_per_launch=T)
        dc = time.perf_counter() - t0
        t0 = time.perf_counter()
        fit = actor_critic_fit(ac_env, ac, critic, col, gamma=args.gamma, lam=args.lam, n_value_steps=args.value_steps,
                               n_policy_steps=args.policy_steps, batch_size=args.batch, seed=i)
        df = time.perf_counter() - t0
        rcol = reward_collect(rf_env, rf, n_actions=T, gamma=1.0, scheme="advantage", policy_noise=noise, slots_per_launch=T)
        rfit = reward_fit(rf_env, rf, rcol, n_steps=args.policy_steps, batch_size=args.batch, seed=i)
        say("iteration %d: actor-critic %4d rows + %d leaves, %3d completed episodes, mean return %.4f | reward-fit %4d rows (%d of open "
            "episodes, weight 0), %3d completed episodes, mean return %.4f | actor-critic collect %.0f ms (append %.2f ms, set_transitions "
            "%.2f ms), fit %.0f ms: critic loss %.5f -> %.5f, weighted policy loss %.5f -> %.5f, mean |adv| %.4f | reward-fit loss %.5f -> %.5f" % (
                i, col["appended"], col["open_rows"], len(col["episode_return"]), mean(col["episode_return"]), rcol["appended"],
                rcol["open_rows"], len(rcol["episode_return"]), mean(rcol["episode_return"]), dc * 1e3, col["t_append"] * 1e3,
                col["t_set_transitions"] * 1e3, df * 1e3, fit["value_losses"][0], fit["value_losses"][-1], fit["policy_losses"][0],
                fit["policy_losses"][-1], float(np.abs(fit["adv"]).mean()), rfit["losses"][0], rfit["losses"][-1]))
    ac_env.close()
    rf_env.close()


def bench_section(args, reps=10, steps=20, rounds=5):
    E, T = args.envs, args.slots
    env = make_env(E)
    for e in range(E):
        env.np_randoms[e] = np.random.RandomState(1000 + e)
    env.reset()
    tr = MLPTrainer(env, MLPPolicy(env, make_layers([3 * env.P, 64, 64, 4], seed=7)))
    critic = ValueTrainer(env, make_layers([3 * env.P, 64, 64, 1], seed=8))
    b = env.batch
    col = actor_critic_collect(env, tr, n_actions=T, slots_per_launch=T)
    n = col["appended"] + col["open_rows"]
    say("gae bench: the %d rows (%d of them leaves) of one %d x %d-slot collection (25x25, critic hidden [64, 64]), gamma 0.99, lambda 0.95, "
        "normalised weights written; %d repetitions each, medians" % (n, col["open_rows"], E, T, reps))
    b.fit_gae(0.99, 0.95, n=n, normalize=True, want=False)                    # (allocates the scratch)
    kern, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.fit_gae(0.99, 0.95, n=n, normalize=True, want=False)
        wall.append(time.perf_counter() - t0)
        kern.append(b.last_kernel_ms * 1e-3)
    say("    clothhip_fit_data_gae, nothing downloaded:             device (the critic's forward + the scan) %s, call %s" % (stats(kern), stats(wall)))
    w_dev, ret_dev = b.fit_get_weights(), b.fit_get_returns()
    parts = {"predict": [], "reference": [], "upload": [], "all": []}
    idx = np.arange(n)
    for _ in range(reps):
        t0 = time.perf_counter()
        v = b.value_predict(idx)
        t1 = time.perf_counter()
        adv, ret, w = gae_reference(v, col["rew"], col["next"], 0.99, 0.95, normalize=True)
        t2 = time.perf_counter()
        b.fit_set_weights(w)
        b.fit_set_returns(ret)
        t3 = time.perf_counter()
        for k, d in zip(("predict", "reference", "upload", "all"), (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
            parts[k].append(d)
    say("    the host route: value_predict with its download %s, policies.gae_reference (numpy, a Python loop per row) %s, set_weights + "
        "set_returns %s; together %s" % tuple(stats(parts[k]) for k in ("predict", "reference", "upload", "all")))
    say("    both routes leave the same bytes in the weight and value-target columns: %s" % (
        w_dev.tobytes() == b.fit_get_weights().tobytes() and ret_dev.tobytes() == b.fit_get_returns().tobytes()))
    env.close()
    # a critic step beside a policy step, on fit_bench's dataset
    from gym_cloth_amd.batch import ClothBatch
    one = ClothBatch(bench.bench_cfg(25, 0.02, "tier1"), n_envs=1, precision="f32")
    r = np.random.RandomState(3)
    rows = r.uniform(-1, 1, size=(8192, 3 * one.P)).astype(np.float32)
    one.fit_append(rows, r.uniform(-1, 1, size=(8192, 4)))
    one.fit_set_returns(r.uniform(-1, 1, size=8192))
    one.set_policy_mlp(make_layers([3 * one.P, 64, 64, 4], seed=7))
    one.set_value_mlp(make_layers([3 * one.P, 64, 64, 1], seed=8))
    say("step bench: 25x25, 8192 uniform rows, hidden [64, 64], Adam, %d steps per call, median of %d calls after one warm-up call; device ms by "
        "HIP events around all steps of a call" % (steps, rounds))
    for B in (256, 4096):
        table = r.randint(0, 8192, size=(steps, B)).astype(np.int32)
        line = []
        for name, fit in (("critic [64, 64, 1]", one.value_fit), ("policy [64, 64, 4]", one.fit)):
            fit(table)
            dev = []
            for _ in range(rounds):
                fit(table)
                dev.append(one.last_kernel_ms / steps)
            line.append("%s %.3f ms/step (min %.3f, max %.3f)" % (name, float(np.median(dev)), min(dev), max(dev)))
        say("    B %4d: %s" % (B, "; ".join(line)))
    one.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--sigma", type=float, default=0.1, help="standard deviation of the exploration noise added to the network's output")
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--hidden", default="64,64")
    ap.add_argument("--value-steps", type=int, default=200)
    ap.add_argument("--policy-steps", type=int, default=10, help="policy steps per iteration, in both runs (few: see the docstring)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--bench", action="store_true", help="measure fit_gae against the host route, and a critic step beside a policy step")
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    if args.envs is None:
        args.envs = 512 if args.bench else 64
    if args.bench:
        bench_section(args)
    else:
        run(args)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
