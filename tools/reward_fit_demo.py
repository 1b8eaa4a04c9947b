#!/usr/bin/env python3
"""Fitting from reward, end to end and small: a few iterations of  collect under the present network plus Gaussian
exploration noise (demos.reward_collect: the rows are appended where they lie, labelled with the action the slot EXECUTED, weight 0) ->
write the weights of the completed episodes' returns (one set_weights call) -> Adam steps on everything gathered so far
(demos.reward_fit),  all of it on the device: nothing is downloaded but the [T, E] records. It prints, per iteration, the mean return of
the episodes that completed, the mean coverage after each env's last collected action, and where the time went (launches, append,
set_weights, fit); with --out FILE it also appends the lines there. profiles/reward_fit.txt holds a run. The tool claims nothing about
learning curves: it says what came out.
With --append-bench it measures instead what the executed-action label costs (profiles/fit_weighted.txt): k_fit_gather over the rows
of one --envs x --slots launch with labels from the records against labels from the expert's table, the same rows, the kernel alone
(clothhip_last_kernel_ms), and clothhip_fit_data_set_weights of that many rows.
    python3 tools/reward_fit_demo.py [--envs 64] [--slots 12] [--iters 4] [--scheme filter|exp|advantage] [--sigma 0.1] [--gamma 1.0]
                                     [--hidden 64,64] [--fit-steps 200] [--batch 256] [--lr 1e-3] [--out FILE]
    python3 tools/reward_fit_demo.py --append-bench [--envs 512] [--slots 12] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd.demos import reward_collect, reward_fit        # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv, slot_start_sources    # noqa: E402
from gym_cloth_amd.policies import MLPPolicy, MLPTrainer          # noqa: E402

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


def run(args):
    E, T = args.envs, args.slots
    hidden = [int(w) for w in args.hidden.split(",") if w]
    env = make_env(E)
    widths = [3 * env.P] + hidden + [4]
    trainer = MLPTrainer(env, MLPPolicy(env, make_layers(widths)), optimizer="adam", lr=args.lr)
    kw = {"filter": dict(q=args.q), "exp": dict(temperature=args.temperature, w_max=args.w_max), "advantage": {}}[args.scheme]
    say("reward-fit demo: %d cloths 25x25 fp32 tier 1 (force_grab), MLP policy hidden %r, %d slots per iteration in one launch, Gaussian "
        "exploration noise sigma %g, returns with gamma %g, weights '%s' %r, Adam lr %g, %d steps of %d rows per iteration" % (
            E, hidden, T, args.sigma, args.gamma, args.scheme, kw, args.lr, args.fit_steps, args.batch))
    for i in range(args.iters):
        env.seed([2000 + e for e in range(E)])                                # every iteration from the same start states
        env.reset()
        noise = np.random.RandomState(100 + i).normal(size=(T, E, 4)) * args.sigma
        t0 = time.perf_counter()
        col = reward_collect(env, trainer, n_actions=T, gamma=args.gamma, scheme=args.scheme, policy_noise=noise, slots_per_launch=T, **kw)
        dc = time.perf_counter() - t0
        last = np.full(E, np.nan)
        for rec in col["records"]:
            counted = rec["ran"] & (rec["slot"] < T)
            for t, e in zip(*np.nonzero(counted)):
                last[e] = rec["actual_coverage"][t, e]
        t0 = time.perf_counter()
        fit = reward_fit(env, trainer, col, n_steps=args.fit_steps, batch_size=args.batch, seed=i)
        df = time.perf_counter() - t0
        ret = col["episode_return"]
        say("iteration %d: %4d rows (%d of open episodes, weight 0; %d with a non-zero weight), %3d completed episodes, mean return %.4f, "
            "mean coverage after the last action %.4f | collect %.0f ms: launches %.0f ms (kernels %.0f ms), append %.2f ms, set_weights %.2f ms | "
            "fit on %d rows %.0f ms (device %.0f ms), weighted loss %.5f -> %.5f" % (
                i, col["appended"], col["open_rows"], fit["weighted"], len(ret), float(ret.mean()) if len(ret) else float("nan"),
                float(np.nanmean(last)), dc * 1e3, (col["took"] - col["t_append"]) * 1e3, col["kernel_ms"], col["t_append"] * 1e3,
                col["t_set_weights"] * 1e3, fit["rows"], df * 1e3, env.batch.last_kernel_ms, fit["losses"][0], fit["losses"][-1]))
    env.close()


def append_bench(args, reps=10):
    E, T = args.envs, args.slots
    env = make_env(E)
    for e in range(E):
        env.np_randoms[e] = np.random.RandomState(1000 + e)
    env.reset()
    layers = make_layers([3 * env.P, 64, 64, 4], seed=7)
    tr = MLPTrainer(env, MLPPolicy(env, layers))
    b = env.batch
    b.fit_hold()
    out = env.step_many(policy="mlp", n_actions=T, want_obs="device", expert="oracle_corner")
    t_, e_ = np.nonzero(out["ran"])
    rows = np.concatenate([slot_start_sources(out)[t_, e_], (t_ * E + e_)[:, None].astype(np.int32)], axis=1)
    n = len(rows)
    w = np.random.RandomState(1).normal(size=n).astype(np.float32)
    say("append bench: the %d rows that ran of one %d x %d-slot armed launch (25x25: %d B per row), %d repetitions each, medians" % (n, E, T, 3 * env.P * 4, reps))
    res = {}
    for name, kw in (("expert labels (clothhip_fit_data_append_launch)", dict(labels="expert")),
                     ("action labels, no weights", dict(labels="action")),
                     ("action labels + a weight table", dict(labels="action", weights=w))):
        tr.clear()
        tr.append_launch(rows, **kw)                                          # (allocates the tables)
        kern, wall = [], []
        for _ in range(reps):
            tr.clear()
            t0 = time.perf_counter()
            tr.append_launch(rows, **kw)
            wall.append(time.perf_counter() - t0)
            kern.append(b.last_kernel_ms * 1e-3)
        res[name] = np.median(kern)
        say("    %-50s kernel %s, call %s" % (name, stats(kern), stats(wall)))
    lab = tr.data()[1]
    same = np.array_equal(lab, out["actions"][t_, e_].astype(np.float32))
    say("    the stored labels are the launch's action records rounded to float32: %s" % same)
    kern, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        tr.set_weights(w)
        wall.append(time.perf_counter() - t0)
        kern.append(b.last_kernel_ms * 1e-3)
    say("    clothhip_fit_data_set_weights of %d rows (%d B):          device (events around the copy) %s, call %s" % (n, 4 * n, stats(kern), stats(wall)))
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--scheme", choices=("filter", "exp", "advantage"), default="filter")
    ap.add_argument("--q", type=float, default=0.25, help="filter: the fraction of rows kept")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--w-max", type=float, default=20.0)
    ap.add_argument("--sigma", type=float, default=0.1, help="standard deviation of the exploration noise added to the network's output")
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--hidden", default="64,64")
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--append-bench", action="store_true", help="measure the append with action labels against expert labels, and set_weights")
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    if args.envs is None:
        args.envs = 512 if args.append_bench else 64
    if args.append_bench:
        append_bench(args)
    else:
        run(args)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
