#!/usr/bin/env python3
"""DAgger with the expert inside the episode launch, end to end and small: a one-layer (linear) policy over the '1d' observation, a few
iterations of  roll out under the beta-mixture (demos.dagger_rollout: ONE launch per iteration) -> aggregate (observation, label) ->
refit by numpy.linalg.lstsq on everything gathered so far,  with beta = 0.5^i (iteration 0 is half the expert's). No torch. It prints
the mean coverage after each env's last action per iteration (and with --out FILE also appends the lines there); profiles/dagger.txt
holds a run. That record claims nothing: a linear map of 1875 positions is a poor smoother, the point is that the loop runs and what
it costs.
With --hidden 64,64 --fit device the policy is an MLP with those hidden widths and the refit runs ON THE DEVICE (policies.MLPTrainer
through demos.dagger_fit: the rows are appended to the handle's dataset and Adam steps update the network in place, so the next
iteration's launch runs the fitted weights with no upload); each iteration's line then splits its time into rollout / append / fit.
With --collect device (beside --fit device) the rollout's rows never leave the device either: demos.dagger_collect appends them by index
from the launch's resident tables, and with --time-budget-ms X it collects in time slices of X ms instead of whole-slot launches.
    python3 tools/dagger_demo.py [--envs 64] [--slots 12] [--iters 4] [--out FILE] [--hidden 64,64 --fit device [--fit-steps 200] [--batch 256]
                                 [--collect device [--time-budget-ms X]]]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd.demos import dagger_collect, dagger_fit, dagger_rollout        # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv            # noqa: E402
from gym_cloth_amd.policies import MLPPolicy, MLPTrainer          # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def fit_linear(obs, labels):
    """Least squares [obs, 1] @ X = labels -> one (W [4, 3P], b [4]) layer, float32."""
    A = np.concatenate([obs.astype(np.float64), np.ones((len(obs), 1))], axis=1)
    X = np.linalg.lstsq(A, labels, rcond=None)[0]
    return [(X[:-1].T.astype(np.float32), X[-1].astype(np.float32))]


def run_device(args):
    """The MLP / device-fit variant: one MLPTrainer for the whole run, its dataset and its network stay on the device."""
    E, T = args.envs, args.slots
    hidden = [int(w) for w in args.hidden.split(",") if w]
    cfg = bench.bench_cfg(25, 0.02, "tier1")
    cfg["env"]["force_grab"] = True
    env = ClothVecEnv(cfg, n_envs=E, precision="f32", consume_domrand_draws=False)
    widths = [3 * env.P] + hidden + [4]
    r = np.random.RandomState(0)
    layers = [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32), np.zeros(widths[l + 1], dtype=np.float32))
              for l in range(len(widths) - 1)]
    trainer = MLPTrainer(env, MLPPolicy(env, layers), optimizer="adam", lr=args.lr)
    say("DAgger demo: %d cloths 25x25 fp32 tier 1 (force_grab), MLP policy hidden %r fitted on the device (Adam, lr %g, %d steps of %d rows per "
        "iteration), %d slots per launch, beta = 0.5^i, expert oracle_corner" % (E, hidden, args.lr, args.fit_steps, args.batch, T))
    for i in range(args.iters):
        env.seed([2000 + e for e in range(E)])
        env.reset()
        if args.collect == "device":
            collect_iteration(args, env, trainer, i)
            continue
        t0 = time.perf_counter()
        roll = dagger_rollout(env, expert="oracle_corner", n_actions=T, beta=0.5 ** i, seed=i)
        dt = time.perf_counter() - t0
        kernel_ms = env.batch.last_kernel_ms
        ran = roll["ran"]
        cov = roll["out"]["actual_coverage"]
        last = np.array([cov[np.nonzero(ran[:, e])[0][-1], e] for e in range(E) if ran[:, e].any()])
        err = np.abs(roll["out"]["actions"][ran & ~roll["took"]] - roll["labels"][ran & ~roll["took"]])
        t0 = time.perf_counter()
        rows = trainer.append(roll["obs"][ran], roll["labels"][ran])
        da = time.perf_counter() - t0
        t0 = time.perf_counter()
        fit = dagger_fit(env, trainer, {"ran": np.zeros_like(ran), "obs": roll["obs"], "labels": roll["labels"]}, n_steps=args.fit_steps,
                         batch_size=args.batch, seed=i)
        df = time.perf_counter() - t0
        say("iteration %d: beta %.3f, %4d labelled states (%4d acted by the expert), mean coverage after the last action %.4f, "
            "mean |learner action - label| %.4f, rollout %.0f ms (kernel %.0f ms), append %.1f ms, fit on %d rows %.0f ms (device %.0f ms), "
            "loss %.4f -> %.4f" % (i, 0.5 ** i, int(ran.sum()), int(roll["took"].sum()), float(last.mean()),
                                  float(err.mean()) if err.size else float("nan"), dt * 1e3, kernel_ms, da * 1e3, rows, df * 1e3,
                                  env.batch.last_kernel_ms, fit["losses"][0], fit["losses"][-1]))
    env.close()


def collect_iteration(args, env, trainer, i):
    """One iteration with the rows appended on the device (demos.dagger_collect), in whole-slot launches or in time slices."""
    E, T = args.envs, args.slots
    t0 = time.perf_counter()
    col = dagger_collect(env, trainer, "oracle_corner", n_actions=T, beta=0.5 ** i, seed=i, slots_per_launch=T, time_budget_ms=args.time_budget_ms)
    dt = time.perf_counter() - t0
    last, took = np.full(E, np.nan), 0
    for rec in col["records"]:                                               # launches in order: the last counted slot of every env wins
        counted = rec["ran"] & (rec["slot"] < T)
        took += int((rec["expert_took"] & counted).sum())
        for t, e in zip(*np.nonzero(counted)):
            last[e] = rec["actual_coverage"][t, e]
    t0 = time.perf_counter()
    losses = trainer.step(args.fit_steps, args.batch, i)
    df = time.perf_counter() - t0
    say("iteration %d: beta %.3f, %4d labelled states (%4d acted by the expert), mean coverage after the last action %.4f, "
        "collect on the device %.0f ms in %d launches%s (kernels %.0f ms; rows appended by index), fit on %d rows %.0f ms (device %.0f ms), "
        "loss %.4f -> %.4f" % (i, 0.5 ** i, col["appended"], took, float(np.nanmean(last)), dt * 1e3, col["launches"],
                              " of %.1f ms slices" % args.time_budget_ms if args.time_budget_ms > 0 else "", col["kernel_ms"], col["rows"],
                              df * 1e3, env.batch.last_kernel_ms, losses[0], losses[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    ap.add_argument("--hidden", default="", help="hidden widths of an MLP policy, e.g. 64,64 (needs --fit device); default: the linear policy")
    ap.add_argument("--fit", choices=("lstsq", "device"), default="lstsq", help="lstsq: numpy on the host (linear policy); device: MLPTrainer")
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--collect", choices=("host", "device"), default="host", help="device: demos.dagger_collect, the rows stay on the device (needs --fit device)")
    ap.add_argument("--time-budget-ms", type=float, default=0.0, help="--collect device: collect in time slices of this length")
    args = ap.parse_args()
    if args.collect == "device" and args.fit != "device":
        ap.error("--collect device appends to the device-resident dataset: it needs --fit device")
    if args.time_budget_ms and args.collect != "device":
        ap.error("--time-budget-ms goes with --collect device")
    if (args.fit == "device") != bool(args.hidden):
        ap.error("--hidden WIDTHS and --fit device go together (the lstsq refit is for the linear policy)")
    if args.fit == "device":
        run_device(args)
    else:
        run_linear(args)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


def run_linear(args):
    E, T = args.envs, args.slots
    cfg = bench.bench_cfg(25, 0.02, "tier1")
    cfg["env"]["force_grab"] = True
    env = ClothVecEnv(cfg, n_envs=E, precision="f32", consume_domrand_draws=False)
    env.seed([2000 + e for e in range(E)])
    P = env.P
    layers = [(np.zeros((4, 3 * P), dtype=np.float32), np.zeros(4, dtype=np.float32))]
    data_obs, data_lab = [], []
    say("DAgger demo: %d cloths 25x25 fp32 tier 1 (force_grab), linear policy, %d slots per launch, beta = 0.5^i, expert oracle_corner" % (E, T))
    for i in range(args.iters):
        env.seed([2000 + e for e in range(E)])
        env.reset()
        env.set_policy(MLPPolicy(env, layers))
        t0 = time.perf_counter()
        roll = dagger_rollout(env, expert="oracle_corner", n_actions=T, beta=0.5 ** i, seed=i)
        dt = time.perf_counter() - t0
        ran = roll["ran"]
        data_obs.append(roll["obs"][ran]); data_lab.append(roll["labels"][ran])
        cov = roll["out"]["actual_coverage"]
        last = np.array([cov[np.nonzero(ran[:, e])[0][-1], e] for e in range(E) if ran[:, e].any()])
        err = np.abs(roll["out"]["actions"][ran & ~roll["took"]] - roll["labels"][ran & ~roll["took"]])
        t0 = time.perf_counter()
        layers = fit_linear(np.concatenate(data_obs), np.concatenate(data_lab))
        df = time.perf_counter() - t0
        say("iteration %d: beta %.3f, %4d labelled states (%4d acted by the expert), mean coverage after the last action %.4f, "
            "mean |learner action - label| %.4f, rollout %.0f ms (kernel %.0f ms), fit on %d rows %.0f ms" % (
                i, 0.5 ** i, int(ran.sum()), int(roll["took"].sum()), float(last.mean()), float(err.mean()) if err.size else float("nan"),
                dt * 1e3, env.batch.last_kernel_ms, sum(len(o) for o in data_obs), df * 1e3))
    env.close()


if __name__ == "__main__":
    main()
