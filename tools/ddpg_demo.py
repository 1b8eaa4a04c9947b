#!/usr/bin/env python3
"""DDPG on the device, end to end and small: tools/ppo_demo.py's loop with the off-policy step in the place of the
clipped surrogate. Per iteration: collect under the present network plus Gaussian exploration noise made on the device
(demos.actor_critic_collect with policies.DeviceNoise) -> demos.ddpg_fit: --steps DDPG steps, each a TD step of the Q critic, a step of
the policy up the critic's action gradient and the soft update of both targets, on minibatches drawn from the non-leaf rows of the WHOLE
dataset -- the replay buffer: no collection is thrown away. It prints, per iteration, the mean return of the episodes that completed,
the rows in the buffer, and the first and last step's critic loss, mean Q, gated fraction and mean |dL/da|; with --out FILE it also
appends the lines there. profiles/ddpg.txt holds a run. The tool claims nothing about learning curves: it says what came out.
With --expert NAME the launches are armed: the expert labels every state the learner reaches and, with --beta, takes the
action over on that share of the slots; the rows carry its action in the dataset's expert column, and --bc-coef / --q-coef /
--no-q-filter / --demo-fraction shape the actor's loss of DDPG from demonstrations; a second line per iteration then reports the BC loss,
the labelled share and the filter-pass share. Without these options the run is the plain one. profiles/ddpg_bc.txt holds both.
With --bench it measures instead, on the four shapes of tools/fit_bench.py (25x25; hidden [64, 64] and [256, 256, 256]; B = 256 and
4096): the device time of one clothhip_ddpg_fit step beside a clothhip_policy_fit step plus a clothhip_value_fit step of the same shapes
on the same handle, alternated, and the step's launch count; and the BC actor's step (clothhip_policy_fit_dpg_bc, half of the rows
labelled, bc_coef 1), filter on and off, beside the plain actor's step on that handle, with its launch count. With --one-shape it runs clothhip_ddpg_fit calls of that one shape
and nothing else: under a kernel trace (rocprofv3 --kernel-trace --stats -- python3 tools/ddpg_demo.py --bench --one-shape ...) the
per-kernel totals then are a DDPG step's, k_fit_concat's share among them (profiles/ddpg.txt).
    python3 tools/ddpg_demo.py [--envs 64] [--slots 12] [--iters 4] [--steps 100] [--batch 256] [--sigma 0.1] [--out FILE]
    python3 tools/ddpg_demo.py --expert oracle_corner [--beta 0.5] [--bc-coef 1.0] [--q-coef 1.0] [--no-q-filter] [--demo-fraction 0.5]
    python3 tools/ddpg_demo.py --bench [--bench-steps 20] [--rounds 5] [--out FILE]
    python3 tools/ddpg_demo.py --bench --one-shape 256,256,256:4096 [--bench-steps 20] [--rounds 1]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd.batch import ClothBatch            # noqa: E402
from gym_cloth_amd.demos import actor_critic_collect, ddpg_fit      # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv            # noqa: E402
from gym_cloth_amd.policies import DeviceNoise, MLPPolicy, MLPTrainer, QTrainer   # noqa: E402

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


def mean(x):
    return float(np.mean(x)) if len(x) else float("nan")


def run(args):
    E, T = args.envs, args.slots
    hidden = [int(w) for w in args.hidden.split(",") if w]
    env = make_env(E)
    pol = MLPTrainer(env, MLPPolicy(env, make_layers([3 * env.P] + hidden + [4])), optimizer="adam", lr=args.lr)
    qc = QTrainer(env, make_layers([3 * env.P + 4] + hidden + [1], seed=1), optimizer="adam", lr=args.q_lr)
    say("ddpg demo: %d cloths 25x25 fp32 tier 1 (force_grab), MLP policy and Q critic hidden %r, %d slots per iteration in one launch, Gaussian "
        "exploration noise sigma %g made on the device; per iteration %d DDPG steps on minibatches of %d rows from the whole replay buffer, gamma %g, "
        "tau %g, act_bound %g, Adam lr %g (policy) and %g (critic)" % (E, hidden, T, args.sigma, args.steps, args.batch, args.gamma, args.tau, args.act_bound,
                                                                    args.lr, args.q_lr))
    bc = args.expert is not None or args.bc_coef != 0.0 or args.q_coef != 1.0
    if bc:
        say("    from demonstrations: expert %s beside the policy, beta %g; actor loss q_coef %g (-mean Q) + bc_coef %g BC, Q-filter %s, demo_fraction %r"
            % (args.expert, args.beta, args.q_coef, args.bc_coef, "off" if args.no_q_filter else "on", args.demo_fraction))
    for i in range(args.iters):
        env.seed([2000 + e for e in range(E)])                                # every iteration from the same start states
        env.reset()
        try:
            col = actor_critic_collect(env, pol, n_actions=T, policy_noise=DeviceNoise(100 + i, sigma=args.sigma), slots_per_launch=T, expert=args.expert,
                                       beta=args.beta, seed=i)
        except ValueError as e:                                               # a network that ran away acts with values that are not finite
            say("iteration %d: the collection was refused (%s): the run ends here" % (i, e))
            break
        t0 = time.perf_counter()
        fit = ddpg_fit(env, pol, qc, col, gamma=args.gamma, tau=args.tau, n_steps=args.steps, batch_size=args.batch, seed=i, act_bound=args.act_bound,
                       q_coef=args.q_coef, bc_coef=args.bc_coef, q_filter=not args.no_q_filter, demo_fraction=args.demo_fraction)
        dt = time.perf_counter() - t0
        st = fit["stats"]
        say("iteration %d: %4d rows + %d leaves collected (%.0f ms), %3d completed episodes, mean return %.4f; replay buffer %d rows, %d with a "
            "transition, %.0f %% of the sampled rows from earlier collections" % (i, col["appended"], col["open_rows"], col["took"] * 1e3, len(col["episode_return"]),
                                                                                  mean(col["episode_return"]), pol.size(), len(fit["replay"]),
                                                                                  100.0 * float((fit["rows"] < col["first"]).mean())))
        say("    %d steps in %.0f ms (device %.1f ms)%s; critic loss %.5f -> %.5f, mean Q %.4f -> %.4f, mean y %.4f -> %.4f; actor -mean Q %.4f -> %.4f, "
            "gated %.3f -> %.3f, mean |dL/da| %.2e -> %.2e" % (len(st), dt * 1e3, env.batch.last_kernel_ms, ", targets synced" if fit["synced"] else "", st[0, 0], st[-1, 0],
                                                            st[0, 1], st[-1, 1], st[0, 2], st[-1, 2], st[0, 3], st[-1, 3], st[0, 4], st[-1, 4], st[0, 5], st[-1, 5]))
        if st.shape[1] == 9:
            say("    BC loss %.5f -> %.5f (mean over the steps %.5f), labelled share %.3f -> %.3f, filter-pass share %.3f -> %.3f (mean %.3f)"
                % (st[0, 6], st[-1, 6], st[:, 6].mean(), st[0, 7], st[-1, 7], st[0, 8], st[-1, 8], st[:, 8].mean()))
    env.close()


def launches_per_step(pw, qw, B):
    """Kernel launches of one clothhip_ddpg_fit step, counted from the order api_fit_ddpg.hip's run_ddpg enqueues (a forward layer is one launch; a
    backward layer is the weight gradient, with B > 256 its slab sum, the bias sum, and below the last layer the input gradient)."""
    Lp, Lq, split = len(pw) - 1, len(qw) - 1, 1 if B > 256 else 0
    back = lambda L: L * (2 + split) + (L - 1)
    critic = Lp + 1 + Lq + 1 + Lq + 1 + back(Lq) + 1          # target policy, concat, target Q, concat, Q, TD loss, backward, optimizer
    actor = Lp + 1 + Lq + 1 + Lq + 1 + back(Lp) + 1           # policy, concat, Q, the constant fill, the input-gradient chain, the gate, backward, optimizer
    return critic + actor + 2                                  # ... and the two soft updates


def bc_launches_per_step(pw, qw, B, q_filter):
    """Kernel launches of one clothhip_policy_fit_dpg_bc step: the plain actor's, k_fit_dpg_bc in the place of the gate, and under the
    Q-filter one concat and one Q forward in front."""
    Lp, Lq, split = len(pw) - 1, len(qw) - 1, 1 if B > 256 else 0
    back = lambda L: L * (2 + split) + (L - 1)
    return Lp + 1 + Lq + 1 + Lq + 1 + back(Lp) + 1 + ((1 + Lq) if q_filter else 0)


def bench_section(args):
    shapes = [([64, 64], 256), ([64, 64], 4096), ([256, 256, 256], 256), ([256, 256, 256], 4096)]
    if args.one_shape:
        h, B = args.one_shape.split(":")
        shapes = [([int(w) for w in h.split(",")], int(B))]
    b = ClothBatch(bench.bench_cfg(25, 0.02, "tier1"), n_envs=1, precision="f32")
    r = np.random.RandomState(3)
    n = args.rows
    rows, labels = r.uniform(-1, 1, size=(n, 3 * b.P)).astype(np.float32), r.uniform(-1, 1, size=(n, 4))
    b.fit_append(rows, labels)
    nxt = np.where(np.arange(n) % 12 == 11, -1, np.arange(n) + 1)
    nxt[-1] = -1
    b.fit_set_transitions(r.normal(size=n).astype(np.float32), nxt)
    b.fit_set_returns(r.normal(size=n).astype(np.float32))
    ex = r.uniform(-1, 1, size=(n, 4)).astype(np.float32)
    ex[r.random_sample(n) < 0.5] = np.nan                                     # half of the rows carry an expert action
    b.fit_set_expert(ex)
    say("ddpg bench: one 25x25 cloth, a dataset of %d uniform rows in episodes of 12; Adam; %d steps per call, %d calls of each kind ALTERNATED after one warm-up "
        "call each; device ms per step by HIP events around all steps of a call (median; min-max)" % (n, args.bench_steps, args.rounds))
    for hidden, B in shapes:
        pw, qw, vw = [3 * b.P] + hidden + [4], [3 * b.P + 4] + hidden + [1], [3 * b.P] + hidden + [1]
        b.set_policy_mlp(make_layers(pw, 7))
        b.set_value_mlp(make_layers(vw, 8))
        b.set_q_mlp(make_layers(qw, 9))
        b.ddpg_sync_targets()
        table = r.randint(0, n, size=(args.bench_steps, B)).astype(np.int32)
        kinds = {"ddpg": lambda: b.ddpg_fit(table, 0.99, 0.005, 1.0), "policy": lambda: b.fit(table), "value": lambda: b.value_fit(table),
                 "critic": lambda: b.q_fit(table, 0.99, 1.0), "actor": lambda: b.dpg_fit(table, 1.0),
                 "bc_filter": lambda: b.dpg_bc_fit(table, 1.0, 1.0, 1.0, True), "bc_nofilter": lambda: b.dpg_bc_fit(table, 1.0, 1.0, 1.0, False)}
        if args.one_shape:                                                    # for a kernel trace: DDPG steps and nothing else
            for _ in range(args.rounds + 1):
                kinds["ddpg"]()
            say("hidden %-15r B %4d: %d clothhip_ddpg_fit calls of %d steps, last one %.3f ms per step on the device; %d launches per step"
                % (hidden, B, args.rounds + 1, args.bench_steps, b.last_kernel_ms / args.bench_steps, launches_per_step(pw, qw, B)))
            continue
        dev = {k: [] for k in kinds}
        for k, f in kinds.items():
            f()
        for _ in range(args.rounds):
            for k, f in kinds.items():
                f()
                dev[k].append(b.last_kernel_ms / args.bench_steps)
        med = {k: float(np.median(v)) for k, v in dev.items()}
        base = med["policy"] + med["value"]
        say("hidden %-15r B %4d: ddpg_fit step %.3f ms (%.3f-%.3f) = critic %.3f + actor %.3f + the soft updates; policy_fit step %.3f (%.3f-%.3f) + value_fit step "
            "%.3f (%.3f-%.3f) = %.3f ms; ratio %.2f; %d launches per DDPG step" % (hidden, B, med["ddpg"], min(dev["ddpg"]), max(dev["ddpg"]), med["critic"], med["actor"],
                                                                                   med["policy"], min(dev["policy"]), max(dev["policy"]), med["value"], min(dev["value"]),
                                                                                   max(dev["value"]), base, med["ddpg"] / base, launches_per_step(pw, qw, B)))
        say("    BC actor step, filter on %.3f ms (%.3f-%.3f), ratio to the plain actor step %.3f, %d launches; filter off %.3f ms (%.3f-%.3f), ratio %.3f, %d launches; "
            "plain actor step %.3f ms (%.3f-%.3f), %d launches" % (med["bc_filter"], min(dev["bc_filter"]), max(dev["bc_filter"]), med["bc_filter"] / med["actor"],
                                                                   bc_launches_per_step(pw, qw, B, True), med["bc_nofilter"], min(dev["bc_nofilter"]), max(dev["bc_nofilter"]),
                                                                   med["bc_nofilter"] / med["actor"], bc_launches_per_step(pw, qw, B, False), med["actor"], min(dev["actor"]),
                                                                   max(dev["actor"]), bc_launches_per_step(pw, qw, B, False)))
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100, help="DDPG steps per iteration")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=0.1, help="standard deviation of the exploration noise")
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--act-bound", type=float, default=1.0)
    ap.add_argument("--hidden", default="64,64")
    ap.add_argument("--lr", type=float, default=1e-4, help="the policy's Adam learning rate")
    ap.add_argument("--q-lr", type=float, default=1e-3, help="the critic's Adam learning rate")
    ap.add_argument("--expert", default=None, help="arm this expert beside the policy (oracle_corner, highest_point): the rows carry its action")
    ap.add_argument("--beta", type=float, default=0.0, help="with --expert: the share of the slots on which the expert takes the action over")
    ap.add_argument("--bc-coef", type=float, default=0.0, help="the coefficient of the behaviour-cloning term of the actor's loss")
    ap.add_argument("--q-coef", type=float, default=1.0, help="the coefficient of the policy-gradient term of the actor's loss")
    ap.add_argument("--no-q-filter", action="store_true", help="clone on every labelled row, not only where the critic rates the expert's action higher")
    ap.add_argument("--demo-fraction", type=float, default=None, help="that share of every minibatch is drawn from the rows with an expert action")
    ap.add_argument("--bench", action="store_true", help="time a DDPG step beside a policy_fit step plus a value_fit step")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--one-shape", default=None, help="with --bench: one shape only, as HIDDEN:B, e.g. 256,256,256:4096 (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    if args.bench:
        bench_section(args)
    else:
        run(args)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
