#!/usr/bin/env python3
"""What a step of the device trainer (clothhip_policy_fit, csrc/cloth_policy_fit.hpp) costs, measured. It prints its figures (and with
--out FILE also appends them there); a run of it is quoted, with the command, in profiles/policy_fit.txt and DESIGN 4.3.4.

One ClothBatch of one 25x25 cloth (3P = 1875 inputs), a dataset of 8192 uniform rows with uniform labels, networks with hidden widths
[64, 64] and [256, 256, 256], minibatches of B = 256 and 4096 rows:
  * ms per Adam step: `--steps` steps in ONE clothhip_policy_fit call (no host work between the steps), device time by HIP events
    (clothhip_last_kernel_ms) and wall time of the call, the median of `--rounds` calls after one warm-up call;
  * the f32 FLOP/s that is: 6 B sum_l in_l out_l per step (forward, weight gradient, input gradient: 2 B in out each; the input gradient of
    layer 0 is not computed, so 4 B in_0 out_0 there), beside the 157 TF f32-matrix peak of the MI355X;
  * the same steps in numpy float32 (BLAS matmuls, the same Adam) on the host, wall time.
The smaller shapes are launch- and latency-bound (a step is 4 to 6 kernel launches per layer): the tool says what a step costs there, it
does not claim a rate.
    python3 tools/fit_bench.py [--steps 20] [--rounds 5] [--out FILE]
--members runs the members section instead (clothhip_policy_fit_members; profiles/fit_members.txt, profiles/fit_unified.txt, DESIGN
4.3.7): a grouped Adam step of G = 1, 4, 16, 64 networks at B = 256 against G single-network steps timed in the same process. Both
calls run the same kernels (k_fit_gemm, k_fit_loss, k_fit_reduce, k_fit_colsum, k_fit_adam): the single network is the call
members = {0}, n_m = 1.
    python3 tools/fit_bench.py --members [--steps 20] [--rounds 5] [--out FILE]
--ppo runs the PPO section instead (clothhip_policy_fit_ppo; profiles/ppo.txt): on the four shapes above, an Adam step
of the clipped surrogate beside the squared-error step timed in the same process on the same handle and rows. The two differ in ONE
launch per step: k_fit_loss_ppo in the place of k_fit_loss, reading its constants from a table of one row (profiles/fit_loss_modes.txt).
    python3 tools/fit_bench.py --ppo [--steps 20] [--rounds 5] [--out FILE]
--ppo-sigma runs the learned-sigma section instead (clothhip_policy_fit_ppo_sigma; profiles/ppo_sigma.txt): on the four
shapes, an Adam step with the log-sigma head beside the fixed-sigma PPO step, alternated on one handle. The two differ in the loss launch
(k_fit_loss_ppo_sigma: nine exp_fixed per row in one workgroup, seven reductions) and in one more optimizer launch over the head.
    python3 tools/fit_bench.py --ppo-sigma [--steps 20] [--rounds 5] [--out FILE]
--ppo-members runs the grouped PPO section instead (clothhip_policy_fit_ppo_members; profiles/ppo_members.txt): a grouped
PPO Adam step of G = 1, 4, 16, 64 networks at B = 256, every member under its own sigma and clip, beside the grouped squared-error step
(--members' call) alternated on the same handle, and beside G single-network PPO steps timed in the same process. The grouped steps
differ in ONE launch: k_fit_loss_ppo (the single-network step's kernel, member j under row j of the table) in the place of k_fit_loss, one
workgroup per member either way.
    python3 tools/fit_bench.py --ppo-members [--steps 20] [--rounds 5] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                                    # noqa: E402
from gym_cloth_amd.batch import ClothBatch                      # noqa: E402

LINES = []
PEAK_TF = 157.0


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def layers_of(widths, seed=7):
    r = np.random.RandomState(seed)
    return [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32),
             (r.normal(size=widths[l + 1]) / np.sqrt(widths[l])).astype(np.float32)) for l in range(len(widths) - 1)]


def flop_per_step(widths, B):
    return sum((4 if l == 0 else 6) * B * widths[l] * widths[l + 1] for l in range(len(widths) - 1))


def numpy_steps(layers, rows, labels, table, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """The same Adam steps in numpy float32 (BLAS); returns the wall seconds."""
    f = np.float32
    Ws, bs = [W.copy() for W, _ in layers], [b.copy() for _, b in layers]
    par = Ws + bs
    ms, vs = [np.zeros_like(p) for p in par], [np.zeros_like(p) for p in par]
    L = len(Ws)
    t0 = time.perf_counter()
    for t, idx in enumerate(table, start=1):
        hs = [rows[idx]]
        for l in range(L):
            z = hs[-1] @ Ws[l].T + bs[l]
            hs.append(np.maximum(z, 0) if l + 1 < L else z)
        g = (hs[-1] - labels[idx]) / f(2 * len(idx))
        gW, gb = [None] * L, [None] * L
        for l in range(L - 1, -1, -1):
            gW[l], gb[l] = g.T @ hs[l], g.sum(axis=0)
            if l:
                g = (g @ Ws[l]) * (hs[l] > 0)
        a_t = f(lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t))
        for p, m, v, gr in zip(par, ms, vs, gW + gb):
            m *= f(b1); m += f(1 - b1) * gr
            v *= f(b2); v += f(1 - b2) * gr * gr
            p -= a_t * m / (np.sqrt(v) + f(eps))
    return time.perf_counter() - t0


def members_section(args, rows, labels):
    """The grouped trainer (clothhip_policy_fit_members): ms per grouped Adam step of G networks at B = 256 against G times
    the ms of a single-network step -- clothhip_policy_fit on a shared-network handle in this very process, `--rounds` repetitions, so
    its own spread is known."""
    single, group = (ClothBatch(bench.bench_cfg(25, 0.02, "tier1"), n_envs=1, precision="f32") for _ in range(2))
    for x in (single, group):
        x.fit_append(rows, labels)
    B = 256
    r = np.random.RandomState(5)
    say("fit_bench members: 25x25, B = %d, Adam, %d steps per call, %d calls after one warm-up call; device ms by HIP events around all steps of a call"
        % (B, args.steps, args.rounds))
    for hidden in ([64, 64], [256, 256, 256]):
        widths = [3 * single.P] + hidden + [4]
        single.set_policy_mlp(layers_of(widths))
        table = r.randint(0, args.rows, size=(args.steps, B)).astype(np.int32)
        single.fit(table)
        dev1, wall1 = [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            single.fit(table)
            wall1.append((time.perf_counter() - t0) * 1e3 / args.steps)
            dev1.append(single.last_kernel_ms / args.steps)
        s1, spread = float(np.median(dev1)), max(dev1) - min(dev1)
        say("hidden %-15r single network: device %.3f ms/step (the %d calls: %s; spread %.3f), wall %.3f ms/step"
            % (hidden, s1, args.rounds, " ".join("%.3f" % d for d in dev1), spread, float(np.median(wall1))))
        for G in (1, 4, 16, 64):
            group.set_policy_population([layers_of(widths, seed=7 + g) for g in range(G)], np.zeros(1, dtype=np.int32))
            members = np.arange(G)
            tbl = r.randint(0, args.rows, size=(args.steps, G, B)).astype(np.int32)
            group.fit_members(members, tbl)
            dev, wall = [], []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                group.fit_members(members, tbl)
                wall.append((time.perf_counter() - t0) * 1e3 / args.steps)
                dev.append(group.last_kernel_ms / args.steps)
            d = float(np.median(dev))
            say("hidden %-15r G %2d grouped: device %.3f ms/step (min %.3f, max %.3f), wall %.3f ms/step; G single steps %.3f ms (+- %.3f) -> "
                "grouped / (G x single) = %.3f, %.2f TF" % (hidden, G, d, min(dev), max(dev), float(np.median(wall)), G * s1, G * spread, d / (G * s1),
                                                            G * flop_per_step(widths, B) / d / 1e9))
    single.close()
    group.close()


def ppo_members_section(args, rows, labels):
    """The grouped PPO step (clothhip_policy_fit_ppo_members) at B = 256: ms per grouped Adam step of G networks beside
    the grouped squared-error step of the same handle, rows and tables (alternated), and beside G times the single-network PPO step
    (clothhip_policy_fit_ppo on a shared-network handle in this process). Old means from one member snapshot, row i under member i % G."""
    single, group = (ClothBatch(bench.bench_cfg(25, 0.02, "tier1"), n_envs=1, precision="f32") for _ in range(2))
    adv = np.random.RandomState(9).normal(size=len(rows)).astype(np.float32)
    for x in (single, group):
        x.fit_append(rows, labels, weights=adv)
    B = 256
    r = np.random.RandomState(5)
    say("fit_bench ppo-members: 25x25, B = %d, Adam lr 1e-5, Gaussian advantages, member j under sigma 0.5 + 0.01 j and clip 0.2; %d steps per call, "
        "%d calls of each kind alternated after one warm-up call; device ms by HIP events around all steps of a call" % (B, args.steps, args.rounds))
    for hidden in ([64, 64], [256, 256, 256]):
        widths = [3 * single.P] + hidden + [4]
        single.set_policy_mlp(layers_of(widths))
        single.fit_snapshot_policy()
        table = r.randint(0, args.rows, size=(args.steps, B)).astype(np.int32)
        single.fit_ppo(table, 0.5, 0.2, lr=1e-5)
        dev1 = []
        for _ in range(args.rounds):
            single.fit_ppo(table, 0.5, 0.2, lr=1e-5)
            dev1.append(single.last_kernel_ms / args.steps)
        s1, spread = float(np.median(dev1)), max(dev1) - min(dev1)
        say("hidden %-15r single-network PPO: device %.3f ms/step (the %d calls: %s; spread %.3f)"
            % (hidden, s1, args.rounds, " ".join("%.3f" % d for d in dev1), spread))
        for G in (1, 4, 16, 64):
            group.set_policy_population([layers_of(widths, seed=7 + g) for g in range(G)], np.zeros(1, dtype=np.int32))
            group.fit_snapshot_policy_members(np.arange(args.rows, dtype=np.int32) % G)
            snap_ms = group.last_kernel_ms
            members, sigma = np.arange(G), 0.5 + 0.01 * np.arange(G)
            tbl = r.randint(0, args.rows, size=(args.steps, G, B)).astype(np.int32)
            hyper = dict(lr=1e-5)
            group.fit_members(members, tbl, hyper)
            group.fit_ppo_members(members, tbl, sigma, 0.2, hyper)
            mse, ppo = [], []
            for _ in range(args.rounds):
                group.fit_members(members, tbl, hyper)
                mse.append(group.last_kernel_ms / args.steps)
                stats = group.fit_ppo_members(members, tbl, sigma, 0.2, hyper)
                ppo.append(group.last_kernel_ms / args.steps)
            m, p = float(np.median(mse)), float(np.median(ppo))
            say("hidden %-15r G %2d: grouped squared error %.3f ms/step (min %.3f, max %.3f) | grouped PPO %.3f ms/step (min %.3f, max %.3f) | PPO / "
                "squared error = %.3f | G single PPO steps %.3f ms (+- %.3f) -> grouped / (G x single) = %.3f; member snapshot of %d rows %.3f ms; "
                "last mean clip_fraction %.3f, kl %.5f" % (hidden, G, m, min(mse), max(mse), p, min(ppo), max(ppo), p / m, G * s1, G * spread,
                                                         p / (G * s1), args.rows, snap_ms, stats[-1, :, 1].mean(), stats[-1, :, 2].mean()))
    single.close()
    group.close()


def ppo_section(args, b, rows, labels):
    """A PPO Adam step beside the squared-error step: the same handle, network, rows and minibatch table, `--rounds` calls of `--steps`
    steps each after one warm-up call, alternated; Gaussian advantages in the weight column, old means from one snapshot."""
    r = np.random.RandomState(3)
    b.fit_append(rows, labels, weights=np.random.RandomState(9).normal(size=len(rows)).astype(np.float32))
    say("fit_bench ppo: 25x25 (1875 inputs), dataset %d rows, Gaussian advantages, sigma 0.5, clip 0.2; %d Adam steps per call, %d calls of each kind "
        "alternated after one warm-up call; device ms by HIP events around all steps of a call" % (args.rows, args.steps, args.rounds))
    for hidden in ([64, 64], [256, 256, 256]):
        widths = [3 * b.P] + hidden + [4]
        for B in (256, 4096):
            table = r.randint(0, args.rows, size=(args.steps, B)).astype(np.int32)
            b.set_policy_mlp(layers_of(widths))
            b.fit_snapshot_policy()
            b.fit(table, lr=1e-5)
            b.fit_ppo(table, 0.5, 0.2, lr=1e-5)
            mse, ppo = [], []
            for _ in range(args.rounds):
                b.fit(table, lr=1e-5)
                mse.append(b.last_kernel_ms / args.steps)
                stats = b.fit_ppo(table, 0.5, 0.2, lr=1e-5)
                ppo.append(b.last_kernel_ms / args.steps)
            m, p = float(np.median(mse)), float(np.median(ppo))
            say("hidden %-15r B %4d: squared error %.3f ms/step (min %.3f, max %.3f) | PPO %.3f ms/step (min %.3f, max %.3f) | PPO - squared error "
                "%+.3f ms (%+.1f %%); last clip_fraction %.3f, kl %.5f" % (hidden, B, m, min(mse), max(mse), p, min(ppo), max(ppo), p - m,
                                                                        100.0 * (p - m) / m, stats[-1, 1], stats[-1, 2]))


def ppo_sigma_section(args, b, rows, labels):
    """A learned-sigma PPO Adam step beside the fixed-sigma one: the same handle, network, rows and minibatch table, `--rounds` calls of
    `--steps` steps each after one warm-up call, alternated; Gaussian advantages, old means and old log sigmas from one snapshot."""
    r = np.random.RandomState(3)
    b.fit_append(rows, labels, weights=np.random.RandomState(9).normal(size=len(rows)).astype(np.float32))
    say("fit_bench ppo-sigma: 25x25 (1875 inputs), dataset %d rows, Gaussian advantages, sigma 0.5 / head log 0.5, clip 0.2, ent_coef 0.01; %d Adam "
        "steps per call, %d calls of each kind alternated after one warm-up call; device ms by HIP events around all steps of a call"
        % (args.rows, args.steps, args.rounds))
    head = np.full(4, np.log(0.5))
    for hidden in ([64, 64], [256, 256, 256]):
        widths = [3 * b.P] + hidden + [4]
        for B in (256, 4096):
            table = r.randint(0, args.rows, size=(args.steps, B)).astype(np.int32)
            b.set_policy_mlp(layers_of(widths))
            b.set_policy_log_sigma(head)
            b.fit_snapshot_policy()
            b.fit_ppo(table, 0.5, 0.2, lr=1e-5)
            b.fit_ppo_sigma(table, 0.2, 0.01, lr=1e-5)
            fixed, learned = [], []
            for _ in range(args.rounds):
                b.fit_ppo(table, 0.5, 0.2, lr=1e-5)
                fixed.append(b.last_kernel_ms / args.steps)
                stats, _ = b.fit_ppo_sigma(table, 0.2, 0.01, lr=1e-5)
                learned.append(b.last_kernel_ms / args.steps)
            m, p = float(np.median(fixed)), float(np.median(learned))
            say("hidden %-15r B %4d: fixed sigma %.3f ms/step (min %.3f, max %.3f) | learned sigma %.3f ms/step (min %.3f, max %.3f) | learned - fixed "
                "%+.3f ms (%+.1f %%), the fixed step's spread %.3f ms; last clip_fraction %.3f, kl %.5f, entropy %.4f"
                % (hidden, B, m, min(fixed), max(fixed), p, min(learned), max(learned), p - m, 100.0 * (p - m) / m, max(fixed) - min(fixed),
                   stats[-1, 1], stats[-1, 2], stats[-1, 3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--members", action="store_true", help="run the members section (the grouped trainer) instead of the single-network one")
    ap.add_argument("--ppo", action="store_true", help="run the PPO section (a clipped-surrogate step beside the squared-error step) instead")
    ap.add_argument("--ppo-sigma", action="store_true", help="run the learned-sigma section (a step with the log-sigma head beside the fixed-sigma PPO step) instead")
    ap.add_argument("--ppo-members", action="store_true", help="run the grouped PPO section (a grouped clipped-surrogate step beside the grouped squared-error step) instead")
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    b = ClothBatch(bench.bench_cfg(25, 0.02, "tier1"), n_envs=1, precision="f32")
    r = np.random.RandomState(3)
    rows = r.uniform(-1, 1, size=(args.rows, 3 * b.P)).astype(np.float32)
    labels = r.uniform(-1, 1, size=(args.rows, 4)).astype(np.float32)
    if args.members or args.ppo_members:
        b.close()
        (ppo_members_section if args.ppo_members else members_section)(args, rows, labels)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write("\n".join(LINES) + "\n")
        return
    if args.ppo or args.ppo_sigma:
        (ppo_sigma_section if args.ppo_sigma else ppo_section)(args, b, rows, labels)
        b.close()
        if args.out:
            with open(args.out, "a") as fh:
                fh.write("\n".join(LINES) + "\n")
        return
    t0 = time.perf_counter()
    b.fit_append(rows, labels)
    say("fit_bench: 25x25 (1875 inputs), dataset %d rows appended in %.1f ms; %d Adam steps per call, median of %d calls; f32-matrix peak %.0f TF"
        % (args.rows, (time.perf_counter() - t0) * 1e3, args.steps, args.rounds, PEAK_TF))
    for hidden in ([64, 64], [256, 256, 256]):
        widths = [3 * b.P] + hidden + [4]
        layers = layers_of(widths)
        for B in (256, 4096):
            table = r.randint(0, args.rows, size=(args.steps, B)).astype(np.int32)
            b.set_policy_mlp(layers)
            b.fit(table)                                        # warm-up (allocations, first launches)
            dev, wall = [], []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                b.fit(table)
                wall.append((time.perf_counter() - t0) * 1e3 / args.steps)
                dev.append(b.last_kernel_ms / args.steps)
            host = numpy_steps(layers, rows, labels, table) * 1e3 / args.steps
            fl = flop_per_step(widths, B)
            d = float(np.median(dev))
            say("hidden %-15r B %4d: device %.3f ms/step (min %.3f, max %.3f), wall %.3f ms/step, %.2f GFLOP/step -> %.2f TF (%.1f %% of peak); "
                "numpy float32 on the host %.2f ms/step" % (hidden, B, d, min(dev), max(dev), float(np.median(wall)), fl / 1e9, fl / d / 1e9,
                                                          100.0 * fl / d / 1e9 / PEAK_TF, host))
    b.close()
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
