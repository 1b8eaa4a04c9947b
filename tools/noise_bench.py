#!/usr/bin/env python3
"""What the exploration noise made on the device costs, measured beside the host route it replaces. Per shape [T, E, 4]:
  the fill      ClothBatch.policy_noise_fill: the kernel by the handle's events (clothhip_last_kernel_ms), and the call on a host clock
                around fill + the wait for the kernel -- under a host sigma (one small upload and its wait in front of the kernel) and
                under the log-sigma head (no upload, nothing waited for before the launch);
  the host      RandomState.standard_normal((T, E, 4)) times sigma, then the upload of the table (clothhip_device_upload, synchronous) --
                what a caller of step_many(policy_noise=ndarray) pays per launch; with a learned sigma also the head's download and np.exp.
Every figure is the median of --reps repetitions after --warmup, with min and max; the table of the last fill is compared with
references.policy_noise_reference by bytes. The shapes are one PPO iteration's collection as tools/ppo_demo.py --bench runs it
([12, 512, 4]) and a larger one ([48, 2048, 4]). It prints its figures and with --out FILE appends them there; profiles/policy_noise.txt
holds a run. A run without a GPU fails: nothing here falls back.
    python3 tools/noise_bench.py [--reps 200] [--warmup 20] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd import ClothBatch                  # noqa: E402
from gym_cloth_amd.policies import exp_fixed_reference, policy_noise_reference      # noqa: E402

SHAPES = [(12, 512), (48, 2048)]
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def stats(xs, unit=1e6, name="us"):
    xs = np.asarray(xs) * unit
    return "%.1f %s (min %.1f, max %.1f)" % (np.median(xs), name, xs.min(), xs.max())


def section(T, E, reps, warmup):
    b = ClothBatch(bench.bench_cfg(25, 0.02), n_envs=E, precision="f32")
    sigma = np.array([0.1, 0.1, 0.05, 0.05])
    head = np.log(sigma).astype(np.float32)
    b.set_policy_log_sigma(head)
    nbytes = T * E * 4 * 8
    say("[%d, %d, 4] float64: %d threads in %d workgroups of 256, a table of %.1f KB; %d repetitions after %d, medians"
        % (T, E, T * E, (T * E + 255) // 256, nbytes / 1024.0, reps, warmup))
    for name, sg in (("host sigma [4]", sigma), ("the log-sigma head", None)):
        kern, wall = [], []
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            b.policy_noise_fill(1000 + i, T, sigma=sg)
            ms = b.last_kernel_ms                                  # (waits for the kernel's second event)
            t1 = time.perf_counter()
            if i >= warmup:
                kern.append(ms * 1e-3)
                wall.append(t1 - t0)
        want = policy_noise_reference(1000 + warmup + reps - 1, T, E, sigma if sg is not None else exp_fixed_reference(head.astype(np.float64)))
        say("    fill under %-18s: kernel %s, call with the wait for it %s; the table is the reference's by bytes: %s"
            % (name, stats(kern), stats(wall), b.policy_noise_get().tobytes() == want.tobytes()))
    ptr = b.device_alloc(nbytes)
    draw, up, both, head_dl = [], [], [], []
    for i in range(warmup + reps):
        r = np.random.RandomState(1000 + i)
        t0 = time.perf_counter()
        tab = r.standard_normal((T, E, 4)) * sigma
        t1 = time.perf_counter()
        b.device_upload(ptr, tab)
        t2 = time.perf_counter()
        sg = np.exp(b.get_policy_log_sigma().astype(np.float64))      # what a learned sigma adds per iteration on this route
        t3 = time.perf_counter()
        if i >= warmup:
            draw.append(t1 - t0); up.append(t2 - t1); both.append(t2 - t0); head_dl.append(t3 - t2)
    b.device_free(ptr)
    say("    the host route          : standard_normal times sigma %s, the upload %s, together %s; the head's download and np.exp %s"
        % (stats(draw), stats(up), stats(both), stats(head_dl)))
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    say("noise bench: clothhip_policy_noise_fill beside numpy's draw and the upload it replaces")
    for T, E in SHAPES:
        section(T, E, args.reps, args.warmup)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
