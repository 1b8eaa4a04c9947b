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
  (d) k_fit_gather (clothhip_fit_data_append_launch) on the rows of one armed launch of --envs x --slots slots that kept its tables on the
      device, against hipMemcpyAsync device-to-device of the same bytes on the same handle's stream: kernel time (HIP events) and call
      time (host clock; both calls synchronise).
  (e) the device route (append_launch of those rows) against the host route on the same launch: download of both tables +
      envs.slot_start_obs + clothhip_fit_data_append.
  (f) demos.dagger_collect over --collect-actions actions per env in whole-slot launches of --slots slots and in time slices, on the same
      build and from the same seeds. The slice is sized as bench.py sizes its own: fuse x (the measured duration of one env step), here
      --slots x (the mean time an env was busy per slot in the whole-slot launches, from the launch's per-env ticks), with bench.py's
      rule for the slots offered per slice, max(4 fuse, slice / 40 ms, 8).
    python3 tools/dagger_bench.py [--envs 512] [--slots 12] [--launches 3] [--rows 196608] [--collect-actions 36] [--only-collect] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from fork_bench import EventTimer, hip_runtime, stats                # noqa: E402
from gym_cloth_amd import _lib                                       # noqa: E402
from gym_cloth_amd.demos import dagger_collect                       # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv, slot_start_obs, slot_start_sources   # noqa: E402
from gym_cloth_amd.policies import MLPPolicy, MLPTrainer, OracleCornerPolicy     # noqa: E402

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


def gather_and_routes(E, T, layers, reps=10):
    """(d) and (e): one armed launch that keeps its tables on the device AND, from a twin, one that downloads them."""
    import ctypes as C
    hip = hip_runtime()
    env, _ = make_env(E, layers)
    tr = MLPTrainer(env, MLPPolicy(env, layers))
    b = env.batch
    b.fit_hold()
    before = np.asarray(env.state, dtype=np.float32).reshape(E, -1)
    out = env.step_many(policy="mlp", n_actions=T, want_obs="device", expert="oracle_corner")
    t_, e_ = np.nonzero(out["ran"])
    rows = np.concatenate([slot_start_sources(out)[t_, e_], (t_ * E + e_)[:, None].astype(np.int32)], axis=1)
    n, row_bytes = len(rows), 3 * env.P * 4
    moved = 2 * n * (row_bytes + 16)                                         # read + written: the rows and their labels (doubles in, floats out)
    timer = EventTimer(hip, b.stream)
    tr.append_launch(rows)                                                   # (allocates the tables)
    dev, wall, kern = [], [], []
    for _ in range(reps):
        tr.clear()
        d, w = timer(lambda: tr.append_launch(rows))
        dev.append(d); wall.append(w); kern.append(b.last_kernel_ms * 1e-3)
    a, c = b.device_alloc(n * row_bytes), b.device_alloc(n * row_bytes)
    copy = lambda: (hip.hipMemcpyAsync(C.c_void_p(c), C.c_void_p(a), n * row_bytes, 3, C.c_void_p(b.stream)), hip.hipStreamSynchronize(C.c_void_p(b.stream)))
    copy()
    mdev, mwall = zip(*[timer(copy) for _ in range(reps)])
    b.device_free(a); b.device_free(c)
    say()
    say("(d) k_fit_gather: the %d rows that ran of one %d x %d-slot launch, %d B per row, %.1f MB read + written" % (n, E, T, row_bytes, moved / 1e6))
    say("    sources: %d held, %d reset rows, %d slot rows" % tuple(int((rows[:, 0] == k).sum()) for k in (_lib.FIT_SRC_HELD, _lib.FIT_SRC_RESETS, _lib.FIT_SRC_SLOTS)))
    say("    clothhip_fit_data_append_launch, the kernel alone (events inside the call):        %s" % stats(kern))
    say("    ... HIP events around the call (index upload, flag clear, kernel, flag download):  %s" % stats(dev))
    say("    ... host clock around the call (it synchronises; incl. the Python wrapper):        %s" % stats(wall))
    say("    hipMemcpyAsync device-to-device of the rows' %d bytes, events:                     %s" % (n * row_bytes, stats(mdev)))
    say("    ... host clock (with its synchronise):                                             %s" % stats(mwall))
    gb, mb = moved / np.median(kern), 2 * n * row_bytes / np.median(mdev)
    say("    -> gather kernel %.2f TB/s read + written, copy %.2f TB/s; kernel time gather / copy = %.2f, call time = %.2f" % (
        gb / 1e12, mb / 1e12, np.median(kern) / np.median(mdev), np.median(wall) / np.median(mwall)))
    got = tr.data()
    # (e) the host route on a twin's launch from the same seeds
    twin, _ = make_env(E, layers)
    tw = MLPTrainer(twin, MLPPolicy(twin, layers))
    out2 = twin.step_many(policy="mlp", n_actions=T, want_obs="device", expert="oracle_corner")      # warm-up of the twin's buffers
    twin.close()
    twin, _ = make_env(E, layers)
    tw = MLPTrainer(twin, MLPPolicy(twin, layers))
    before2 = np.asarray(twin.state, dtype=np.float32).reshape(E, -1)
    same_start = np.array_equal(before2, before)
    t0 = time.perf_counter()
    out2 = twin.step_many(policy="mlp", n_actions=T, want_obs=True, expert="oracle_corner")
    t_launch_host = time.perf_counter() - t0
    ran = out2["ran"]
    host = []
    for _ in range(3):
        tw.clear()
        t0 = time.perf_counter()
        obs_rows = slot_start_obs(out2, before2)[ran]
        t1 = time.perf_counter()
        tw.append(obs_rows, out2["expert_actions"][ran])
        host.append((t1 - t0, time.perf_counter() - t1))
    same = np.array_equal(got[0], tw.data()[0]) and np.array_equal(got[1], tw.data()[1])
    say("(e) the same launch, host route: slot_start_obs %s + fit_data_append %s; device route (d): %s; the twin started from the same states: %s; stored rows equal: %s" % (
        stats([h[0] for h in host]), stats([h[1] for h in host]), stats(wall), same_start, same))
    say("    (the host route's launch also downloads both tables: step_many(want_obs=True) took %.1f ms on a fresh handle)" % (t_launch_host * 1e3))
    env.close(); twin.close()


def collect_slices(E, T, N, layers):
    """(f): dagger_collect in whole-slot launches and in time slices, same seeds, same build."""
    res = {}
    busy_ms = None
    for name in ("whole", "sliced"):
        env, _ = make_env(E, layers)
        tr = MLPTrainer(env, MLPPolicy(env, layers))
        env.step_many(policy="mlp", n_actions=1, want_obs="device", expert="oracle_corner")          # warm-up: buffers, code objects
        env.seed([1000 + e for e in range(E)])
        env.reset()
        if name == "whole":
            r = dagger_collect(env, tr, "oracle_corner", n_actions=N, beta=0.5, seed=3, slots_per_launch=T)
            ticks = np.sum([np.asarray(x) for x in r["op_ticks"]], axis=0)[:, :3].sum(axis=1)      # actions + reset pulls + settling, per env
            busy_ms = float(ticks.mean()) / 1e5 / N                                                  # 100 MHz ticks -> ms per slot
            budget, slots = 0.0, T
        else:
            budget = T * busy_ms
            slots = max(4 * T, int(budget / 40.0), 8)
            r = dagger_collect(env, tr, "oracle_corner", n_actions=N, beta=0.5, seed=3, slots_per_launch=slots, time_budget_ms=budget)
        res[name] = (r, budget, slots)
        env.close()
    say()
    say("(f) demos.dagger_collect, %d cloths, %d actions per env, beta 0.5: whole-slot launches of %d slots against time slices of "
        "%d x %.2f ms (the mean busy time of an env per slot, measured in the whole-slot run) = %.1f ms, %d slots offered per slice" % (
            E, N, T, T, busy_ms, res["sliced"][1], res["sliced"][2]))
    rate = {}
    for name in ("whole", "sliced"):
        r = res[name][0]
        rate[name] = (r["substeps"] / r["took"], r["substeps"] / (r["kernel_ms"] * 1e-3), r["appended"] / r["took"])
        say("    %-6s %3d launches, %6d rows appended, %9d substeps (actions + resets, all slots that ran), %.0f ms wall (launch kernels %.0f ms): "
            "%.3f M substeps/s wall, %.3f M substeps/s kernel, %.0f labelled rows/s" % (
                name, r["launches"], r["appended"], r["substeps"], r["took"] * 1e3, r["kernel_ms"], rate[name][0] / 1e6, rate[name][1] / 1e6, rate[name][2]))
    say("    sliced / whole: substeps/s wall %.3f, substeps/s kernel %.3f, labelled rows/s %.3f" % tuple(
        rate["sliced"][k] / rate["whole"][k] for k in range(3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--rows", type=int, default=196608)
    ap.add_argument("--numpy-rows", type=int, default=4096)
    ap.add_argument("--collect-actions", type=int, default=36, help="(f): actions per env of each dagger_collect run")
    ap.add_argument("--only-collect", action="store_true", help="skip (a) .. (c): only the device-route sections (d) .. (f)")
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    E, T, n_l = args.envs, args.slots, args.launches
    r = np.random.RandomState(7)
    widths = [1875, 64, 64, 4]
    layers = [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32),
               (r.normal(size=widths[l + 1]) / np.sqrt(widths[l])).astype(np.float32)) for l in range(3)]
    if not args.only_collect:
        expert_cost(args, E, T, n_l, widths, layers)
    gather_and_routes(E, T, layers)
    collect_slices(E, T, args.collect_actions, layers)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


def expert_cost(args, E, T, n_l, widths, layers):
    """(a) .. (c)"""
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


if __name__ == "__main__":
    main()
