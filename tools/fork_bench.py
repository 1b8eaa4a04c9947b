#!/usr/bin/env python3
"""What clothhip_fork and ClothVecEnv.lookahead cost, measured: stated figures for DESIGN.md, written to profiles/fork_lookahead.txt.

  1. fork bandwidth: 512 cloths (25x25, fp32) branched into 8 192 (16 each) by ONE fork; bytes read + written per second from HIP
     events around the call, beside a plain hipMemcpyAsync device-to-device of the same byte count in the same run and the HBM peak.
  2. the same replication through the host route the fork replaces (get_state + set_state + the tear flags; the rest table is shared
     and equal, the materials uniform, so nothing else is needed for equal content), host clock around calls that synchronise.
  3. one lookahead at E = 512, K = 16 against the only way without it: K rounds of upload the state, step, read the metrics on the
     512-env handle -- same actions, results compared (fp64); and the fp32 lookahead with the stepper build its 8 192-cloth batch runs.
Every timed call is warmed up once and repeated; median and min .. max are printed.
    python3 tools/fork_bench.py [--out profiles/fork_lookahead.txt] [--bench label=bench_output.json ...]
--bench: result lines of bench.py runs to list beside each other (the headline value and config.variant of each)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd import ClothBatch, _lib            # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv            # noqa: E402

HBM_PEAK = 8.0e12                                     # bytes/s, MI355X
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def stats(v, unit="ms", scale=1e3):
    v = np.asarray(v) * scale
    return "median %.3f %s (min %.3f .. max %.3f, n = %d)" % (np.median(v), unit, v.min(), v.max(), len(v))


def hip_runtime():
    _lib.load()
    for name in (None, "libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            h = C.CDLL(name)
            h.hipEventCreate
            break
        except (OSError, AttributeError):
            continue
    else:
        raise RuntimeError("HIP runtime not found in the process")
    h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    h.hipEventSynchronize.argtypes = [C.c_void_p]
    h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    return h


class EventTimer(object):
    """milliseconds between two HIP events recorded on `stream` around fn()"""

    def __init__(self, hip, stream):
        self.hip, self.stream = hip, C.c_void_p(stream)
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(self.e0)) == 0 and hip.hipEventCreate(C.byref(self.e1)) == 0

    def __call__(self, fn):
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0 and self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value * 1e-3, wall


def fork_bandwidth(n_src=512, fan=16, reps=20):
    hip = hip_runtime()
    cfg = bench.bench_cfg(25, 0.02)
    src = ClothBatch(cfg, n_envs=n_src, precision="f32")
    dst = ClothBatch(cfg, n_envs=n_src * fan, precision="f32")
    xy = np.random.RandomState(0).uniform(0.2, 0.8, size=(n_src, 2))
    src.grab_top(xy); src.update(20, delta=[0.0005, 0.0, 0.0025])           # 512 different cloths in the middle of a lift
    idx = np.repeat(np.arange(n_src), fan)
    n = len(idx)
    Ppad = (src.P + 63) // 64 * 64
    per = 2 * 3 * Ppad * 4 + Ppad + 4                                        # pos + prev rows, pin bytes, tear flag of one cloth
    moved = 2 * n * per                                                      # read + written
    timer = EventTimer(hip, dst.stream)
    dst.fork_from(src, idx)
    dev, wall = zip(*[timer(lambda: dst.fork_from(src, idx)) for _ in range(reps)])
    assert np.array_equal(dst.positions(n - 1, 1)[0], src.positions(n_src - 1, 1)[0]) and np.array_equal(dst.pin_counts(5, 1), src.pin_counts(0, 1))
    small, _ = zip(*[timer(lambda: dst.fork_from(src, idx[:fan])) for _ in range(reps)])      # what a call costs before it moves anything
    a, b = dst.device_alloc(n * per), dst.device_alloc(n * per)
    copy = lambda: (hip.hipMemcpyAsync(C.c_void_p(b), C.c_void_p(a), n * per, 3, C.c_void_p(dst.stream)), hip.hipStreamSynchronize(C.c_void_p(dst.stream)))
    copy()
    mdev, mwall = zip(*[timer(copy) for _ in range(reps)])
    dst.device_free(a); dst.device_free(b)
    say("1. fork bandwidth: %d -> %d cloths (25x25, fp32), %d bytes per cloth, %.1f MB read + written per fork" % (n_src, n, per, moved / 1e6))
    say("   clothhip_fork, HIP events around the call (index upload + kernel): %s" % stats(dev))
    say("   clothhip_fork, host clock around the call (it synchronises):       %s" % stats(wall))
    say("   the same call for %d cloths (the call's fixed cost: index upload, launch, synchronise): %s" % (fan, stats(small)))
    fb, mb = moved / np.median(dev), moved / np.median(mdev)
    say("   -> %.2f TB/s read + written = %.0f %% of the 8 TB/s HBM peak (the 512 sources are 8 MB: re-read from cache, so the bound is the 134 MB written)" % (fb / 1e12, 100 * fb / HBM_PEAK))
    say("   hipMemcpyAsync device-to-device of the same %d bytes, same run:    %s" % (n * per, stats(mdev)))
    say("   -> %.2f TB/s read + written; fork / memcpy bandwidth = %.2f" % (mb / 1e12, fb / mb))
    # 2. the host route
    def host_route():
        pos, prev, pin = src.get_state()
        tear = src.tear
        dst.set_state(np.repeat(pos, fan, axis=0), np.repeat(prev, fan, axis=0), np.repeat(pin, fan, axis=0))
        dst.tear = np.repeat(tear, fan)
    host_route()
    hw = []
    for _ in range(3):
        t0 = time.perf_counter(); host_route(); hw.append(time.perf_counter() - t0)
    assert np.array_equal(dst.positions(n - 1, 1)[0], src.positions(n_src - 1, 1)[0])
    say("2. the same replication through the host (get_state, set_state, tear flags; host clock): %s" % stats(hw))
    say("   -> the fork is %.0f x faster than the host round trip it replaces (medians, host clock both: %.3f ms vs %.1f ms)"
        % (np.median(hw) / np.median(wall), np.median(wall) * 1e3, np.median(hw) * 1e3))
    src.close(); dst.close()
    return np.median(hw) / np.median(wall), fb / mb


HOST_ARRAYS = ClothVecEnv._SNAP_ARRAYS


def lookahead_cost(E=512, K=16):
    cfg = bench.bench_cfg(25, 0.02)
    cand = np.random.RandomState(1).uniform(-1, 1, size=(E, K, 4))
    for prec in ("f64", "f32"):
        env = ClothVecEnv(cfg, n_envs=E, precision=prec, consume_domrand_draws=False)
        env.seed(1000); env.reset()
        env.step(np.random.RandomState(2).uniform(-0.5, 0.5, size=(E, 4)))
        out = env.lookahead(cand)                                            # creates the scratch batch, warms its kernels
        lt = []
        for _ in range(3):
            t0 = time.perf_counter(); out = env.lookahead(cand); lt.append(time.perf_counter() - t0)
        v = env._scratch.last_variant()
        sub = int(out["executed"].sum())
        say("3. lookahead E = %d, K = %d, %s: %s; %d substeps -> %.1f M cloth-substeps/s end to end" %
            (E, K, prec, stats(lt, "s", 1.0), sub, sub / np.median(lt) / 1e6))
        say("   scratch batch of %d cloths ran %s%s" % (E * K, v["name"], "" if v["dispatches"] == 1 else " in %d dispatches" % v["dispatches"]))
        if prec == "f64":
            # the only way without the fork: K rounds of upload the state, step, read the results, on the env's own 512-cloth handle
            pos, prev, pin = env.batch.get_state()
            tear = env.batch.tear
            host = {k: np.array(getattr(env, k), copy=True) for k in HOST_ARRAYS}
            rew = np.zeros((E, K)); done = np.zeros((E, K), dtype=bool); cov = np.zeros((E, K))
            t0 = time.perf_counter()
            for k in range(K):
                env.batch.set_state(pos, prev, pin, keep_tear=True)
                env.batch.tear = tear
                for name in HOST_ARRAYS:
                    setattr(env, name, host[name].copy())
                _, rew[:, k], done[:, k], info = env.step(cand[:, k])
                cov[:, k] = info["actual_coverage"]
            seq = time.perf_counter() - t0
            same = np.array_equal(rew, out["rew"]) and np.array_equal(done, out["done"]) and np.array_equal(cov, out["actual_coverage"])
            say("   %d sequential rounds of set_state + step on the %d-cloth handle (%s): %.3f s, results identical to the lookahead's: %s" %
                (K, E, env.batch.last_variant()["name"], seq, same))
            say("   -> lookahead / sequential = %.2f x" % (seq / np.median(lt)))
            assert same
        env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fork_lookahead.txt"))
    ap.add_argument("--bench", action="append", default=[], metavar="LABEL=FILE")
    ap.add_argument("--skip-lookahead", action="store_true")
    a = ap.parse_args()
    say("tools/fork_bench.py -- clothhip_fork and ClothVecEnv.lookahead, measured on %s" % time.strftime("%Y-%m-%d"))
    factor, rel = fork_bandwidth()
    if not a.skip_lookahead:
        lookahead_cost()
    if a.bench:
        say("4. bench.py --gpus 1, headline value and variant of each run:")
        for item in a.bench:
            label, path = item.split("=", 1)
            with open(path) as fh:
                rec = [json.loads(l) for l in fh if l.lstrip().startswith("{")][-1]
            say("   %-10s value %.4g %s   %s" % (label, rec["value"], rec.get("unit", ""), rec.get("config", {}).get("variant", "")))
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    if factor <= 1.0:
        sys.exit("the fork is not faster than the host round trip: a finding to explain")


if __name__ == "__main__":
    main()
