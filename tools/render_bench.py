#!/usr/bin/env python3
"""What image observations for every slot of an episode launch cost, measured: figures for DESIGN.md, written to
profiles/render_slots.txt.

Workload: 512 envs x 12 slots of one step_many(policy='oracle_corner') launch (25x25, fp32), RGBD 224 x 224: 6 144 images.
  (a) clothhip_render_obs on the launch's resident observation table (CLOTHHIP_OBS_SLOTS): device time of its kernels (HIP events
      around a call that renders into a device buffer, no download) and the host clock around the call that fills a host buffer.
      Repeated for each band plan: one workgroup per band / one workgroup walking all bands of an image, and LDS budgets of
      160 / 80 / 40 KiB per workgroup (CLOTHHIP_DEBUG_RENDER_WALK, CLOTHHIP_DEBUG_RENDER_LDS; read when the handle is created).
  (b) the route a caller had before: per slot, set_state of the slot's observations into a 512-cloth batch, then
      image_obs(rgbd=True) (clothhip_render, 7 bytes per pixel to the host, depth normalisation and packing in numpy).
  (c) clothhip_render alone on the same states (host clock around the call: its z-buffer hipMalloc, kernel, 7 B per pixel download);
      its kernel alone comes from a kernel trace of `--trace` (rocprofv3 --kernel-trace --stats -- python3 tools/render_bench.py --trace),
      a run of its own.
Every timed call is warmed up once and repeated; median and min .. max are printed. The images of (a) and (b) are compared.
    python3 tools/render_bench.py [--out profiles/render_slots.txt] [--envs 512] [--slots 12] [--size 224] [--trace]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd import _lib                        # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv            # noqa: E402
from tools.fork_bench import EventTimer, hip_runtime  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def stats(v, unit="ms", scale=1e3):
    v = np.asarray(v) * scale
    return "median %.2f %s (min %.2f .. max %.2f, n = %d)" % (np.median(v), unit, v.min(), v.max(), len(v))


def launch(E, T, knobs):
    """A seeded env after one oracle-corner launch of T slots with the observation tables resident; knobs: CLOTHHIP_DEBUG_* for its handle."""
    for k in ("CLOTHHIP_DEBUG_RENDER_WALK", "CLOTHHIP_DEBUG_RENDER_LDS"):
        os.environ.pop(k, None)
    os.environ.update(knobs)
    env = ClothVecEnv(bench.bench_cfg(25, 0.02), n_envs=E, precision="f32", consume_domrand_draws=False)
    env.seed(1000); env.reset()
    out = env.step_many(policy="oracle_corner", n_actions=T, want_obs=True)
    return env, out


def plan_of(env, size):
    o = np.zeros(4, dtype=np.int32)
    _lib.check(_lib.load().clothhip_selftest_render_plan(C.byref(env.batch.params), size, size, _lib.i32p(o)))
    return o.tolist()


def raw_call(env, p, n, out, d_out):
    _lib.check(_lib.load().clothhip_render_obs(env.batch.handle, C.byref(p), _lib.OBS_SLOTS, None, n, None, None, _lib.IMG_RGBD,
                                               _lib.u8p(out), None if d_out is None else C.c_void_p(d_out)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_slots.txt"))
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="only a few kernel launches of (a) and (c), for a kernel trace")
    a = ap.parse_args()
    E, T, S, n = a.envs, a.slots, a.size, a.envs * a.slots
    hip = hip_runtime()
    say("tools/render_bench.py -- %d envs x %d slots, RGBD %d x %d = %d images, %.1f MB finished (%s)" %
        (E, T, S, S, n, n * S * S * 4 / 1e6, time.strftime("%Y-%m-%d")))
    plans = [("one workgroup per band, 160 KiB", {}),
             ("one workgroup per image walks its bands, 160 KiB", {"CLOTHHIP_DEBUG_RENDER_WALK": "1"}),
             ("one workgroup per band, 80 KiB", {"CLOTHHIP_DEBUG_RENDER_LDS": "80"}),
             ("one workgroup per band, 40 KiB", {"CLOTHHIP_DEBUG_RENDER_LDS": "40"})]
    if a.trace:
        plans = plans[:1]
    host = np.zeros((n, S, S, 4), dtype=np.uint8)             # touched once: page faults are not the call's
    first = None
    for label, knobs in plans:
        env, out = launch(E, T, knobs)
        p = env.batch.render_params(width=S, height=S)
        rows, bands, lds, _ = plan_of(env, S)
        d_out = env.batch.device_alloc(n * S * S * 4)
        timer = EventTimer(hip, env.batch.stream)
        raw_call(env, p, n, None, d_out)
        dev, _ = zip(*[timer(lambda: raw_call(env, p, n, None, d_out)) for _ in range(3 if a.trace else a.reps)])
        env.batch.device_free(d_out)
        say("(a) %s: %d bands of %d rows, %d B of LDS per workgroup" % (label, bands, rows, lds))
        say("    kernels (HIP events, rendering into a device buffer): %s -> %.0f images/s" % (stats(dev), n / np.median(dev)))
        if not a.trace:
            raw_call(env, p, n, host, None)
            wall = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); raw_call(env, p, n, host, None); wall.append(time.perf_counter() - t0)
            say("    call filling a host buffer (host clock, 4 B per pixel down): %s -> %.0f images/s" % (stats(wall), n / np.median(wall)))
            say("    device scratch of the call: %.1f MB (one chunk of 256 images: finished images + raw depth), whatever n is" %
                (256 * S * S * 8 / 1e6))
            if first is None:
                first = (host.copy(), np.median(wall), np.median(dev), out["obs_t"].copy())
            else:
                assert np.array_equal(host, first[0]), "band plans must give the same images"
        elif first is None:
            first = (None, None, np.median(dev), out["obs_t"].copy())
        env.close()
    for k in ("CLOTHHIP_DEBUG_RENDER_WALK", "CLOTHHIP_DEBUG_RENDER_LDS"):
        os.environ.pop(k, None)
    # (b), (c): a 512-cloth env as the staging batch
    obs_t = first[3]
    st = ClothVecEnv(bench.bench_cfg(25, 0.02), n_envs=E, precision="f32", consume_domrand_draws=False)
    pin = np.zeros((E, st.P), dtype=np.uint8)

    def slot(t):
        pos = obs_t[t].reshape(E, st.P, 3)
        st.batch.set_state(pos, pos, pin)
        return st.image_obs(rgbd=True, width=S, height=S)

    if not a.trace:
        got = np.stack([slot(t) for t in range(T)])
        assert np.array_equal(got.reshape(first[0].shape), first[0]), "(a) and (b) must give the same images"
        wall_b = []
        for _ in range(3):
            t0 = time.perf_counter()
            for t in range(T):
                slot(t)
            wall_b.append(time.perf_counter() - t0)
        say("(b) per slot set_state + image_obs(rgbd=True), %d slots (host clock): %s -> %.0f images/s" % (T, stats(wall_b), n / np.median(wall_b)))
        say("    images identical to (a)'s: True")
        say("    -> (a) call / (b) = %.2f x faster per image" % (np.median(wall_b) / first[1]))
    slot(0)
    wall_c = []
    for _ in range(3 if a.trace else a.reps):
        t0 = time.perf_counter(); st.batch.render(width=S, height=S); wall_c.append(time.perf_counter() - t0)
    say("(c) clothhip_render of %d cloths, one call (host clock: hipMalloc of the z-buffer, kernel, 7 B per pixel down): %s -> %.0f images/s" %
        (E, stats(wall_c), E / np.median(wall_c)))
    say("    its scratch: %.1f MB for %d images (8 B per pixel per image; %.2f GB for %d)" % (E * S * S * 8 / 1e6, E, n * S * S * 8 / 1e9, n))
    st.close()
    if not a.trace:
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
