"""Exact reference of the gripper and of the action decode: Gripper.grab_top / grab (gripper.pyx:23-53), the force_grab radius loop
(cloth_env.py:434-444) and the action -> schedule arithmetic (cloth_env.py:396-475), as the device states them twice -- k_grab
(gym_cloth_amd/csrc/cloth_state_kernels.hpp) and the episode launch's own grab and decode (csrc/episode_plan.inc.hpp).

TEST INFRASTRUCTURE, NOT PRODUCT CODE (only tests/ import it). numpy and fractions only.

The library is built with -ffp-contract=off, so every operation of both grabs is ONE rounding in the handle's type T (float64 or
float32), and what a grab must select is a restatement, not a bound. With p the positions the handle holds (exact in T):

  gx = T(x), gy = T(y)                                  the gripper's xy arrives as doubles and is cast once
  dx = p.x - gx, dy = p.y - gy                          one rounding each
  in the cylinder:  dx * dx + dy * dy < T(radius)       three roundings; the radius is NOT squared (gripper.pyx:35)
  in a band:        |p.z - T(level)| < T(2 * thickness) 2 * thickness formed in double, cast once; the level cast per use
  levels            curZ = height; while curZ > 0: ...; curZ -= thickness, accumulated in double (gripper.pyx:31-41)
  grab_top          the first level from the top at which any in-cylinder point lies in the band; then every in-cylinder point
                    in THAT level's band
  force_grab        radius = grip_radius; while nothing is grabbed: radius += radius_inc (in double), cast to T per try

`classify` is an independent statement of the two tests in exact rational arithmetic on the real numbers the casts produce: it says
for every particle inside / outside / exactly ON each boundary. Where T arithmetic is exact (dyadic states) the two must agree --
the restatement must not share a misreading with the kernel -- and it proves that a state does put a particle on a boundary.

`decode` is the action decode in double in the reference's own order, with the clip as Python's builtin min / max evaluate it: a
NaN component stays a NaN (min(nan, high) is nan: `high < nan` is False), so a NaN delta makes the iters_pull loop endless -- the
'does not terminate' verdict, which the device's 200 000-step guard and the host's FloatingPointError report.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

CNT_GRAB_MASK = 0x7F            # the pin byte's grab multiplicity saturates here (csrc/cloth_common.hpp)
EPS = 1e-5                      # cloth_env.py:48
PULL_GUARD = 200000             # the device decode's guard on the iters_pull loop


def ftype(prec):
    return np.float64 if prec == "f64" else np.float32


def levels(height, thickness):
    """The curZ table (gripper.pyx:31-41), accumulated in double."""
    lv = []
    z = float(height)
    if not thickness > 0:
        return np.zeros(0)
    while z > 0 and len(lv) < 100000:
        lv.append(z)
        z -= float(thickness)
    return np.array(lv, dtype=np.float64)


def dist2(pos_held, xy, prec):
    """dx * dx + dy * dy of every particle in T, operation by operation."""
    ft = ftype(prec)
    p = np.asarray(pos_held, dtype=np.float64).astype(ft)
    gx, gy = ft(xy[0]), ft(xy[1])
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = p[:, 0] - gx, p[:, 1] - gy
        return dx * dx + dy * dy


def band_dist(pos_held, lv, prec):
    """|z - T(level)| of every particle and level in T, [P, n_levels]."""
    ft = ftype(prec)
    z = np.asarray(pos_held, dtype=np.float64).astype(ft)[:, 2]
    with np.errstate(invalid="ignore"):
        return np.abs(z[:, None] - np.asarray(lv, dtype=np.float64).astype(ft)[None, :])


def grab(pos_held, xy, radius, prec):
    """Gripper.grab (gripper.pyx:44-53): the sorted indices of the particles in the cylinder."""
    with np.errstate(invalid="ignore"):
        return np.nonzero(dist2(pos_held, xy, prec) < ftype(prec)(radius))[0]


def grab_top(pos_held, xy, radius, lv, thickness, prec):
    """Gripper.grab_top (gripper.pyx:23-42): (sorted indices, index of the chosen level or None)."""
    ft = ftype(prec)
    with np.errstate(invalid="ignore"):
        inc = dist2(pos_held, xy, prec) < ft(radius)
        hit = (band_dist(pos_held, lv, prec) < ft(2 * float(thickness))) & inc[:, None]
    at = np.nonzero(hit.any(axis=0))[0]
    if not len(at):
        return np.zeros(0, dtype=np.int64), None
    return np.nonzero(hit[:, at[0]])[0], int(at[0])


def force_grab(pos_held, xy, lv, thickness, radius0, inc, prec, max_tries=10000):
    """grab_top with the force_grab loop (cloth_env.py:434-444): the radius grows in double and is cast to T per try.
    -> (indices, level, tries: 0 = the first grab_top took something, the radius of the last try as a double)."""
    radius = float(radius0)
    tries = 0
    while True:
        idx, lev = grab_top(pos_held, xy, radius, lv, thickness, prec)
        if len(idx) or tries >= max_tries:
            return idx, lev, tries, radius
        radius += float(inc)
        tries += 1


# ---- the independent classification ---------------------------------------------------------------------------------------------
Classes = namedtuple("Classes", "cyl band")      # cyl[P], band[P, n_levels]: -1 inside, 0 exactly on the boundary, +1 outside


def _sign(q):
    return (q > 0) - (q < 0)


def classify(pos_held, xy, radius, lv, thickness, prec):
    """Every particle against both boundaries in exact rational arithmetic, on the numbers the device compares: the held positions,
    T(x), T(y), T(radius), T(level), T(2 * thickness). No rounding inside: sign(dx^2 + dy^2 - radius), sign(|z - level| - 2 thickness)."""
    ft = ftype(prec)
    F = lambda v: Fraction(float(ft(v)))
    p = np.asarray(pos_held, dtype=np.float64)
    gx, gy, rad, tt = F(xy[0]), F(xy[1]), F(radius), F(2 * float(thickness))
    lvq = [F(v) for v in lv]
    cyl = np.empty(len(p), dtype=np.int64)
    band = np.empty((len(p), len(lvq)), dtype=np.int64)
    seen_xy, seen_z = {}, {}                               # (a cloth state repeats few distinct values: each is classified once)
    for i in range(len(p)):
        kxy, kz = (p[i, 0], p[i, 1]), p[i, 2]
        if kxy not in seen_xy:
            x, y = F(p[i, 0]), F(p[i, 1])
            seen_xy[kxy] = _sign((x - gx) ** 2 + (y - gy) ** 2 - rad)
        if kz not in seen_z:
            z = F(p[i, 2])
            seen_z[kz] = [_sign(abs(z - q) - tt) for q in lvq]
        cyl[i] = seen_xy[kxy]
        band[i] = seen_z[kz]
    return Classes(cyl, band)


def grab_top_from_classes(c):
    """grab_top read off a classification (strictly inside both): (sorted indices, level or None)."""
    hit = (c.band < 0) & (c.cyl < 0)[:, None]
    at = np.nonzero(hit.any(axis=0))[0]
    if not len(at):
        return np.zeros(0, dtype=np.int64), None
    return np.nonzero(hit[:, at[0]])[0], int(at[0])


# ---- the action decode ----------------------------------------------------------------------------------------------------------
Decoded = namedtuple("Decoded", "x y dx_pull dy_pull total_length step iters_pull bounds terminates")


def _py_clip(x, low, high):
    """max(min(x, high), low) as Python's builtins evaluate it (cloth_env.py:406-409): the first argument stays unless the second is
    strictly beyond it, so a NaN stays a NaN and -0.0 stays -0.0."""
    m = high if high < x else x
    return low if low > m else m


def decode(action, ep):
    """The delta-action decode (cloth_env.py:396-475) in double. ep: a mapping with act_low[4], act_high[4], clip_act_space,
    reduce_factor, iters_up (may be fractional), iters_up_rest, iters_grip_rest, iters_rest. bounds: the ceilings of the five
    cumulative phase boundaries, summed left to right; iters_pull and bounds are None where the loop does not terminate."""
    a = [float(v) for v in action]
    low, high = [float(v) for v in ep["act_low"]], [float(v) for v in ep["act_high"]]
    x, y, c2, c3 = (_py_clip(a[k], low[k], high[k]) for k in range(4))
    if ep["clip_act_space"]:
        x = (x / 2.0) + 0.5
        y = (y / 2.0) + 0.5
    tl = math.sqrt(c2 * c2 + c3 * c3) if not (math.isnan(c2) or math.isnan(c3)) else float("nan")
    xd, yd = c2 / (tl + EPS), c3 / (tl + EPS)
    xr, yr = xd * float(ep["reduce_factor"]), yd * float(ep["reduce_factor"])
    stp = math.sqrt(xr * xr + yr * yr) if not (math.isnan(xr) or math.isnan(yr)) else float("nan")
    cl, ii, ok = 0.0, 0, True
    while True:
        cl = cl + stp
        if cl >= tl:
            break
        ii += 1
        if ii >= PULL_GUARD:
            ok = False
            break
    if not ok:
        return Decoded(x, y, xr, yr, tl, stp, None, None, False)
    iu = float(ep["iters_up"])
    b = (iu, iu + ep["iters_up_rest"], iu + ep["iters_up_rest"] + ii, iu + ep["iters_up_rest"] + ii + ep["iters_grip_rest"],
         iu + ep["iters_up_rest"] + ii + ep["iters_grip_rest"] + ep["iters_rest"])
    return Decoded(x, y, xr, yr, tl, stp, ii, tuple(int(math.ceil(v)) for v in b), True)
