"""Exact-rational reference of the per-env metrics (gym_cloth_amd/csrc/cloth_metrics.hpp: metrics_block; the host's clothhip_hull_area).

TEST INFRASTRUCTURE, NOT PRODUCT CODE (only tests/ import it). It takes the float64 positions a handle holds (read back, so the
rounding to the handle's precision is part of the input) and computes with fractions.Fraction what ClothEnv computes with
scipy / Qhull and numpy (cloth_env.py:603-609, :620-640, :1020-1098): a double IS a rational number, so nothing below rounds
until the caller converts a result.

  coverage      area of the convex hull of the distinct points clip(xy, 0, 1): Andrew's monotone chain with exact cross
                products (collinear points dropped), then the shoelace sum; 0 for fewer than three distinct points or an
                all-collinear set. `k` is the hull's vertex count.
  variance_inv  from the exact population variance of z: 1000 if var < 1e-6 (the double 0.000001, as the env compares), else 0.001 / var
  out_of_bounds max x >= 1.25, min x < -0.25, the same on y, max z >= 1, min z < 0        (cloth_env.py:1031-1036)
  n_below       #(z < thickness / 2), the division done in double as the env does it     (cloth_env.py:604)
"""
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

Exact = namedtuple("Exact", "area k hull var variance_inv oob n_below n_distinct")

_VAR_MIN = Fraction(0.000001)       # the double the env compares with
_VINV_NUM = Fraction(0.001)         # ... and divides


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(points):
    """Andrew's monotone chain over an iterable of (Fraction, Fraction) -- or of any exact number type: the hull's vertices,
    counter-clockwise, collinear points dropped. Fewer than three vertices: the set is degenerate (a point, a segment)."""
    p = sorted(set(points))
    if len(p) < 3:
        return p
    lo = []
    for q in p:
        while len(lo) >= 2 and _cross(lo[-2], lo[-1], q) <= 0:
            lo.pop()
        lo.append(q)
    up = []
    for q in reversed(p):
        while len(up) >= 2 and _cross(up[-2], up[-1], q) <= 0:
            up.pop()
        up.append(q)
    return lo[:-1] + up[:-1]


def shoelace(h):
    """Exact area of the polygon h (list of (Fraction, Fraction))."""
    if len(h) < 3:
        return Fraction(0)
    s = Fraction(0)
    for i in range(len(h)):
        a, b = h[i], h[(i + 1) % len(h)]
        s += a[0] * b[1] - b[0] * a[1]
    return abs(s) / 2


def _scaled_ints(values):
    """The doubles `values` as integers over one power of two: (ints, shift) with values[i] == ints[i] / 2**shift exactly. Integer
    arithmetic on them is the same exact arithmetic as on Fractions, much faster."""
    ratios = [float(v).as_integer_ratio() for v in values]
    shift = max([d.bit_length() - 1 for _, d in ratios] + [0])
    return [n * ((1 << shift) // d) for n, d in ratios], shift


def clipped_points(pos):
    """[(Fraction x, Fraction y)] of np.clip(pos[:, :2], 0, 1), one per particle (duplicates kept)."""
    pts, shift = _clipped_ints(pos)
    return [(Fraction(x, 1 << shift), Fraction(y, 1 << shift)) for x, y in pts]


def _clipped_ints(pos):
    xy = np.clip(np.asarray(pos, dtype=np.float64)[:, :2], 0.0, 1.0)
    v, shift = _scaled_ints(xy.reshape(-1))
    return list(zip(v[0::2], v[1::2])), shift


def variance(z):
    """Exact population variance (np.var) of the doubles z."""
    zs, shift = _scaled_ints(np.asarray(z, dtype=np.float64))
    n = len(zs)
    s = sum(zs)
    s2 = sum(v * v for v in zs)
    return Fraction(s2 * n - s * s, n * n << (2 * shift))


def out_of_bounds(pos):
    pos = np.asarray(pos, dtype=np.float64)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    return bool(x.max() >= 1.25 or x.min() < -0.25 or y.max() >= 1.25 or y.min() < -0.25 or z.max() >= 1.0 or z.min() < 0.0)


# States that differ in z alone share their hull, states that differ in xy alone their variance: each is computed once per session.
@functools.lru_cache(maxsize=512)
def _hull_cached(xy_bytes):
    pts, shift = _clipped_ints(np.frombuffer(xy_bytes, dtype=np.float64).reshape(-1, 2))
    return [(Fraction(x, 1 << shift), Fraction(y, 1 << shift)) for x, y in hull(pts)], len(set(pts))


@functools.lru_cache(maxsize=512)
def _variance_cached(z_bytes):
    return variance(np.frombuffer(z_bytes, dtype=np.float64))


def metrics(pos, thickness):
    """pos float64 [P, 3], thickness: the cfg's double. -> Exact(area, k, hull, var, variance_inv: Fractions / int; oob bool;
    n_below int; n_distinct: distinct clipped points)."""
    pos = np.asarray(pos, dtype=np.float64)
    assert pos.ndim == 2 and pos.shape[1] == 3 and np.isfinite(pos).all()
    h, n_distinct = _hull_cached(np.ascontiguousarray(pos[:, :2]).tobytes())
    k = len(h) if len(h) >= 3 else 0
    var = _variance_cached(np.ascontiguousarray(pos[:, 2]).tobytes())
    vinv = Fraction(1000) if var < _VAR_MIN else _VINV_NUM / var
    half = float(thickness) / 2.0
    return Exact(shoelace(h), k, h, var, vinv, out_of_bounds(pos), int((pos[:, 2] < half).sum()), n_distinct)


def coverage_bound(k):
    """|coverage - exact| allowed for a hull of k vertices: k shoelace terms of four roundings each on magnitudes <= 1, k accumulations
    of partial sums <= 2, halved, with slack for a vertex whose cross product is below rounding."""
    return 8.0 * (k + 1) * 2.0 ** -53


def variance_inv_rel_bound(P):
    """Relative error allowed on variance_inv where var >= 1e-6: a two-pass sum over P values (the mean's error enters at second order)."""
    return 4.0 * P * 2.0 ** -53
