"""Hand-made cloth states for the metrics tests (test_metrics_exact_host.py, test_gpu_metrics_exact.py) and the cached exact reference.

A state is a MetricsState(name, pos float64 [P, 3], flags). `held(pos, prec)` is what a handle of that precision holds after
set_state (fp32: round to nearest) -- the CPU tests use it where the GPU tests read positions() back."""
import functools
from collections import namedtuple

import numpy as np

from oracle import metrics_exact

# stand-alone grids of the issue: (n_side, precision)
GRIDS = [(3, "f64"), (12, "f32"), (16, "f32"), (16, "f64"), (25, "f32"), (25, "f64"), (33, "f64"), (50, "f64"), (64, "f32")]

# dyadic: every clipped coordinate is a multiple of 2^-10 at most 1, so the double chain and shoelace are exact: coverage == float(exact).
# zero_area: collinear / too few distinct points by construction (the chain's cross products are exactly 0): coverage == 0.0.
MetricsState = namedtuple("MetricsState", "name pos dyadic zero_area")


def thickness_of(prec):
    """The stand-alone handles' cloth thickness: 0.02 (thickness / 2 is no fp32 number) for fp64; 2^-5 for fp32, so that a fp32 z can EQUAL
    thickness / 2 and the strict < of the height count is met on its boundary in both precisions."""
    return 0.02 if prec == "f64" else 0.03125


def ftype(prec):
    return np.float64 if prec == "f64" else np.float32


def held(pos, prec):
    return np.asarray(pos, dtype=np.float64).astype(ftype(prec)).astype(np.float64)


def _base(P):
    """In bounds, in general position, inside (0.25, 0.75)^2 x (0.125, 0.375): the state the one-particle threshold cases start from."""
    i = np.arange(P, dtype=np.float64)
    pos = np.empty((P, 3))
    pos[:, 0] = 0.25 + 0.5 * ((i * 7919.0) % P + 0.37) / P
    pos[:, 1] = 0.25 + 0.5 * ((i * 104729.0) % P + 0.61) / P
    pos[:, 2] = 0.125 + 0.25 * ((i * 31.0) % P) / P
    return pos


def _orders(name, pos):
    """The same particles in ascending, descending and shuffled order (whole rows move: coverage must not notice)."""
    perm = np.random.RandomState(5).permutation(len(pos))
    return [(name + "_asc", pos), (name + "_desc", pos[::-1].copy()), (name + "_shuf", pos[perm].copy())]


def states(n_side, prec):
    """Every hand-made state of one (grid, precision), in a fixed order."""
    P = n_side * n_side
    ft = ftype(prec)
    half = ft(thickness_of(prec) / 2.0)               # thickness / 2 as the handle holds it
    i = np.arange(P, dtype=np.float64)
    base = _base(P)
    out = []

    def add(name, pos, dyadic=False, zero_area=False):
        assert pos.shape == (P, 3)
        out.append(MetricsState(name, np.ascontiguousarray(pos, dtype=np.float64), dyadic, zero_area))

    def with_xy(x, y, **kw):
        p = base.copy()
        p[:, 0], p[:, 1] = x, y
        return p

    # the deep hull stack: every particle a hull vertex
    th = 2.0 * np.pi * i / P
    for name, p in _orders("circle", with_xy(0.5 + 0.45 * np.cos(th), 0.5 + 0.45 * np.sin(th))):
        add(name, p)
    # dyadic lattice: borders exactly collinear
    s = min(n_side, 33)
    add("lattice", with_xy((i % s) / 32.0, ((i // s) % s) / 32.0), dyadic=True)
    # degenerate hulls
    add("all_equal", with_xy(0.3, 0.6), zero_area=True)
    add("two_values", with_xy(np.where(i % 2 == 0, 0.25, 0.75), np.where(i % 2 == 0, 0.25, 0.5)), dyadic=True, zero_area=True)
    tri = np.array([[0.125, 0.125], [0.875, 0.25], [0.5, 0.75]])
    add("triangle", with_xy(tri[(i % 3).astype(int), 0], tri[(i % 3).astype(int), 1]), dyadic=True)
    d = (i + 1.0) / (P + 1.0)
    add("diagonal", with_xy(d, d), zero_area=True)
    add("vertical", with_xy(0.4, d), zero_area=True)
    add("beyond_x", with_xy(1.05 + 0.15 * ((i * 7919.0) % P) / P, 0.1 + 0.8 * ((i * 104729.0) % P) / P), zero_area=True)
    # a disc that crosses the clip edges x = 1 and y = 0 (sunflower filling; the last two particles beyond the corner -> both clip to (1, 0))
    r, ga = 0.3 * np.sqrt((i + 0.5) / P), i * (np.pi * (3.0 - np.sqrt(5.0)))
    disc = with_xy(0.9 + r * np.cos(ga), 0.15 + r * np.sin(ga))
    disc[P - 2, :2], disc[P - 1, :2] = (1.1, -0.1), (1.15, -0.05)
    for name, p in _orders("disc", disc):
        add(name, p)
    # signed zeros
    nz = base.copy()
    nz[0::5, 0], nz[1::5, 1], nz[2::5, 2] = -0.0, -0.0, -0.0
    nz[3::5, 0], nz[3::5, 2] = 0.0, 0.0
    add("neg_zero", nz)
    # out-of-bounds thresholds in x and y, one particle moved
    hi, lo = ft(1.25), ft(-0.25)
    for tag, v in (("hi", hi), ("hi_prev", np.nextafter(hi, ft(0))), ("lo", lo), ("lo_next", np.nextafter(lo, ft(-1)))):
        for ax in (0, 1):
            p = base.copy()
            p[P // 2, ax] = float(v)
            add("oob_%s_%s" % ("xy"[ax], tag), p)
    # z thresholds
    fi = np.finfo(ft)
    for tag, v in (("one", ft(1.0)), ("one_prev", np.nextafter(ft(1), ft(0))), ("neg_zero", ft(-0.0)), ("neg_normal", -fi.tiny),
                   ("neg_subnormal", -np.nextafter(ft(0), ft(1)))):
        p = base.copy()
        p[P // 3, 2] = float(v)
        add("z_" + tag, p)
    # variance on both sides of 1e-6, never near it
    for tag, z in (("flat", np.full(P, 0.25)), ("small", np.where(i % 2 == 0, 5e-4, -5e-4)), ("large", np.where(i % 2 == 0, 2e-3, -2e-3))):
        p = base.copy()
        p[:, 2] = z
        add("var_" + tag, p)
    # the height count on its boundary: z == thickness / 2 as held, its two neighbours, and values well off
    zs = np.array([float(half), float(np.nextafter(half, ft(0))), float(np.nextafter(half, ft(1))), 0.0, 0.5])
    p = base.copy()
    p[:, 2] = zs[(i % 5).astype(int)]
    add("height", p)
    return out


@functools.lru_cache(maxsize=None)
def _exact_cached(key, P, thickness):
    pos = np.frombuffer(key, dtype=np.float64).reshape(P, 3)
    return metrics_exact.metrics(pos, thickness)


def exact(pos, thickness):
    """oracle.metrics_exact.metrics, computed once per distinct state of a session."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    return _exact_cached(pos.tobytes(), pos.shape[0], float(thickness))


def host_hull_area(pos):
    """clothhip_hull_area on the clipped xy of pos, as test_device_metrics_match_reference feeds it."""
    from gym_cloth_amd import _lib
    xy = np.ascontiguousarray(np.clip(np.asarray(pos, dtype=np.float64)[:, :2], 0, 1))
    return _lib.load().clothhip_hull_area(_lib.dp(xy), len(xy))


def min_disc_vertices(P):
    """The clipped disc must put at least 8 vertices on the hull; the 3x3 grid has 9 particles, two of them the duplicate pair, so 4 there."""
    return 8 if P >= 16 else 4


def check_non_vacuity(st, pos, ex, prec):
    """What a state must BE for its case to mean something, asserted on the positions the handle holds (pos) and their exact reference (ex)."""
    P = len(pos)
    name = st.name
    lo, hi = 0.999e-6, 1.001e-6
    assert not (lo <= ex.var <= hi), (name, float(ex.var))                          # the variance branch is never a coin toss
    if name.startswith("circle"):
        assert ex.k == P == ex.n_distinct, (name, ex.k)
    if name == "lattice":
        s = min(int(round(P ** 0.5)), 33)
        assert ex.k == 4 and ex.n_distinct == s * s and ex.area == ((s - 1) / 32.0) ** 2, (name, ex.k, ex.n_distinct)
    if st.zero_area:
        assert ex.area == 0 and ex.k == 0, (name, ex.area)
    if name == "all_equal":
        assert ex.n_distinct == 1
    if name == "two_values":
        assert ex.n_distinct == 2
    if name == "triangle":
        assert ex.n_distinct == 3 and ex.k == 3 and ex.area > 0
    if name in ("diagonal", "vertical", "beyond_x"):
        assert ex.n_distinct >= min(P, 9) - 1, (name, ex.n_distinct)
    if name == "beyond_x":
        assert pos[:, 0].min() > 1.0 and pos[:, 0].max() < 1.25 and not ex.oob
    if name.startswith("disc"):
        assert ex.k >= min_disc_vertices(P), (name, ex.k)
        assert any(x == 1 for x, y in ex.hull) and any(y == 0 for x, y in ex.hull), name      # a hull vertex on each of the two clip edges
        assert ex.n_distinct < P, name                                                        # a duplicate pair after clipping
        assert pos[:, 0].max() > 1.0 and pos[:, 1].min() < 0.0
    if name == "neg_zero":
        for ax in range(3):
            assert (np.signbit(pos[:, ax]) & (pos[:, ax] == 0)).any(), (name, ax)
        assert not ex.oob
    if name.startswith("oob_"):
        _, axis, tag = name.split("_", 2)
        v = pos[P // 2, "xy".index(axis)]
        ft = ftype(prec)
        want = {"hi": 1.25, "hi_prev": float(np.nextafter(ft(1.25), ft(0))), "lo": -0.25, "lo_next": float(np.nextafter(ft(-0.25), ft(-1)))}[tag]
        assert v == want and ex.oob == (tag in ("hi", "lo_next")), (name, v, ex.oob)
    if name.startswith("z_"):
        v = pos[P // 3, 2]
        tag = name[2:]
        fi = np.finfo(ftype(prec))
        want = {"one": 1.0, "one_prev": float(np.nextafter(ftype(prec)(1), ftype(prec)(0))), "neg_zero": -0.0, "neg_normal": -float(fi.tiny),
                "neg_subnormal": -float(np.nextafter(ftype(prec)(0), ftype(prec)(1)))}[tag]
        assert v == want and np.signbit(v) == np.signbit(want), (name, v, want)
        assert ex.oob == (tag in ("one", "neg_normal", "neg_subnormal")), (name, ex.oob)
    if name == "var_flat":
        assert ex.var == 0 and ex.variance_inv == 1000
    if name == "var_small":
        assert ex.var < 1e-6 / 2 and ex.variance_inv == 1000
    if name == "var_large":
        want = 250.0 / (1.0 - (P % 2) / float(P * P))       # z = +-a: var = a^2 for even P, a^2 (1 - 1 / P^2) for odd P (the mean is a / P)
        assert abs(float(ex.variance_inv) - want) < 1e-6 * want and ex.var > 2e-6, (name, float(ex.variance_inv))
    if name == "height":
        half = ftype(prec)(thickness_of(prec) / 2.0)
        z = pos[:, 2]
        for v in (float(half), float(np.nextafter(half, ftype(prec)(0))), float(np.nextafter(half, ftype(prec)(1)))):
            assert (z == v).any(), (name, v)
        assert 0 < ex.n_below < P
        if P >= 5:          # the count is decided by the strict <: the particles AT thickness / 2 as held are not all on one side by accident
            below = float(half) < thickness_of(prec) / 2.0
            assert ex.n_below == int((z == 0.0).sum() + (z == float(np.nextafter(half, ftype(prec)(0)))).sum() + (below * (z == float(half))).sum())
