"""Hand-made cloth states for the gripper tests (test_gripper_exact_host.py, test_gpu_gripper_exact.py).

A state is a GripState(name, pos float64 [P, 3], xy, radius, flags...): one env. All particles but a few PROBES are parked well outside the
cylinder (radius R = 2^-8 around the gripper at (0.5, 0.5): the test is dx^2 + dy^2 < radius, so it reaches 2^-4) at z = 0.25; the probes
are placed relative to the gripper and to the level table. `held(pos, prec)` is what a handle of that precision holds after set_state --
the CPU tests use it where the GPU tests read positions() back.

flags: dyadic    every number the two tests see is a dyadic rational with few bits, so T arithmetic is exact: the exact classification
                 (oracle.gripper_exact.classify) and the restatement in T must agree on every particle
       tie       None, or ('cyl', particle) / ('band', particle, level): that particle sits EXACTLY on that boundary
       differs   None, or the name of the sibling state (one ulp or one particle away) whose grab_top set must differ from this one's
       launch    False: for the stand-alone kernel only (another radius than the handle's; thousands of particles packed into a few collision
                 cells, which an episode launch would have to step through)"""
from collections import namedtuple

import numpy as np

from oracle import gripper_exact as ge

# stand-alone grids of the issue: (n_side, precision)
GRIDS = [(3, "f32"), (3, "f64"), (8, "f32"), (9, "f64"), (25, "f32"), (25, "f64"), (33, "f64"), (50, "f32"), (64, "f32")]

GripState = namedtuple("GripState", "name pos xy radius dyadic tie differs launch")

XY = (0.5, 0.5)
R = 2.0 ** -8
HEIGHT = 1.0


def thickness_of(n_side, prec):
    """The stand-alone handles' cloth thickness: the config's 0.02 (the casts of the levels and of 2 * thickness matter) or the dyadic 2^-5
    (a float32 z can sit EXACTLY on a band's edge), both in both precisions over the grids."""
    return {(3, "f32"): 0.03125, (3, "f64"): 0.02, (8, "f32"): 0.02, (9, "f64"): 0.03125, (25, "f32"): 0.03125, (25, "f64"): 0.02,
            (33, "f64"): 0.03125, (50, "f32"): 0.02, (64, "f32"): 0.03125}[(n_side, prec)]


def ftype(prec):
    return ge.ftype(prec)


def held(pos, prec):
    return np.asarray(pos, dtype=np.float64).astype(ftype(prec)).astype(np.float64)


def parked(P):
    """Every particle outside the cylinder of any radius below 0.118 (dx >= 0.34375: beyond the fifth force_grab try from 0.003 in steps of
    0.02), at z = 0.25: the cloth's own grid, squeezed into [0.84375, 0.96875] x [0.0625, 0.9375], so that no two particles coincide and an
    episode launch can step the state."""
    n = int(round(P ** 0.5))
    i = np.arange(P)
    pos = np.empty((P, 3))
    pos[:, 0] = 0.84375 + 0.125 * (i % n) / (n - 1.0)
    pos[:, 1] = 0.0625 + 0.875 * (i // n) / (n - 1.0)
    pos[:, 2] = 0.25
    return pos


def _ulp(v, prec, up):
    ft = ftype(prec)
    return float(np.nextafter(ft(v), ft(np.inf if up else -np.inf)))


def states(n_side, prec, thickness, radius=R):
    """Every hand-made state of one (grid, precision, thickness), in a fixed order. `radius`: the cylinder's radius of all states but
    'everything_r4' (the in-launch tests pass the env's grip_radius: one per handle)."""
    P = n_side * n_side
    ft = ftype(prec)
    t = float(thickness)
    dy_t = t == 2.0 ** -5 and radius == R              # dyadic thickness and radius: levels k / 32, band half-width 2^-4, exact ties exist
    lv = ge.levels(HEIGHT, t)
    lvT = lv.astype(ft).astype(np.float64)             # the levels as the kernel compares them
    tt = float(ft(2 * t))
    j = int(np.argmin(np.abs(lv - 0.5)))               # a level in the middle of the table
    base = parked(P)
    out = []

    def add(name, probes, xy=XY, rad=radius, dyadic=False, tie=None, differs=None, launch=True):
        pos = base.copy()
        for idx, dx, dy, z in probes:
            pos[idx] = (xy[0] + dx, xy[1] + dy, z)
        out.append(GripState(name, pos, xy, rad, dyadic, tie, differs, launch))

    def edge(level, sign):
        """The T number nearest level + sign * T(2 * thickness) that is NOT strictly inside the band while its neighbour towards the level is,
        decided in exact arithmetic (with a dyadic thickness: the edge itself)."""
        from fractions import Fraction
        inside = lambda z: abs(Fraction(z) - Fraction(float(level))) < Fraction(tt)
        z = float(ft(level + sign * tt))
        while inside(z):
            z = _ulp(z, prec, up=sign > 0)
        while not inside(_ulp(z, prec, up=sign < 0)):
            z = _ulp(z, prec, up=sign < 0)
        return z

    last, mid = P - 1, P // 2
    well_in = float(ft(lvT[j] - tt / 4))               # a z well inside level j's band (its first level from the top is j - 1)

    # ---- the cylinder's edge: d2 == radius exactly, one ulp inside, one ulp outside; dx and dy, both signs. Particle `mid` is on the edge,
    # particle 0 sits on the axis and is always taken.
    e = float(np.sqrt(radius))                         # 2^-4 for the default radius
    for ax in (0, 1):
        for sg in (1.0, -1.0):
            on = XY[ax] + sg * e
            tag = "xy"[ax] + ("p" if sg > 0 else "m")
            for kind, c in (("on", on), ("in", _ulp(on, prec, up=sg < 0)), ("out", _ulp(on, prec, up=sg > 0))):
                d = [0.0, 0.0]
                d[ax] = c - XY[ax]
                add("cyl_%s_%s" % (tag, kind), [(0, 0.0, 0.0, well_in), (mid, d[0], d[1], well_in)], dyadic=kind == "on" and radius == R,
                    tie=("cyl", mid) if kind == "on" and radius == R else None, differs="cyl_%s_in" % tag if kind != "in" else None)

    # ---- a band's edge: particle 0 on the axis at z = level j - 2 * thickness as held (exactly on the lower edge where the thickness is
    # dyadic), one ulp to either side; particle `mid` lies in the band of level j + 1 and not of level j, so it tells which level was chosen
    lo_edge = edge(lvT[j], -1)
    below = float(ft(lvT[j + 1] - 1.5 * t))
    for kind, z in (("on", lo_edge), ("in", _ulp(lo_edge, prec, up=True)), ("out", _ulp(lo_edge, prec, up=False))):
        add("band_lo_" + kind, [(0, 0.0, 0.0, z), (mid, 0.0, 2.0 ** -6, below)], dyadic=dy_t, tie=("band", 0, j) if dy_t and kind == "on" else None,
            differs="band_lo_in" if kind != "in" else None)
    # above the top level by less than the band / by the band exactly / beyond it: only level 0 can take it
    hi_edge = edge(lvT[0], +1)
    for kind, z in (("on", hi_edge), ("in", _ulp(hi_edge, prec, up=False)), ("out", _ulp(hi_edge, prec, up=True))):
        add("band_top_" + kind, [(0, 0.0, 0.0, z)], dyadic=dy_t, tie=("band", 0, 0) if dy_t and kind == "on" else None,
            differs="band_top_in" if kind != "in" else None)
    # below the plane: the last level reaches under z = 0 (it is > 0 and the band is 2 * thickness wide)
    n = len(lv) - 1
    z_edge = edge(lvT[n], -1)
    assert z_edge < 0.0
    # (z and the level have opposite signs, so z - level is a sum and ROUNDS: one ulp inside the edge in exact arithmetic is still ON it in T --
    # 'near', where the restatement and not the exact classification says what the kernel does; 'in' is the first z that T calls inside)
    z_in = _ulp(z_edge, prec, up=True)
    while not ft(abs(ft(ft(z_in) - ft(lvT[n])))) < ft(tt):
        z_in = _ulp(z_in, prec, up=True)
    for kind, z in (("on", z_edge), ("near", _ulp(z_edge, prec, up=True)), ("in", z_in), ("out", _ulp(z_edge, prec, up=False))):
        add("band_neg_" + kind, [(0, 0.0, 0.0, z)], dyadic=dy_t and kind != "near", tie=("band", 0, n) if dy_t and kind == "on" else None,
            differs="band_neg_in" if kind in ("on", "out") else None)

    # ---- the level choice
    # a z in the bands of three (on a level) / four (between two) consecutive levels takes the highest: particle `mid` lies in the band of the
    # next level down and not of the highest, and is left alone
    add("levels_three", [(0, 0.0, 0.0, lvT[j]), (mid, 0.0, 2.0 ** -6, float(ft(lvT[j] - 1.5 * t)))], dyadic=dy_t, differs="levels_three_alone")
    add("levels_three_alone", [(mid, 0.0, 2.0 ** -6, float(ft(lvT[j] - 1.5 * t)))], dyadic=dy_t)
    add("levels_four", [(0, 0.0, 0.0, float(ft(lvT[j] - t / 2))), (mid, 0.0, 2.0 ** -6, float(ft(lvT[j] - 1.75 * t)))], dyadic=dy_t,
        differs="levels_four_alone")
    add("levels_four_alone", [(mid, 0.0, 2.0 ** -6, float(ft(lvT[j] - 1.75 * t)))], dyadic=dy_t)
    # two layers under the gripper, the upper layer's ONLY in-cylinder particle in the last slot / in the first: the minimum over the levels
    # has to cross lanes (and, in the launch, waves). The lower layer is out of the chosen level's band.
    low_z = float(ft(lvT[j] - 3 * t))
    others = sorted(set(k for k in (0, 1, 31, 62, 63, 64, 65, 127, 128, mid, P - 2) if 0 <= k < P - 1))
    ring = lambda q: (((q % 5) - 2) / 256.0, ((q // 5) - 1) / 256.0)          # 15 distinct places around the axis
    add("layers_top_last", [(last, 0.0, 0.0, lvT[j])] + [(k,) + ring(q) + (low_z,) for q, k in enumerate(others)], dyadic=dy_t, differs="layers_low_only_a")
    add("layers_low_only_a", [(k,) + ring(q) + (low_z,) for q, k in enumerate(others)], dyadic=dy_t)
    others0 = sorted(set(P - 1 - k for k in others))
    add("layers_top_first", [(0, 0.0, 0.0, lvT[j])] + [(k,) + ring(q) + (low_z,) for q, k in enumerate(others0)], dyadic=dy_t, differs="layers_low_only_b")
    add("layers_low_only_b", [(k,) + ring(q) + (low_z,) for q, k in enumerate(others0)], dyadic=dy_t)
    # a lower layer just inside the chosen level's band (level j - 1: it reaches down to level j - thickness) is grabbed with the upper one; on
    # the band's edge it is not
    edge2 = edge(lvT[j - 1], -1)
    up_z = float(ft(lvT[j] - t / 2))                   # (between two levels: no tie of its own at any level)
    add("lower_inside", [(0, 0.0, 0.0, up_z), (last, 2.0 ** -6, 0.0, _ulp(edge2, prec, up=True))], dyadic=dy_t, differs="lower_on_edge")
    add("lower_on_edge", [(0, 0.0, 0.0, up_z), (last, 2.0 ** -6, 0.0, edge2)], dyadic=dy_t, tie=("band", last, j - 1) if dy_t else None)

    # ---- nothing to grab: in the cylinder but in no band; nobody in the cylinder
    add("none_no_band", [(0, 0.0, 0.0, float(ft(lvT[0] + 3 * t))), (last, 2.0 ** -6, 0.0, float(ft(lvT[0] + 4 * t)))], dyadic=dy_t)
    add("none_no_cylinder", [], dyadic=dy_t)
    # ---- everything grabbed: radius 4 (one band: every parked particle is at z = 0.25), and every particle packed into the cylinder
    add("everything_r4", [], rad=4.0, dyadic=dy_t, launch=False)
    k = np.arange(P)
    add("everything_packed", [(int(q), ((q % 16) - 8) / 512.0, (((q // 16) % 16) - 8) / 512.0, 0.25) for q in k], dyadic=dy_t, launch=False)
    # ---- slots: a single hit at one index
    for idx in sorted(set(q for q in (0, 63, 64, last) if q < P)):
        add("slot_%d" % idx, [(idx, 2.0 ** -7, -2.0 ** -7, well_in)], differs="none_no_cylinder")
    return out


def check_states(sts, pos_of, lv, t, prec):
    """What the states must BE for their cases to mean something, on the positions a handle holds (pos_of[name]): shared with the GPU tests,
    which pass the positions read back."""
    P = len(sts[0].pos)
    sets = {st.name: set(ge.grab_top(pos_of[st.name], st.xy, st.radius, lv, t, prec)[0].tolist()) for st in sts}
    n_tie = {"cyl": 0, "band": 0}
    for st in sts:
        pos = pos_of[st.name]
        if st.differs is not None:                                   # each sibling pair differs in its set
            assert sets[st.name] != sets[st.differs], (st.name, st.differs, sorted(sets[st.name]))
        if st.tie is not None or st.dyadic:
            c = ge.classify(pos, st.xy, st.radius, lv, t, prec)
        if st.tie is not None:                                       # an exact tie where one is claimed
            if st.tie[0] == "cyl":
                assert c.cyl[st.tie[1]] == 0, st.name
            else:
                assert c.band[st.tie[1], st.tie[2]] == 0 and c.cyl[st.tie[1]] < 0, st.name
            n_tie[st.tie[0]] += 1
        if st.dyadic:                                                # exact and T arithmetic agree, particle by particle
            ft = ge.ftype(prec)
            with np.errstate(invalid="ignore"):
                assert np.array_equal(ge.dist2(pos, st.xy, prec) < ft(st.radius), c.cyl < 0), st.name
                assert np.array_equal(ge.band_dist(pos, lv, prec) < ft(2 * t), c.band < 0), st.name
            idx, lev = ge.grab_top_from_classes(c)
            ref = ge.grab_top(pos, st.xy, st.radius, lv, t, prec)
            assert idx.tolist() == ref[0].tolist() and lev == ref[1], st.name
    assert n_tie["cyl"] == 4 and (n_tie["band"] >= 4 or t != 2.0 ** -5), n_tie
    assert sets["none_no_band"] == sets["none_no_cylinder"] == set()
    assert sets["everything_r4"] == sets["everything_packed"] == set(range(P))
    for idx in (0, 63, 64, P - 1):
        if idx < P:
            assert sets["slot_%d" % idx] == {idx}
    assert sets["layers_top_last"] == {P - 1} and sets["layers_top_first"] == {0} and len(sets["layers_low_only_a"]) >= 3
    assert sets["lower_inside"] == {0, P - 1} and sets["lower_on_edge"] == {0}
    assert sets["levels_three"] == sets["levels_four"] == {0} and sets["levels_three_alone"] == {P // 2}
    # three and four consecutive levels do hold the upper particle
    j = int(np.argmin(np.abs(lv - 0.5)))
    with np.errstate(invalid="ignore"):
        n3 = (ge.band_dist(pos_of["levels_three"], lv, prec)[0] < ge.ftype(prec)(2 * t)).sum()
        n4 = (ge.band_dist(pos_of["levels_four"], lv, prec)[0] < ge.ftype(prec)(2 * t)).sum()
    assert (n3, n4) == (3, 4) if t == 2.0 ** -5 else (n3 >= 3 and n4 >= 3), (n3, n4, j)   # (0.02: the accumulated levels drift by an ulp or two)
    return sets


def force_states(n_side, prec, thickness, radius0, inc, k=3):
    """force_grab states for a handle with grip_radius radius0 and radius_inc inc: the nearest particle (`mid`) sits exactly on the radius of
    try k (d2 == T(radius0 + k inc), the radius grown in double), so it is taken at try k + 1 -- together with particle mid + 1, which lies
    between the radii of the tries k and k + 1 --; one ulp inside, at try k, alone. 'force_t_*': the
    same at the first try whose radius differs between an accumulation in double and one in T (fp32 only: None in fp64, and where the two
    agree on every try up to 5). -> [(GripState, expected tries)]"""
    P = n_side * n_side
    ft = ftype(prec)
    lv = ge.levels(HEIGHT, thickness).astype(ft).astype(np.float64)
    j = int(np.argmin(np.abs(lv - 0.5)))
    z = float(ft(lv[j] - float(ft(2 * thickness)) / 4))
    base = parked(P)
    mid = P // 2
    out = []

    def on_radius(target):
        """(dx, dy) as T numbers with T(T(dx * dx) + T(dy * dy)) == target, the gripper at 0.5 (dx, dy multiples of the ulp of [0.5, 1)): exactly,
        with small dyadic dx and dy, where the target allows it."""
        for a in range(1, 64):
            for b in range(0, a + 1):
                if (a * a + b * b) / 4096.0 == float(target):
                    return a / 64.0, b / 64.0
        u = float(np.finfo(ft).eps) / 2.0                  # the spacing of T in [0.5, 1)
        dx0 = np.floor(np.sqrt(target) / u) * u
        for a in range(0, 64):
            dx = ft(dx0 - a * u)
            rem = float(target) - float(dx * dx)
            if rem < 0:
                continue
            dy0 = np.floor(np.sqrt(rem) / u)
            for b in range(-64, 65):
                dy = ft((dy0 + b) * u)
                if dy >= 0 and ft(dx * dx + dy * dy) == ft(target):
                    return float(dx), float(dy)
        return None

    def add(name, dxy, tries, on_try):
        """... and particle mid + 1 between the radius of try `on_try` and the next one, so that the number of tries shows in the set"""
        pos = base.copy()
        pos[mid] = (XY[0] + dxy[0], XY[1] + dxy[1], z)
        pos[mid + 1] = (XY[0] - float(np.sqrt(radius0 + (on_try + 0.5) * inc)), XY[1], z)
        out.append((GripState(name, pos, XY, radius0, False, None, None, True), tries))

    rk = float(ft(radius0 + k * inc))
    d = on_radius(rk)
    assert d is not None
    add("force_on_try%d" % k, d, k + 1, k)
    add("force_inside_try%d" % k, (_ulp(XY[0] + d[0], prec, up=False) - XY[0], d[1]), k, k)
    # double against T accumulation
    rd, rt = float(radius0), ft(radius0)
    for q in range(1, 6):
        rd += float(inc)
        rt = ft(rt + ft(inc))
        if ft(rd) != rt:
            lo_r = min(float(ft(rd)), float(rt))       # a particle ON the smaller of the two radii is inside the larger one only
            d = on_radius(lo_r)
            if d is not None:
                add("force_t_try%d" % q, d, q if float(ft(rd)) > lo_r else q + 1, q)
                break
    return out


def edge_actions(reduce_factor=0.002, low=(-1.0,) * 4, high=(1.0,) * 4):
    """The decode's edge actions, float64 [n, 4]: zero and negative-zero deltas, a delta shorter than one step, lengths that are k steps
    exactly (k * step == total_length at total_length = k * reduce_factor - 1e-5) and one and two ulps to either side, along x and along the
    diagonal, and every component at, beyond and far beyond both of its bounds."""
    base = np.array([0.25, -0.375, 0.05, -0.02])
    acts = [[0.25, -0.375, 0.0, 0.0], [0.25, -0.375, -0.0, -0.0], [-0.0, -0.0, 0.0, -0.0], [0.25, -0.375, 0.001, 0.0],
            [0.25, -0.375, 0.0, -1e-7], [0.25, -0.375, 1e-300, 0.0]]
    ep = dict(act_low=low, act_high=high, clip_act_space=True, reduce_factor=reduce_factor, iters_up=0, iters_up_rest=0, iters_grip_rest=0,
              iters_rest=0)
    dirs = ((1.0, 0.0), (0.0, -1.0), (np.sqrt(0.5), np.sqrt(0.5)))
    for k in (1, 2, 3, 7, 50, 400):
        for ux, uy in dirs:
            # the largest length v (as the delta's scale) that still decodes to k - 1 pulls: found by bisection on the reference decode (the
            # accumulated current_l rounds, so it is not k * reduce_factor - 1e-5 to the ulp), then its neighbours one and two ulps away
            ip = lambda v: ge.decode([0.25, -0.375, v * ux, v * uy], ep).iters_pull
            lo_v, hi_v = (k * reduce_factor - ge.EPS) * (1 - 1e-6), (k * reduce_factor - ge.EPS) * (1 + 1e-6)
            assert ip(lo_v) == k - 1 and ip(hi_v) == k, (k, ip(lo_v), ip(hi_v))
            while float(np.nextafter(lo_v, np.inf)) < hi_v:
                m_v = 0.5 * (lo_v + hi_v)
                lo_v, hi_v = (m_v, hi_v) if ip(m_v) == k - 1 else (lo_v, m_v)
            for m in (-2, -1, 0, 1, 2):
                v = lo_v
                for _ in range(abs(m)):
                    v = float(np.nextafter(v, np.inf if m > 0 else -np.inf))
                acts.append([0.25, -0.375, v * ux, v * uy])
    for comp in range(4):
        lo, hi = float(low[comp]), float(high[comp])
        for v in (hi, float(np.nextafter(hi, np.inf)), float(np.nextafter(hi, -np.inf)), hi + 3.0, 1e300, np.inf,
                  lo, float(np.nextafter(lo, -np.inf)), float(np.nextafter(lo, np.inf)), lo - 3.0, -1e300, -np.inf):
            a = base.copy()
            a[comp] = v
            acts.append(a.tolist())
    return np.array(acts, dtype=np.float64)
