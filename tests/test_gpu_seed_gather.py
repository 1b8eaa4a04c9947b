"""The eight-wave fp32 LEAN build of a 25x25 handle (512 threads x 2 particles, window table in LDS, grid-specialised: the headline kernel)
reads a stencil neighbour at the owner's LDS address plus a compile-time offset and takes its validity from one bit of the particle's mask
(Hooke gather, strain pre-pass) instead of building and decoding a gather entry per slot. Same numbers from another home: held here to the
standard fp32 variant bit for bit -- on crowded cells of every size class of the collision phase, on the grid border (where a stencil
position does not exist and its read lands in the unused records in front of the particle array) and with a non-finite record in the cloth --
and the same states to the oracle in fp64. One CPU test pins the headline layout's LDS (two cloths per CU)."""
import ctypes as C

import numpy as np
import pytest

from helpers import max_abs

N = 25
CELL = np.float32(3.0 * (1.0 / (N - 1)))                # cloth.pyx:308-310 at width = height = 1: w = h = t = 3 dx, as the fp32 stepper holds it
LEAN_KNOBS = ("CLOTHHIP_DEBUG_LEAN", "CLOTHHIP_DEBUG_W8", "CLOTHHIP_DEBUG_NOSPEC", "CLOTHHIP_DEBUG_PHASES", "CLOTHHIP_DEBUG_TAB_LDS",
              "CLOTHHIP_DEBUG_CELL_COPY", "CLOTHHIP_DEBUG_REST_REG")


def _cfg(g):
    c = g["cfg"]
    return {"cloth": {"num_width_points": c["n_side"], "num_height_points": c["n_side"], "width": c["width"],
                      "height": c["height"], "density": c["density"], "ks": c["ks"], "damping": c["damping"],
                      "thickness": c["thickness"], "plane_friction": c["plane_friction"],
                      "tear_thresh": c["tear_thresh"]},
            "frames_per_sec": c["frames_per_sec"], "simulation_steps": c["simulation_steps"],
            "env": {"grip_radius": c["grip_radius"]}}


def _f32(p):
    return p.astype(np.float32).astype(np.float64)      # every side starts from the same fp32-representable state


def _squeezed(pos0, scale, lift, rng):
    """A crowded state as test_crowded_cells_selfcollision_f32 builds it: the cloth squeezed into a fraction of its size, a thin slab."""
    p = pos0 * scale + 0.3
    p += rng.uniform(-0.004, 0.004, size=p.shape)
    p[:, 2] = lift * rng.uniform(0.0, 0.05, size=len(p)) + 0.001
    return _f32(p)


def _blocked(rng, transpose):
    """A crowded state with PRESCRIBED cell populations: column groups of 8, 8, 5, 3, 1 and row groups of 8, 4, 4, 2, 1, 5, 1 grid lines, every
    group squeezed into one collision cell (0.025 clear of its walls), so cell (cg, rg) holds |cg| x |rg| particles: 64, 32, 16, 15, 3, 2
    among them; three particles are then moved into a neighbouring cell: 32 / 32 -> 31 / 33, 16 -> 17, 64 -> 65 (one 64 and one 16 stay)."""
    colg, rowg = [8, 8, 5, 3, 1], [8, 4, 4, 2, 1, 5, 1]

    def axis(groups):
        xs, gid = [], []
        for g_, s_ in enumerate(groups):
            lo, hi = float(CELL) * (g_ + 1) + 0.025, float(CELL) * (g_ + 2) - 0.025
            xs += [lo + (hi - lo) * (k_ + 0.5) / s_ for k_ in range(s_)]
            gid += [g_] * s_
        return np.array(xs), np.array(gid)

    xc, gc = axis(colg)
    yr, gr = axis(rowg)
    r, c = np.divmod(np.arange(N * N), N)
    p = np.empty((N * N, 3))
    p[:, 0], p[:, 1] = xc[c], yr[r]
    p[:, :2] += rng.uniform(-0.002, 0.002, size=(N * N, 2))
    p[:, 2] = 0.1 * rng.uniform(0.0, 0.05, size=N * N) + 0.001
    cell = lambda cg, rg: np.nonzero((gc[c] == cg) & (gr[r] == rg))[0]
    for src, dst in (((0, 1), (1, 1)), ((0, 4), (0, 3)), ((2, 0), (1, 0))):
        i, j = cell(*src)[-1], cell(*dst)[0]
        p[i, :2] = p[j, :2] + 0.003
    if transpose:
        p[:, [0, 1]] = p[:, [1, 0]]
    return _f32(p)


def _held_prev(p, c):
    """Previous positions with which the first Hooke + Verlet leaves the cloth (nearly) where it is, so that the FIRST collision phase sees the
    populations _blocked prescribes: x' = x + damp (x - prev) + f dt^2 / m (cloth.pyx:249) stays x for prev = x + f dt^2 / (m damp). The force is
    summed here in fp64 over the grid's springs (cloth.pyx:117-146); what the steppers make of it is read back by the test, not assumed."""
    n = c["n_side"]
    r, col = np.divmod(np.arange(n * n), n)
    d0 = c["width"] / (n - 1)
    f = np.zeros_like(p)
    for dr, dc, rest, ks in ((1, 0, d0, 1.0), (0, 1, d0, 1.0), (1, 1, d0 * 2 ** 0.5, 1.0), (1, -1, d0 * 2 ** 0.5, 1.0), (2, 0, 2 * d0, 0.2), (0, 2, 2 * d0, 0.2)):
        a = np.nonzero((r + dr < n) & (col + dc < n) & (col + dc >= 0))[0]
        b = a + dr * n + dc
        d = p[b] - p[a]
        ln = np.linalg.norm(d, axis=1)
        fm = (c["ks"] * ks * (ln - rest) / ln)[:, None] * d
        np.add.at(f, a, fm)
        np.add.at(f, b, -fm)
    dsm = (1.0 / c["frames_per_sec"] / c["simulation_steps"]) ** 2 / (c["density"] / n / n)
    return _f32(p + f * dsm / (1.0 - c["damping"] / 100.0))


def _crowded_states(pos0, c):
    pos = np.stack([_blocked(np.random.RandomState(11), False), _blocked(np.random.RandomState(12), True),
                    _squeezed(pos0, 0.38, 0.1, np.random.RandomState(380)), _squeezed(pos0, 0.22, 0.3, np.random.RandomState(220))])
    return pos, np.stack([_held_prev(pos[0], c), _held_prev(pos[1], c), pos[2], pos[3]])


def _cell_counts(pos):
    """Members per occupied collision cell, recomputed on the host in the fp32 arithmetic of cell_key (cloth.pyx:307-311)."""
    f = np.floor(pos.astype(np.float32) / CELL).astype(np.int64)
    return np.unique(f, axis=0, return_counts=True)[1]


def _batch(cfg, E, prec, lean, monkeypatch, phases=None):
    """A handle on the standard fp32 variant (lean 0), on the eight-wave LEAN build (8) or on whatever the plan picks (None)."""
    from gym_cloth_amd import ClothBatch
    for k_ in LEAN_KNOBS:
        monkeypatch.delenv(k_, raising=False)
    if lean is not None:
        monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", str(lean))
    if phases is not None:
        monkeypatch.setenv("CLOTHHIP_DEBUG_PHASES", str(phases))
    return ClothBatch(cfg, n_envs=E, precision=prec)


def _assert_headline(b):
    v = b.last_variant()
    assert (v["lean"] and v["threads"] == 512 and v["particles_per_thread"] == 2 and v["table_mode"] == 2 and v["spec_n_side"] == 25
            and v["precision"] == "f32" and v["cloths_per_cu"] >= 2), v


def _assert_standard(b, spec=25):
    v = b.last_variant()
    assert not v["lean"] and v["precision"] == "f32" and v["spec_n_side"] == spec, v


def _trajectory(b, pos, prev, pin, rest, steps):
    b.set_state(pos, prev, pin, rest)
    out = []
    for _ in range(steps):
        b.update(1)
        out.append([x.copy() for x in b.get_state()[:2]])
    return out


@pytest.mark.gpu
def test_crowded_cells_headline_build_equals_standard_f32_and_oracle_f64(oracle_lib, monkeypatch):
    """Four crowded cloths, four substeps. The cells the first collision phase sees (the positions after the first Hooke + Verlet, taken from
    a Hooke-only run of the standard variant and binned on the host; two of the cloths start with previous positions that hold them in place for it) hold 2, 3, 15, 16, 17, 31, 32, 33, 64 and more than 64 members, and at
    least two cells of odd population in each of the two cloths built for it -- so, whatever order the cells get in the member list, cell ranges start at even AND
    at odd positions. The headline build equals the standard fp32 variant bit for bit after every substep (positions and previous
    positions); the fp64 stepper run from the same states equals the oracle, max |delta| = 0."""
    g = oracle_lib.load_golden("g_traj_lift_pull_25.npz")
    cfg = _cfg(g)
    E, steps = 4, 4
    probe = _batch(cfg, E, "f32", 0, monkeypatch, phases=1)               # Hooke + Verlet only
    pos0, rest0 = probe.init_grid(1)
    states, prevs = _crowded_states(pos0, g["cfg"])
    pin = np.zeros((E, probe.P), dtype=np.uint8)
    pin[:, 0] = 1
    probe.set_state(states, prevs, pin, rest0)
    probe.update(1)
    after_hooke = probe.positions()
    probe.close()
    counts = [_cell_counts(after_hooke[e]) for e in range(E)]
    seen = set(np.concatenate(counts).tolist())
    print("cell populations at the first collision phase:", [sorted(set(c.tolist())) for c in counts])
    assert {2, 3, 15, 16, 17, 31, 32, 33, 64} <= seen and max(seen) > 64, sorted(seen)
    for e in range(2):                                                     # (the two cloths with prescribed populations)
        assert len(counts[e]) >= 3 and (counts[e] % 2 == 1).sum() >= 2, (e, counts[e])

    std = _batch(cfg, E, "f32", 0, monkeypatch)
    a = _trajectory(std, states, prevs, pin, rest0, steps)
    _assert_standard(std)
    std.close()
    new = _batch(cfg, E, "f32", 8, monkeypatch)
    b = _trajectory(new, states, prevs, pin, rest0, steps)
    _assert_headline(new)
    new.close()
    for s_ in range(steps):
        assert np.array_equal(a[s_][0], b[s_][0]) and np.array_equal(a[s_][1], b[s_][1]), (s_, max_abs(a[s_][0], b[s_][0]))
    assert np.abs(a[0][0] - after_hooke).max() > 1e-4, "the case must exercise self-collision"

    f64 = _batch(cfg, E, "f64", None, monkeypatch)
    f64.set_state(states, prevs, pin, rest0)
    ocs = []
    for e in range(E):
        oc = oracle_lib.OracleCloth(g["cfg"])
        oc.set_state(states[e], prevs[e], pin[e], rest0)
        ocs.append(oc)
    for s_ in range(steps):
        f64.update(1)
        got = f64.positions()
        for e, oc in enumerate(ocs):
            oc.update(1)
            assert max_abs(got[e], oc.get_state()[0]) == 0.0, (s_, e)
    assert f64.last_variant()["precision"] == "f64"
    assert all(oc.last_stats()[1] > 0 for oc in ocs), "the case must exercise self-collision"
    f64.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stretch", [1.08, 1.15])
def test_border_stencil_one_substep(stretch, oracle_lib, monkeypatch):
    """One substep from a perturbed flat cloth in which EVERY spring is stretched (below the strain limit of 1.1 at 1.08: no spring may be
    flagged; beyond it at 1.15: every one is): rows and columns 0, 1, 23, 24 are where stencil positions are absent, their reads land
    outside the particle array and their values must be discarded by the selects. fp64: every border particle (every particle) equals the
    oracle bit for bit. fp32: the headline build equals the standard variant, in positions, previous positions and in the number of strain
    sweeps run (an absent position taken for a spring would flag it and start a sweep)."""
    g = oracle_lib.load_golden("g_traj_lift_pull_25.npz")
    cfg = _cfg(g)
    E = 2
    std = _batch(cfg, E, "f32", 0, monkeypatch)
    pos0, rest0 = std.init_grid(1)
    rng = np.random.RandomState(int(stretch * 100))
    states = []
    for e in range(E):
        p = pos0 * stretch
        p[:, :2] += rng.uniform(-0.0001, 0.0001, size=(len(p), 2))           # (a spring's length moves by 3e-4 at the most: 1.08 stays below 1.1)
        p[:, 2] = 0.3 + rng.uniform(-0.0001, 0.0001, size=len(p))
        states.append(_f32(p))
    states = np.stack(states)
    pin = np.zeros((E, std.P), dtype=np.uint8)
    a = _trajectory(std, states, states, pin, rest0, 1)[0]
    sweeps_a = std.debug_stats()[:, 0].copy()
    _assert_standard(std)
    std.close()
    new = _batch(cfg, E, "f32", 8, monkeypatch)
    b = _trajectory(new, states, states, pin, rest0, 1)[0]
    sweeps_b = new.debug_stats()[:, 0].copy()
    _assert_headline(new)
    new.close()
    r, c = np.divmod(np.arange(N * N), N)
    border = np.isin(r, (0, 1, N - 2, N - 1)) | np.isin(c, (0, 1, N - 2, N - 1))
    assert np.array_equal(a[0][:, border], b[0][:, border]) and np.array_equal(a[1][:, border], b[1][:, border]), max_abs(a[0], b[0])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(sweeps_a, sweeps_b) and (sweeps_a == (0 if stretch < 1.1 else 1)).all(), (sweeps_a, sweeps_b)

    f64 = _batch(cfg, E, "f64", None, monkeypatch)
    f64.set_state(states, states, pin, rest0)
    f64.update(1)
    got = f64.positions()
    for e in range(E):
        oc = oracle_lib.OracleCloth(g["cfg"])
        oc.set_state(states[e], states[e], pin[e], rest0)
        oc.update(1)
        ref = oc.get_state()[0]
        assert max_abs(got[e][border], ref[border]) == 0.0 and max_abs(got[e], ref) == 0.0, e
    f64.close()


@pytest.mark.gpu
def test_non_finite_record_in_a_crowded_cloth(oracle_lib, monkeypatch):
    """One unpinned particle of a crowded cloth holds a NaN coordinate: after the Hooke + Verlet of a substep its twelve neighbours do too, and
    all thirteen share the cell of the non-finite keys, where every distance is NaN and the seed test's !(d2 > thr2) accepts it (the plane
    phase, whose z >= minimum_z fails on a NaN, then puts the neighbours back on their previous positions; the particle itself stays NaN).
    Two substeps: the headline build equals the standard fp32 variant, NaNs in the same places."""
    g = oracle_lib.load_golden("g_traj_lift_pull_25.npz")
    cfg = _cfg(g)
    E = 2
    std = _batch(cfg, E, "f32", 0, monkeypatch)
    pos0, rest0 = std.init_grid(1)
    states = np.stack([_blocked(np.random.RandomState(21), False), _squeezed(pos0, 0.38, 0.1, np.random.RandomState(381))])
    states[:, 12 * N + 12, 0] = np.nan
    pin = np.zeros((E, std.P), dtype=np.uint8)
    pin[:, 0] = 1
    a = _trajectory(std, states, states, pin, rest0, 2)
    _assert_standard(std)
    std.close()
    new = _batch(cfg, E, "f32", 8, monkeypatch)
    b = _trajectory(new, states, states, pin, rest0, 2)
    _assert_headline(new)
    new.close()
    for s_ in range(2):
        assert np.array_equal(a[s_][0], b[s_][0], equal_nan=True) and np.array_equal(a[s_][1], b[s_][1], equal_nan=True), s_
    bad = np.isnan(a[0][0]).any(axis=2).sum(axis=1)
    assert (bad >= 1).all() and (bad < N * N).all(), bad                    # the record stays non-finite, the cloth around it does not blow up


def test_headline_layout_keeps_two_cloths_per_cu():
    """The records in front of the particle array are part of the LDS plan: the headline layout (25x25, fp32, 512 cloths: eight-wave LEAN,
    table in LDS) stays within 64 of the CU's 128 LDS granules of 1 280 bytes, i.e. two cloths per CU remain resident."""
    import os
    import __graft_entry__ as ge
    from gym_cloth_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    L = _lib.load()
    p = _lib.params_from_cfg({"cloth": {"num_width_points": N, "num_height_points": N, "width": 1, "height": 1, "density": 200.0, "ks": 1e4,
                                        "damping": 2.0, "thickness": 0.02, "plane_friction": 1.0, "tear_thresh": 2.0},
                              "frames_per_sec": 30, "simulation_steps": 30, "env": {"grip_radius": 0.003}})
    out = np.zeros(24, dtype=np.int32)
    _lib.check(L.clothhip_selftest_layout(C.byref(p), 1, 512, 256, _lib.i32p(out), 24))
    lean, lean_r, threads, ppt, tab, lds = bool(out[10]), int(out[11]), int(out[12]), int(out[13]), int(out[14]), int(out[17])
    assert lean and lean_r == 2 and (threads, ppt, tab) == (512, 2, 2), out.tolist()
    assert -(-lds // 1280) <= 64, lds
    assert bool(out[22]) and bool(out[23]), out.tolist()                      # the episode launches still fit
