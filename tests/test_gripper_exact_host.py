"""CPU tests of the gripper's exact reference (oracle/gripper_exact.py) and of the hand-made states (gripper_states.py) the GPU tests
(test_gpu_gripper_exact.py) rest on: the reference agrees with the C oracle, with the reference implementation's own index sets and
with envs.decode_actions; the states ARE what they claim (exact ties, siblings that differ, dyadic states on which exact and T
arithmetic agree); and a numpy model of each of the mutants 13-16 (tools/run_mutants.sh) is told from the reference by these states."""
import numpy as np
import pytest

import gripper_states as gs
from oracle import gripper_exact as ge

EP = dict(act_low=[-1.0] * 4, act_high=[1.0] * 4, clip_act_space=True, reduce_factor=0.002, iters_up=50, iters_up_rest=80,
          iters_grip_rest=300, iters_rest=1000)


def _ocfg(n_side, thickness):
    return {"n_side": n_side, "width": 1, "height": 1, "density": 200.0, "ks": 10000.0, "damping": 2.0, "thickness": thickness,
            "plane_friction": 1.0, "tear_thresh": 2.0, "frames_per_sec": 30, "simulation_steps": 30, "gravity": -9.8, "minimum_z": 0.0,
            "grip_radius": gs.R}


def _all(n_side, prec):
    t = gs.thickness_of(n_side, prec)
    return t, ge.levels(gs.HEIGHT, t), gs.states(n_side, prec, t)


# ---- the reference against the project's other statements of the same rules -------------------------------------------------------------
@pytest.mark.parametrize("n_side", [n for n, p in gs.GRIDS if p == "f64"])
def test_reference_matches_the_c_oracle_on_every_fp64_state(n_side, oracle_lib):
    t, lv, sts = _all(n_side, "f64")
    oc = oracle_lib.OracleCloth(_ocfg(n_side, t))
    P = n_side * n_side
    for st in sts:
        for top in (True, False):
            oc.set_state(st.pos, st.pos, np.zeros(P, dtype=np.uint8))
            oc.release()
            n = (oc.grab_top if top else oc.grab)(st.xy[0], st.xy[1], st.radius)
            want = ge.grab_top(st.pos, st.xy, st.radius, lv, t, "f64")[0] if top else ge.grab(st.pos, st.xy, st.radius, "f64")
            assert n == len(want) and sorted(oc.grabbed.tolist()) == want.tolist(), (st.name, top, n, len(want))


def test_reference_matches_the_reference_implementations_index_sets(oracle_lib):
    g = oracle_lib.load_golden("g_gripper_25.npz")
    t, rad = g["cfg"]["thickness"], g["cfg"]["grip_radius"]
    lv = ge.levels(g["cfg"]["height"], t)
    assert np.array_equal(lv, np.asarray(g["levels"], dtype=np.float64))
    multi = 0
    for q in range(len(g["xy"])):
        top = ge.grab_top(g["pos"][q], g["xy"][q], rad, lv, t, "f64")[0]
        assert top.tolist() == sorted(g["grab_top"][q]), q
        assert ge.grab(g["pos"][q], g["xy"][q], rad, "f64").tolist() == sorted(g["grab"][q]), q
        multi += len(top) > 5
    assert multi


def _decode_both(acts, ep):
    from gym_cloth_amd.envs import decode_actions
    d = decode_actions(acts, ep["act_low"], ep["act_high"], ep["clip_act_space"], True, ep["reduce_factor"], ep["iters_up"],
                       ep["iters_up_rest"], 400, ep["iters_grip_rest"], ep["iters_rest"])
    for k, a in enumerate(acts):
        r = ge.decode(a, ep)
        assert r.terminates, a
        got = (d["x"][k], d["y"][k], d["x_dir_r"][k], d["y_dir_r"][k], int(d["iters_pull"][k]), tuple(d["bounds"][k].tolist()))
        want = (r.x, r.y, r.dx_pull, r.dy_pull, r.iters_pull, r.bounds)
        # (x, y by value: numpy's maximum(-0.0, 0.0) is +0.0 where Python's max keeps -0.0, and the gripper's xy only enters differences)
        assert got[:2] == want[:2] and np.array([got[2:4]]).tobytes() == np.array([want[2:4]]).tobytes() and got[4:] == want[4:], (k, a, got, want)
    return d


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("iters_up", [50, 49.5])
def test_decode_matches_decode_actions_on_the_edge_actions(clip, iters_up):
    ep = dict(EP, clip_act_space=clip, iters_up=iters_up, act_low=[-1.0] * 4 if clip else [0.0, 0.0, -1.0, -1.0])
    acts = gs.edge_actions(ep["reduce_factor"], ep["act_low"], ep["act_high"])
    d = _decode_both(acts, ep)
    ip = d["iters_pull"]
    # the actions do sit on the decode's edges: every k-steps-exactly group changes iters_pull within its five neighbours, zero deltas
    # decode to no pull, clipped components end on their bounds
    assert ip[0] == ip[1] == ip[2] == 0 and np.signbit(d["x_dir_r"][1]) and not np.signbit(d["x_dir_r"][0])
    grp = ip[6:6 + 6 * 15].reshape(6, 3, 5)
    assert (grp.max(axis=2) == np.array([1, 2, 3, 7, 50, 400])[:, None]).all() and (grp.max(axis=2) == grp.min(axis=2) + 1).all(), grp
    assert d["bounds"][0, 0] == 50 and (d["bounds"][:, 1] - d["bounds"][:, 0] == 80).all()
    assert d["x"].max() == 1.0 and d["x"].min() == (0.0) and ip.max() <= 500


def test_decode_matches_the_goldens_of_test_host_logic(oracle_lib):
    for name in ["g_env_tier1_1337.npz", "g_env_tier2_1337.npz", "g_env_tier3_1337.npz", "g_env_tier3_1339.npz"]:
        g = oracle_lib.load_golden(name)
        e = g["cfg"]["env"]
        frac = 0
        for k in range(len(g["act"])):
            iu = float(g["act_iters_up"][k])
            ep = dict(EP, reduce_factor=e["reduce_factor"], iters_up=iu, iters_up_rest=e["iters_up_rest"], iters_grip_rest=e["iters_grip_rest"],
                      iters_rest=e["iters_rest"])
            _decode_both(np.asarray(g["act"][k], dtype=np.float64)[None], ep)
            r = ge.decode(g["act"][k], ep)
            if int(g["act_n_updates"][k]) > 1 and not bool(g["act_tear"][k]):
                assert r.bounds[4] == int(g["act_n_updates"][k]), (name, k)
            frac += iu != int(iu)
        assert frac or "tier3" not in name


def test_decode_keeps_a_nan_and_reports_an_endless_pull_loop():
    """Python's min / max keep a NaN first argument: a NaN coordinate decodes to a NaN gripper position (which grabs nothing), a NaN
    delta makes `current_l >= total_length` False for ever -- what envs.decode_actions reports with FloatingPointError."""
    from gym_cloth_amd import envs
    for comp in range(4):
        a = [0.25, -0.375, 0.05, -0.02]
        a[comp] = float("nan")
        r = ge.decode(a, EP)
        assert r.terminates == (comp < 2), (comp, r)
        if comp < 2:
            d = envs.decode_actions(np.array([a]), EP["act_low"], EP["act_high"], True, True, 0.002, 50, 80, 400, 300, 1000)
            assert np.isnan((r.x, r.y)[comp]) and np.isnan((d["x"], d["y"])[comp][0]) and d["iters_pull"][0] == r.iters_pull > 0
            assert len(ge.grab_top(gs.parked(9), (r.x, r.y), 4.0, ge.levels(1.0, 0.02), 0.02, "f64")[0]) == 0
    assert ge._py_clip(float("nan"), -1.0, 1.0) != ge._py_clip(float("nan"), -1.0, 1.0)
    assert np.signbit(ge._py_clip(-0.0, -1.0, 1.0)) and ge._py_clip(np.inf, -1.0, 1.0) == 1.0 and ge._py_clip(-np.inf, -1.0, 1.0) == -1.0


# ---- the states are what they claim ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_side,prec", gs.GRIDS)
def test_states_are_not_vacuous(n_side, prec):
    t, lv, sts = _all(n_side, prec)
    gs.check_states(sts, {st.name: gs.held(st.pos, prec) for st in sts}, lv, t, prec)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_force_grab_states_sit_on_the_radius_of_a_try(prec):
    for r0, inc, t in ((2.0 ** -10, 2.0 ** -8, 2.0 ** -5), (0.003, 0.02, 0.02)):
        lv = ge.levels(gs.HEIGHT, t)
        fs = gs.force_states(25, prec, t, r0, inc)
        names = [st.name for st, _ in fs]
        assert names[:2] == ["force_on_try3", "force_inside_try3"]
        for st, tries in fs:
            pos = gs.held(st.pos, prec)
            idx, lev, n, rad = ge.force_grab(pos, st.xy, lv, t, r0, inc, prec)
            on_try = int(st.name[-1])                                # the try whose radius the particle is on / just inside
            assert n == tries and idx.tolist() == ([312] if n == on_try else [312, 313]) and 1 <= n <= 5, (st.name, n, tries, idx)
            assert rad == r0 + sum([inc] * n) or abs(rad - (r0 + n * inc)) < 1e-15
        on = gs.held(fs[0][0].pos, prec)
        if r0 == 2.0 ** -10:                                                                   # exactly ON the radius of try 3
            assert ge.classify(on, gs.XY, float(r0 + 3 * inc), lv, t, prec).cyl[312] == 0
        assert (len(fs) == 3) == (prec == "f32" and r0 == 0.003), names                        # double and T accumulation part ways in fp32 only


# ---- a numpy model of each mutant is told from the reference by the states --------------------------------------------------------------
def _model_grab_top(pos, xy, radius, lv, t, prec, cyl=np.less, band=np.less, pick=0):
    ft = ge.ftype(prec)
    with np.errstate(invalid="ignore"):
        hit = band(ge.band_dist(pos, lv, prec), ft(2 * t)) & cyl(ge.dist2(pos, xy, prec), ft(radius))[:, None]
    at = np.nonzero(hit.any(axis=0))[0]
    return set(np.nonzero(hit[:, at[pick]])[0].tolist()) if len(at) else set()


def _model_force_radius(r0, inc, tries, prec, in_t):
    ft = ge.ftype(prec)
    r = ft(r0) if in_t else float(r0)
    for _ in range(tries):
        r = ft(r + ft(inc)) if in_t else r + float(inc)
    return float(ft(r))


_MUTANTS = {13: dict(cyl=np.less_equal), 14: dict(band=np.less_equal), 15: dict(pick=-1)}


@pytest.mark.parametrize("n_side,prec", gs.GRIDS)
def test_the_model_is_the_reference_and_every_mutant_model_is_rejected(n_side, prec):
    t, lv, sts = _all(n_side, prec)
    killed = {m: [] for m in _MUTANTS}
    for st in sts:
        pos = gs.held(st.pos, prec)
        ref = set(ge.grab_top(pos, st.xy, st.radius, lv, t, prec)[0].tolist())
        assert _model_grab_top(pos, st.xy, st.radius, lv, t, prec) == ref, st.name
        for m, kw in _MUTANTS.items():
            if _model_grab_top(pos, st.xy, st.radius, lv, t, prec, **kw) != ref:
                killed[m].append(st.name)
    assert all(any(n.startswith("cyl_") and n.endswith("_on") for n in killed[13]) for _ in [0]), killed[13]
    assert len([n for n in killed[13] if n.endswith("_on")]) == 4, killed[13]              # dx and dy, both signs
    if t == 2.0 ** -5:                                                                      # the band's exact ties need the dyadic thickness
        assert {"band_lo_on", "band_top_on", "band_neg_on", "lower_on_edge"} <= set(killed[14]), killed[14]
    assert {"levels_three", "levels_four", "layers_top_last", "layers_top_first"} <= set(killed[15]), killed[15]


def test_mutant_16s_model_is_rejected_by_the_fp32_force_grab_state():
    """Mutant 16 accumulates the force_grab radius in T: in fp64 that IS the reference; in fp32, with the config's 0.003 + k * 0.02, the two
    radii part ways at some try <= 5 and the 'force_t' state has its particle between them."""
    r0, inc, t = 0.003, 0.02, 0.02
    lv = ge.levels(gs.HEIGHT, t)
    (st, tries), = [f for f in gs.force_states(25, "f32", t, r0, inc) if f[0].name.startswith("force_t_")]
    pos = gs.held(st.pos, "f32")

    def run(in_t):
        for k in range(8):
            got = _model_grab_top(pos, st.xy, _model_force_radius(r0, inc, k, "f32", in_t), lv, t, "f32")
            if got:
                return k, got
    ref = ge.force_grab(pos, st.xy, lv, t, r0, inc, "f32")
    assert run(False) == (tries, set(ref[0].tolist())) == (ref[2], set(ref[0].tolist()))
    assert run(True)[0] != tries and run(True)[1] != run(False)[1]           # another try AND another set: the launch's record shows it
