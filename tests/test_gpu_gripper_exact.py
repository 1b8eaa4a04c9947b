"""Both device grabs and the episode launch's action decode against the exact reference (oracle/gripper_exact.py), computed from the
positions READ BACK from the handle: k_grab (csrc/cloth_state_kernels.hpp) on hand-made states at every grid class (gripper_states.py:
particles exactly on the cylinder's and a band's edge and one ulp to either side, level choices across lanes and waves, nothing /
everything grabbed, single slots), its multiplicity / active / radius arguments; the in-launch grab (csrc/episode_plan.inc.hpp) on the
same states in every variant class, with force_grab off and on; the in-launch decode on its edge actions; NaN actions.

Every assertion is an equality: with -ffp-contract=off each operation of the grabs is one rounding in the handle's type, and the decode is
double arithmetic in the reference's order, so the reference is a restatement. Nothing is excluded in either precision.

NaN: the decode clips as Python's max(min(x, high), low) does (a NaN stays a NaN). Before that it clipped with fmin / fmax, which turn a
NaN into a bound: a NaN delta pulled at full length and the 200 000-step guard could never fire (this file's NaN tests failed on it)."""
import numpy as np
import pytest

import gripper_states as gs
from oracle import gripper_exact as ge
from test_gpu_metrics_exact import _LAUNCH_CASES, _SWITCHES, _THICKNESS, _spy_records

pytestmark = pytest.mark.gpu

SHORT = dict(iters_up=2, iters_up_rest=1, iters_grip_rest=1, iters_rest=2)      # the in-launch schedule around the pull
PULL = (0.0042, -0.001)                                                          # the in-launch tests' delta: two or three pull steps


def _cfg(n_side, thickness, **env):
    import bench
    cfg = bench.bench_cfg(n_side, thickness)
    cfg["env"].update(dict(grip_radius=gs.R), **env)
    return cfg


def _pins(b):
    return b.pin_counts().astype(np.int64)


def _expect(idx, P, mult=1):
    w = np.zeros(P, dtype=np.int64)
    w[idx] = mult
    return w


# ---- the stand-alone kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_side,prec", gs.GRIDS)
def test_standalone_grabs_on_hand_made_states(n_side, prec):
    """k_grab, one ClothBatch per (grid, precision) with every hand-made state as one env: grab_top and grab with the per-env radius array,
    grab_top with the handle's default radius -- pin bytes and returned counts against the reference on the read-back positions."""
    from gym_cloth_amd import ClothBatch
    t = gs.thickness_of(n_side, prec)
    sts = gs.states(n_side, prec, t)
    lv = ge.levels(gs.HEIGHT, t)
    P, E = n_side * n_side, len(sts)
    b = ClothBatch(_cfg(n_side, t), n_envs=E, precision=prec)
    allpos = np.stack([s.pos for s in sts])
    xy = np.array([s.xy for s in sts])
    rad = np.array([s.radius for s in sts])
    b.set_state(allpos, allpos, np.zeros((E, P), dtype=np.uint8))
    pos = b.positions()
    got = {}
    for key, call in (("top", lambda: b.grab_top(xy, radius=rad)), ("grab", lambda: b.grab(xy, radius=rad)), ("top_default", lambda: b.grab_top(xy))):
        n = call()
        got[key] = (n.copy(), _pins(b))
        b.release()
        assert not _pins(b).any()
    assert np.array_equal(b.positions(), pos)
    b.close()
    gs.check_states(sts, {s.name: pos[i] for i, s in enumerate(sts)}, lv, t, prec)            # on what the device holds
    sizes = set()
    for i, s in enumerate(sts):
        top = ge.grab_top(pos[i], s.xy, s.radius, lv, t, prec)[0]
        assert np.array_equal(got["top"][1][i], _expect(top, P)) and got["top"][0][i] == len(top), (s.name, np.nonzero(got["top"][1][i])[0], top)
        cyl = ge.grab(pos[i], s.xy, s.radius, prec)
        assert np.array_equal(got["grab"][1][i], _expect(cyl, P)) and got["grab"][0][i] == len(cyl), (s.name, np.nonzero(got["grab"][1][i])[0], cyl)
        dflt = ge.grab_top(pos[i], s.xy, gs.R, lv, t, prec)[0]
        assert np.array_equal(got["top_default"][1][i], _expect(dflt, P)) and got["top_default"][0][i] == len(dflt), s.name
        sizes.add(len(top))
    assert {0, 1, 2, P} <= sizes


@pytest.mark.parametrize("n_side,prec", [(3, "f32"), (25, "f64")])
def test_standalone_multiplicity_active_and_radius(n_side, prec):
    """Grabbing twice counts 2; at 3x3 the count saturates at CNT_GRAB_MASK and every call still reports n; release clears; the active mask
    leaves inactive envs' bytes and counts alone; a per-env radius array where every env differs."""
    from gym_cloth_amd import ClothBatch
    t = gs.thickness_of(n_side, prec)
    lv = ge.levels(gs.HEIGHT, t)
    P, E = n_side * n_side, 6
    st = {s.name: s for s in gs.states(n_side, prec, t)}["everything_packed"]
    b = ClothBatch(_cfg(n_side, t), n_envs=E, precision=prec)
    b.set_state(st.pos, st.pos, np.zeros((E, P), dtype=np.uint8))
    pos = b.positions()
    xy = np.broadcast_to(st.xy, (E, 2))
    # every env its own radius: from "one particle or none" up to "all of them"
    rad = np.array([2.0 ** -18, 3.0 * 2.0 ** -16, 2.0 ** -13, 1.5 * 2.0 ** -12, 2.0 ** -11, 2.0 ** -8])
    want = [ge.grab_top(pos[e], st.xy, rad[e], lv, t, prec)[0] for e in range(E)]
    assert len(set(len(w) for w in want)) == (E if P > 9 else 4) and len(want[-1]) == P, [len(w) for w in want]
    n1 = b.grab_top(xy, radius=rad)
    n2 = b.grab_top(xy, radius=rad)
    for e in range(E):
        assert n1[e] == n2[e] == len(want[e]) and np.array_equal(_pins(b)[e], _expect(want[e], P, 2)), e
    # the active mask: envs 1, 3, 5 untouched (bytes and returned count 0), the others go to 3
    act = np.array([1, 0, 1, 0, 1, 0], dtype=np.uint8)
    n3 = b.grab(xy, radius=rad, active=act)
    for e in range(E):
        cyl = ge.grab(pos[e], st.xy, rad[e], prec)
        assert cyl.tolist() == want[e].tolist()                       # (one band: grab and grab_top agree on this state)
        assert n3[e] == (len(cyl) if act[e] else 0) and np.array_equal(_pins(b)[e], _expect(want[e], P, 3 if act[e] else 2)), e
    b.release(active=act)
    for e in range(E):
        assert np.array_equal(_pins(b)[e], _expect(want[e], P, 0 if act[e] else 2)), e
    b.release()
    assert not _pins(b).any()
    if P == 9:                                                        # saturation
        for k in range(ge.CNT_GRAB_MASK + 3):
            n = b.grab_top(xy, radius=rad)
            assert np.array_equal(n, [len(w) for w in want]), k
        for e in range(E):
            assert np.array_equal(_pins(b)[e], _expect(want[e], P, ge.CNT_GRAB_MASK)), e
        b.release()
        assert not _pins(b).any()
    assert np.array_equal(b.positions(), pos)
    b.close()


# ---- the in-launch grab in every variant class -----------------------------------------------------------------------------------------
def _env(n_side, prec, thickness, E, **env_cfg):
    from gym_cloth_amd.envs import ClothVecEnv
    return ClothVecEnv(_cfg(n_side, thickness, **env_cfg), n_envs=E, precision=prec, consume_domrand_draws=False)


def _ep_of(env):
    return dict(act_low=[float(v) for v in env.action_space.low], act_high=[float(v) for v in env.action_space.high],
                clip_act_space=bool(env._clip_act_space), reduce_factor=env.reduce_factor, iters_up=env.iters_up, iters_up_rest=env.iters_up_rest,
                iters_grip_rest=env.iters_grip_rest, iters_rest=env.iters_rest)


def _launch_one_action(env, sts, acts):
    """set_state the states, ONE action per env with auto_reset off -> (positions read back before the launch, the launch's step records)."""
    E, P = len(sts), env.P
    allpos = np.stack([s.pos for s in sts])
    env.batch.set_state(allpos, allpos, np.zeros((E, P), dtype=np.uint8))
    before = env.batch.get_state()
    recs = _spy_records(env)
    env.step_many(np.ascontiguousarray(acts[None]), auto_reset=False)
    (rec,) = recs
    return before, rec[0]


def _twin_end_state(cfg, prec, sts, xy, radius, dec, n_want):
    """The same states on a second handle: grab_top with the reference's final radius, run() with the reference's schedule."""
    from gym_cloth_amd import ClothBatch
    from gym_cloth_amd.batch import make_schedules
    E = len(sts)
    b = ClothBatch(cfg, n_envs=E, precision=prec)
    allpos = np.stack([s.pos for s in sts])
    b.set_state(allpos, allpos, np.zeros((E, b.P), dtype=np.uint8))
    n = b.grab_top(xy, radius=radius)
    assert np.array_equal(n, n_want), (n, n_want)                     # the stand-alone kernel: verified against the reference above
    s = make_schedules(E, break_on_tear=1, dz_up=0.0025)
    bounds = np.array([d.bounds for d in dec])
    s["n_up_end"], s["n_uprest_end"], s["n_pull_end"], s["n_griprest_end"], s["n_total"] = bounds.T
    s["dx_pull"], s["dy_pull"] = [d.dx_pull for d in dec], [d.dy_pull for d in dec]
    s["active"] = n_want > 0
    ex = b.run(s)
    ex[n_want == 0] = 0
    end = b.get_state()
    b.close()
    return ex, end


@pytest.mark.parametrize("force", [False, True], ids=["plain", "force_grab"])
@pytest.mark.parametrize("case", _LAUNCH_CASES, ids=[c[0] for c in _LAUNCH_CASES])
def test_in_launch_grab_on_hand_made_states(case, force, monkeypatch):
    """The episode launch's own grab_top (per-thread level scan, wave butterfly, atomicMin across waves, atomicAdd count, force_grab radius
    loop) on the hand-made states, one action per env: n_grabbed against the reference on the read-back positions, and the end state, by
    bytes, against a twin handle that grabs with the stand-alone kernel at the reference's final radius and runs the reference's schedule."""
    _, n_side, prec, switches, _, (nt, ppt, tab, lean) = case
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in switches.items():
        monkeypatch.setenv("CLOTHHIP_DEBUG_" + k, val)
    t = _THICKNESS[n_side]
    lv = ge.levels(gs.HEIGHT, t)
    r0, inc = (2.0 ** -10, 2.0 ** -8) if force else (gs.R, 0.02)
    if force:
        # (the state that tells an accumulation in double from one in T needs the radii 0.003 + k * 0.02: a launch of its own, below)
        sts = [p[0] for p in gs.force_states(n_side, prec, t, r0, inc)]
        sts += [s for s in gs.states(n_side, prec, t, radius=r0) if s.name.startswith(("layers_", "slot_", "lower_", "none_"))]
    else:
        sts = [s for s in gs.states(n_side, prec, t) if s.launch]
    E, P = len(sts), n_side * n_side
    env = _env(n_side, prec, t, E, force_grab=force, grip_radius=r0, **SHORT)
    env._radius_inc = inc
    acts = np.tile(np.array([0.0, 0.0, PULL[0], PULL[1]]), (E, 1))        # clip space: the gripper at (0.5, 0.5)
    dec = [ge.decode(a, _ep_of(env)) for a in acts]
    assert (dec[0].x, dec[0].y) == gs.XY and dec[0].iters_pull in (2, 3) and dec[0].bounds[4] == 6 + dec[0].iters_pull
    before, r = _launch_one_action(env, sts, acts)
    v = env.batch.last_variant()
    after = env.batch.get_state()
    cfg = env.cfg
    env.close()
    assert v["fused"] >= 1 and v["precision"] == prec and v["threads"] == nt and v["particles_per_thread"] == ppt and v["lean"] == lean, v
    assert tab is None or v["table_mode"] == tab, v
    pos = before[0]
    want, radius, tries = [], np.empty(E), []
    for i, s in enumerate(sts):
        if force:
            idx, _, k, rad = ge.force_grab(pos[i], s.xy, lv, t, r0, inc, prec)
        else:
            (idx, _), k, rad = ge.grab_top(pos[i], s.xy, r0, lv, t, prec), 0, r0
        want.append(idx); radius[i] = rad; tries.append(k)
    n_want = np.array([len(w) for w in want])
    assert (r["ran"] == 1).all()
    assert np.array_equal(r["n_grabbed"], n_want), [(s.name, int(a), int(b)) for s, a, b in zip(sts, r["n_grabbed"], n_want) if a != b]
    assert np.array_equal(r["iters_pull"], [d.iters_pull for d in dec])
    ex, end = _twin_end_state(cfg, prec, sts, np.array([s.xy for s in sts]), radius, dec, n_want)
    assert np.array_equal(r["executed"], ex), (r["executed"], ex)
    assert ((r["executed"] == 0) == (n_want == 0)).all()
    for k in range(3):                                                   # positions, previous positions, pin bytes
        assert after[k].tobytes() == end[k].tobytes(), (k, [s.name for i, s in enumerate(sts) if not np.array_equal(after[k][i], end[k][i])])
    idle = n_want == 0
    for k in range(3):                                                   # nothing grabbed: the state is untouched
        assert after[k][idle].tobytes() == before[k][idle].tobytes(), k
    if force:
        assert not idle.any() and tries[0] == 4 and tries[1] == 3 and 0 in tries and max(tries) >= 5, tries
    else:
        rest = [s for s in gs.states(n_side, prec, t) if not s.launch]          # (the stand-alone kernel's alone: as a handle would hold them)
        gs.check_states(sts + rest, dict({s.name: pos[i] for i, s in enumerate(sts)}, **{s.name: gs.held(s.pos, prec) for s in rest}), lv, t, prec)
        assert idle.sum() >= 4 and {1, 2} <= set(n_want.tolist()) and n_want.max() >= 3


@pytest.mark.parametrize("case", [c for c in _LAUNCH_CASES if c[2] == "f32" and c[0] in ("25_f32_lean0", "25_f32_lean3", "33_f32", "64_f32")],
                         ids=lambda c: c[0])
def test_in_launch_force_grab_grows_its_radius_in_double(case, monkeypatch):
    """force_grab with the config's radii 0.003 + k * 0.02 in fp32: at some try the radius accumulated in double and cast differs from one
    accumulated in float32, and the state's nearest particle sits exactly on the smaller of the two."""
    _, n_side, prec, switches, _, (nt, ppt, tab, lean) = case
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in switches.items():
        monkeypatch.setenv("CLOTHHIP_DEBUG_" + k, val)
    t = _THICKNESS[n_side]
    lv = ge.levels(gs.HEIGHT, t)
    pairs = gs.force_states(n_side, prec, t, 0.003, 0.02)
    assert len(pairs) == 3 and pairs[2][0].name.startswith("force_t_")
    sts = [p[0] for p in pairs]
    env = _env(n_side, prec, t, len(sts), force_grab=True, grip_radius=0.003, **SHORT)
    acts = np.tile(np.array([0.0, 0.0, PULL[0], PULL[1]]), (len(sts), 1))
    dec = [ge.decode(a, _ep_of(env)) for a in acts]
    before, r = _launch_one_action(env, sts, acts)
    v = env.batch.last_variant()
    after = env.batch.get_state()
    cfg = env.cfg
    env.close()
    assert v["threads"] == nt and v["particles_per_thread"] == ppt and v["lean"] == lean, v
    ref = [ge.force_grab(before[0][i], s.xy, lv, t, 0.003, 0.02, prec) for i, s in enumerate(sts)]
    assert [q[2] for q in ref] == [p[1] for p in pairs]
    n_want = np.array([len(q[0]) for q in ref])
    assert np.array_equal(r["n_grabbed"], n_want) and set(n_want.tolist()) == {1, 2}
    ex, end = _twin_end_state(cfg, prec, sts, np.array([s.xy for s in sts]), np.array([q[3] for q in ref]), dec, n_want)
    assert np.array_equal(r["executed"], ex)
    for k in range(3):
        assert after[k].tobytes() == end[k].tobytes(), k


# ---- the in-launch decode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:overflow encountered")      # (the host's out-of-bounds penalty squares the 1e300 actions)
@pytest.mark.parametrize("iters_up", [50, 49.5])
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
def test_in_launch_decode_on_edge_actions(clip, iters_up):
    """The launch's decode (clip, un-clip, direction, the iters_pull loop, five ceil'ed boundaries) on the edge actions, one flat 25x25 cloth
    per action: the record's action, iters_pull, n_grabbed and executed against the reference decode and the reference grab."""
    n_side, prec, t = 25, "f64", 0.02
    env0 = _env(n_side, prec, t, 1, clip_act_space=clip)
    acts = gs.edge_actions(env0.reduce_factor, env0.action_space.low, env0.action_space.high)
    env0.close()
    E = len(acts)
    env = _env(n_side, prec, t, E, clip_act_space=clip, grip_radius=0.003, iters_up=iters_up, iters_up_rest=1, iters_grip_rest=1, iters_rest=2)
    ep = _ep_of(env)
    lv = ge.levels(gs.HEIGHT, t)
    flat = env.batch.init_grid()[0]
    sts = [gs.GripState("flat", flat, None, 0.003, False, None, None, True)] * E
    before, r = _launch_one_action(env, sts, acts)
    env.close()
    dec = [ge.decode(a, ep) for a in acts]
    assert r["action"].tobytes() == acts.tobytes()                       # as given: unclipped, signed zeros and infinities included
    assert (r["ran"] == 1).all()
    assert np.array_equal(r["iters_pull"], [d.iters_pull for d in dec])
    n_want = np.array([len(ge.grab_top(before[0][i], (d.x, d.y), 0.003, lv, t, prec)[0]) for i, d in enumerate(dec)])
    assert np.array_equal(r["n_grabbed"], n_want) and (n_want > 0).all()
    total = np.array([d.bounds[4] for d in dec])
    assert np.array_equal(r["executed"][r["tear"] == 0], total[r["tear"] == 0])
    assert (r["tear"][:66] == 0).all() and (r["executed"] <= total).all() and (r["executed"] > 0).all()       # (pulls of up to 7 steps tear nothing)
    assert (total == int(np.ceil(iters_up)) + 4 + np.array([d.iters_pull for d in dec])).all() and len(set(total.tolist())) >= 10


# ---- NaN actions ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_nan_action_is_an_ordinary_input(prec):
    """A NaN in each of the four components, one env each, beside a healthy env. The reference's clip keeps the NaN: a NaN coordinate is a
    gripper position that grabs nothing (step() exits early, so does the launch: n_grabbed 0, executed 0), a NaN delta makes the iters_pull
    loop endless -- step() raises FloatingPointError from decode_actions, step_many from the launch's guard (`ran` == 2). The healthy
    env's record is that of a launch without the NaN neighbours."""
    n_side, t, E = 25, 0.02, 5
    healthy = np.array([0.1, -0.2, 0.05, -0.02])
    acts = np.tile(healthy, (E, 1))
    for c in range(4):
        acts[c, c] = np.nan

    def launch(a, raises):
        env = _env(n_side, prec, t, E, grip_radius=0.003, **SHORT)
        flat = env.batch.init_grid()[0]
        env.batch.set_state(flat, flat, np.zeros((E, env.P), dtype=np.uint8))
        recs = _spy_records(env)
        if raises:
            with pytest.raises(FloatingPointError):
                env.step_many(np.ascontiguousarray(a[None]), auto_reset=False)
        else:
            env.step_many(np.ascontiguousarray(a[None]), auto_reset=False)
        state = env.batch.get_state()
        env.close()
        return recs[0][0], state, flat
    dec = [ge.decode(a, dict(act_low=[-1.0] * 4, act_high=[1.0] * 4, clip_act_space=True, reduce_factor=0.002, **SHORT)) for a in acts]
    assert [d.terminates for d in dec] == [True, True, False, False, True]
    r, state, flat = launch(acts, raises=True)
    clean, state0, _ = launch(np.tile(healthy, (E, 1)), raises=False)
    assert r[4].tobytes() == clean[4].tobytes() and clean["ran"][4] == 1 and clean["n_grabbed"][4] > 0 and clean["executed"][4] == dec[4].bounds[4]
    for k in range(3):
        assert state[k][4].tobytes() == state0[k][4].tobytes()
    assert r["ran"].tolist() == [1, 1, 2, 2, 1], r["ran"]
    assert r["n_grabbed"][:2].tolist() == [0, 0] and r["executed"][:4].tolist() == [0, 0, 0, 0], (r["n_grabbed"], r["executed"])
    assert r["iters_pull"][:2].tolist() == [dec[0].iters_pull, dec[1].iters_pull]
    assert r["action"].tobytes() == acts.tobytes()
    for e in range(4):                                                   # no NaN env moved its cloth
        assert np.array_equal(state[0][e], gs.held(flat, prec)), e
    assert not state[2][:2].any()
    # NaN coordinates alone do not raise, in step_many as in step()
    only_xy = acts.copy()
    only_xy[2], only_xy[3] = healthy, healthy
    r2, _, _ = launch(only_xy, raises=False)
    assert r2["ran"].tolist() == [1] * 5 and r2["n_grabbed"][:2].tolist() == [0, 0] and r2[2:].tobytes() == clean[2:].tobytes()
    from gym_cloth_amd.envs import ClothVecEnv
    env = ClothVecEnv(_cfg(n_side, t, grip_radius=0.003, **SHORT), n_envs=E, precision=prec, consume_domrand_draws=False)
    env.batch.set_state(flat, flat, np.zeros((E, env.P), dtype=np.uint8))
    _, _, _, info = env.step(only_xy, auto_reset=False)
    env.close()
    assert np.array_equal(info["n_grabbed"], r2["n_grabbed"]) and np.array_equal(info["executed"], r2["executed"])
