"""GPU tests of per-env materials (clothhip_set_material): one handle steps cloths of different fabrics. The six material quantities are what
Cloth.update() reads from the cfg on every call (cloth.pyx:175-186), so the references are the real reference's capture at a non-default
material (g_traj_friction_25), the CPU oracle with a cfg per cloth, and uniform handles built from each material's cfg -- bit for bit in
fp64 and, for the same constants from another source, in fp32 too."""
import numpy as np
import pytest

from helpers import BatchReplay, max_abs
from test_gpu_parity import cfg_from_golden, f32_stated_band

pytestmark = pytest.mark.gpu

FIELDS = ("density", "ks", "damping", "plane_friction", "tear_thresh", "gravity")
FRICTION = dict(ks=7000.0, damping=1.2, plane_friction=0.5)          # what g_traj_friction_25's cfg changes in the default cfg


def material(cfg, **changes):
    m = {k: float(cfg[k]) for k in FIELDS}
    m.update(changes)
    return m


def set_env_material(b, env, m):
    b.set_material(m, env0=env, n=1)


def spec_of(b):
    return b.last_variant()["spec_n_side"]


def checkpoints(b):
    pos, prev, pin = b.get_state()
    return pos, prev, pin.astype(bool), b.tear


def same_as_fixture(g, k, st, e):
    pos, prev, pin, tear = st
    return (np.array_equal(pos[e], g["cp_pos"][k]) and np.array_equal(prev[e], g["cp_prev"][k]) and
            np.array_equal(pin[e], g["cp_pinned"][k].astype(bool)) and bool(tear[e]) == bool(g["cp_tear"][k]))


def oracle_run(oracle_lib, cfg, ops, stop=None):
    """[(pos, prev, pinned, tear)] per checkpoint of an OracleCloth of `cfg` replaying `ops` from the flat grid."""
    oc = oracle_lib.OracleCloth(cfg)
    out = []

    def cp(k):
        pos, prev, pin = oc.get_state()
        out.append((pos.copy(), prev.copy(), pin.astype(bool), oc.have_tear))
    oracle_lib.replay_ops(oc, ops, cp, stop=stop)
    return out


# ---- 1. the real reference's capture at a non-default material, on one env of a default handle ----------------------------------------------
@pytest.mark.parametrize("lean", [None, 0])
def test_one_env_of_a_default_handle_replays_the_friction_capture_f64(lean, oracle_lib, monkeypatch):
    """A handle of the default cfg, E = 3; env 1 holds ks 7000, damping 1.2, friction 0.5 and must equal the reference's capture of that
    cfg at all nine checkpoints, bit for bit; envs 0 and 2 must equal a uniform default handle replaying the same ops. (The oracle with
    the default material is 5.8e-3 off the capture at the third checkpoint: a kernel that ignores the table fails.) On the default plan
    (the fp64 LEAN build, which has a grid-specialised build: the uniform handle runs it, the mixed one must not) and on the standard
    build (CLOTHHIP_DEBUG_LEAN=0, which has no specialised fp64 build: both run the generic one)."""
    from gym_cloth_amd import ClothBatch
    if lean is None:
        monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    else:
        monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", str(lean))
    monkeypatch.delenv("CLOTHHIP_DEBUG_NOSPEC", raising=False)
    g = oracle_lib.load_golden("g_traj_friction_25.npz")
    base = oracle_lib.load_golden("g_traj_lift_pull_25.npz")["cfg"]
    mixed = ClothBatch(cfg_from_golden({"cfg": base}), n_envs=3, precision="f64")
    uni = ClothBatch(cfg_from_golden({"cfg": base}), n_envs=1, precision="f64")
    set_env_material(mixed, 1, material(base, **FRICTION))
    states = {}
    for name, b in (("mixed", mixed), ("uni", uni)):
        got = states[name] = []
        oracle_lib.replay_ops(BatchReplay(b), g["ops"], lambda k, b=b, got=got: got.append(checkpoints(b)))
    assert len(states["mixed"]) == len(g["cp_pos"]) == 9
    bad = [k for k in range(9) if not same_as_fixture(g, k, states["mixed"][k], 1)]
    assert not bad, [(k, max_abs(states["mixed"][k][0][1], g["cp_pos"][k])) for k in bad]
    assert max_abs(states["uni"][2][0][0], g["cp_pos"][2]) > 1e-3             # ... and the default material does not give the capture
    for k in range(9):
        for e in (0, 2):
            assert all(np.array_equal(states["mixed"][k][q][e], states["uni"][k][q][0]) for q in range(4)), (k, e)
    assert mixed.last_variant()["lean"] == uni.last_variant()["lean"] == (lean is None)
    assert spec_of(mixed) == 0
    assert spec_of(uni) == (25 if lean is None else 0)
    mixed.close(); uni.close()


# ---- 2. every field alone -----------------------------------------------------------------------------------------------------------------------
ONE_FIELD = [dict(), dict(density=150.0), dict(ks=6000.0), dict(damping=3.5), dict(plane_friction=0.7), dict(tear_thresh=1.05),
             dict(gravity=-4.9),
             dict(density=150.0, ks=6000.0, damping=3.5, plane_friction=0.7, tear_thresh=1.6, gravity=-4.9)]


@pytest.fixture(scope="module")
def tear_reference(oracle_lib):
    """The oracle's six checkpoints of g_traj_tear_25's ops for each of the eight materials (computed once, never modified)."""
    g = oracle_lib.load_golden("g_traj_tear_25.npz")
    refs = []
    for ch in ONE_FIELD:
        cfg = dict(g["cfg"]); cfg.update(ch)
        refs.append(oracle_run(oracle_lib, cfg, g["ops"]))
    return g, refs


def test_the_oracle_separates_the_eight_materials(tear_reference):
    """What makes the next test non-vacuous, asserted on the oracle's output alone (needs no GPU work): when each material tears, how far
    each one-field change moves the cloth, and that the tear_thresh 1.05 env differs from the default one in its flag only (the
    `tear_thresh < 1.1` branch of cloth.pyx:272-275)."""
    g, refs = tear_reference
    assert all(len(r) == 6 for r in refs)
    first_tear = [next((k for k in range(6) if r[k][3]), None) for r in refs]
    assert first_tear == [4, None, 4, 4, None, 2, None, 4], first_tear
    for e in (1, 2, 3, 4, 6):
        assert max_abs(refs[e][5][0], refs[0][5][0]) >= 2.6e-2, (e, max_abs(refs[e][5][0], refs[0][5][0]))
    assert np.array_equal(refs[5][5][0], refs[0][5][0]) and np.array_equal(refs[5][5][1], refs[0][5][1])
    assert [r[3] for r in refs[5]] != [r[3] for r in refs[0]]


def test_every_material_field_alone_matches_its_oracle_f64(tear_reference, oracle_lib):
    """E = 8: the default material, each of the six fields changed alone, all six changed. Every env must match an OracleCloth of its own
    cfg at every checkpoint, bit for bit: positions, previous positions, pinned, tear flag."""
    from gym_cloth_amd import ClothBatch
    g, refs = tear_reference
    b = ClothBatch(cfg_from_golden(g), n_envs=8, precision="f64")
    mats = np.zeros(8, dtype=b.get_material().dtype)
    for e, ch in enumerate(ONE_FIELD):
        for k, v in material(g["cfg"], **ch).items():
            mats[k][e] = v
    b.set_material(mats)
    got = []
    oracle_lib.replay_ops(BatchReplay(b), g["ops"], lambda k: got.append(checkpoints(b)))
    bad = []
    for k in range(6):
        pos, prev, pin, tear = got[k]
        for e in range(8):
            r = refs[e][k]
            if not (np.array_equal(pos[e], r[0]) and np.array_equal(prev[e], r[1]) and np.array_equal(pin[e], r[2]) and bool(tear[e]) == r[3]):
                bad.append((k, e, max_abs(pos[e], r[0]), max_abs(prev[e], r[1]), bool(tear[e]), r[3]))
    assert not bad, bad[:8]
    assert spec_of(b) == 0
    b.close()


# ---- 3. fp32 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lean", [None, 3])
def test_f32_material_env_is_bit_identical_to_a_uniform_handle_of_that_cfg(lean, oracle_lib, monkeypatch):
    """The same arithmetic with the same constants from another source gives the same bits: env 1 of a default fp32 handle holding the
    friction fixture's material against a uniform fp32 handle created from the fixture's cfg (same batch size, so the same variant --
    asserted first). lean 3: the four-wave family."""
    from gym_cloth_amd import ClothBatch
    if lean is None:
        monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    else:
        monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", str(lean))
    g = oracle_lib.load_golden("g_traj_friction_25.npz")
    base = oracle_lib.load_golden("g_traj_lift_pull_25.npz")["cfg"]
    mixed = ClothBatch(cfg_from_golden({"cfg": base}), n_envs=3, precision="f32")
    uni = ClothBatch(cfg_from_golden(g), n_envs=3, precision="f32")
    set_env_material(mixed, 1, material(base, **FRICTION))
    states = {}
    for name, b in (("mixed", mixed), ("uni", uni)):
        got = states[name] = []
        oracle_lib.replay_ops(BatchReplay(b), g["ops"], lambda k, b=b, got=got: got.append(checkpoints(b)))
    assert mixed.last_variant() == uni.last_variant(), (mixed.last_variant(), uni.last_variant())
    if lean == 3:
        assert mixed.last_variant()["threads"] == 256 and mixed.last_variant()["lean"], mixed.last_variant()
    assert len(states["mixed"]) == 9
    for k in range(9):
        for q in range(4):
            assert np.array_equal(states["mixed"][k][q][1], states["uni"][k][q][1]), (k, q)
    assert max_abs(states["mixed"][8][0][0], states["mixed"][8][0][1]) > 1e-3        # the default envs beside it went elsewhere
    mixed.close(); uni.close()


def test_f32_material_env_stays_in_the_stated_bands_teacher_forced(oracle_lib, monkeypatch):
    """Env 1 of the mixed fp32 handle, restarted from every checkpoint of the reference's friction capture and run to the next one: within
    the band stated for the window's length (test_gpu_parity.f32_stated_band, the friction fixture's row)."""
    from gym_cloth_amd import ClothBatch
    monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    name = "g_traj_friction_25.npz"
    g = oracle_lib.load_golden(name)
    base = oracle_lib.load_golden("g_traj_lift_pull_25.npz")["cfg"]
    b = ClothBatch(cfg_from_golden({"cfg": base}), n_envs=3, precision="f32")
    set_env_material(b, 1, material(base, **FRICTION))
    rp = BatchReplay(b)
    ops = g["ops"]
    cps = [i for i, op in enumerate(ops) if op[0] == "checkpoint"]
    worst = []
    for k in range(len(cps) - 1):
        seg = ops[cps[k] + 1:cps[k + 1]]
        nsub = sum(op[-1] for op in seg if op[0] in ("update", "adjust_update"))
        if nsub == 0 or nsub > 200 or any(op[0] == "pin" for op in seg):
            continue
        b.set_state(g["cp_pos"][k], g["cp_prev"][k], g["cp_pinned"][k], g["rest"])
        oracle_lib.replay_ops(rp, seg)
        worst.append((k, nsub, max_abs(b.positions(1, 1)[0], g["cp_pos"][k + 1]), f32_stated_band(name, nsub)))
    print("\nfp32 windows of the material env: %s" % ["cp%d n=%d err=%.2e band=%.0e" % w for w in worst])
    assert len(worst) >= 5
    assert all(w[2] <= w[3] for w in worst), worst
    assert np.array_equal(b.get_material(1, 1)["ks"], [7000.0])                       # set_state kept the material
    b.close()


# ---- 4. the large-grid family -----------------------------------------------------------------------------------------------------------------
def test_large_grid_family_reads_the_table_f64(oracle_lib):
    """50x50, E = 2, env 1 with ks x 0.8 and damping 3.0, the ops of g_traj_fold_50 up to its third checkpoint: both envs match their
    oracle cloths bit for bit."""
    from gym_cloth_amd import ClothBatch
    g = oracle_lib.load_golden("g_traj_fold_50.npz")
    stop = [i for i, op in enumerate(g["ops"]) if op[0] == "checkpoint"][2] + 1
    changes = [dict(), dict(ks=g["cfg"]["ks"] * 0.8, damping=3.0)]
    refs = []
    for ch in changes:
        cfg = dict(g["cfg"]); cfg.update(ch)
        refs.append(oracle_run(oracle_lib, cfg, g["ops"], stop=stop))
    assert len(refs[0]) == 3 and max_abs(refs[0][2][0], refs[1][2][0]) > 1e-6
    b = ClothBatch(cfg_from_golden(g), n_envs=2, precision="f64")
    set_env_material(b, 1, material(g["cfg"], **changes[1]))
    got = []
    oracle_lib.replay_ops(BatchReplay(b), g["ops"], lambda k: got.append(checkpoints(b)), stop=stop)
    assert b.last_variant()["threads"] * b.last_variant()["particles_per_thread"] >= 2500 and spec_of(b) == 0
    for k in range(3):
        pos, prev, pin, tear = got[k]
        for e in range(2):
            r = refs[e][k]
            assert np.array_equal(pos[e], r[0]) and np.array_equal(prev[e], r[1]), (k, e, max_abs(pos[e], r[0]))
            assert np.array_equal(pin[e], r[2]) and bool(tear[e]) == r[3], (k, e)
    b.close()


# ---- 5. episode launches ------------------------------------------------------------------------------------------------------------------------
EP_MATERIALS = [dict(), dict(ks=7000.0, damping=1.2, plane_friction=0.5), dict(density=150.0, tear_thresh=1.6),
                dict(ks=13000.0, damping=3.0, plane_friction=0.8)]
EP_KEYS = ("rew", "done", "ran", "executed", "n_grabbed", "reset_before", "reset_substeps", "actual_coverage", "start_coverage",
           "variance_inv", "start_variance_inv", "have_tear", "out_of_bounds", "num_steps", "num_sim_steps")


def _episode_env(E, changes, seeds):
    import bench
    from gym_cloth_amd.envs import ClothVecEnv
    cfg = bench.bench_cfg(25, 0.02, "tier1")
    cfg["env"]["max_actions"] = 2
    if len(changes) == 1:                       # a uniform handle built from the material's cfg
        cfg["cloth"].update(changes[0])
    env = ClothVecEnv(cfg, n_envs=E, precision="f64", consume_domrand_draws=False)
    for e in range(E):
        env.np_randoms[e] = np.random.RandomState(seeds[e])
    if len(changes) > 1:
        for e, ch in enumerate(changes):
            env.set_material([e], **ch)
    return env


def test_step_many_on_a_mixed_handle_equals_sequential_steps_and_uniform_handles_f64():
    """E = 4 with four materials, max_actions 2 and three action slots (every env resets inside the launch), table policy: the launch
    equals the same actions through sequential step(auto_reset=True) calls on a second mixed handle, and each env equals a uniform
    single-env handle built from its material's cfg -- records, reset records and final particles, bit for bit."""
    E, T = 4, 3
    acts = np.stack([np.random.RandomState(2000 + e).uniform(-1, 1, size=(T, 4)) for e in range(E)], axis=1)
    seeds = [1000 + e for e in range(E)]
    a = _episode_env(E, EP_MATERIALS, seeds); a.reset()
    b = _episode_env(E, EP_MATERIALS, seeds); b.reset()
    assert np.array_equal(a.batch.get_state()[0], b.batch.get_state()[0])
    seq = [a.step(acts[t], auto_reset=True) for t in range(T)]
    out = b.step_many(acts, reset_tail=True)
    assert b.batch.last_variant()["spec_n_side"] == 0
    assert out["ran"].all() and (out["reset_before"].sum(axis=0) >= 1).all(), out["reset_before"]
    for t in range(T):
        obs, rew, done, info = seq[t]
        assert np.array_equal(rew, out["rew"][t]) and np.array_equal(done, out["done"][t]), t
        assert np.array_equal(info["executed"], out["executed"][t]) and np.array_equal(info["n_grabbed"], out["n_grabbed"][t]), t
        for k in ("num_steps", "num_sim_steps", "actual_coverage", "start_coverage", "variance_inv", "start_variance_inv", "have_tear",
                  "out_of_bounds"):
            assert np.array_equal(np.asarray(info[k]), out[k][t]), (t, k)
    sa, sb = a.batch.get_state(), b.batch.get_state()
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb)) and np.array_equal(a.batch.tear, b.batch.tear)
    assert np.array_equal(a.material, b.material) and len({m.tobytes() for m in b.material}) == 4      # the resets kept the materials
    # the materials matter: no two envs given the SAME action stream would agree -- here they get different streams, so pin each env to
    # a uniform handle of its own cfg instead
    for e in range(E):
        u = _episode_env(1, [EP_MATERIALS[e]], [seeds[e]]); u.reset()
        ou = u.step_many(acts[:, e:e + 1], reset_tail=True)
        for k in EP_KEYS:
            assert np.array_equal(ou[k][:, 0], out[k][:, e]), (e, k, ou[k][:, 0], out[k][:, e])
        su = u.batch.get_state()
        assert all(np.array_equal(x[0], y[e]) for x, y in zip(su, sb)), e
        u.close()
    a.close(); b.close()


# ---- 6. the surface -----------------------------------------------------------------------------------------------------------------------------
def test_material_surface_round_trip_clear_validation_and_persistence(monkeypatch):
    from gym_cloth_amd import ClothBatch, ClothHipError
    import bench
    monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    monkeypatch.delenv("CLOTHHIP_DEBUG_NOSPEC", raising=False)
    cfg = bench.bench_cfg(25, 0.02)
    b = ClothBatch(cfg, n_envs=4, precision="f64")
    own = b.get_material()
    assert own.shape == (4,) and own.dtype.names == FIELDS
    assert own[0].tolist() == (200.0, 10000.0, 2.0, 1.0, 2.0, -9.8) and all(own[e] == own[0] for e in range(4))
    m = own[1:3].copy()
    m["ks"] = [7000.0, 8000.0]; m["gravity"] = [-4.9, -9.8]
    b.set_material(m, env0=1)
    assert np.array_equal(b.get_material(1, 2), m) and np.array_equal(b.get_material()[[0, 3]], own[[0, 3]])
    b.update(2)
    assert spec_of(b) == 0
    # a structured array with the fields in another order is taken by name, not by position
    swapped = np.zeros(2, dtype=[(k, "<f8") for k in reversed(FIELDS)])
    for k in FIELDS:
        swapped[k] = m[k]
    swapped["damping"] = [1.5, 2.5]
    b.set_material(swapped, env0=1)
    m["damping"] = [1.5, 2.5]
    assert np.array_equal(b.get_material(1, 2), m)
    # bad values and ranges: CLOTHHIP_EINVAL (ValueError), nothing changed
    before = b.get_material()
    bad = own[:2].copy(); bad["density"][1] = 0.0
    for call in (lambda: b.set_material(bad, env0=0), lambda: b.set_material(own[:2], env0=3, n=2), lambda: b.set_material(own[:1], env0=-1),
                 lambda: b.get_material(2, 3)):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(b.get_material(), before)
    # set_state and reset_flat keep the material; a material equal to the handle's is no material
    pos, prev, pin = b.get_state()
    b.set_state(pos, prev, pin)
    b.reset_flat()
    assert np.array_equal(b.get_material(), before)
    b.set_material(own[:1], env0=2)
    b.update(1)
    assert spec_of(b) == 0                                       # env 1 still holds one
    b.set_material(None, env0=1, n=1)
    assert np.array_equal(b.get_material(), own)
    b.update(1)
    assert spec_of(b) == 25                                      # cleared: the grid-specialised build is back
    b.close()
    # the relaxed-order companion is bench-only: with a material, episode launches are refused
    from gym_cloth_amd.envs import ClothVecEnv
    v = ClothVecEnv(cfg, n_envs=2, precision="f32", consume_domrand_draws=False)
    v.seed(5); v.reset()
    v.set_material([1], ks=8000.0)
    v.batch.set_relaxed_order(True)
    with pytest.raises(ClothHipError, match=r"^\[-5\]"):
        v.step_many(np.zeros((1, 2, 4)))
    v.close()


def test_randomize_material_is_reproducible_and_leaves_the_reset_streams_alone():
    import bench
    from gym_cloth_amd.envs import ClothVecEnv, ClothEnv
    cfg = bench.bench_cfg(25, 0.02)
    ranges = {"ks": (7000.0, 13000.0), "damping": (1.4, 2.6)}
    tables = []
    for trial in range(2):
        v = ClothVecEnv(cfg, n_envs=4, precision="f64", consume_domrand_draws=False)
        v.seed(11)
        before = [r.get_state() for r in v.np_randoms]
        t = v.randomize_material(ranges, seed=42, envs=[1, 2, 3])
        after = [r.get_state() for r in v.np_randoms]
        assert all(x[0] == y[0] and np.array_equal(x[1], y[1]) and x[2:] == y[2:] for x, y in zip(before, after))
        assert t.flags.writeable is False and np.array_equal(t, v.batch.get_material())
        assert t[0].tolist() == (200.0, 10000.0, 2.0, 1.0, 2.0, -9.8)
        assert ((t["ks"][1:] >= 7000.0) & (t["ks"][1:] < 13000.0) & (t["damping"][1:] >= 1.4) & (t["damping"][1:] < 2.6)).all()
        assert len(set(t["ks"][1:].tolist())) == 3 and (t["density"] == 200.0).all()
        tables.append(t.copy())
        if trial == 1:
            assert not np.array_equal(v.randomize_material(ranges, seed=43)["ks"], t["ks"])
            with pytest.raises(ValueError):
                v.set_material(stiffness=1.0)
        v.close()
    assert np.array_equal(tables[0], tables[1])
    s = ClothEnv(cfg, precision="f64")
    s.set_material(ks=9000.0, plane_friction=0.9)
    assert s.material["ks"] == 9000.0 and s.material["plane_friction"] == 0.9 and s.material["density"] == 200.0
    s.close()


def test_two_runs_of_a_mixed_handle_are_bit_identical(oracle_lib):
    from gym_cloth_amd import ClothBatch
    g = oracle_lib.load_golden("g_traj_lift_pull_25.npz")
    stop = [i for i, op in enumerate(g["ops"]) if op[0] == "checkpoint"][9] + 1
    outs = []
    for trial in range(2):
        b = ClothBatch(cfg_from_golden(g), n_envs=5, precision="f32")
        for e, ch in enumerate(ONE_FIELD[1:5]):
            set_env_material(b, e + 1, material(g["cfg"], **ch))
        oracle_lib.replay_ops(BatchReplay(b), g["ops"], stop=stop)
        outs.append(checkpoints(b))
        b.close()
    assert all(np.array_equal(x, y) for x, y in zip(*outs))
    assert all(max_abs(outs[0][0][e], outs[0][0][0]) > 1e-4 for e in range(1, 5))
