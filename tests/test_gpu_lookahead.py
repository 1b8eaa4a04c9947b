"""GPU tests of ClothVecEnv.snapshot / restore / lookahead / commit and of LookaheadPolicy: everything is pinned to what the env itself does
without them -- a twin env put into the same state and stepped the ordinary way -- bit for bit, in fp64 and (same stepper variant asserted)
in fp32; one case is anchored in the reference's own episode capture."""
import numpy as np
import pytest

from test_gpu_env import base_cfg
from test_gpu_fork import full_state, same_cloth

pytestmark = pytest.mark.gpu

HOST_ARRAYS = ("num_steps", "num_sim_steps", "have_tear", "_prev_reward", "_start_coverage", "_start_variance_inv", "_current_coverage",
               "_iters_up_env", "init_side", "_ep_done", "last_executed", "last_grabbed", "last_iters_pull")
INFO_KEYS = ("num_steps", "num_sim_steps", "actual_coverage", "start_coverage", "variance_inv", "start_variance_inv", "have_tear",
             "out_of_bounds", "executed", "n_grabbed")
LOOK_KEYS = ("actual_coverage", "variance_inv", "out_of_bounds", "have_tear", "executed", "n_grabbed")
MANY_KEYS = ("rew", "done", "ran", "executed", "n_grabbed", "reset_before", "reset_substeps", "actual_coverage", "start_coverage",
             "variance_inv", "start_variance_inv", "have_tear", "out_of_bounds", "num_steps", "num_sim_steps", "obs", "actions")


def make_env(E, prec, tier="tier1", seeds=None, domrand=False, **env_changes):
    import bench
    from gym_cloth_amd.envs import ClothVecEnv
    cfg = bench.bench_cfg(25, 0.02, tier)
    cfg["env"].update(env_changes)
    env = ClothVecEnv(cfg, n_envs=E, precision=prec, consume_domrand_draws=domrand)
    for e in range(E):
        env.np_randoms[e] = np.random.RandomState((1000 + e) if seeds is None else seeds[e])
    return env


def rng_states(env):
    return [r.get_state() for r in env.np_randoms]


def rng_equal(sa, sb):
    return all(a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:] for a, b in zip(sa, sb))


def whole_env(env):
    return ([full_state(env.batch, e) for e in range(env.E)], env.batch.get_material(), {k: np.array(getattr(env, k)) for k in HOST_ARRAYS},
            rng_states(env))


def same_env(x, y):
    return (all(same_cloth(p, q) for p, q in zip(x[0], y[0])) and np.array_equal(x[1], y[1]) and
            all(np.array_equal(x[2][k], y[2][k]) for k in HOST_ARRAYS) and rng_equal(x[3], y[3]))


def branch_equals_step(out, k, stepped):
    obs, rew, done, info = stepped
    assert np.array_equal(out["rew"][:, k], rew) and np.array_equal(out["done"][:, k], done), (k, out["rew"][:, k], rew)
    for key in LOOK_KEYS:
        assert np.array_equal(out[key][:, k], np.asarray(info[key])), (k, key, out[key][:, k], info[key])


# ---- 1. lookahead == step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_lookahead_equals_step_and_leaves_the_env_alone(prec, monkeypatch):
    monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    E, K = 3, 4
    env = make_env(E, prec); env.reset()
    env.set_material([2], ks=8000.0, damping=1.5)                            # a branch must carry its env's fabric
    warm = np.random.RandomState(5).uniform(-0.6, 0.6, size=(2, E, 4))
    for t in range(2):
        env.step(warm[t])
    cand = np.random.RandomState(6).uniform(-1, 1, size=(E, K, 4))
    snap = env.snapshot()
    before = whole_env(env)
    substeps = env.total_substeps
    out = env.lookahead(cand)
    assert same_env(before, whole_env(env)) and env.total_substeps == substeps
    assert all(out[k].shape == (E, K) for k in ("rew", "done") + LOOK_KEYS)
    assert len(set(out["executed"].ravel().tolist())) > 4                    # the candidates are different pulls
    twin = make_env(E, prec)
    for k in range(K):
        twin.restore(snap)
        assert same_env(before, whole_env(twin))
        stepped = twin.step(cand[:, k])
        if prec == "f32":
            assert twin.batch.last_variant() == env._scratch.last_variant(), (twin.batch.last_variant(), env._scratch.last_variant())
        branch_equals_step(out, k, stepped)
    assert np.array_equal(env.lookahead(cand)["rew"], out["rew"])            # the scratch batch is reused: same answer
    env.close(); twin.close(); snap.close()


# ---- 2. commit == step, anchored in the reference's episode capture ----------------------------------------------------------------------------
@pytest.mark.parametrize("auto_reset", [False, True])
def test_commit_equals_step_f64(auto_reset, oracle_lib):
    """E = 3 seeded 1337, 1338, 1339 as the reference's captures were: env 0 after reset() is the start of g_episodes_tier1_1337, whose
    first action takes the cloth out of bounds and ends the episode. That action is env 0's candidate 2; commit adopts it (the others
    take candidates 0 and 3) and must return what step() returns on a twin -- with auto_reset the twin's reset of env 0 included --,
    and the capture's reward."""
    from gym_cloth_amd.envs import ClothVecEnv
    g = oracle_lib.load_golden("g_episodes_tier1_1337.npz")
    assert bool(g["done"][0]) and g["info"][0]["out_of_bounds"] and int(g["reset_before"][0]) == 1
    E, K = 3, 4
    envs = []
    for _ in range(2):
        v = ClothVecEnv(base_cfg("tier1", 1337), n_envs=E, precision="f64")
        v.seed(1337); v.reset()
        envs.append(v)
    env, twin = envs
    cand = np.random.RandomState(8).uniform(-0.7, 0.7, size=(E, K, 4))
    cand[0, 2] = g["act"][0]
    choice = np.array([2, 0, 3])
    out = env.lookahead(cand)
    assert out["done"][0, 2] and out["out_of_bounds"][0, 2] and out["rew"][0, 2] == g["rew"][0]
    got = env.commit(choice, auto_reset=auto_reset)
    want = twin.step(cand[np.arange(E), choice], auto_reset=auto_reset)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[2][0] and got[1][0] == g["rew"][0]
    assert set(got[3]) == set(want[3]) and ("reset_mask" in got[3]) == auto_reset
    for k in got[3]:
        assert np.array_equal(np.asarray(got[3][k]), np.asarray(want[3][k])), k
    for e in range(E):
        assert out["rew"][e, choice[e]] == got[1][e] and out["done"][e, choice[e]] == got[2][e]
    assert same_env(whole_env(env), whole_env(twin)) and env.total_substeps == twin.total_substeps
    nxt = np.random.RandomState(9).uniform(-0.5, 0.5, size=(E, 4))           # ... and they stay together
    a, b = env.step(nxt), twin.step(nxt)
    assert np.array_equal(a[1], b[1]) and same_env(whole_env(env), whole_env(twin))
    env.close(); twin.close()


# ---- 3. commit needs the env untouched since the lookahead ------------------------------------------------------------------------------------
def test_commit_after_any_change_raises():
    E, K = 2, 2
    env = make_env(E, "f64"); env.reset()
    snap = env.snapshot()
    cand = np.random.RandomState(3).uniform(-0.5, 0.5, size=(E, K, 4))
    zero = np.zeros(E, dtype=np.int64)
    with pytest.raises(RuntimeError):
        env.commit(zero)                                                     # nothing to commit yet
    changes = [lambda: env.step(cand[:, 1]), lambda: env.step_many(cand[:, :1].transpose(1, 0, 2).copy()), lambda: env.reset(mask=[True, False]),
               lambda: env.restore(snap), lambda: env.restore(snap, envs=[1]), lambda: env.set_material([0], ks=9000.0),
               lambda: env.seed(3)]
    for change in changes:
        env.lookahead(cand)
        change()
        with pytest.raises(RuntimeError, match="changed since the last lookahead"):
            env.commit(zero)
    env.lookahead(cand)
    for bad in (np.array([0, 2]), np.array([0]), np.array([0.0, 1.0])):
        with pytest.raises(ValueError):
            env.commit(bad)
    env.commit(zero)
    with pytest.raises(RuntimeError):
        env.commit(zero)                                                     # a lookahead is adopted once
    with pytest.raises(ValueError):
        env.lookahead(cand[:1])
    env.close(); snap.close()


# ---- 4. snapshot / restore ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["tier1", "tier2", "tier3"])
def test_restore_replays_a_launch_with_resets_bit_for_bit_f64(tier):
    """step_many over actions that end episodes inside the launch (the kernel draws the resets from the envs' numpy streams; tier 2
    rebuilds the env's sheet and rest lengths), restore, the same call again: every output and every stream equal. Then a subset."""
    E, T = (4, 4) if tier == "tier1" else (3, 3)
    acts = np.stack([np.random.RandomState(2000 + e).uniform(-1, 1, size=(T, 4)) for e in range(E)], axis=1)
    env = make_env(E, "f64", tier, max_actions=2); env.reset()
    snap = env.snapshot()
    at_snap = whole_env(env)
    rest_at_snap = env.batch.get_rest()
    out1 = env.step_many(acts)
    assert out1["reset_before"].sum() > 0, "an env must reset inside the launch"
    after1 = whole_env(env)
    assert not rng_equal(at_snap[3], after1[3])
    env.restore(snap)
    assert same_env(at_snap, whole_env(env)) and np.array_equal(env.batch.get_rest(), rest_at_snap)
    out2 = env.step_many(acts)
    for k in MANY_KEYS:
        assert np.array_equal(out1[k], out2[k]), k
    assert same_env(after1, whole_env(env))
    env.restore(snap, envs=[1])                                              # a subset: env 1 back, the others where they were
    now = whole_env(env)
    for e in range(E):
        ref = at_snap if e == 1 else after1
        assert same_cloth(now[0][e], ref[0][e]) and all(np.array_equal(now[2][k][e], ref[2][k][e]) for k in HOST_ARRAYS), e
        assert rng_equal([now[3][e]], [ref[3][e]]), e
    env.close(); snap.close()


def test_single_env_snapshot_and_restore_f64():
    from gym_cloth_amd.envs import ClothEnv
    env = ClothEnv(base_cfg("tier1", 1337), precision="f64")
    env.seed(1337); env.reset()
    snap = env.snapshot()
    a = env.step(np.array([0.1, -0.2, 0.3, 0.2]))
    env.restore(snap)
    b = env.step(np.array([0.1, -0.2, 0.3, 0.2]))
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]
    env.close(); snap.close()


# ---- 5. force_grab and per-env iters_up ----------------------------------------------------------------------------------------------------------
def test_lookahead_with_force_grab_and_per_env_iters_up_f64():
    """tier 3, force_grab on, the envs holding different (fractional) iters_up as during a tier-3 reset pull (cloth_env.py:960): the
    branches decode with their env's value and run the radius loop; candidate 1 picks at the plane's corner, off the cloth."""
    E, K = 2, 2
    env = make_env(E, "f64", "tier3", force_grab=True); env.reset()
    env._iters_up_env = np.array([230.5, 261.25])
    pos, prev, _ = env.batch.get_state()                                     # the cloths moved off the plane's (1, 1) corner
    shift = np.array([-0.2, -0.2, 0.0])
    env.batch.set_state(pos + shift, prev + shift, keep_tear=True)
    cand = np.random.RandomState(4).uniform(-0.5, 0.5, size=(E, K, 4))
    cand[:, 1, :2] = 1.0
    snap = env.snapshot()
    out = env.lookahead(cand)
    assert (out["n_grabbed"] > 0).all() and (out["executed"] > 0).all()
    twin = make_env(E, "f64", "tier3", force_grab=True)
    twin.restore(snap)
    assert np.array_equal(twin._iters_up_env, [230.5, 261.25])
    plain = make_env(E, "f64", "tier3"); plain.restore(snap)
    assert (plain.step(cand[:, 1])[3]["n_grabbed"] == 0).all()               # without force_grab that pick holds nothing
    branch_equals_step(out, 1, twin.step(cand[:, 1]))
    assert out["executed"][0, 1] != out["executed"][1, 1]                    # 231 vs 262 lift iterations
    env.close(); twin.close(); plain.close(); snap.close()


# ---- 6. LookaheadPolicy in the demonstration writer ---------------------------------------------------------------------------------------------
def test_lookahead_policy_through_collect_demos_f64():
    from gym_cloth_amd.demos import collect_demos
    from gym_cloth_amd.policies import LookaheadPolicy

    class Recording(LookaheadPolicy):
        def __init__(self, *a, **k):
            LookaheadPolicy.__init__(self, *a, **k)
            self.log = []

        def get_action(self, obs=None, t=0):
            snap = self.env.snapshot()
            act = LookaheadPolicy.get_action(self, obs, t)
            self.log.append((snap, self.last_candidates.copy(), self.last_choice.copy(), act.copy(), self.last_lookahead["rew"].copy()))
            return act

    E, K = 2, 3
    env = make_env(E, "f64", max_actions=2)
    pol = Recording(env, n_candidates=K, seed=11)
    episodes = collect_demos(env, pol, max_episodes=2)
    assert len(episodes) == 2
    used = [0] * E
    for ep in episodes:                                                      # the documented layout (analytic.py:866-882)
        n, e = len(ep["act"]), ep["env"]
        assert 1 <= n <= 2 and len(ep["obs"]) == n + 1 and len(ep["rew"]) == len(ep["done"]) == len(ep["info"]) == n
        assert ep["done"][-1] and not any(ep["done"][:-1])
        for i in range(n):                                                   # every stored action is that step's chosen candidate
            snap, cand, choice, act, rew = pol.log[used[e] + i]
            assert ep["act"][i] == tuple(act[e]) == tuple(cand[e, choice[e]])
        used[e] += n
    twin = make_env(E, "f64", max_actions=2)
    for snap, cand, choice, act, rew in pol.log[:3]:                          # ... and the arg-max of its candidates, recomputed
        twin.restore(snap)
        again = twin.lookahead(cand)["rew"]
        assert np.array_equal(again, rew) and np.array_equal(np.argmax(again, axis=1), choice)
        assert (again[np.arange(E), choice] >= again.max(axis=1)).all()
    for rec in pol.log:
        rec[0].close()
    env.close(); twin.close()
