"""The device metrics (csrc/cloth_metrics.hpp: metrics_block) against the exact-rational reference (oracle/metrics_exact.py) computed from
the positions READ BACK from the handle, so the rounding to the handle's precision is part of the input and fp32 out-of-bounds is pinned
too: the stand-alone kernel on hand-made states at every grid class (metrics_states.py), the in-launch call in every variant class with both
forms of its hull stack, the reset records, and the 'height' rewards.

Bounds, derived (oracle/metrics_exact.py), never measured:
  coverage      |cov - exact| <= 8 (k + 1) 2^-53, k the hull's vertex count; == float(exact) where the coordinates are dyadic, == 0.0 where
                the hull is degenerate by construction; == clothhip_hull_area(clipped read-back xy) bit for bit on every state
  variance_inv  relative 4 P 2^-53 where var >= 1e-6, == 1000.0 below
  out_of_bounds, n_below_half_thickness   equal

MEASURED on an MI355X (every test prints its own line, `pytest -s`); the bounds above stay as derived, they are not tightened to these:
  stand-alone   |cov - exact| <= 1.74e-15 (50x50 fp64, the circle of 2500 vertices: bound 2.2e-12), at most 1.3 % of the bound on any state;
                variance_inv relative <= 3.4e-16 (64x64 fp32: bound 1.8e-12), at most 6.4 % of the bound (3x3: bound 4.0e-15)
  in-launch     |cov - exact| <= 9.8e-17 (33x33 fp64, hull stack of indices), at most 0.64 % of the bound; variance_inv relative <= 2.8e-16,
                at most 0.36 % of the bound (12x12)
  reset records |cov - exact| <= 1.8e-16 (0.79 % of the bound), variance_inv relative <= 2.6e-16 (0.094 %)
  Every equality (host routine, stand-alone kernel against in-launch call, dyadic and degenerate states, both flags, the count) held exactly.
"""
import numpy as np
import pytest

from metrics_states import GRIDS, check_non_vacuity, exact, host_hull_area, states, thickness_of
from oracle import metrics_exact
from oracle.metrics_exact import Fraction

pytestmark = pytest.mark.gpu


def _cfg(n_side, thickness, tier="tier1"):
    import bench
    return bench.bench_cfg(n_side, thickness, tier)


def _check_against_exact(tag, pos, thickness, cov, vinv, oob, nlow, stats):
    """One env's four numbers against the exact reference of the state `pos` (float64 [P, 3], read back). Returns the reference."""
    P = len(pos)
    ex = exact(pos, thickness)
    dcov = abs(float(Fraction(float(cov)) - ex.area))
    stats["cov"] = max(stats.get("cov", 0.0), dcov)
    stats["cov_vs_bound"] = max(stats.get("cov_vs_bound", 0.0), dcov / metrics_exact.coverage_bound(ex.k))
    assert dcov <= metrics_exact.coverage_bound(ex.k), (tag, dcov, ex.k)
    assert cov == host_hull_area(pos), (tag, cov)                    # the same arithmetic as the host routine
    if ex.var < metrics_exact._VAR_MIN:
        assert vinv == 1000.0, (tag, vinv)
    else:
        rel = abs(float(Fraction(float(vinv)) / ex.variance_inv - 1))
        stats["vinv_rel"] = max(stats.get("vinv_rel", 0.0), rel)
        stats["vinv_vs_bound"] = max(stats.get("vinv_vs_bound", 0.0), rel / metrics_exact.variance_inv_rel_bound(P))
        assert rel <= metrics_exact.variance_inv_rel_bound(P), (tag, rel)
    assert bool(oob) == ex.oob, (tag, oob, ex.oob)
    assert int(nlow) == ex.n_below, (tag, nlow, ex.n_below)
    return ex


# ---- the stand-alone kernel on hand-made states ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_side,prec", GRIDS)
def test_standalone_metrics_on_hand_made_states(n_side, prec):
    """k_metrics (256 threads, hull stack of doubles), one ClothBatch per (grid, precision) with every hand-made state as one env and one
    metrics(want_height=True) call: the deep hull stack (every particle a vertex), dyadic lattice, degenerate hulls, a disc across two clip
    edges, particle order, signed zeros, every out-of-bounds / z / variance / height threshold from both sides."""
    from gym_cloth_amd import ClothBatch
    sts = states(n_side, prec)
    thick = thickness_of(prec)
    P = n_side * n_side
    b = ClothBatch(_cfg(n_side, thick), n_envs=len(sts), precision=prec)
    allpos = np.stack([s.pos for s in sts])
    b.set_state(allpos, allpos, np.zeros((len(sts), P), dtype=np.uint8))
    cov, vinv, oob, tear, height = b.metrics(want_height=True)
    pos = b.positions()
    b.close()
    nlow = np.rint(height * P).astype(np.int64)
    assert np.array_equal(nlow / float(P), height) and not tear.any()
    stats, by_name = {}, {}
    for i, st in enumerate(sts):
        ex = exact(pos[i], thick)
        check_non_vacuity(st, pos[i], ex, prec)                      # on what the device holds
        _check_against_exact((n_side, prec, st.name), pos[i], thick, cov[i], vinv[i], oob[i], nlow[i], stats)
        if st.dyadic:
            assert cov[i] == float(ex.area), (st.name, cov[i], float(ex.area))
        if st.zero_area:
            assert cov[i] == 0.0, (st.name, cov[i])
        by_name[st.name] = i
    for shape in ("circle", "disc"):                                  # particle order: the same bits of coverage (the z-sum may differ in its last bits)
        a, d, s = (by_name[shape + sfx] for sfx in ("_asc", "_desc", "_shuf"))
        assert cov[a] == cov[d] == cov[s], (shape, cov[a], cov[d], cov[s])
        assert oob[a] == oob[d] == oob[s] and nlow[a] == nlow[d] == nlow[s]
    print("MEASURED standalone %dx%d %s: %s" % (n_side, n_side, prec, " ".join("%s=%.3e" % kv for kv in sorted(stats.items()))))


# ---- the in-launch metrics in every variant class -------------------------------------------------------------------------------------
_SWITCHES = ("CLOTHHIP_DEBUG_LEAN", "CLOTHHIP_DEBUG_NOSPEC", "CLOTHHIP_DEBUG_LARGE2", "CLOTHHIP_DEBUG_W8", "CLOTHHIP_DEBUG_NT1024",
             "CLOTHHIP_DEBUG_TAB_LDS", "CLOTHHIP_DEBUG_REST_REG", "CLOTHHIP_DEBUG_COLD", "CLOTHHIP_DEBUG_PHASES")

# Env seeds per grid (env i: RandomState(1000 + s) draws its reset, RandomState(2000 + s) its action, the benchmark's kind), chosen so that
# the state after reset + one action has, among the six envs, a coordinate outside [0, 1], an out-of-bounds env beside one in bounds, and a
# hull of six vertices or more. The test asserts these itself.
_SEEDS = {(25, "f32"): (0, 5, 8, 20, 1, 12), (25, "f64"): (0, 5, 8, 20, 1, 12), (12, "f32"): (0, 5, 7, 11, 1, 8), (27, "f64"): (0, 8, 9, 20, 1, 5),
          (33, "f32"): (0, 8, 9, 11, 1, 14), (33, "f64"): (0, 8, 9, 11, 1, 14), (50, "f32"): (0, 15, 26, 6, 1, 27), (50, "f64"): (0, 14, 26, 1, 2, 30),
          (64, "f32"): (0, 24, 10, 1, 2, 3)}
_THICKNESS = {12: 0.02, 25: 0.02, 27: 0.0095, 33: 0.0095, 50: 0.0095, 64: 0.007}

# (id, n_side, precision, switches, hull stack as indices, (threads, particles per thread, table mode, lean) of the kernel that must run)
_LAUNCH_CASES = [
    ("25_f32_lean0", 25, "f32", {"LEAN": "0"}, False, (512, 2, None, False)),
    ("25_f32_lean3", 25, "f32", {"LEAN": "3"}, False, (256, 3, 0, True)),
    ("25_f32_lean4", 25, "f32", {"LEAN": "4"}, False, (256, 3, -1, True)),
    ("25_f32_lean5", 25, "f32", {"LEAN": "5"}, True, (256, 3, -2, True)),
    ("25_f32_lean6", 25, "f32", {"LEAN": "6"}, True, (256, 3, -3, True)),
    ("25_f32_lean8", 25, "f32", {"LEAN": "8"}, False, (512, 2, 2, True)),
    ("25_f32_lean0_nospec", 25, "f32", {"LEAN": "0", "NOSPEC": "1"}, False, (512, 2, None, False)),
    ("25_f64", 25, "f64", {}, False, (512, 2, 0, True)),
    ("12_f32", 12, "f32", {}, False, (512, 2, 2, True)),
    ("27_f64", 27, "f64", {}, False, (512, 2, 0, True)),
    ("33_f32", 33, "f32", {}, False, (1024, 3, 3, True)),
    ("33_f64", 33, "f64", {}, True, (512, 5, 0, False)),
    ("50_f32_large2_0", 50, "f32", {"LARGE2": "0"}, False, (1024, 3, 3, True)),
    ("50_f32_large2_1", 50, "f32", {"LARGE2": "1"}, True, (512, 5, 4, True)),
    ("50_f64", 50, "f64", {}, True, (512, 5, 0, False)),
    ("64_f32", 64, "f32", {}, True, (1024, 4, 3, True)),
]


def _hull_as_indices(v):
    """Variant::hull_as_indices() (csrc/stepper_traits.hpp) from what clothhip_last_variant reports."""
    tsz, slots, tab = (4 if v["precision"] == "f32" else 8), v["threads"] * v["particles_per_thread"], v["table_mode"]
    return tab == 4 or tab <= -2 or (tsz == 8 and slots > 1024) or slots >= 4096


def _seeded_env(n_side, prec, seeds, tier="tier1", **env_cfg):
    from gym_cloth_amd.envs import ClothVecEnv
    cfg = _cfg(n_side, _THICKNESS[n_side], tier)
    cfg["env"].update(env_cfg)
    env = ClothVecEnv(cfg, n_envs=len(seeds), precision=prec, consume_domrand_draws=False)
    for i, s in enumerate(seeds):
        env.np_randoms[i] = np.random.RandomState(1000 + s)
    return env


def _actions(seeds, T=1):
    return np.ascontiguousarray(np.stack([np.random.RandomState(2000 + s).uniform(-1, 1, size=(T, 4)) for s in seeds], axis=1))


def _spy_records(env):
    """The step records of the env's next episode launches, as run_actions_end returns them."""
    got, orig = [], env.batch.run_actions_end

    def spy():
        r = orig()
        got.append(r[0].copy())
        return r
    env.batch.run_actions_end = spy
    return got


@pytest.mark.parametrize("case", _LAUNCH_CASES, ids=[c[0] for c in _LAUNCH_CASES])
def test_in_launch_metrics_match_exact_reference(case, monkeypatch):
    """metrics_block inside the episode launch (the launch's own thread count; hull stack of doubles or of u16 indices): reset, ONE action per
    env with auto_reset off -- so the state left on the handle is the state the metrics saw --, then the record's four numbers against the
    exact reference of that state, and bit for bit against the stand-alone kernel on it."""
    _, n_side, prec, switches, want_idx, (nt, ppt, tab, lean) = case
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in switches.items():
        monkeypatch.setenv("CLOTHHIP_DEBUG_" + k, val)
    seeds = _SEEDS[(n_side, prec)]
    E, P, thick = len(seeds), n_side * n_side, _THICKNESS[n_side]
    env = _seeded_env(n_side, prec, seeds)
    env.reset()
    recs = _spy_records(env)
    out = env.step_many(_actions(seeds), auto_reset=False)
    v = env.batch.last_variant()
    pos = env.batch.positions()
    cov, vinv, oob, tear, height = env.batch.metrics(want_height=True)
    env.close()
    # the intended kernel ran, with the listed form of the hull stack
    assert v["fused"] >= 1 and v["precision"] == prec and v["threads"] == nt and v["particles_per_thread"] == ppt and v["lean"] == lean, v
    assert tab is None or v["table_mode"] == tab, v
    want_spec = 0 if "NOSPEC" in switches else (25 if n_side == 25 else (50 if switches.get("LARGE2") == "1" else 0))
    assert v["spec_n_side"] == want_spec, v                           # the grid-specialised build (25x25; 50x50 at two cloths per CU), or the generic one
    assert _hull_as_indices(v) == want_idx, v
    (rec,) = recs
    r = rec[0]
    assert (r["ran"] == 1).all() and out["ran"].all()
    stats, exs = {}, []
    for e in range(E):
        exs.append(_check_against_exact((case[0], e), pos[e], thick, r["coverage"][e], r["variance_inv"][e], r["oob"][e],
                                        r["n_below_half_thickness"][e], stats))
    # ... and independent of NT and of the stack's form: the stand-alone kernel's bits
    assert np.array_equal(r["coverage"], cov) and np.array_equal(r["variance_inv"], vinv)
    assert np.array_equal(r["oob"] != 0, oob) and np.array_equal(r["n_below_half_thickness"] / float(P), height)
    assert np.array_equal(out["actual_coverage"][0], cov) and np.array_equal(out["out_of_bounds"][0], oob)
    # the case is not vacuous
    assert any((pos[e][:, :2] < 0).any() or (pos[e][:, :2] > 1).any() for e in range(E))
    assert any(ex.oob for ex in exs) and not all(ex.oob for ex in exs)
    assert max(ex.k for ex in exs) >= 6
    assert any(0 < ex.n_below < P for ex in exs)
    print("MEASURED in-launch %s (%s, hull stack of %s): %s" % (case[0], v["name"], "indices" if want_idx else "doubles",
                                                               " ".join("%s=%.3e" % kv for kv in sorted(stats.items()))))


@pytest.mark.parametrize("tier", ["tier1", "tier2"])
def test_reset_records_match_exact_reference(tier, monkeypatch):
    """A device-drawn reset inside a launch (tier 2: the build that carries the tier-2 resets): the reset record's start_coverage and
    start_variance_inv against the exact reference of the new episode's first state -- fp32, so the launch's float32 reset observation IS
    that state -- and bit for bit against the stand-alone kernel on it."""
    from gym_cloth_amd import ClothBatch
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    seeds = (0, 1, 5, 20)
    E, P, thick = len(seeds), 625, _THICKNESS[25]
    env = _seeded_env(25, "f32", seeds, tier=tier, max_actions=1)       # every episode ends with its first action: slot 1 starts with a reset
    env.reset()
    out = env.step_many(_actions(seeds, T=2), auto_reset=True, want_obs=True)
    v = env.batch.last_variant()
    env.close()
    assert v["fused"] == (2 if tier == "tier2" else 1), v
    assert out["ran"].all() and out["done"][0].all() and (out["reset_before"][1] == 1).all()
    pos = out["reset_obs"][:, 0].reshape(E, P, 3).astype(np.float64)
    b = ClothBatch(_cfg(25, thick, tier), n_envs=E, precision="f32")
    b.set_state(pos, pos, np.zeros((E, P), dtype=np.uint8))
    cov, vinv, oob, _, height = b.metrics(want_height=True)
    assert np.array_equal(b.positions(), pos)
    b.close()
    stats = {}
    for e in range(E):
        _check_against_exact((tier, e), pos[e], thick, out["start_coverage"][1, e], out["start_variance_inv"][1, e], oob[e],
                             np.rint(height[e] * P), stats)
    assert np.array_equal(out["start_coverage"][1], cov) and np.array_equal(out["start_variance_inv"][1], vinv)
    assert len(set(out["start_coverage"][1])) == E                      # four different episodes, not one number four times
    print("MEASURED reset records %s (%s): %s" % (tier, v["name"], " ".join("%s=%.3e" % kv for kv in sorted(stats.items()))))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("reward_type", ["height", "height-delta"])
def test_height_rewards_use_the_reference_fraction(reward_type, prec, monkeypatch):
    """reward_type 'height' / 'height-delta' (cloth_env.py:603-609, :656-679): the rewards of step() and of step_many() equal compute_reward
    fed with the exact reference's fraction of points below thickness / 2 on the state read back. (ClothEnv, like the reference's
    constructor, only accepts the coverage types; the reward code itself serves all of them, so the type is set on the built env.)"""
    from gym_cloth_amd.envs import compute_reward
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    seeds = (0, 3, 5, 20)                                              # (env 2 ends its episode out of bounds: it idles in the launch)
    E, P, thick = len(seeds), 625, _THICKNESS[25]
    env = _seeded_env(25, prec, seeds)
    env.reset()
    env.reward_type = reward_type
    acts = _actions(seeds, T=2)

    def expected(rew_mask, info_cov, info_vinv, info_oob, n_grabbed, have_tear, prev, a):
        pos = env.batch.positions()
        frac = np.array([exact(pos[e], thick).n_below / float(P) for e in range(E)])
        rew, tracked = compute_reward(reward_type, a, rew_mask & (n_grabbed == 0), info_cov, info_vinv, info_oob, rew_mask, have_tear, prev,
                                      height=frac, clip_act_space=True, act_low=env.action_space.low, act_high=env.action_space.high,
                                      consts=env._reward_consts())
        return rew, frac

    prev = env._prev_reward.copy()
    obs, rew, done, info = env.step(acts[0], auto_reset=False)                                   # the per-step path: stand-alone kernel
    want, frac = expected(np.ones(E, dtype=bool), info["actual_coverage"], info["variance_inv"], info["out_of_bounds"], info["n_grabbed"],
                          info["have_tear"], prev, acts[0])
    assert np.array_equal(rew, want), (rew, want)
    assert ((frac > 0) & (frac < 1)).all() and len(set(frac)) > 1
    if reward_type == "height-delta":
        assert np.array_equal(env._prev_reward, frac)
    prev = env._prev_reward.copy()
    out = env.step_many(acts[1:], auto_reset=False)                                              # the episode launch: in-kernel metrics
    ran = out["ran"][0]
    assert np.array_equal(ran, ~done) and ran.sum() >= 2, (ran, done)
    want, frac2 = expected(ran, out["actual_coverage"][0], out["variance_inv"][0], out["out_of_bounds"][0], out["n_grabbed"][0],
                           out["have_tear"][0], prev, acts[1])
    assert np.array_equal(out["rew"][0], want), (out["rew"][0], want)
    assert not np.array_equal(frac2[ran], frac[ran])                                            # the second action moved the count
    env.close()
