"""GPU tests of the expert beside the acting policy (clothhip_run_actions_expert / _labels, clothhip_policy_label): the labels
are the oracle's bits, a silent expert changes nothing, an acting expert is the oracle launch, a mixed table is the host loop, time slices
keep (record, label) pairs together, a population, the refusals. Every comparison is array_equal."""
import numpy as np
import pytest

from test_gpu_env import base_cfg

pytestmark = pytest.mark.gpu

E = 6
_RECORDS = ("actions", "rew", "done", "ran", "executed", "n_grabbed", "num_steps", "num_sim_steps", "actual_coverage", "variance_inv",
            "have_tear", "out_of_bounds", "reset_before")


def _layers(widths, seed, bias=None):
    r = np.random.RandomState(seed)
    L = [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32),
          (r.normal(size=widths[l + 1]) / np.sqrt(widths[l])).astype(np.float32)) for l in range(len(widths) - 1)]
    if bias is not None:
        L[-1] = (L[-1][0], np.asarray(bias, dtype=np.float32))
    return L


def _env(prec="f64", tier="tier1", n_side=25, max_actions=None, force_grab=True):
    from gym_cloth_amd.envs import ClothVecEnv
    cfg = base_cfg(tier, 1337)
    cfg["cloth"]["num_width_points"] = cfg["cloth"]["num_height_points"] = n_side
    cfg["env"]["force_grab"] = force_grab
    if max_actions is not None:
        cfg["env"]["max_actions"] = max_actions
    v = ClothVecEnv(cfg, n_envs=E, precision=prec, consume_domrand_draws=False)
    v.seed([1337 + e for e in range(E)])
    return v


def _net(v, seed=21, **kw):
    from gym_cloth_amd.policies import MLPPolicy
    v.set_policy(MLPPolicy(v, _layers([3 * v.P, 5, 4], seed, **kw)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, keys=_RECORDS, where=""):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (where, k)


CHECKER = (np.add.outer(np.arange(4), np.arange(E)) % 2).astype(bool)       # [4, E]: (t + e) odd -> the expert acts
CHOICES = np.array([[0, 1, 4, 0, 1, 4], [4, 0, 1, 1, 4, 0], [1, 4, 0, 4, 0, 1], [0, 0, 4, 4, 1, 1]], dtype=np.int32)


@pytest.mark.parametrize("tier", ["tier1", "tier2"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_labels_are_the_oracles_bits(prec, tier):
    """From one state: expert_actions(obs=None) == labels[0] of an armed policy='mlp' launch == the action records of slot 0 of a launch
    with the expert as its acting policy from a fork of that state -- oracle corner, and highest point with choices from {0, 1, 4}. Tier 2
    with cloths dropped from both sides. On the fp32 handle every label of a slot that ran is the stand-alone kernel on the observation
    that slot's policy saw (episodes of two actions, so slots begin on reset observations too; on tier 2 a reset draws the side anew)."""
    from gym_cloth_amd.envs import slot_start_obs
    t2 = tier == "tier2"
    T = 3 if t2 else 4
    v = _env(prec, tier, max_actions=2)
    pre = v.reset()
    if t2:
        assert v.init_side.any() and not v.init_side.all(), v.init_side
    side = v.init_side.copy()
    _net(v)
    snap = v.snapshot()
    for expert in ("oracle_corner", "highest_point"):
        hp = expert == "highest_point"
        v.restore(snap)
        here = v.expert_actions(expert, choices=CHOICES[0] if hp else None)
        assert here.shape == (E, 4) and np.isfinite(here).all()
        out = v.step_many(policy="mlp", n_actions=T, want_obs=True, expert=expert,
                          expert_choices=CHOICES[:T] if hp else None)
        assert v.batch.last_variant()["fused"] == 2
        lab = out["expert_actions"]
        assert out["ran"][0].all() and not out["expert_took"].any()
        assert np.array_equal(_bits(lab[0]), _bits(here)), (expert, lab[0] - here)
        assert np.isnan(lab[~out["ran"]]).all() and np.isfinite(lab[out["ran"]]).all()
        v.restore(snap)
        ref = v.step_many(policy=expert, n_actions=1, policy_choices=CHOICES[:1] if hp else None)
        assert np.array_equal(_bits(ref["actions"][0]), _bits(here)), (expert, ref["actions"][0] - here)
        assert len({here[e].tobytes() for e in range(E)}) > 1               # the expert reads the state
        if hp:
            v.restore(snap)
            other = v.expert_actions(expert, choices=CHOICES[1])
            assert not np.array_equal(other, here)                           # ... and its choice
        if prec == "f32":
            assert (out["reset_before"] > 0).any()
            assert np.array_equal(out["init_side_t"][0], side)
            rows = slot_start_obs(out, pre)
            got = v.expert_actions(expert, obs=rows.reshape(T * E, -1), choices=CHOICES[:T].reshape(-1) if hp else None,
                                   init_side=out["init_side_t"].reshape(-1) if t2 else None).reshape(T, E, 4)
            ran = out["ran"]
            assert ran.sum() > E and np.array_equal(_bits(got[ran]), _bits(lab[ran])), expert
    v.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_silent_expert_changes_nothing(prec, monkeypatch):
    """expert_mix == 0, no table at all, and a highest-point expert without a table: records, actions, final particles and obs_t are the un-armed MLP launch's, on the default
    variant and on the standard arithmetic's other thread layout; episodes of two actions, so resets run inside the launch."""
    T = 3
    noise = np.random.RandomState(9).normal(size=(T, E, 4)) * 0.05
    threads = []
    for run in range(2):
        for k in ("CLOTHHIP_DEBUG_LEAN", "CLOTHHIP_DEBUG_W8", "CLOTHHIP_DEBUG_NOSPEC"):
            monkeypatch.delenv(k, raising=False)
        if run == 1:
            monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", "0")
            monkeypatch.setenv("CLOTHHIP_DEBUG_W8", "0" if threads[0] != 256 else "1")
        v = _env(prec, max_actions=2)
        v.reset()
        _net(v)
        snap = v.snapshot()
        plain = v.step_many(policy="mlp", n_actions=T, want_obs=True, policy_noise=noise)
        plain_state = v.batch.get_state()[0].copy()
        threads.append(v.batch.last_variant()["threads"])
        assert (plain["reset_before"] > 0).any()
        for expert, mix in (("oracle_corner", np.zeros((T, E), dtype=bool)), ("oracle_corner", None), ("highest_point", None)):
            v.restore(snap)                                                  # (the highest-point trip borrows the member list as scratch)
            out = v.step_many(policy="mlp", n_actions=T, want_obs=True, policy_noise=noise, expert=expert, expert_mix=mix,
                              expert_choices=CHOICES[:T] if expert == "highest_point" else None)
            assert v.batch.last_variant()["threads"] == threads[-1]
            _same(out, plain, where=(prec, threads[-1]))
            assert np.array_equal(out["obs_t"], plain["obs_t"]) and np.array_equal(out["reset_obs"], plain["reset_obs"])
            assert np.array_equal(_bits(v.batch.get_state()[0]), _bits(plain_state))
            assert not out["expert_took"].any() and np.isfinite(out["expert_actions"][out["ran"]]).all()
        v.close()
    assert sorted(threads) == [256, 512], threads


def test_an_acting_expert_is_the_oracle_launch_f64():
    """expert_mix == 1 beside a network whose output would leave the action box: everything equals the policy='oracle_corner' launch
    from the same state, in-kernel resets included."""
    T = 4
    v = _env("f64", max_actions=2)
    v.reset()
    _net(v, bias=[5.0, -5.0, 5.0, -5.0])
    assert (np.abs(v.policy_actions()) > 2.0).any()
    snap = v.snapshot()
    ref = v.step_many(policy="oracle_corner", n_actions=T, want_obs=True)
    ref_state = v.batch.get_state()[0].copy()
    assert (ref["reset_before"] > 0).any() and ref["ran"].all()
    v.restore(snap)
    out = v.step_many(policy="mlp", n_actions=T, want_obs=True, expert="oracle_corner", expert_mix=np.ones((T, E), dtype=bool),
                      policy_noise=np.full((T, E, 4), 0.25))
    _same(out, ref)
    assert np.array_equal(out["obs_t"], ref["obs_t"]) and np.array_equal(out["reset_obs"], ref["reset_obs"])
    assert np.array_equal(_bits(v.batch.get_state()[0]), _bits(ref_state))
    assert out["expert_took"].all() and np.array_equal(_bits(out["expert_actions"]), _bits(out["actions"]))
    v.close()


def test_a_mixed_table_is_the_host_loop_f64():
    """A checkerboard over (t, e), a noise table, episodes of two actions: actions, rewards, dones, labels and the final state equal
    the host loop that steps the oracle's action on the present state where the table says so and network + noise elsewhere. Noise is not
    added where the expert acts; after a reset the label is the oracle on the new episode's first state."""
    T = 4
    noise = np.random.RandomState(11).normal(size=(T, E, 4)) * 0.05
    a, b = _env("f64", max_actions=2), _env("f64", max_actions=2)
    for v in (a, b):
        v.reset()
        _net(v)
    out = a.step_many(policy="mlp", n_actions=T, want_obs=True, reset_tail=True, policy_noise=noise, expert="oracle_corner", expert_mix=CHECKER)
    assert out["ran"].all() and (out["reset_before"] > 0).any()
    assert np.array_equal(out["expert_took"], CHECKER)
    for t in range(T):
        label = b.expert_actions("oracle_corner")
        act = np.where(CHECKER[t][:, None], label, b.policy_actions() + noise[t])
        _, rew, done, _ = b.step(act, auto_reset=True)
        assert np.array_equal(_bits(out["expert_actions"][t]), _bits(label)), t
        assert np.array_equal(_bits(out["actions"][t]), _bits(act)), t
        assert np.array_equal(rew, out["rew"][t]) and np.array_equal(done, out["done"][t]), t
    after_reset = out["reset_before"] > 0
    assert (after_reset & CHECKER).any() and (after_reset & ~CHECKER).any()   # both kinds of slot began on a reset state
    assert np.array_equal(_bits(a.batch.get_state()[0]), _bits(b.batch.get_state()[0]))
    a.close(); b.close()


def test_time_slices_keep_record_and_label_together_f64():
    """N actions per env in one launch, and in a sequence of time-sliced launches that cut actions (the unused mix / noise rows passed
    again, every launch armed): per env, in order, the (record, label) pairs are the same."""
    N, T = 4, 4
    noise = np.random.RandomState(13).normal(size=(N, E, 4)) * 0.05
    a, b = _env("f64"), _env("f64")
    for v in (a, b):
        v.reset()
        _net(v)
    whole = a.step_many(policy="mlp", n_actions=N, policy_noise=noise, expert="oracle_corner", expert_mix=CHECKER[:N])
    assert whole["ran"].all()
    used = np.zeros(E, dtype=np.int64)
    pairs = [[] for _ in range(E)]
    cut = parked = 0
    for launch in range(60):
        if (used >= N).all():
            break
        idx = np.minimum(used[None, :] + np.arange(T)[:, None], N - 1)      # [T, E] rows of the tables; past the end: the last again
        ee = np.arange(E)[None, :]
        out = b.step_many(policy="mlp", n_actions=T, policy_noise=noise[idx, ee], expert="oracle_corner", expert_mix=CHECKER[:N][idx, ee],
                          time_budget_ms=15.0)
        ran = out["ran"]
        assert np.isfinite(out["expert_actions"][ran]).all() and np.isnan(out["expert_actions"][~ran]).all()
        cut += int((~ran).sum())
        parked += int(b.batch.in_flight().sum())                             # actions cut in mid-flight: their labels travel in the resume record
        for e in range(E):
            n = int(ran[:, e].sum())
            assert ran[:n, e].all()
            for t in range(n):
                pairs[e].append((out["actions"][t, e].tobytes(), out["expert_actions"][t, e].tobytes(), bool(out["expert_took"][t, e])))
            used[e] += n
    assert (used >= N).all() and cut > 0 and parked > 0, (used, cut, parked)
    for e in range(E):
        for t in range(N):
            exp = (whole["actions"][t, e].tobytes(), whole["expert_actions"][t, e].tobytes(), bool(CHECKER[t, e]))
            assert pairs[e][t] == exp, (e, t)
    a.close(); b.close()


def test_a_population_under_a_mixed_table():
    """The map [0, 1, 2, 0, 1, 2] with the checkerboard: env by env the launch equals the shared-network launch of that env's network
    under the same table."""
    from gym_cloth_amd.policies import MLPPopulation
    T = 3
    member = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    v = _env("f32")
    v.reset()
    pop = MLPPopulation(v, _layers([3 * v.P, 5, 4], 21), 2, 0.1, 20261019, member=member)
    v.set_policy(pop)
    nets = pop.members()
    snap = v.snapshot()
    kw = dict(policy="mlp", n_actions=T, expert="oracle_corner", expert_mix=CHECKER[:T])
    out = v.step_many(**kw)
    state = v.batch.get_state()[0].copy()
    assert out["ran"].all()
    assert len({out["actions"][0, e].tobytes() for e in (1, 3, 5)}) == 3     # slot 0 of the odd envs: three networks, three actions
    for g in range(3):
        v.restore(snap)
        v.set_policy(nets[g])
        ref = v.step_many(**kw)
        ref_state = v.batch.get_state()[0]
        for e in np.nonzero(member == g)[0]:
            for k in _RECORDS + ("expert_actions", "expert_took"):
                assert np.array_equal(out[k][:, e], ref[k][:, e]), (g, e, k)
            assert np.array_equal(_bits(state[e]), _bits(ref_state[e])), (g, e)
    v.close()


def test_refusals_and_the_one_shot_arming():
    """Every CLOTHHIP_EINVAL / CLOTHHIP_ESTATE case of clothhip.h, through the library itself; the arming is for one launch; after each
    refusal an ordinary launch on the same handle equals a fresh handle's. (A handle whose variant lacks the build with the cold policies
    cannot be made: clothhip_create prepares that build for every handle it returns, so that one refusal has no case here.)"""
    import ctypes as C
    from gym_cloth_amd import _lib
    OC, HP = _lib.POLICY_ORACLE_CORNER, _lib.POLICY_HIGHEST_POINT
    acts = np.random.RandomState(3).uniform(-1, 1, size=(1, E, 4))
    fresh = _env("f32")
    fresh.reset()
    want = fresh.step_many(acts)
    want_state = fresh.batch.get_state()[0].copy()
    fresh.close()
    v = _env("f32")
    v.reset()
    snap = v.snapshot()
    L, h = v.batch._L, v.batch._h
    mix, cho = np.zeros((2, E), dtype=np.uint8), np.zeros((2, E), dtype=np.int32)
    lab = np.zeros((2, E, 4))

    def still_fine():
        v.restore(snap)
        out = v.step_many(acts)
        _same(out, want)
        assert np.array_equal(_bits(v.batch.get_state()[0]), _bits(want_state))
        assert L.clothhip_run_actions_labels(h, _lib.dp(lab), None) == _lib.ESTATE      # that launch was not armed

    def arm(expert, T, m=None, c=None):
        return L.clothhip_run_actions_expert(h, expert, T, _lib.u8p(m), _lib.i32p(c))

    def begin(T, policy=_lib.POLICY_TABLE):
        v.restore(snap)
        nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
        v.batch.run_actions_begin(v._episode_params(), T, nsteps, done, actions=np.zeros((T, E, 4)) if policy == _lib.POLICY_TABLE else None,
                                  policy=policy)

    for expert in (_lib.POLICY_TABLE, _lib.POLICY_MLP, 7, -1):              # an unknown expert
        assert arm(expert, 2, mix, cho) == _lib.EINVAL
    still_fine()
    assert arm(OC, 0, mix) == _lib.EINVAL                                   # T < 1
    still_fine()
    assert arm(HP, 2, mix, None) == _lib.EINVAL                             # highest point without its choices
    still_fine()
    assert arm(OC, 2, mix) == _lib.OK                                       # a T at _begin other than the armed one ...
    with pytest.raises(ValueError):
        begin(3)
    still_fine()                                                            # ... and the failed call has consumed the arming
    assert arm(OC, 2, mix) == _lib.OK                                       # an acting policy other than TABLE / MLP
    with pytest.raises(ValueError):
        begin(2, policy=OC)
    still_fine()
    assert arm(OC, 2, mix) == _lib.OK                                       # a failed arming takes an earlier one with it
    assert arm(7, 2, mix) == _lib.EINVAL
    still_fine()
    # with a launch in flight: arming, labelling, the labels
    begin(1)
    assert arm(OC, 1, None) == _lib.ESTATE
    out4 = np.zeros((E, 4))
    assert L.clothhip_policy_label(h, OC, 1, None, E, None, None, _lib.dp(out4)) == _lib.ESTATE
    assert L.clothhip_run_actions_labels(h, _lib.dp(lab), None) == _lib.ESTATE
    v.batch.run_actions_end()
    still_fine()
    # a relaxed-order handle
    v.batch.set_relaxed_order(True)
    assert arm(OC, 2, mix) == _lib.ESTATE
    v.batch.set_relaxed_order(False)
    still_fine()
    # clothhip_policy_label's own argument checks
    assert L.clothhip_policy_label(h, 7, 1, None, E, None, None, _lib.dp(out4)) == _lib.EINVAL
    assert L.clothhip_policy_label(h, OC, 1, None, E + 1, None, None, _lib.dp(out4)) == _lib.EINVAL
    assert L.clothhip_policy_label(h, OC, 1, None, -1, None, None, _lib.dp(out4)) == _lib.EINVAL
    assert L.clothhip_policy_label(h, HP, 1, None, E, None, None, _lib.dp(out4)) == _lib.EINVAL
    assert L.clothhip_policy_label(h, OC, 1, None, E, None, None, None) == _lib.EINVAL
    still_fine()
    # one shot: the armed launch has labels, the next launch has none
    v.restore(snap)
    out = v.step_many(acts, expert="oracle_corner")
    _same(out, want)
    assert np.isfinite(out["expert_actions"]).all()
    p = C.c_void_p()
    assert L.clothhip_run_actions_labels(h, None, C.byref(p)) == _lib.OK and p.value
    still_fine()
    v.close()
    # oracle corner on a grid other than 25x25; the highest point runs there
    w = _env("f32", n_side=10)
    w.reset()
    L, h = w.batch._L, w.batch._h
    assert L.clothhip_run_actions_expert(h, OC, 2, None, None) == _lib.ESTATE
    assert L.clothhip_policy_label(h, OC, 1, None, E, None, None, _lib.dp(out4)) == _lib.ESTATE
    with pytest.raises(ValueError):
        w.step_many(np.zeros((1, E, 4)), expert="oracle_corner")
    k = np.array([0, 1, 4, 99, 150, -3], dtype=np.int32)                    # (clamped to [0, P - 1] as in the launch)
    here = w.expert_actions("highest_point", choices=k)
    out = w.step_many(np.zeros((1, E, 4)), expert="highest_point", expert_choices=k[None, :])
    assert np.array_equal(_bits(out["expert_actions"][0]), _bits(here))
    w.close()
