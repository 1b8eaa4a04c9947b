"""GPU tests of the cross-entropy planner over forked cloths (clothhip_plan_cem / _sample / _refit): each kernel against its
numpy restatement, the whole loop against cem_reference on the same scratch batch, the best-so-far rule, a replay of the chosen plan, an
env that is not planned, every refusal, and CEMPolicy through collect_demos. Every comparison is array_equal."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_dagger as D
from test_gpu_env import base_cfg

pytestmark = pytest.mark.gpu

LO, HI = np.full(4, -1.0), np.full(4, 1.0)


def _env(E, prec="f64", n_side=10, **kw):
    """test_gpu_dagger's _env helper (tier 1, seeds 1337 + e) with E envs instead of its six."""
    old = D.E
    D.E = E
    try:
        return D._env(prec, n_side=n_side, force_grab=False, **kw)
    finally:
        D.E = old


@functools.lru_cache(maxsize=None)
def _device_batch():
    """a one-cloth batch: the stand-alone kernels take a handle for its device and stream only"""
    from gym_cloth_amd import ClothBatch
    cfg = base_cfg("tier1", 1337)
    cfg["cloth"]["num_width_points"] = cfg["cloth"]["num_height_points"] = 10
    return ClothBatch(cfg, n_envs=1, precision="f32")


@pytest.mark.parametrize("E,K,H", [(1, 2, 1), (3, 65, 2), (2, 256, 8)])
def test_sample_equals_reference(E, K, H):
    """K across a wave boundary (65), a table larger than one workgroup (2 * 256 * 8 * 4 elements); means outside the bounds on both
    sides, so both clips are taken."""
    from gym_cloth_amd.policies import plan_sample_reference
    r = np.random.RandomState(100 + K)
    mean = r.uniform(-1.4, 1.4, size=(E, H, 4))
    std = r.uniform(0.0, 0.6, size=(E, H, 4))
    std[0, 0, 1] = 0.0
    seed, iter0, it = 0x9E3779B97F4A7C15, 5, 2
    got = _device_batch().plan_sample(mean, std, LO, HI, it=it, horizon=H, n_candidates=K, seed=seed, iter0=iter0)
    ref = plan_sample_reference(mean, std, LO, HI, K, seed=seed, iteration=iter0 + it)
    assert got.shape == (H, E * K, 4)
    assert np.array_equal(got, ref)
    if got.size >= 100:
        assert (got == -1.0).any() and (got == 1.0).any()
    assert np.array_equal(got[:, 0::K, :], np.clip(mean, LO, HI).transpose(1, 0, 2))


@pytest.mark.parametrize("K,M", [(2, 1), (2, 2), (65, 1), (65, 3), (65, 65), (1024, 1), (1024, 3), (1024, 1024)])
def test_refit_equals_reference(K, M):
    """Small-integer scores with many ties, one env that is not planned: mean, std, elite mask and top index, all exact."""
    from gym_cloth_amd.policies import plan_refit_reference
    E, H = 3, 2
    r = np.random.RandomState(7 * K + M)
    x = r.uniform(-1, 1, size=(H, E * K, 4))
    scores = r.randint(0, 4, size=(E, K)).astype(np.float64)
    scores[2, K // 2] = -np.inf
    mean = r.uniform(-1, 1, size=(E, H, 4))
    std = r.uniform(0.1, 0.5, size=(E, H, 4))
    done = np.array([False, True, False])
    ms = np.array([0.05, 0.0, 0.3, 0.01])
    got = _device_batch().plan_refit(x, scores, mean, std, done=done, horizon=H, n_elite=M, alpha=0.7, min_std=ms)
    ref = plan_refit_reference(x, scores, mean, std, M, alpha=0.7, min_std=ms, done=done)
    for g, w, name in zip(got, ref, ("mean", "std", "elite", "top")):
        assert np.array_equal(g, w), (name, K, M)
    assert got[2].sum(axis=1).tolist() == [M, 0, M] and got[3][1] == -1
    assert np.array_equal(got[0][1], mean[1]) and np.array_equal(got[1][1], std[1])
    if M == 1:                                                                # alpha sd = 0: std = max(min_std, 0.3 old std)
        assert np.array_equal(got[1][0], np.maximum(ms, (1.0 - 0.7) * std[0]))


_KEYS = ("candidates", "scores", "mean", "std", "actions", "score")


@functools.lru_cache(maxsize=None)
def _loop(n_side, E, K, H, n_iters, prec):
    """One env, planned by the library and by cem_reference on the same scratch batch; nothing afterwards changes either result."""
    from gym_cloth_amd.policies import cem_reference
    v = _env(E, prec, n_side)
    v.reset()
    r = np.random.RandomState(5)
    mean = r.uniform(-0.5, 0.5, size=(E, H, 4))
    std = np.full((E, H, 4), 0.3)
    kw = dict(min_std=0.02, alpha=0.8, penalty=1.0, seed=77, iter0=3)
    got = v.plan(H, K, 3, n_iters, mean=mean, std=std, want_scores=True, want_candidates=True, **kw)
    ref = cem_reference(v, v._plan_scratch, H, K, 3, n_iters, mean, std, **kw)
    v.close()
    return got, ref


@pytest.mark.parametrize("n_side,E,K,H,prec", [(10, 3, 8, 2, "f32"), (10, 3, 8, 2, "f64"), (25, 2, 6, 1, "f32")])
def test_loop_equals_reference(n_side, E, K, H, prec):
    got, ref = _loop(n_side, E, K, H, 2, prec)
    assert got["planned"].all()
    for k in _KEYS:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    assert np.isfinite(got["scores"]).all() and (got["std"] >= 0.02).all()
    assert not np.array_equal(got["candidates"][0], got["candidates"][1])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_best_score_is_the_running_maximum(prec):
    got, _ = _loop(10, 3, 8, 2, 2, prec)
    sc = got["scores"]                                                           # [n_iters, E, K]
    assert (got["score"] >= sc[0, :, 0]).all()                                   # candidate 0 of iteration 0: the given mean's own rollout
    assert np.array_equal(got["score"], sc.max(axis=2).max(axis=0))
    # the best actions are a row of the candidate tables: the first (iteration, k) that reaches the maximum
    E, K = sc.shape[1], sc.shape[2]
    for e in range(E):
        it = int(np.argmax(sc[:, e].max(axis=1)))
        k = int(np.argmax(sc[it, e]))
        assert np.array_equal(got["actions"][e], got["candidates"][it][:, e * K + k, :])


def _host_state(v):
    pos, prev, pin = v.batch.get_state()
    return dict(pos=pos, prev=prev, pin=pin, cnt=v.batch.pin_counts(), tear=v.batch.tear, rest=v.batch.get_rest(),
                num_steps=v.num_steps.copy(), num_sim_steps=v.num_sim_steps.copy(), ep_done=v._ep_done.copy(), have_tear=v.have_tear.copy(),
                prev_reward=v._prev_reward.copy(), version=v._version,
                rng=[r.get_state()[1].copy() for r in v.np_randoms] + [np.array([r.get_state()[2] for r in v.np_randoms])])


def _same_state(a, b):
    for k in a:
        if k == "rng":
            assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert np.array_equal(a[k], b[k]), k


def test_replay_reproduces_the_score_and_the_env_does_not_move():
    """fp64 (fp32 bits may differ between the variants an E-cloth and an E K-cloth handle pick): the chosen sequence, stepped from the
    state plan() saw, scores what the planner said, bit for bit; and plan() left the env exactly where it was."""
    E, K, H = 3, 8, 2
    v = _env(E, "f64", 10)
    v.reset()
    v.step_many(np.random.RandomState(1).uniform(-0.3, 0.3, size=(1, E, 4)), auto_reset=False)      # not a fresh cloth, one action used
    before = _host_state(v)
    plan = v.plan(H, K, 3, 2, std=np.full((E, H, 4), 0.4), penalty=1.5, seed=9)
    _same_state(before, _host_state(v))
    assert plan["planned"].any() and np.array_equal(plan["planned"], ~v._ep_done)
    out = v.step_many(np.ascontiguousarray(np.nan_to_num(plan["actions"]).transpose(1, 0, 2)), auto_reset=False)
    for e in np.nonzero(plan["planned"])[0]:
        ran = out["ran"][:, e]
        assert ran[0]
        last = int(np.nonzero(ran)[0][-1])
        bad = (out["out_of_bounds"][ran, e] | out["have_tear"][ran, e]).any()
        cov = out["actual_coverage"][last, e]
        assert (cov - 1.5 if bad else cov) == plan["score"][e], e
    v.close()


def test_a_done_env_is_not_planned():
    E, K, H = 3, 4, 2
    v = _env(E, "f64", 10)
    v.reset()
    r = np.random.RandomState(2)
    mean, std = r.uniform(-0.5, 0.5, size=(E, H, 4)), r.uniform(0.1, 0.4, size=(E, H, 4))
    kw = dict(mean=mean, std=std, seed=4, want_scores=True)
    full = v.plan(H, K, 2, 2, **kw)
    v._ep_done[1] = True                                                         # as step_many(auto_reset=False) leaves an env whose episode ended
    part = v.plan(H, K, 2, 2, **kw)
    v._ep_done[1] = False
    assert part["planned"].tolist() == [True, False, True]
    assert np.isnan(part["actions"][1]).all() and np.isnan(part["score"][1])
    assert np.array_equal(part["mean"][1], mean[1]) and np.array_equal(part["std"][1], std[1])
    assert (part["scores"][:, 1] == -np.inf).all()                               # its branches ran nothing
    for k in ("actions", "score", "mean", "std"):
        assert np.array_equal(part[k][[0, 2]], full[k][[0, 2]]), k
    assert np.array_equal(part["scores"][:, [0, 2]], full["scores"][:, [0, 2]])
    v.close()


def _raw_plan(scratch, src, ep, ns, dn, mean, std, **fields):
    """clothhip_plan_cem itself, with a ClothPlanParams filled by hand (ClothBatch.plan_params would refuse first). -> status"""
    from gym_cloth_amd import _lib
    p = _lib.ClothPlanParams()
    d = dict(horizon=1, n_candidates=2, n_elite=1, n_iters=1, seed=3, iter0=0, alpha=1.0, penalty=1.0)
    d.update(fields)
    ms = d.pop("min_std", 0.0)
    for k, val in d.items():
        setattr(p, k, val)
    for a in range(4):
        p.min_std[a] = ms
    E = src.E
    best_a, best_s = np.full((E, 1, 4), 7.0), np.full(E, 7.0)
    rc = scratch._L.clothhip_plan_cem(scratch._h, src._h, C.byref(ep), C.byref(p), _lib.i32p(ns), _lib.u8p(dn), _lib.dp(mean), _lib.dp(std),
                                      _lib.dp(best_a), _lib.dp(best_s), None, None)
    if rc != 0:
        assert (best_a == 7.0).all() and (best_s == 7.0).all()
    return rc


def test_refusals_change_nothing():
    """Every CLOTHHIP_EINVAL / CLOTHHIP_ESTATE case of clothhip.h through the library itself; after each one the same env plans what a fresh
    env plans. (No creatable handle of these grids lacks the fused launch, so that refusal has no case here.)"""
    from gym_cloth_amd import ClothBatch, _lib
    E, K = 2, 2
    fresh = _env(E, "f64", 10); fresh.reset()
    want = fresh.plan(1, K, 1, 1, seed=3, min_std=0.0, want_scores=True)
    fresh.close()
    v = _env(E, "f64", 10); v.reset()
    state = _host_state(v)
    ep = v._episode_params()
    ns, dn = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
    mean0, std0 = np.zeros((E, 1, 4)), np.full((E, 1, 4), 0.5)
    scratch = ClothBatch(v.cfg, n_envs=E * K, precision="f64")
    v._plan_scratch = scratch                                                    # the successful plans run on the handle that saw the refusals

    def refused(code, scr=None, **fields):
        m, s = fields.pop("mean", mean0).copy(), fields.pop("std", std0).copy()
        m_in, s_in = m.copy(), s.copy()
        assert _raw_plan(scratch if scr is None else scr, v.batch, fields.pop("ep", ep), ns, dn, m, s, **fields) == code, fields
        assert np.array_equal(m, m_in, equal_nan=True) and np.array_equal(s, s_in)
        _same_state(state, _host_state(v))
        got = v.plan(1, K, 1, 1, seed=3, min_std=0.0, want_scores=True)
        for k in ("actions", "score", "mean", "std", "scores"):
            assert np.array_equal(got[k], want[k]), (fields, k)

    EINVAL, ESTATE = _lib.EINVAL, _lib.ESTATE
    for bad in [dict(horizon=0), dict(horizon=9), dict(n_candidates=1), dict(n_candidates=1025), dict(n_elite=0), dict(n_elite=3),
                dict(n_iters=0), dict(iter0=2 ** 31), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float("nan")),
                dict(penalty=float("inf")), dict(min_std=-0.1), dict(min_std=float("nan"))]:
        refused(EINVAL, **bad)
    nan_mean, neg_std, inf_std = mean0.copy(), std0.copy(), std0.copy()
    nan_mean[1, 0, 2], neg_std[0, 0, 0], inf_std[1, 0, 3] = np.nan, -0.1, np.inf
    refused(EINVAL, mean=nan_mean); refused(EINVAL, std=neg_std); refused(EINVAL, std=inf_std)
    bad_ep = v._episode_params(); bad_ep.max_actions = 0
    refused(EINVAL, ep=bad_ep)
    refused(EINVAL, scr=v.batch)                                                 # scratch == src
    others = [ClothBatch(v.cfg, n_envs=E * K + 1, precision="f64"), ClothBatch(v.cfg, n_envs=E * K, precision="f32")]
    cfg25 = base_cfg("tier1", 1337)
    others.append(ClothBatch(cfg25, n_envs=E * K, precision="f64"))              # another grid
    cfg_ks = base_cfg("tier1", 1337)
    cfg_ks["cloth"]["num_width_points"] = cfg_ks["cloth"]["num_height_points"] = 10
    cfg_ks["cloth"]["thickness"] = 0.03
    others.append(ClothBatch(cfg_ks, n_envs=E * K, precision="f64"))             # the same grid, other ClothParams
    for o in others:
        refused(EINVAL, scr=o)
        o.close()
    # a launch in flight, on the source and on the scratch handle (every env of it marked done: the launch itself moves nothing)
    v.batch.run_actions_begin(ep, 1, ns.copy(), np.ones(E, dtype=np.uint8), actions=np.zeros((1, E, 4)))
    m, s = mean0.copy(), std0.copy()
    assert _raw_plan(scratch, v.batch, ep, ns, dn, m, s) == ESTATE
    rec = v.batch.run_actions_end()[0]
    assert not rec["ran"].any()
    _same_state(state, _host_state(v))
    scratch.run_actions_begin(ep, 1, np.zeros(E * K, dtype=np.int32), np.ones(E * K, dtype=np.uint8), actions=np.zeros((1, E * K, 4)))
    assert _raw_plan(scratch, v.batch, ep, ns, dn, m, s) == ESTATE
    scratch.run_actions_end()
    refused(EINVAL, horizon=0)                                                   # (and the pair still plans what a fresh one does)
    scratch.set_relaxed_order(True)
    assert _raw_plan(scratch, v.batch, ep, ns, dn, m, s) == ESTATE
    scratch.set_relaxed_order(False)
    refused(EINVAL, horizon=0)
    v.close()


def test_a_parked_time_slice_is_refused():
    """A time-sliced launch cut the source's actions in the middle: planning from there is refused (ClothVecEnv.plan raises before the
    library is asked; the library says CLOTHHIP_ESTATE), unless the env is not planned anyway."""
    from test_gpu_fused import _bench_env
    from gym_cloth_amd import ClothBatch, _lib
    E, K = 2, 2
    a = _bench_env(E, "f64"); a.reset()
    acts = np.stack([np.random.RandomState(2000 + e).uniform(-0.5, 0.5, size=(3, 4)) for e in range(E)], axis=1)
    out = a.step_many(acts, time_budget_ms=5.0)
    assert not out["ran"].any() and a.batch.in_flight().all()
    with pytest.raises(RuntimeError, match="in flight"):
        a.plan(1, K, 1, 1)
    scratch = ClothBatch(a.cfg, n_envs=E * K, precision="f64")
    ns, m, s = np.zeros(E, dtype=np.int32), np.zeros((E, 1, 4)), np.full((E, 1, 4), 0.5)
    assert _raw_plan(scratch, a.batch, a._episode_params(), ns, np.zeros(E, dtype=np.uint8), m, s) == _lib.ESTATE
    assert _raw_plan(scratch, a.batch, a._episode_params(), ns, np.ones(E, dtype=np.uint8), m, s) == 0      # nothing planned, nothing refused
    assert a.batch.in_flight().all()
    scratch.close(); a.close()


def test_cem_policy_through_collect_demos():
    from gym_cloth_amd.demos import collect_demos
    from gym_cloth_amd.policies import CEMPolicy
    E = 2
    v = _env(E, "f32", 10, max_actions=2)
    log = [[] for _ in range(E)]

    class Logged(CEMPolicy):
        def get_action(self, obs=None, t=0):
            act = CEMPolicy.get_action(self, obs, t)
            assert self.last_plan["planned"].all() and np.array_equal(act, self.last_plan["actions"][:, 0])
            for e in range(E):
                log[e].append(tuple(act[e]))
            return act

    pol = Logged(v, horizon=2, n_candidates=4, n_elite=2, n_iters=1, init_std=0.4, seed=1)
    eps = collect_demos(v, policy=pol, max_episodes=2)
    assert len(eps) == 2 and pol.iter0 == len(log[0])
    used = [0] * E
    for ep in sorted(eps, key=lambda d: d["env"]):
        e, n = ep["env"], len(ep["act"])
        assert 1 <= n <= 2 and ep["done"][-1] and len(ep["obs"]) == n + 1
        assert ep["act"] == log[e][used[e]:used[e] + n]                          # the planner's actions, in order
        used[e] += n
        assert all(np.isfinite(a).all() and (np.abs(a) <= 1.0).all() for a in ep["act"])
    v.close()
