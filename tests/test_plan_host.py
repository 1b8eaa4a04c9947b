"""CPU tests of the cross-entropy planner's host side: the numpy restatements that tests/test_gpu_plan.py holds the kernels
against -- philox_eps on the generator's known-answer vectors, plan_refit_reference and plan_sample_reference on hand-made tables --, the
bindings against the header's signatures, the wrappers' refusals, and CEMPolicy's shift / warm-start bookkeeping on a stub env. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.policies import (CEMPolicy, philox4x32_10, philox_eps, plan_refit_reference, plan_sample_reference,
                                    plan_score_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("clothhip_plan_cem", "clothhip_plan_sample", "clothhip_plan_refit")
LO, HI = np.array([-1.0, -1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0, 1.0])


def _words(c):
    return ["%08x" % int(x) for x in c]


def test_philox_known_answer_vectors_and_eps():
    """The vectors tests/test_mlp_population_host.py states for its own restatement, here for the package's."""
    assert _words(philox4x32_10((0, 0, 0, 0), (0, 0))) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert _words(philox4x32_10((f, f, f, f), (f, f))) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _words(philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    # eps from the words: counter (i lo, i hi, k, 0), key (seed lo, seed hi); top 24 bits summed, centred, times (float)(sqrt(3) / 2^24)
    seed, k, i = 0x299F31D0A4093822, 0x13198A2E, np.array([0x85A308D3243F6A88], dtype=np.uint64)
    r = philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0), (0xA4093822, 0x299F31D0))
    D = sum(int(x) >> 8 for x in r) - (2 ** 25 - 2)
    scale = np.float32(np.sqrt(3.0) / 2.0 ** 24)
    assert scale.view(np.uint32) == 0x33DDB3D7
    e = philox_eps(seed, k, i)
    assert e.dtype == np.float32 and e[0] == np.float32(D) * scale
    # a fixed-seed sample: zero mean, unit variance, bounded, and a function of its arguments alone
    s = philox_eps(7, 3, np.arange(1 << 16))
    assert abs(float(s.mean())) < 0.02 and abs(float(s.var()) - 1.0) < 0.02 and float(np.abs(s).max()) <= 3.47
    assert np.array_equal(s, philox_eps(7, 3, np.arange(1 << 16))) and not np.array_equal(s, philox_eps(7, 4, np.arange(1 << 16)))


def _table(E, K, H, seed=0):
    r = np.random.RandomState(seed)
    return np.round(r.uniform(-1, 1, size=(H, E * K, 4)), 3)


def test_refit_ties_take_the_lower_k():
    E, K, H = 1, 6, 2
    x = _table(E, K, H)
    sc = np.array([[1.0, 3.0, 3.0, 2.0, 3.0, 2.0]])
    _, _, elite, top = plan_refit_reference(x, sc, np.zeros((E, H, 4)), np.ones((E, H, 4)), n_elite=2)
    assert top.tolist() == [1] and elite[0].tolist() == [False, True, True, False, False, False]
    _, _, elite, _ = plan_refit_reference(x, sc, np.zeros((E, H, 4)), np.ones((E, H, 4)), n_elite=4)
    assert elite[0].tolist() == [False, True, True, True, True, False]          # the 2.0 at k = 3 before the one at k = 5
    _, _, elite, top = plan_refit_reference(x, np.full((1, K), -np.inf), np.zeros((E, H, 4)), np.ones((E, H, 4)), n_elite=1)
    assert top.tolist() == [0] and elite[0].tolist() == [True] + [False] * 5


def test_refit_one_elite_all_elites_and_alpha():
    E, K, H = 2, 5, 3
    x = _table(E, K, H, 1)
    sc = np.array([[0.0, 4.0, 1.0, 2.0, 3.0], [5.0, 4.0, 1.0, 2.0, 3.0]])
    m0, s0 = np.full((E, H, 4), 0.25), np.full((E, H, 4), 0.5)
    ms = np.array([0.01, 0.02, 0.03, 0.04])
    # M = 1: the mean is the top candidate, the spread is zero, so std = min_std
    m, s, elite, top = plan_refit_reference(x, sc, m0, s0, n_elite=1, min_std=ms)
    assert top.tolist() == [1, 0] and elite.sum(axis=1).tolist() == [1, 1]
    for e in range(E):
        assert np.array_equal(m[e], x[:, e * K + top[e], :])
    assert np.array_equal(s, np.broadcast_to(ms, (E, H, 4)))
    # M = K: every candidate, summed in ascending k
    m, s, elite, _ = plan_refit_reference(x, sc, m0, s0, n_elite=K)
    assert elite.all()
    for e in range(E):
        tot = np.zeros((H, 4))
        for k in range(K):
            tot = tot + x[:, e * K + k, :]
        mu = tot / K
        assert np.array_equal(m[e], mu)
        assert np.allclose(s[e], x[:, e * K:(e + 1) * K, :].std(axis=1), rtol=1e-12, atol=1e-15)
    # alpha = 0.5 is half way between the old distribution and alpha = 1's
    m1, s1, _, _ = plan_refit_reference(x, sc, m0, s0, n_elite=3, alpha=1.0)
    mh, sh, _, _ = plan_refit_reference(x, sc, m0, s0, n_elite=3, alpha=0.5)
    assert np.array_equal(mh, 0.5 * m1 + 0.5 * m0) and np.array_equal(sh, 0.5 * s1 + 0.5 * s0)
    assert not np.array_equal(mh, m1)
    # the inputs are left alone
    assert (m0 == 0.25).all() and (s0 == 0.5).all()


def test_refit_leaves_an_unplanned_env_untouched():
    E, K, H = 3, 4, 2
    x = _table(E, K, H, 2)
    sc = np.arange(E * K, dtype=np.float64).reshape(E, K)
    m0 = np.random.RandomState(3).normal(size=(E, H, 4))
    s0 = np.full((E, H, 4), 0.3)
    m0[1] = np.nan                                                              # never read
    m, s, elite, top = plan_refit_reference(x, sc, m0, s0, n_elite=2, done=np.array([False, True, False]))
    assert np.array_equal(m[1], m0[1], equal_nan=True) and np.array_equal(s[1], s0[1])
    assert not elite[1].any() and top.tolist() == [3, -1, 3]
    full, _, _, _ = plan_refit_reference(x, sc, np.nan_to_num(m0), s0, n_elite=2)
    assert np.array_equal(m[[0, 2]], full[[0, 2]])


def test_sample_candidate_zero_zero_std_and_clipping():
    E, K, H = 3, 5, 2
    r = np.random.RandomState(4)
    mean = r.uniform(-1.5, 1.5, size=(E, H, 4))
    std = r.uniform(0.1, 0.5, size=(E, H, 4))
    x = plan_sample_reference(mean, std, LO, HI, K, seed=11, iteration=2)
    assert x.shape == (H, E * K, 4) and x.flags['C_CONTIGUOUS']
    clipped = np.clip(mean, LO, HI).transpose(1, 0, 2)                          # [H, E, 4]
    assert np.array_equal(x[:, 0::K, :], clipped)                               # candidate 0 is the clipped mean
    assert (x >= LO).all() and (x <= HI).all()
    assert (x == -1.0).any() and (x == 1.0).any()                               # both bounds are reached with means outside them
    # element by element from the definition
    for (h, slot, a) in [(0, 1, 0), (1, 7, 3), (1, E * K - 1, 2)]:
        e = slot // K
        eps = np.float64(philox_eps(11, 2, np.array([(slot * H + h) * 4 + a]))[0])
        v = mean[e, h, a] + std[e, h, a] * eps
        assert x[h, slot, a] == min(max(v, -1.0), 1.0)
    # std = 0: every candidate is the clipped mean
    x0 = plan_sample_reference(mean, np.zeros_like(std), LO, HI, K, seed=11, iteration=2)
    assert np.array_equal(x0, np.repeat(clipped, K, axis=1))
    # another iteration, other noise; the same one, the same table
    assert not np.array_equal(x, plan_sample_reference(mean, std, LO, HI, K, seed=11, iteration=3))
    assert np.array_equal(x, plan_sample_reference(mean, std, LO, HI, K, seed=11, iteration=2))


def test_score_reference():
    rec = np.zeros((3, 4), dtype=_lib.STEP_RECORD_DTYPE)
    rec['coverage'] = np.array([[0.1, 0.2, 0.3, 0.4], [0.5, 0.6, 0.7, 0.8], [0.9, 1.0, 1.1, 1.2]])
    rec['ran'] = np.array([[1, 1, 0, 1], [1, 1, 0, 0], [1, 0, 0, 0]])
    rec['oob'][1, 1] = 1          # an executed slot: counts
    rec['tear'][2, 3] = 1         # not executed: does not
    s = plan_score_reference(rec, penalty=2.0)
    assert s.tolist() == [0.9, 0.6 - 2.0, -np.inf, 0.4]


_CTYPES = {"clothhip_handle *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int32_t *": C.POINTER(C.c_int32), "int32_t": C.c_int32,
           "const double *": C.POINTER(C.c_double), "double *": C.POINTER(C.c_double), "const uint8_t *": C.POINTER(C.c_uint8),
           "uint8_t *": C.POINTER(C.c_uint8), "const ClothEpisodeParams *": C.POINTER(_lib.ClothEpisodeParams),
           "const ClothPlanParams *": C.POINTER(_lib.ClothPlanParams), "const double": C.POINTER(C.c_double)}


def test_symbols_declared_exported_bound_with_the_headers_signatures():
    hdr = open(os.path.join(ROOT, "include", "clothhip.h")).read()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    L = _lib.load()
    for name in NEW:
        m = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        types = [re.sub(r"\s*\w+(\[4\])?$", "", p.strip()).strip() for p in m.group(1).split(",")]
        assert name in bound and bound[name][0] is C.c_int, name
        assert bound[name][1] == [_CTYPES[t] for t in types], (name, types)
        assert getattr(L, name) is not None
    # the struct, field by field as the header lays it out
    m = re.search(r"typedef struct ClothPlanParams \{(.*?)\} ClothPlanParams;", hdr, re.S)
    names = re.findall(r"(\w+)(?:\[4\])?\s*[,;]", m.group(1))
    assert names == [f[0] for f in _lib.ClothPlanParams._fields_]
    assert C.sizeof(_lib.ClothPlanParams) == 80 and _lib.ClothPlanParams.alpha.offset == 32 and _lib.ClothPlanParams.min_std.offset == 48
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7                     # the change is additive
    assert L.clothhip_plan_cem(None, None, None, None, None, None, None, None, None, None, None, None) == _lib.EINVAL
    assert L.clothhip_plan_sample(None, None, None, None, 1, 0, None, None, None) == _lib.EINVAL
    assert L.clothhip_plan_refit(None, None, 1, None, None, None, None, None, None, None) == _lib.EINVAL


def test_plan_params_refuses_what_the_library_would():
    ok = dict(horizon=2, n_candidates=8, n_elite=2, n_iters=2)
    p = ClothBatch.plan_params(alpha=0.5, penalty=2.0, min_std=[0.1, 0.2, 0.3, 0.4], seed=2 ** 63 + 5, iter0=9, **ok)
    assert (p.horizon, p.n_candidates, p.n_elite, p.n_iters, p.seed, p.iter0, p.alpha, p.penalty) == (2, 8, 2, 2, 2 ** 63 + 5, 9, 0.5, 2.0)
    assert list(p.min_std) == [0.1, 0.2, 0.3, 0.4]
    for bad in [dict(horizon=0), dict(horizon=9), dict(n_candidates=1), dict(n_candidates=1025), dict(n_elite=0), dict(n_elite=9),
                dict(n_iters=0), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float('nan')), dict(penalty=float('inf')),
                dict(min_std=-0.1), dict(min_std=float('nan')), dict(seed=-1), dict(seed=2 ** 64), dict(iter0=-1), dict(iter0=2 ** 31)]:
        with pytest.raises(ValueError):
            ClothBatch.plan_params(**dict(ok, **bad))


class _Box(object):
    low, high = LO, HI


class _StubEnv(object):
    """What CEMPolicy reads of an env: E, the action space, and plan() -- which records its arguments and answers with a made-up plan."""

    def __init__(self, E=3, planned=None):
        self.E, self.action_space, self.calls = E, _Box(), []
        self.planned = np.ones(E, dtype=bool) if planned is None else np.asarray(planned)

    def plan(self, horizon, n_candidates, n_elite, n_iters, **kw):
        self.calls.append(dict(kw, horizon=horizon, n_candidates=n_candidates, n_elite=n_elite, n_iters=n_iters,
                               mean=kw['mean'].copy(), std=kw['std'].copy()))
        n = len(self.calls)
        mean = kw['mean'] + np.arange(horizon)[None, :, None] + 10.0 * n        # row h of call n: old + h + 10 n
        actions = np.where(self.planned[:, None, None], 0.01 * n + np.zeros((self.E, horizon, 4)), np.nan)
        return dict(actions=actions, score=np.where(self.planned, 1.0, np.nan), mean=mean, std=np.full_like(mean, 0.05),
                    planned=self.planned.copy())


class _Const(object):
    def __init__(self, v):
        self.v, self.seen = v, []

    def get_action(self, obs, t=0):
        self.seen.append((obs, t))
        return np.full((3, 4), self.v)


def test_cem_policy_shifts_the_mean_resets_std_and_advances_iter0():
    env = _StubEnv()
    pol = CEMPolicy(env, horizon=3, n_candidates=8, n_elite=2, n_iters=4, init_std=[0.5, 0.5, 0.2, 0.2], min_std=0.02, alpha=0.7,
                    penalty=3.0, seed=5)
    a = pol.get_action("obs0", t=0)
    c = env.calls[0]
    assert (c['horizon'], c['n_candidates'], c['n_elite'], c['n_iters']) == (3, 8, 2, 4)
    assert (c['iter0'], c['seed'], c['alpha'], c['penalty'], c['min_std']) == (0, 5, 0.7, 3.0, 0.02)
    assert np.array_equal(c['mean'], np.zeros((3, 3, 4)))
    assert np.array_equal(c['std'], np.broadcast_to([0.5, 0.5, 0.2, 0.2], (3, 3, 4)))
    assert np.array_equal(a, np.full((3, 4), 0.01)) and pol.last_plan['score'].tolist() == [1.0, 1.0, 1.0]
    # the returned mean had rows 10, 11, 12: shifted by one action, the last row repeated
    assert np.array_equal(pol.mean[:, :, 0], np.broadcast_to([11.0, 12.0, 12.0], (3, 3)))
    pol.get_action("obs1", t=1)
    c = env.calls[1]
    assert c['iter0'] == 4 and np.array_equal(c['mean'], pol.last_plan['mean'] - np.arange(3)[None, :, None] - 20.0)
    assert np.array_equal(c['mean'][:, :, 1], np.broadcast_to([11.0, 12.0, 12.0], (3, 3)))
    assert np.array_equal(c['std'], np.broadcast_to([0.5, 0.5, 0.2, 0.2], (3, 3, 4)))      # not the plan's 0.05
    assert pol.iter0 == 8


def test_cem_policy_warm_start_fills_the_first_row_and_unplanned_envs_fall_back():
    env = _StubEnv(planned=[True, False, True])
    warm = _Const(2.5)                                                          # outside the action space: the fallback is clipped
    pol = CEMPolicy(env, horizon=2, n_candidates=4, n_elite=1, n_iters=1, warm_start=warm)
    a = pol.get_action("obs", t=7)
    assert warm.seen == [("obs", 7)]
    c = env.calls[0]
    assert np.array_equal(c['mean'][:, 0], np.full((3, 4), 2.5)) and np.array_equal(c['mean'][:, 1], np.zeros((3, 4)))
    assert np.array_equal(a[[0, 2]], np.full((2, 4), 0.01)) and np.array_equal(a[1], np.ones(4))
    pol.get_action("obs", t=8)
    assert np.array_equal(env.calls[1]['mean'][:, 0], np.full((3, 4), 2.5))     # the proposal again, over the shifted mean
    assert np.array_equal(env.calls[1]['mean'][:, 1], np.full((3, 4), 11.0))
    with pytest.raises(ValueError):
        CEMPolicy(env, horizon=9)
