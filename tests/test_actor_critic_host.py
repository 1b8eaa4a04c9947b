"""Host tests of the actor-critic's numpy side (no GPU): policies.gae_reference against a per-episode loop written
another way, against the one-step TD error and against demos.returns_to_go; demos.episode_links on hand-made collections;
policies.value_fit_reference against central differences of its own loss; the bindings against the header's signatures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.demos import episode_links, returns_to_go
from gym_cloth_amd.policies import NEXT_NONE, NEXT_TERMINAL, gae_reference, value_fit_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_, L_ = NEXT_TERMINAL, NEXT_NONE


def chain_case(seed=0):
    """Twelve hand-made rows (shared with tests/test_gpu_actor_critic.py): row 0 a chain of ONE row that ends its episode; rows 1, 3,
    5, 7, 9 a chain of FIVE that ends in a terminal row, INTERLEAVED as [t][e] order interleaves two envs with rows 2, 4, 6, 8, a chain
    of four that ENDS IN A LEAF, row 10; row 11 a chain of one again, behind the leaf. Returns (rew float32[12], next int[12],
    episodes): the episodes as (rows, leaf row or None) for the per-episode loop."""
    r = np.random.RandomState(seed)
    nxt = np.array([T_, 3, 4, 5, 6, 7, 8, 9, 10, T_, L_, T_])
    rew = r.normal(size=12).astype(np.float32)
    rew[10] = 0.0
    return rew, nxt, [([0], None), ([1, 3, 5, 7, 9], None), ([2, 4, 6, 8], 10), ([11], None)]


def gae_by_episode(v, rew, episodes, gamma, lam):
    """The textbook recursion, backwards over each episode: A_t = delta_t + gamma lam A_t+1 -- another order of the same sum than
    gae_reference's forward accumulation, so equal to rounding only. Rows outside every episode (the leaves) keep A = 0."""
    v, rew = np.asarray(v, dtype=np.float64), np.asarray(rew, dtype=np.float64)
    A = np.zeros(len(v))
    for rows, leaf in episodes:
        nv, run = (0.0 if leaf is None else v[leaf]), 0.0
        for r in reversed(rows):
            delta = rew[r] + gamma * nv - v[r]
            run = delta + gamma * lam * run
            A[r], nv = run, v[r]
    return A


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.7), (0.5, 1.0)])
def test_gae_reference_equals_the_per_episode_loop(gamma, lam):
    rew, nxt, episodes = chain_case()
    v = np.random.RandomState(5).normal(size=12).astype(np.float32)
    adv, ret, w = gae_reference(v, rew, nxt, gamma, lam)
    A = gae_by_episode(v, rew, episodes, gamma, lam)
    leaf = nxt == L_
    assert adv.dtype == ret.dtype == w.dtype == np.float32
    assert np.abs(adv.astype(np.float64) - A).max() <= 2.0 ** -24 * np.abs(A).max() + 1e-15      # one float32 rounding of a float64 sum
    assert np.abs(ret.astype(np.float64) - np.where(leaf, v, A + v)).max() <= 2.0 ** -23 * (np.abs(A) + np.abs(v)).max()
    assert np.array_equal(w, np.where(leaf, np.float32(0), adv))                                      # w_scale 1, not normalised
    assert adv[10] == 0.0 and ret[10] == v[10] and w[10] == 0.0                                       # the leaf
    assert np.abs(A[~leaf]).min() > 0.0                                                               # no case passes on zeros


def test_gae_reference_chain_structure():
    """What each kind of chain must give, stated without the loop: a chain of one terminal row is rew - v; a row before a leaf
    bootstraps from the leaf's value; a terminal row ignores whatever v lies behind it; changing a row of the OTHER chain changes
    nothing (the interleaving is followed by `next`, not by position)."""
    rew, nxt, _ = chain_case()
    v = np.random.RandomState(6).normal(size=12).astype(np.float32)
    g, l = 0.9, 0.8
    adv, _, _ = gae_reference(v, rew, nxt, g, l)
    r64, v64 = rew.astype(np.float64), v.astype(np.float64)
    assert adv[0] == np.float32(r64[0] - v64[0]) and adv[11] == np.float32(r64[11] - v64[11])
    assert adv[9] == np.float32(r64[9] - v64[9])
    assert adv[8] == np.float32((r64[8] + g * v64[10]) - v64[8])
    v2 = v.copy(); v2[[2, 4, 6, 8, 10]] += 1.0
    a2, _, _ = gae_reference(v2, rew, nxt, g, l)
    assert np.array_equal(a2[[1, 3, 5, 7, 9, 0, 11]], adv[[1, 3, 5, 7, 9, 0, 11]]) and not np.array_equal(a2[[2, 4, 6, 8]], adv[[2, 4, 6, 8]])
    for bad in ([1, 1], [0, T_], [5, T_], [-3, T_]):                                                  # self, backward, outside, unknown
        with pytest.raises(ValueError):
            gae_reference(np.zeros(2), np.zeros(2), np.array(bad), g, l)


def test_lambda_zero_is_the_one_step_td_error():
    rew, nxt, _ = chain_case(seed=2)
    v = np.random.RandomState(7).normal(size=12).astype(np.float32)
    gamma = 0.97
    adv, ret, _ = gae_reference(v, rew, nxt, gamma, 0.0)
    v64, r64 = v.astype(np.float64), rew.astype(np.float64)
    nv = np.where(nxt >= 0, v64[np.maximum(nxt, 0)], 0.0)
    td = (r64 + gamma * nv) - v64
    leaf = nxt == L_
    assert np.array_equal(adv[~leaf], td[~leaf].astype(np.float32))
    assert np.array_equal(ret[~leaf], (td + v64)[~leaf].astype(np.float32))


def test_normalised_weights_and_scale():
    rew, nxt, _ = chain_case(seed=3)
    v = np.random.RandomState(8).normal(size=12).astype(np.float32)
    leaf = nxt == L_
    for scale in (0.5, 8.0):
        adv, _, w = gae_reference(v, rew, nxt, 0.99, 0.95, w_scale=scale, normalize=True)
        _, _, w1 = gae_reference(v, rew, nxt, 0.99, 0.95, w_scale=1.0, normalize=True)
        assert np.array_equal(w, (np.float32(scale) * w1).astype(np.float32))                         # a power of two scales exactly
        a = adv.astype(np.float64)[~leaf]
        assert np.allclose(w1[~leaf], (a - a.mean()) / (a.std() + 1e-8), rtol=1e-6, atol=1e-6) and w1[leaf].tolist() == [0.0]
    _, _, w = gae_reference(v, rew, np.full(12, L_), 0.99, 0.95, normalize=True)                      # all leaves: nothing to normalise
    assert np.array_equal(w, np.zeros(12, dtype=np.float32))


def _records(seed, T=7, E=3):
    """[T, E] record tables of a launch as step_many gives them: small-integer rewards, an episode end here and there followed by a
    reset before the next slot, env 2 stopping early (slots that did not run)."""
    r = np.random.RandomState(seed)
    rew = r.randint(-3, 4, size=(T, E)).astype(np.float64)
    ran = np.ones((T, E), dtype=bool)
    ran[5:, 2] = False
    done = (r.random_sample((T, E)) < 0.3) & ran
    rb = np.zeros((T, E), dtype=np.int64)
    rb[1:] = done[:-1]
    return rew, ran, done, rb


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gamma_lambda_one_and_a_zero_critic_equal_returns_to_go(seed):
    """An independent check against existing code: with gamma = lam = 1 and v = 0 the advantage of a row is the undiscounted
    return-to-go of its slot -- for an episode still open at the end the rewards so far, as returns_to_go counts them (the leaf
    bootstraps with the value 0). Small integers: every sum is exact, so the two are EQUAL."""
    rew, ran, done, rb = _records(seed)
    T, E = rew.shape
    G, _ = returns_to_go(rew, ran, done, rb, gamma=1.0)
    t_, e_ = np.nonzero(ran)                                                                          # [t][e] order, as rows are appended
    last_open = np.array([e for e in range(E) if not done[np.nonzero(ran[:, e])[0][-1], e]], dtype=np.int64)
    row_env = np.concatenate([e_, last_open])
    row_slot = np.concatenate([t_, np.full(len(last_open), T)])
    row_done = np.concatenate([done[t_, e_], np.zeros(len(last_open), dtype=bool)])
    nxt = episode_links(row_env, row_slot, row_done, E, first=0)
    assert len(last_open) > 0 and done.any()
    r = np.concatenate([rew[t_, e_], np.zeros(len(last_open))]).astype(np.float32)
    adv, ret, _ = gae_reference(np.zeros(len(r), dtype=np.float32), r, nxt, 1.0, 1.0)
    assert np.array_equal(adv[:len(t_)].astype(np.float64), G[t_, e_])
    assert np.array_equal(ret, adv) and np.all(adv[len(t_):] == 0.0)


def test_episode_links():
    """Two launches of 2 slots over 3 envs in [t][e] order, the second launch cut per env (env 1 did not run its second slot): env 0
    ends an episode mid-collection (slot 1) and its next row starts a new chain; env 1's last collected slot is open and is followed by
    its leaf; env 2 ends on its last slot. first = 100 offsets every successor."""
    #            launch 0: t0 e0 e1 e2 | t1 e0 e1 e2 | launch 1: t0 e0 e1 e2 | t1 e0 e2 | leaves: e0, e1
    row_env = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 2, 0, 1]
    row_slot = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 3]
    done = [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    nxt = episode_links(row_env, row_slot, done, 3, first=100)
    assert nxt.dtype == np.int32
    assert nxt.tolist() == [103, 104, 105, T_, 107, 108, 109, 112, 110, 111, T_, L_, L_]
    for i, k in enumerate(nxt):                                                                       # the library's rule: a successor lies later
        assert k < 0 or k > 100 + i
    # an env whose last row is open and has NO leaf behind it is a leaf itself: it cannot bootstrap from anything
    assert episode_links([0, 0], [0, 1], [0, 0], 1, first=0).tolist() == [1, L_]
    assert episode_links([], [], [], 2, first=5).tolist() == []
    with pytest.raises(ValueError):
        episode_links([0, 0], [1, 1], [0, 0], 1, first=0)                                             # not in time order
    with pytest.raises(ValueError):
        episode_links([0, 3], [0, 1], [0, 0], 3, first=0)


def _small_net(widths, seed):
    r = np.random.RandomState(seed)
    return [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32), (0.1 * r.normal(size=widths[l + 1])).astype(np.float32))
            for l in range(len(widths) - 1)]


@pytest.mark.parametrize("widths", [[6, 1], [6, 5, 1], [6, 7, 4, 1]], ids=lambda w: "x".join(map(str, w)))
def test_value_fit_reference_against_central_differences(widths):
    layers = _small_net(widths, seed=len(widths))
    r = np.random.RandomState(3)
    obs, ret = r.uniform(-1, 1, size=(9, widths[0])).astype(np.float32), r.uniform(-1, 1, size=9).astype(np.float32)
    idx = np.array([4, 0, 4, 8, 2])
    loss, grads = value_fit_reference(layers, obs, ret, idx)
    v = obs.astype(np.float64)[idx]
    for l, (W, b) in enumerate(layers):
        v = v @ W.astype(np.float64).T + b.astype(np.float64)
        if l + 1 < len(layers):
            v = np.maximum(v, 0.0)
    assert abs(loss - float(((v[:, 0] - ret.astype(np.float64)[idx]) ** 2).sum() / (2.0 * len(idx)))) <= 1e-15
    h = 2.0 ** -10                                                                                    # exact in float32 beside weights of order 1
    for l in range(len(layers)):
        for part in (0, 1):
            flat = layers[l][part].reshape(-1)
            for i in range(flat.size):
                keep = flat[i]
                flat[i] = keep + np.float32(h); up, _ = value_fit_reference(layers, obs, ret, idx)
                flat[i] = keep - np.float32(h); dn, _ = value_fit_reference(layers, obs, ret, idx)
                flat[i] = keep
                step = float(np.float32(keep + np.float32(h))) - float(np.float32(keep - np.float32(h)))
                assert abs((up - dn) / step - grads[l][part].reshape(-1)[i]) <= 2e-3 * max(1.0, abs(grads[l][part].reshape(-1)[i])), (l, part, i)
    with pytest.raises(ValueError):
        value_fit_reference(_small_net([6, 4], 0), obs, ret, idx)


# ---- the bindings -------------------------------------------------------------------------------------------------------------------------
NEW = ["clothhip_set_value_mlp", "clothhip_get_value_mlp", "clothhip_fit_data_set_transitions", "clothhip_fit_data_get_transitions",
       "clothhip_fit_data_set_returns", "clothhip_fit_data_get_returns", "clothhip_value_fit_grad", "clothhip_value_fit",
       "clothhip_value_fit_reset", "clothhip_value_predict", "clothhip_fit_data_gae"]
_CTYPES = {"clothhip_handle *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int32_t *": C.POINTER(C.c_int32), "int64_t": C.c_int64,
           "int32_t": C.c_int32, "size_t": C.c_size_t, "float *": C.POINTER(C.c_float), "const float *": C.POINTER(C.c_float),
           "double *": C.POINTER(C.c_double), "const ClothFitParams *": C.POINTER(_lib.ClothFitParams),
           "const ClothGaeParams *": C.POINTER(_lib.ClothGaeParams)}


def test_symbols_declared_exported_bound_with_the_headers_signatures():
    hdr = open(os.path.join(ROOT, "include", "clothhip.h")).read()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    L = _lib.load()
    for name in NEW:
        m = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        types = [re.sub(r"\s*\w+$", "", re.sub(r"/\*.*?\*/", "", p).strip()).strip() for p in m.group(1).split(",")]
        assert name in bound and bound[name][0] is C.c_int, name
        assert bound[name][1] == [_CTYPES[t] for t in types], (name, types)
        assert getattr(L, name) is not None
    assert re.search(r"CLOTHHIP_FIT_LABEL_ZERO = 3", hdr) and _lib.FIT_LABEL_ZERO == 3 and _lib.FIT_LABELS == {"expert": 0, "action": 1}
    assert re.search(r"CLOTHHIP_FIT_NEXT_TERMINAL = -1, CLOTHHIP_FIT_NEXT_NONE = -2", hdr)
    assert (_lib.FIT_NEXT_TERMINAL, _lib.FIT_NEXT_NONE) == (NEXT_TERMINAL, NEXT_NONE) == (-1, -2)
    assert re.search(r"CLOTHHIP_GAE_WRITE_WEIGHTS = 1, CLOTHHIP_GAE_NORMALIZE = 2", hdr) and (_lib.GAE_WRITE_WEIGHTS, _lib.GAE_NORMALIZE) == (1, 2)
    m = re.search(r"typedef struct ClothGaeParams \{ double gamma, lambda; float w_scale; int32_t flags", hdr)
    assert m and [f[0] for f in _lib.ClothGaeParams._fields_] == ["gamma", "lambda_", "w_scale", "flags"] and C.sizeof(_lib.ClothGaeParams) == 24
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7                     # the change is additive
    for call in [lambda: L.clothhip_set_value_mlp(None, 0, None, None, 0), lambda: L.clothhip_get_value_mlp(None, None, 0),
                 lambda: L.clothhip_fit_data_set_transitions(None, 0, 0, None, None), lambda: L.clothhip_fit_data_get_transitions(None, 0, 0, None, None),
                 lambda: L.clothhip_fit_data_set_returns(None, 0, 0, None), lambda: L.clothhip_fit_data_get_returns(None, 0, 0, None),
                 lambda: L.clothhip_value_fit_grad(None, None, 1, None, None), lambda: L.clothhip_value_fit(None, None, None, 0, 1, None),
                 lambda: L.clothhip_value_fit_reset(None), lambda: L.clothhip_value_predict(None, None, 1, None),
                 lambda: L.clothhip_fit_data_gae(None, 0, 0, None, None, None)]:
        assert call() == _lib.EINVAL                                              # NULL handle: a status, no device touched


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s) before refusing its arguments" % name)


def test_wrappers_refuse_before_any_library_call():
    b = ClothBatch.__new__(ClothBatch)
    b._L, b._h, b.P, b.E, b._val_n_params = _NoLibrary(), None, 3, 2, 10
    with pytest.raises(ValueError):
        b.set_value_mlp([(np.zeros((4, 9)), np.zeros(4))])                       # an action's width, not a value's
    for rew, nxt in [(np.array([0.0, np.nan]), np.array([1, -1])), (np.zeros(2), np.array([1.0, -1.0])), (np.zeros(2), np.array([1, -3])),
                     (np.zeros(2), np.array([1])), (np.zeros(2), np.array([2 ** 31, -1]))]:
        with pytest.raises(ValueError):
            b.fit_set_transitions(rew, nxt)
    for ret in [np.array([np.inf]), np.zeros((2, 2)), np.array([1e39])]:
        with pytest.raises(ValueError):
            b.fit_set_returns(ret)
    for idx in [np.zeros((2, 2), dtype=int), np.zeros(0, dtype=int), np.zeros(3), np.array([0, -1])]:
        with pytest.raises(ValueError):
            b.value_predict(idx)
        with pytest.raises(ValueError):
            b.value_grad(idx)
    for kw in [dict(gamma=1.5, lam=0.5), dict(gamma=0.5, lam=-0.1), dict(gamma=np.nan, lam=0.5), dict(gamma=0.5, lam=0.5, w_scale=np.inf)]:
        with pytest.raises(ValueError):
            b.fit_gae(first=0, n=0, **kw)
    with pytest.raises(ValueError):
        b.value_fit(np.zeros((2, 3), dtype=int), optimizer="lbfgs")
    b._val_n_params = 0
    with pytest.raises(_lib.ClothHipError):
        b.value_predict(np.array([0]))
