"""CPU tests of the host half of fitting from reward: demos.returns_to_go against a per-env Python loop on hand-made
tables -- an episode ending mid-table, a reset before slot 0, idle tail slots, two discounts, a carry across two tables --, the three
weighting schemes of demos.reward_weights, policies.fit_reference's weighted gradient against central differences of its own weighted
loss, the new entries declared, exported and bound with the header's signatures, and the wrappers' refusals. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.demos import returns_carry, returns_to_go, reward_weights
from gym_cloth_amd.policies import fit_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["clothhip_fit_data_set_weights", "clothhip_fit_data_get_weights", "clothhip_fit_data_append_weighted",
       "clothhip_fit_data_append_launch_ex", "clothhip_policy_fit_predict", "clothhip_policy_fit_predict_members"]


# ---- returns_to_go ------------------------------------------------------------------------------------------------------------------------
def _tables():
    """T = 6 slots, E = 5 envs, by hand. env 0: one episode through the whole table, never done (open). env 1: an episode that ends at
    slot 2, a reset before slot 3, the next episode open. env 2: a reset before slot 0, done at slot 1, a reset before slot 2, done at
    slot 5. env 3: done at slot 1, then idle (no reset left): a tail of slots that did not run. env 4: runs two slots, not done, then
    idle (a time slice cut it)."""
    T, E = 6, 5
    ran = np.ones((T, E), dtype=bool)
    done = np.zeros((T, E), dtype=bool)
    rb = np.zeros((T, E), dtype=np.int64)
    done[2, 1] = True; rb[3, 1] = 1
    rb[0, 2] = 1; done[1, 2] = True; rb[2, 2] = 2; done[5, 2] = True
    done[1, 3] = True; ran[2:, 3] = False
    ran[2:, 4] = False
    rew = np.random.RandomState(3).normal(size=(T, E))
    rew[~ran] = 123.0                                                      # what a slot that did not run holds must not matter
    return rew, ran, done, rb


def _loop(rew, ran, done, rb, gamma):
    """Per env, forward in time: cut the column into episodes, then the discounted sums from the back of each episode."""
    T, E = rew.shape
    G, complete = np.zeros((T, E)), np.zeros((T, E), dtype=bool)
    for e in range(E):
        episodes, cur = [], []
        for t in range(T):
            if not ran[t, e]:
                if cur:
                    episodes.append((cur, False))
                cur = []
                continue
            if cur and rb[t, e] > 0:
                episodes.append((cur, False))
                cur = []
            cur.append(t)
            if done[t, e]:
                episodes.append((cur, True))
                cur = []
        if cur:
            episodes.append((cur, False))
        for slots, ended in episodes:
            acc = 0.0
            for t in reversed(slots):
                acc = rew[t, e] + (gamma * acc if t != slots[-1] else 0.0)
                G[t, e] = acc
                complete[t, e] = ended
    return G, complete


@pytest.mark.parametrize("gamma", [1.0, 0.5])
def test_returns_to_go_is_the_per_env_loop(gamma):
    rew, ran, done, rb = _tables()
    G, complete = returns_to_go(rew, ran, done, rb, gamma)
    want_G, want_c = _loop(rew, ran, done, rb, gamma)
    assert G.dtype == np.float64 and complete.dtype == bool
    assert np.array_equal(G, want_G) and np.array_equal(complete, want_c)
    # the cases by hand
    assert not complete[:, 0].any() and G[5, 0] == rew[5, 0] and G[4, 0] == rew[4, 0] + gamma * rew[5, 0]
    assert complete[:3, 1].all() and not complete[3:, 1].any() and G[2, 1] == rew[2, 1] and G[3, 1] == rew[3, 1] + gamma * G[4, 1]
    assert complete[:, 2].all() and G[1, 2] == rew[1, 2] and G[0, 2] == rew[0, 2] + gamma * rew[1, 2]
    assert complete[:2, 3].all() and (G[2:, 3] == 0).all() and not complete[2:, 3].any()
    assert not complete[:, 4].any() and G[1, 4] == rew[1, 4] and (G[2:, 4] == 0).all()


@pytest.mark.parametrize("gamma", [1.0, 0.5])
@pytest.mark.parametrize("cut", [1, 2, 3, 4])
def test_a_carry_chains_two_tables(gamma, cut):
    """The table cut in two the way time slices cut it -- every env at its own slot, so the first table has idle tails and the second
    starts each env at slot 0 --, the later table first and its returns_carry handed to the earlier one: the returns of one table."""
    rew, ran, done, rb = _tables()
    T, E = rew.shape
    whole_G, whole_c = returns_to_go(rew, ran, done, rb, gamma)
    cuts = [cut, T, max(cut - 1, 1), cut, 0]                                 # env 1 all in the first table, env 4 all in the second
    A = [np.zeros_like(x) for x in (rew, ran, done, rb)]
    Bt = [np.zeros_like(x) for x in (rew, ran, done, rb)]
    for e in range(E):
        c = cuts[e]
        for src, a, b in zip((rew, ran, done, rb), A, Bt):
            a[:c, e] = src[:c, e]
            b[:T - c, e] = src[c:, e]
    GB, cB = returns_to_go(*Bt, gamma)
    carry = returns_carry(GB, cB, Bt[1], Bt[3])
    GA, cA = returns_to_go(*A, gamma, carry=carry)
    for e in range(E):
        c = cuts[e]
        assert np.array_equal(GA[:c, e], whole_G[:c, e]) and np.array_equal(cA[:c, e], whole_c[:c, e]), e
        assert np.array_equal(GB[:T - c, e], whole_G[c:, e]) and np.array_equal(cB[:T - c, e], whole_c[c:, e]), e
    # without the carry the first table's last episodes are open; an env the second table never ran passes ITS carry through
    G0, c0 = returns_to_go(*A, gamma)
    assert not c0[cuts[0] - 1, 0] and G0[cuts[0] - 1, 0] == rew[cuts[0] - 1, 0]
    through = returns_carry(GA, cA, A[1], A[3], carry)
    assert through[0][4] == carry[0][4] and through[1][4] == carry[1][4] and through[2][4] == carry[2][4]
    with pytest.raises(ValueError):
        returns_to_go(rew, ran, done[:-1], rb, gamma)


# ---- reward_weights -----------------------------------------------------------------------------------------------------------------------
def test_the_three_schemes():
    G = np.array([1.0, 4.0, 2.0, 4.0, -3.0, 0.5])
    a = reward_weights(G, "advantage")
    assert a.dtype == np.float32 and np.array_equal(a, ((G - G.mean()) / (G.std() + 1e-8)).astype(np.float32))
    assert (a < 0).any() and (a > 0).any() and abs(float(a.astype(np.float64).sum())) < 1e-5
    x = reward_weights(G, "exp", temperature=0.5, w_max=5.0)
    want = np.minimum(np.exp((G - G.mean()) / 0.5), 5.0).astype(np.float32)
    assert x.dtype == np.float32 and np.array_equal(x, want)
    assert (x == 5.0).sum() == 2 and (x < 5.0).sum() == 4                      # the clip took the two best, and only them
    assert np.array_equal(reward_weights(G, "exp"), np.minimum(np.exp(G - G.mean()), 20.0).astype(np.float32))
    # filter: the best quarter, ties at the quantile included
    f = reward_weights(G, "filter", q=0.25)
    assert f.dtype == np.float32 and np.array_equal(f, [0, 1, 0, 1, 0, 0])    # the 0.75 quantile is 3.5: both 4s
    ties = np.array([2.0, 5.0, 2.0, 2.0, 1.0, 2.0, 0.0, 2.0])
    thr = np.quantile(ties, 0.5)
    assert thr == 2.0 and np.array_equal(reward_weights(ties, "filter", q=0.5), (ties >= 2.0).astype(np.float32))
    assert reward_weights(ties, "filter", q=0.5).sum() == 6                    # every tie at the quantile is kept
    assert np.array_equal(reward_weights(G, "filter", q=1.0), np.ones(6, dtype=np.float32))
    # a callable, and an empty vector
    c = reward_weights(G, lambda g, scale: scale * g, scale=2.0)
    assert c.dtype == np.float32 and np.array_equal(c, (2.0 * G).astype(np.float32))
    for scheme in ("advantage", "exp", "filter"):
        assert reward_weights(np.zeros(0), scheme).shape == (0,)
    for bad in [lambda: reward_weights(G, "nope"), lambda: reward_weights(G, "filter", q=0.0), lambda: reward_weights(G, "exp", temperature=0.0),
                lambda: reward_weights(G, "advantage", q=0.5), lambda: reward_weights(G, lambda g: g[:2]),
                lambda: reward_weights(G, lambda g: g * np.inf)]:
        with pytest.raises(ValueError):
            bad()


# ---- fit_reference(weights=) --------------------------------------------------------------------------------------------------------------
def _case(seed=0, widths=(7, 5, 6, 4), n=9):
    r = np.random.RandomState(seed)
    layers = [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32),
               (r.normal(size=widths[l + 1]) * 0.3).astype(np.float32)) for l in range(len(widths) - 1)]
    obs = r.uniform(-1, 1, size=(n, widths[0])).astype(np.float32)
    labels = r.uniform(-1, 1, size=(n, 4)).astype(np.float32).astype(np.float64)
    w = r.normal(size=n).astype(np.float32)
    w[2] = 0.0
    return layers, obs, labels, w


def test_weighted_gradient_is_the_derivative_of_the_weighted_loss():
    """Central differences of fit_reference's own weighted loss in float64 (steps that are float32 values, so the perturbed weights
    survive fit_reference's rounding to float32): the loss is piecewise quadratic, so away from a ReLU kink the central difference is
    exact up to rounding."""
    layers, obs, labels, w = _case()
    idx = np.array([4, 0, 2, 7, 7, 1])
    assert (w[idx] < 0).any() and (w[idx] > 0).any() and (w[idx] == 0).any()
    loss, grads = fit_reference(layers, obs, labels, idx, weights=w)
    h = 2.0 ** -10
    checked = 0
    for l, (W, b) in enumerate(layers):
        for k, arr in enumerate((W, b)):
            for pos in list(np.ndindex(arr.shape))[::3]:
                def at(d):
                    ls = [(Wl.copy(), bl.copy()) for Wl, bl in layers]
                    ls[l][k][pos] = np.float32(arr[pos] + d)
                    assert float(ls[l][k][pos]) - float(arr[pos]) == d           # the step survived the rounding
                    return fit_reference(ls, obs, labels, idx, weights=w)[0]
                fd = (at(h) - at(-h)) / (2.0 * h)
                assert abs(fd - grads[l][k][pos]) <= 1e-9 + 1e-7 * abs(fd), (l, k, pos, fd, grads[l][k][pos])
                checked += 1
    assert checked > 30
    # the weights matter, and the normaliser is B whatever they sum to
    plain, plain_g = fit_reference(layers, obs, labels, idx)
    assert loss != plain and not np.allclose(grads[0][0], plain_g[0][0])
    twice, twice_g = fit_reference(layers, obs, labels, idx, weights=2.0 * w)
    assert twice == 2.0 * loss and all(np.array_equal(2.0 * a, c) and np.array_equal(2.0 * bb, d) for (a, bb), (c, d) in zip(grads, twice_g))


def test_no_weights_is_weights_of_one_exactly():
    layers, obs, labels, _ = _case(seed=1)
    idx = np.array([3, 3, 8, 0, 5])
    a, ga = fit_reference(layers, obs, labels, idx)
    b, gb = fit_reference(layers, obs, labels, idx, weights=np.ones(len(obs)))
    assert a == b
    for (Wa, ba), (Wb, bb) in zip(ga, gb):
        assert np.array_equal(Wa, Wb) and np.array_equal(ba, bb)


# ---- the bindings -------------------------------------------------------------------------------------------------------------------------
_CTYPES = {"clothhip_handle *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int64_t": C.c_int64, "int32_t": C.c_int32,
           "float *": C.POINTER(C.c_float), "const float *": C.POINTER(C.c_float), "const double *": C.POINTER(C.c_double)}


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
    assert re.search(r"CLOTHHIP_FIT_LABEL_EXPERT = 0, CLOTHHIP_FIT_LABEL_ACTION = 1", hdr)
    assert (_lib.FIT_LABEL_EXPERT, _lib.FIT_LABEL_ACTION) == (0, 1) and _lib.FIT_LABELS == {"expert": 0, "action": 1}
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7                     # the change is additive
    assert "no per-row weights" not in hdr
    for call in [lambda: L.clothhip_fit_data_set_weights(None, 0, 0, None), lambda: L.clothhip_fit_data_get_weights(None, 0, 0, None),
                 lambda: L.clothhip_fit_data_append_weighted(None, None, None, None, 0),
                 lambda: L.clothhip_fit_data_append_launch_ex(None, None, 0, 0, None), lambda: L.clothhip_policy_fit_predict(None, None, 1, None),
                 lambda: L.clothhip_policy_fit_predict_members(None, None, 1, None, 1, None)]:
        assert call() == _lib.EINVAL                                              # NULL handle: a status, no device touched


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s) before refusing its arguments" % name)


def test_wrappers_refuse_before_any_library_call():
    b = ClothBatch.__new__(ClothBatch)
    b._L, b._h, b.P, b.E, b._mlp_n_params = _NoLibrary(), None, 3, 2, 10
    obs, lab = np.zeros((2, 9), dtype=np.float32), np.zeros((2, 4))
    for w in [np.zeros(3), np.zeros((2, 1)), np.array([0.0, np.nan]), np.array([np.inf, 1.0]), np.array([1e39, 1.0])]:
        with pytest.raises(ValueError):
            b.fit_append(obs, lab, weights=w)
        with pytest.raises(ValueError):
            b.fit_append_launch(np.zeros((2, 3), dtype=int), labels="action", weights=w)
    with pytest.raises(ValueError):
        b.fit_append_launch(np.zeros((2, 3), dtype=int), labels="oracle")
    for w in [np.array([np.nan]), np.zeros((2, 2)), np.array([-np.inf, 0.0])]:
        with pytest.raises(ValueError):
            b.fit_set_weights(w)
    with pytest.raises(ValueError):
        b.fit_get_weights(-1, 1)
    for idx in [np.zeros((2, 2), dtype=int), np.zeros(0, dtype=int), np.zeros(3), np.array([0, -1])]:
        with pytest.raises(ValueError):
            b.fit_predict(idx)
