"""Host tests of PPO's numpy side and of the one C function that needs no device (no GPU): policies.exp_fixed_reference
against math.exp and, by bytes, against clothhip_selftest_exp_fixed; policies.ppo_reference's gradient against central differences of
its own loss; the clipping rule on hand-made rows, in ppo_reference and in ppo_loss_reference; the old mean equal to the present mean
gives the weighted regression's gradient; MLPTrainer.ppo_step's epoch tables and its target_kl stop against a stub; the bindings
against the header's signatures."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.policies import MLPTrainer, exp_fixed_reference, fit_reference, ppo_loss_reference, ppo_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_BOUND = 4.0 * 2.0 ** -53          # relative, against math.exp: twice what the prototype of the scheme measured (2.2e-16)


# ---- the exponential ----------------------------------------------------------------------------------------------------------------------
def _grid():
    r = np.random.RandomState(11)
    return np.concatenate([r.uniform(-40.0, 40.0, size=200000), np.linspace(-40.0, 40.0, 4001), [0.0, -0.0, 1e-300, -1e-300, 3.0, -3.0]])


def test_exp_fixed_reference_against_math_exp():
    x = _grid()
    got = exp_fixed_reference(x)
    want = np.array([math.exp(v) for v in x])
    rel = np.abs(got - want) / want
    print("exp_fixed_reference: max relative error %.3e over %d points (bound %.3e)" % (rel.max(), x.size, EXP_BOUND))
    assert got.dtype == np.float64 and rel.max() <= EXP_BOUND
    assert exp_fixed_reference(0.0) == 1.0 and exp_fixed_reference(-0.0) == 1.0
    # clamped beyond +-40: the value AT the bound, which is exp's within the bound
    for big in (40.5, 100.0, 1e300, np.inf):
        assert exp_fixed_reference(big) == exp_fixed_reference(40.0) and exp_fixed_reference(-big) == exp_fixed_reference(-40.0)
    assert abs(exp_fixed_reference(40.0) - math.exp(40.0)) <= EXP_BOUND * math.exp(40.0)
    assert abs(exp_fixed_reference(-40.0) - math.exp(-40.0)) <= EXP_BOUND * math.exp(-40.0)


def test_exp_fixed_reference_equals_the_c_function_by_bytes():
    L = _lib.load()
    x = np.ascontiguousarray(np.concatenate([_grid(), [40.0, -40.0, 40.5, -40.5, 1e300, -1e300, np.inf, -np.inf]]))
    out = np.zeros_like(x)
    assert L.clothhip_selftest_exp_fixed(_lib.dp(x), x.size, _lib.dp(out)) == _lib.OK
    assert out.tobytes() == exp_fixed_reference(x).tobytes()
    assert L.clothhip_selftest_exp_fixed(None, 0, None) == _lib.OK
    nan = np.array([0.0, np.nan])
    assert L.clothhip_selftest_exp_fixed(_lib.dp(nan), 2, _lib.dp(out)) == _lib.EINVAL
    assert L.clothhip_selftest_exp_fixed(None, 1, _lib.dp(out)) == _lib.EINVAL and L.clothhip_selftest_exp_fixed(_lib.dp(nan), -1, _lib.dp(out)) == _lib.EINVAL


# ---- the gradient against central differences ---------------------------------------------------------------------------------------------
def _small_net(widths, seed):
    r = np.random.RandomState(seed)
    return [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32), (0.1 * r.normal(size=widths[l + 1])).astype(np.float32))
            for l in range(len(widths) - 1)]


def _forward(layers, obs):
    h = np.asarray(obs, dtype=np.float32).astype(np.float64)
    for l, (W, b) in enumerate(layers):
        h = h @ W.astype(np.float64).T + b.astype(np.float64)
        if l + 1 < len(layers):
            h = np.maximum(h, 0.0)
    return h


SIGMA, CLIP, MARGIN = 0.7, 0.2, 0.05


def _fd_case(widths, seed):
    """A small network and 24 rows whose old means lie around the present ones, so that the ratios spread over both sides of both
    bounds; the minibatch is the first 8 rows (with one repeat) whose ratio keeps MARGIN from 1 - CLIP and 1 + CLIP -- chosen from the
    reference alone."""
    layers = _small_net(widths, seed)
    r = np.random.RandomState(100 + seed)
    obs = r.uniform(-1, 1, size=(24, widths[0])).astype(np.float32)
    mu = _forward(layers, obs)
    act = (mu + SIGMA * r.normal(size=mu.shape)).astype(np.float32)
    old = (mu + 0.3 * r.normal(size=mu.shape)).astype(np.float32)
    adv = r.normal(size=24).astype(np.float32)
    _, _, rho, _ = ppo_reference(layers, obs, act, old, adv, np.arange(24), SIGMA, CLIP)
    ok = np.minimum(np.abs(rho - (1.0 - CLIP)), np.abs(rho - (1.0 + CLIP))) > MARGIN
    above, below, inside = (np.nonzero(ok & m)[0] for m in (rho > 1.0 + CLIP, rho < 1.0 - CLIP, (rho > 1.0 - CLIP) & (rho < 1.0 + CLIP)))
    assert len(above) >= 3 and len(below) >= 3 and len(inside) >= 2, (len(above), len(below), len(inside))
    idx = np.concatenate([above[:3], below[:3], inside[:2], above[:1]])
    return layers, obs, act, old, adv, idx


@pytest.mark.parametrize("widths", [[6, 4], [6, 5, 4], [6, 7, 5, 4]], ids=lambda w: "x".join(map(str, w)))
def test_ppo_reference_gradient_against_central_differences(widths):
    layers, obs, act, old, adv, idx = _fd_case(widths, seed=len(widths))
    stats, grads, rho, active = ppo_reference(layers, obs, act, old, adv, idx, SIGMA, CLIP)
    assert np.minimum(np.abs(rho - (1.0 - CLIP)), np.abs(rho - (1.0 + CLIP))).min() > MARGIN      # no row near a kink of the loss
    assert active.any() and (~active).any() and (rho > 1.0 + CLIP).any() and (rho < 1.0 - CLIP).any()
    assert stats[1] == (~active).sum() / float(len(idx)) and stats[2] > 0.0
    h = 2.0 ** -10                                                                                    # exact in float32 beside weights of order 1
    for l in range(len(layers)):
        for part in (0, 1):
            flat = layers[l][part].reshape(-1)
            for i in range(flat.size):
                keep = flat[i]
                flat[i] = keep + np.float32(h); up = ppo_reference(layers, obs, act, old, adv, idx, SIGMA, CLIP)
                flat[i] = keep - np.float32(h); dn = ppo_reference(layers, obs, act, old, adv, idx, SIGMA, CLIP)
                flat[i] = keep
                assert np.array_equal(up[3], active) and np.array_equal(dn[3], active), (l, part, i)   # the step crossed no bound
                step = float(np.float32(keep + np.float32(h))) - float(np.float32(keep - np.float32(h)))
                g = grads[l][part].reshape(-1)[i]
                assert abs((up[0][0] - dn[0][0]) / step - g) <= 2e-3 * max(1.0, abs(g)), (l, part, i)


# ---- the clipping rule on hand-made rows --------------------------------------------------------------------------------------------------
def test_the_clipping_rule_on_hand_made_rows():
    """sigma = 1, eps = 0.2, a = 0, mu = (1, 0, 0, 0). Old mean (2, 0, 0, 0): q = 4 - 1, rho = e^1.5 above the interval; old mean 0:
    q = 0 - 1, rho = e^-0.5 below it; old mean = mu: rho = 1."""
    eye = [(np.eye(4, dtype=np.float32), np.zeros(4, dtype=np.float32))]
    mu = np.tile(np.array([1, 0, 0, 0], dtype=np.float32), (8, 1))
    act = np.zeros((8, 4), dtype=np.float32)
    above, below, same = [2, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0]
    #                 0: above A>0   1: above A<0   2: below A<0   3: below A>0   4: above A=0   5: rho=1 A>0   6: rho=1 A<0   7: below A=0
    old = np.array([above, above, below, below, above, same, same, below], dtype=np.float32)
    adv = np.array([1, -1, -1, 1, 0, 1, -1, 0], dtype=np.float32)
    want_active = np.array([False, True, False, True, True, True, True, True])
    idx = np.arange(8)
    stats, grads, rho, active = ppo_reference(eye, mu, act, old, adv, idx, 1.0, 0.2)
    assert rho[0] == math.exp(1.5) and rho[2] == math.exp(-0.5) and rho[5] == 1.0
    assert np.array_equal(active, want_active)
    st, dz, ratio, act2 = ppo_loss_reference(mu, act, old, adv, 1.0, 0.2, 8)
    assert np.array_equal(act2, want_active) and ratio[5] == 1.0 and ratio[0] > 1.2 and ratio[2] < 0.8
    assert st[1] == stats[1] == 2.0 / 8.0
    # the gradient with respect to the last layer's bias is the column sum of dz; row by row: zero where not active or A = 0
    for r in range(8):
        one = ppo_loss_reference(mu[r:r + 1], act[r:r + 1], old[r:r + 1], adv[r:r + 1], 1.0, 0.2, 1)[1][0]
        ref = ppo_reference(eye, mu, act, old, adv, idx[r:r + 1], 1.0, 0.2)[1][0][1]
        if want_active[r] and adv[r] != 0:
            assert one[0] != 0.0 and ref[0] != 0.0 and np.sign(one[0]) == np.sign(adv[r]) == np.sign(ref[0])
            assert abs(float(one[0]) - ref[0]) <= 2.0 ** -22 * abs(ref[0])
        else:
            assert np.all(one == 0.0) and np.all(ref == 0.0)
    # the surrogate of a clipped row is the clipped ratio times A: constant in mu
    assert abs(stats[0] - (-(1.2 * 1 + rho[1] * -1 + 0.8 * -1 + rho[3] * 1 + 0 + 1 - 1 + 0) / 8.0)) <= 1e-15
    assert abs(st[0] - stats[0]) <= 1e-15 and abs(st[2] - stats[2]) <= 1e-15


# ---- old mean = present mean: the weighted regression's gradient ------------------------------------------------------------------------
def _exact_case(widths, dens, seed, n_rows=12):
    """tests/test_gpu_policy_fit.py's exact case (that module needs a GPU to import): weights in {-1, 0, 1}, rows in {-2 .. 2}, labels in
    {-3 .. 3}, all integers."""
    r = np.random.RandomState(seed)
    layers = []
    for l in range(len(widths) - 1):
        shape = (widths[l + 1], widths[l])
        W = (r.randint(0, 2, size=shape) * 2 - 1) * (r.random_sample(shape) < dens)
        layers.append((W.astype(np.float32), r.randint(-1, 2, size=widths[l + 1]).astype(np.float32)))
    rows = r.randint(-2, 3, size=(n_rows, widths[0])).astype(np.float32)
    labels = r.randint(-3, 4, size=(n_rows, 4)).astype(np.float64)
    return layers, rows, labels


@pytest.mark.parametrize("widths,dens", [([300, 5, 4], 1.0), ([300, 37, 64, 4], 0.3)], ids=["300x5x4", "300x37x64x4"])
def test_old_mean_equal_to_the_present_mean_is_the_weighted_regression(widths, dens):
    """Integer data and sigma a power of two: every quantity is exact in float64, so the gradient EQUALS fit_reference's under the
    weights 2 A / sigma^2; no row is clipped and the policy has not moved."""
    layers, rows, labels = _exact_case(widths, dens, 0)
    adv = np.random.RandomState(5000).randint(-2, 4, size=len(rows)).astype(np.float32)
    old = _forward(layers, rows).astype(np.float32)
    assert np.array_equal(old.astype(np.float64), _forward(layers, rows))                             # integers: float32 holds them
    for sigma in (1.0, 0.5):
        for idx in (np.array([7, 2, 11, 0, 5, 9, 4, 1]), np.array([3]), np.array([6, 2, 6, 10, 8, 2, 6, 0])):
            stats, grads, rho, active = ppo_reference(layers, rows, labels, old, adv, idx, sigma, 0.2)
            _, want = fit_reference(layers, rows, labels, idx, weights=2.0 * adv / sigma ** 2)
            assert np.all(rho == 1.0) and active.all() and stats[1] == 0.0 and stats[2] == 0.0
            assert stats[0] == -float(adv.astype(np.float64)[idx].sum()) / len(idx)
            for (dW, db), (wW, wb) in zip(grads, want):
                assert np.array_equal(dW, wW) and np.array_equal(db, wb)
            if len(idx) > 1:
                assert any(np.count_nonzero(dW) for dW, _ in grads)


# ---- ppo_step -----------------------------------------------------------------------------------------------------------------------------
def test_epoch_tables():
    rows = np.arange(100, 110)
    tabs = MLPTrainer.ppo_epoch_tables(rows, 3, 4, seed=7)
    assert len(tabs) == 3 and all(t.shape == (2, 4) and t.dtype == np.int32 for t in tabs)           # 10 rows: two minibatches, the tail of 2 dropped
    for t in tabs:
        assert len(set(t.reshape(-1).tolist())) == 8 and set(t.reshape(-1).tolist()) <= set(rows.tolist())   # a permutation: no row twice
    assert not np.array_equal(tabs[0], tabs[1])                                                       # a new permutation per epoch
    again = MLPTrainer.ppo_epoch_tables(rows, 3, 4, seed=7)
    assert all(np.array_equal(a, b) for a, b in zip(tabs, again))
    assert not np.array_equal(MLPTrainer.ppo_epoch_tables(rows, 1, 4, seed=8)[0], tabs[0])
    r = np.random.RandomState(7)
    assert np.array_equal(tabs[0], rows[r.permutation(10)][:8].reshape(2, 4)) and np.array_equal(tabs[1], rows[r.permutation(10)][:8].reshape(2, 4))
    full = MLPTrainer.ppo_epoch_tables(rows, 1, 5, seed=1)[0]
    assert full.shape == (2, 5) and sorted(full.reshape(-1).tolist()) == rows.tolist()                # no tail: every row once
    short = MLPTrainer.ppo_epoch_tables(np.array([4, 9, 2]), 2, 64, seed=0)                           # fewer rows than a minibatch: one of all
    assert all(t.shape == (1, 3) and sorted(t[0].tolist()) == [2, 4, 9] for t in short)
    assert MLPTrainer.ppo_epoch_tables(rows, 0, 4, seed=0) == []
    for bad in (np.zeros((2, 2), dtype=int), np.zeros(0, dtype=int), np.zeros(3)):
        with pytest.raises(ValueError):
            MLPTrainer.ppo_epoch_tables(bad, 1, 4, 0)
    with pytest.raises(ValueError):
        MLPTrainer.ppo_epoch_tables(rows, 1, 0, 0)


class _StubBatch(object):
    """fit_ppo's place: records every call, returns statistics whose kl is the epoch's number times 0.01 (+ 0.001 per minibatch)."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def fit_size(self):
        return self.n

    def fit_ppo(self, table, sigma, clip, **hyper):
        e = len(self.calls)
        self.calls.append((np.array(table), sigma, clip, hyper))
        s = np.zeros((len(table), 3))
        s[:, 0], s[:, 1], s[:, 2] = -1.0 - e, 0.1 * e, 0.01 * e + 0.001 * np.arange(len(table))
        return s


class _StubEnv(object):
    pass


def _stub_trainer(n):
    t = MLPTrainer.__new__(MLPTrainer)
    t.env = _StubEnv()
    t.env.batch = _StubBatch(n)
    t.hyper = dict(optimizer='sgd', lr=0.5, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0)
    return t


def test_ppo_step_and_its_target_kl_stop():
    t = _stub_trainer(10)
    stats, epochs = t.ppo_step(5, 4, seed=3, sigma=0.3, clip=0.1)
    calls = t.env.batch.calls
    assert epochs == 5 and len(calls) == 5 and stats.shape == (10, 3)                                 # one fit_ppo call per epoch, two steps each
    want = MLPTrainer.ppo_epoch_tables(np.arange(10), 5, 4, 3)
    for (table, sigma, clip, hyper), w in zip(calls, want):
        assert np.array_equal(table, w) and sigma == 0.3 and clip == 0.1 and hyper == t.hyper
    assert np.array_equal(stats[:, 0], np.repeat(-1.0 - np.arange(5), 2))
    # mean kl of epoch e is 0.01 e + 0.0005: the first epoch above 0.02 is e = 2, after which the loop stops
    t = _stub_trainer(10)
    stats, epochs = t.ppo_step(5, 4, seed=3, sigma=0.3, target_kl=0.02)
    assert epochs == 3 and len(t.env.batch.calls) == 3 and stats.shape == (6, 3) and t.env.batch.calls[0][2] == 0.2
    t = _stub_trainer(10)
    assert t.ppo_step(5, 4, seed=3, sigma=0.3, target_kl=0.0)[1] == 1                                 # 0.0005 > 0: one epoch
    t = _stub_trainer(10)
    assert t.ppo_step(5, 4, seed=3, sigma=0.3, target_kl=1.0)[1] == 5                                 # never exceeded
    t = _stub_trainer(10)
    rows = np.array([1, 3, 5, 7, 9])
    stats, epochs = t.ppo_step(2, 2, seed=0, sigma=1.0, rows=rows)
    assert epochs == 2 and all(set(c[0].reshape(-1).tolist()) <= set(rows.tolist()) and c[0].shape == (2, 2) for c in t.env.batch.calls)
    t = _stub_trainer(0)
    with pytest.raises(ValueError):
        t.ppo_step(1, 4, seed=0, sigma=1.0)
    assert _stub_trainer(4).ppo_step(0, 4, seed=0, sigma=1.0)[0].shape == (0, 3)


# ---- the bindings -------------------------------------------------------------------------------------------------------------------------
NEW = ["clothhip_fit_data_snapshot_policy", "clothhip_fit_data_set_old_means", "clothhip_fit_data_get_old_means", "clothhip_policy_fit_ppo_grad",
       "clothhip_policy_fit_ppo", "clothhip_selftest_exp_fixed"]
_CTYPES = {"clothhip_handle *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int64_t": C.c_int64, "int32_t": C.c_int32,
           "float *": C.POINTER(C.c_float), "const float *": C.POINTER(C.c_float), "double *": C.POINTER(C.c_double),
           "const double *": C.POINTER(C.c_double), "const ClothFitParams *": C.POINTER(_lib.ClothFitParams),
           "const ClothPpoParams *": C.POINTER(_lib.ClothPpoParams)}


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
    assert re.search(r"typedef struct ClothPpoParams \{ double sigma, clip; \} ClothPpoParams;", hdr)
    assert [f[0] for f in _lib.ClothPpoParams._fields_] == ["sigma", "clip"] and C.sizeof(_lib.ClothPpoParams) == 16
    assert re.search(r"#define CLOTHHIP_PPO_STATS 3\b", hdr) and _lib.PPO_STATS == 3
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7 and re.search(r"#define CLOTHHIP_ABI_VERSION 7\b", hdr)   # the change is additive
    for call in [lambda: L.clothhip_fit_data_snapshot_policy(None, 0, 0), lambda: L.clothhip_fit_data_set_old_means(None, 0, 0, None),
                 lambda: L.clothhip_fit_data_get_old_means(None, 0, 0, None), lambda: L.clothhip_policy_fit_ppo_grad(None, None, None, 1, None, None, None),
                 lambda: L.clothhip_policy_fit_ppo(None, None, None, None, 0, 1, None)]:
        assert call() == _lib.EINVAL                                              # NULL handle: a status, no device touched


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s) before refusing its arguments" % name)


def test_wrappers_refuse_before_any_library_call():
    b = ClothBatch.__new__(ClothBatch)
    b._L, b._h, b.P, b.E, b._mlp_n_params = _NoLibrary(), None, 3, 2, 10
    for mu in (np.zeros((2, 3)), np.zeros(4), np.array([[0.0, np.nan, 0.0, 0.0]]), np.array([[1e39, 0.0, 0.0, 0.0]])):
        with pytest.raises(ValueError):
            b.fit_set_old_means(mu)
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=np.nan), dict(sigma=np.inf), dict(sigma=1e-200), dict(sigma=1.0, clip=-0.1),
               dict(sigma=1.0, clip=1.0), dict(sigma=1.0, clip=np.nan)):
        with pytest.raises(ValueError):
            b.fit_ppo_grad(np.array([0]), **kw)
        with pytest.raises(ValueError):
            b.fit_ppo(np.zeros((2, 3), dtype=int), **kw)
    for idx in (np.zeros((2, 2), dtype=int), np.zeros(0, dtype=int), np.zeros(3), np.array([0, -1])):
        with pytest.raises(ValueError):
            b.fit_ppo_grad(idx, sigma=1.0)
    with pytest.raises(ValueError):
        b.fit_ppo(np.zeros((2, 3), dtype=int), sigma=1.0, optimizer="lbfgs")
    with pytest.raises(ValueError):
        b.fit_snapshot_policy(first=-1, n=0)
    b._mlp_n_params = 0
    with pytest.raises(_lib.ClothHipError):
        b.fit_ppo_grad(np.array([0]), sigma=1.0)
    with pytest.raises(_lib.ClothHipError):
        b.fit_snapshot_policy(first=0, n=0)
