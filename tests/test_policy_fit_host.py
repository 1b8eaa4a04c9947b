"""CPU tests of the trainer's host side (clothhip_fit_data_*, clothhip_policy_fit*): the new symbols are declared, exported and bound;
ClothFitParams' ctypes mirror; policies.fit_reference against central finite differences; MLPTrainer's index table; the wrappers'
argument checks, which raise before any library call; the float32 restatements of the optimizers on a hand-computed step. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.policies import MLPTrainer, adam_reference, fit_reference, sgd_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["clothhip_fit_data_append", "clothhip_fit_data_clear", "clothhip_fit_data_size", "clothhip_policy_fit_grad", "clothhip_policy_fit",
       "clothhip_policy_fit_reset"]


def test_symbols_declared_exported_bound():
    hdr = open(os.path.join(ROOT, "include", "clothhip.h")).read()
    declared = set(re.findall(r"\b(clothhip_\w+)\s*\(", hdr))
    bound = {n for n, _, _ in _lib.SYMBOLS}
    L = _lib.load()
    for name in NEW:
        assert name in declared and name in bound, name
        assert getattr(L, name) is not None
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7                       # the change is additive
    # NULL handle: a status, no device touched
    assert L.clothhip_fit_data_append(None, None, None, 0) == _lib.EINVAL
    assert L.clothhip_fit_data_clear(None) == _lib.EINVAL
    assert L.clothhip_fit_data_size(None, None) == _lib.EINVAL
    assert L.clothhip_policy_fit_grad(None, None, 1, None, None) == _lib.EINVAL
    assert L.clothhip_policy_fit(None, None, None, 0, 1, None) == _lib.EINVAL
    assert L.clothhip_policy_fit_reset(None) == _lib.EINVAL


def test_fit_params_mirror():
    assert C.sizeof(_lib.ClothFitParams) == 24
    assert [f[0] for f in _lib.ClothFitParams._fields_] == ["optimizer", "lr", "beta1", "beta2", "eps", "momentum"]
    assert all(f[1] is C.c_float for f in _lib.ClothFitParams._fields_)
    hdr = open(os.path.join(ROOT, "include", "clothhip.h")).read()
    m = re.search(r"typedef struct ClothFitParams \{ float ([^;]*); \} ClothFitParams;", hdr)
    names = [re.sub(r"/\*.*?\*/", "", s).strip() for s in m.group(1).split(",")]
    assert names == [f[0] for f in _lib.ClothFitParams._fields_]
    assert re.search(r"CLOTHHIP_FIT_ADAM = 0, CLOTHHIP_FIT_SGD = 1", hdr) and _lib.FIT_OPTIMIZERS == {"adam": 0, "sgd": 1}
    assert int(re.search(r"#define CLOTHHIP_FIT_MAX_BATCH (\d+)", hdr).group(1)) == _lib.FIT_MAX_BATCH


def _net(widths, seed):
    r = np.random.RandomState(seed)
    return [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32),
             (r.normal(size=widths[l + 1]) * 0.5).astype(np.float32)) for l in range(len(widths) - 1)]


def test_fit_reference_against_finite_differences():
    """Every parameter of a [30, 5, 4] net on 6 rows (one of them repeated in idx): central differences in float64 on the loss
    fit_reference itself returns. The loss is piecewise quadratic, so with no pre-activation within reach of the step the central
    difference is exact up to rounding: |fd - g| <= 1e-7 (1e-10 was seen)."""
    layers = _net([30, 5, 4], seed=1)
    r = np.random.RandomState(2)
    obs = r.uniform(-1, 1, size=(6, 30)).astype(np.float32)
    lab = r.uniform(-1, 1, size=(6, 4)).astype(np.float32).astype(np.float64)
    idx = np.array([0, 1, 2, 3, 4, 5, 2])
    loss, grads = fit_reference(layers, obs, lab, idx)
    z = obs.astype(np.float64) @ layers[0][0].astype(np.float64).T + layers[0][1]
    h = 1e-4
    assert np.abs(z).min() > 50 * h and 0.2 < (z > 0).mean() < 0.8            # no kink within reach; both sides of ReLU are exercised
    worst = 0.0
    for l in range(2):
        for k in range(2):
            a = layers[l][k]
            for i in np.ndindex(a.shape):
                up = [[np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)] for W, b in layers]
                dn = [[np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)] for W, b in layers]
                up[l][k][i] += h; dn[l][k][i] -= h
                fd = (_loss64(up, obs, lab, idx) - _loss64(dn, obs, lab, idx)) / (2 * h)
                worst = max(worst, abs(fd - grads[l][k][i]))
    print("finite differences: max |fd - grad| = %.3e, loss %.6f" % (worst, loss))
    assert worst <= 1e-7
    assert abs(loss - _loss64([[W.astype(np.float64), b.astype(np.float64)] for W, b in layers], obs, lab, idx)) <= 1e-15
    assert [g[0].shape for g in grads] == [(5, 30), (4, 5)] and [g[1].shape for g in grads] == [(5,), (4,)]


def _loss64(layers, obs, lab, idx):
    """The definition, written out independently of fit_reference, on float64 weights (which fit_reference would round)."""
    x = obs.astype(np.float64)[idx]
    for l, (W, b) in enumerate(layers):
        x = x @ W.T + b
        if l + 1 < len(layers):
            x = np.where(x > 0, x, 0.0)
    return float(((x - lab[idx]) ** 2).sum() / (4 * len(idx)))


def test_index_table_is_a_function_of_the_seed():
    a = MLPTrainer.index_table(100, 7, 5, seed=3)
    assert a.dtype == np.int32 and a.shape == (7, 5) and a.min() >= 0 and a.max() < 100
    assert np.array_equal(a, MLPTrainer.index_table(100, 7, 5, seed=3))
    assert np.array_equal(a, np.random.RandomState(3).randint(0, 100, size=(7, 5)))
    assert not np.array_equal(a, MLPTrainer.index_table(100, 7, 5, seed=4))
    assert MLPTrainer.index_table(1, 0, 5, seed=0).shape == (0, 5)
    for bad in [(0, 1, 1), (5, -1, 1), (5, 1, 0)]:
        with pytest.raises(ValueError):
            MLPTrainer.index_table(*bad, seed=0)


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s) before refusing its arguments" % name)


def _bare_batch(P=4):
    b = ClothBatch.__new__(ClothBatch)
    b._L, b._h, b.P, b.E, b._mlp_n_params = _NoLibrary(), None, P, 1, 10
    return b


def test_wrappers_refuse_before_any_library_call():
    b = _bare_batch(P=4)
    ok_obs, ok_lab = np.zeros((3, 12), dtype=np.float32), np.zeros((3, 4))
    nan_lab, inf_obs, big_lab = ok_lab.copy(), ok_obs.copy(), ok_lab.copy()
    nan_lab[1, 2], inf_obs[2, 5], big_lab[0, 0] = np.nan, np.inf, 1e300          # 1e300 is finite as a double, not as the float stored
    for obs, lab in [(np.zeros((3, 11)), ok_lab), (np.zeros(12), ok_lab), (ok_obs, np.zeros((2, 4))), (ok_obs, np.zeros((3, 3))),
                     (ok_obs, nan_lab), (inf_obs, ok_lab), (ok_obs, big_lab)]:
        with pytest.raises(ValueError):
            b.fit_append(obs, lab)
    for idx in [np.zeros((2, 2), dtype=int), np.zeros(0, dtype=int), np.zeros(3), np.array([0, -1]), np.zeros(_lib.FIT_MAX_BATCH + 1, dtype=int)]:
        with pytest.raises(ValueError):
            b.fit_grad(idx)
    tbl = np.zeros((2, 3), dtype=int)
    for idx in [np.zeros(3, dtype=int), np.zeros((2, 0), dtype=int), np.zeros((2, 3)), np.full((2, 3), -1)]:
        with pytest.raises(ValueError):
            b.fit(idx)
    for kw in [dict(optimizer="adamw"), dict(lr=-1e-3), dict(lr=np.nan), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=np.inf), dict(momentum=-0.5)]:
        with pytest.raises(ValueError):
            b.fit(tbl, **kw)
    b._mlp_n_params = 0
    with pytest.raises(_lib.ClothHipError):                                       # no shared network: nothing to size the gradient by
        b.fit_grad(np.zeros(3, dtype=int))
    with pytest.raises(ValueError):
        MLPTrainer(object(), [], optimizer="rmsprop")


def test_optimizer_restatements_by_hand():
    """One parameter, values whose float32 roundings are written out: the restatements are what the header defines."""
    f = np.float32
    g, th = f(0.5), f(1.0)
    b1, b2, eps, lr = f(0.9), f(0.999), f(1e-8), f(1e-2)
    m = f(f(b1 * f(0)) + f(f(1.0 - float(b1)) * g))
    v = f(f(b2 * f(0)) + f(f(1.0 - float(b2)) * f(g * g)))
    a1 = f(float(lr) * np.sqrt(1.0 - float(b2) ** 1) / (1.0 - float(b1) ** 1))
    want = f(th - f(a1 * f(m / f(f(np.sqrt(v)) + eps))))
    got = adam_reference(np.array([th]), np.zeros(1, f), np.zeros(1, f), np.array([g]), 1, lr=1e-2)
    assert got[0].dtype == np.float32 and got[0][0] == want and got[1][0] == m and got[2][0] == v
    assert abs(float(want) - (1.0 - 1e-2)) < 1e-6                                  # the first Adam step moves by lr, whatever g's size
    th2, u2 = sgd_reference(np.array([th]), np.array([f(0.25)]), np.array([g]), lr=1e-2, momentum=0.9)
    u = f(f(f(0.9) * f(0.25)) + g)
    assert u2[0] == u and th2[0] == f(th - f(lr * u)) and th2.dtype == np.float32
