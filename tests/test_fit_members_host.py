"""Host tests of the grouped trainer's bindings and of policies.MLPEnsemble (no GPU): the bindings carry the header's signatures and the
library exports them, the ABI version stayed 7, index_table is a function of its arguments, the disagreement formula, and the argument
checks that come before anything reaches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {
    "clothhip_policy_fit_grad_members": ["clothhip_handle *", "const int32_t *", "int32_t", "const int32_t *", "int32_t", "float *", "double *"],
    "clothhip_policy_fit_members": ["clothhip_handle *", "const ClothFitParams *", "const int32_t *", "int32_t", "const int32_t *", "int32_t",
                                    "int32_t", "double *"],
    "clothhip_policy_fit_reset_members": ["clothhip_handle *", "const int32_t *", "int32_t"],
}


def _header():
    with open(os.path.join(ROOT, "include", "clothhip.h")) as fh:
        return fh.read()


def _ctype_of(c_type):
    from gym_cloth_amd import _lib
    return {"clothhip_handle *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int32_t": C.c_int32, "float *": C.POINTER(C.c_float),
            "double *": C.POINTER(C.c_double), "const ClothFitParams *": C.POINTER(_lib.ClothFitParams)}[c_type]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_bindings_carry_the_headers_signatures(name):
    from gym_cloth_amd import _lib
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "include/clothhip.h does not declare %s" % name
    declared = [re.sub(r"\s*\b\w+$", "", re.sub(r"\s+", " ", a.strip())) for a in m.group(1).split(",")]      # drop the parameter names
    assert declared == ENTRIES[name], declared
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    assert name in bound, "gym_cloth_amd._lib.SYMBOLS does not bind %s" % name
    res, args = bound[name]
    assert res is C.c_int and args == [_ctype_of(t) for t in declared]


def test_the_library_exports_the_entries_and_the_abi_stayed_7():
    from gym_cloth_amd import _lib
    assert _lib.ABI_VERSION == 7 and re.search(r"#define\s+CLOTHHIP_ABI_VERSION\s+7\b", _header())
    m = re.search(r"#define\s+CLOTHHIP_FIT_MAX_MEMBER_ROWS\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.FIT_MAX_MEMBER_ROWS == 65536
    L = _lib.load()                                            # dlopen needs no GPU
    assert L.clothhip_abi_version() == 7
    for name in ENTRIES:
        assert hasattr(L, name), name


def _bare_ensemble(G):
    from gym_cloth_amd.policies import MLPEnsemble
    ens = MLPEnsemble.__new__(MLPEnsemble)
    ens.G = G
    return ens


def test_index_table_is_a_function_of_its_arguments():
    from gym_cloth_amd.policies import MLPTrainer
    ens = _bare_ensemble(3)
    t = ens.index_table(40, 5, 7, seed=11)
    assert t.dtype == np.int32 and t.shape == (5, 3, 7) and t.min() >= 0 and t.max() < 40
    assert np.array_equal(t, np.random.RandomState(11).randint(0, 40, size=(5, 3, 7)))
    assert np.array_equal(t, _bare_ensemble(3).index_table(40, 5, 7, 11)) and not np.array_equal(t, ens.index_table(40, 5, 7, 12))
    assert not np.array_equal(t[:, 0], t[:, 1])                # every member its own minibatches
    assert ens.index_table(40, 0, 7, 11).shape == (0, 3, 7)
    same = ens.index_table(40, 5, 7, 11, bootstrap=False)
    one = MLPTrainer.index_table(40, 5, 7, 11)
    assert same.dtype == np.int32 and same.shape == (5, 3, 7) and same.flags["C_CONTIGUOUS"]
    for g in range(3):
        assert np.array_equal(same[:, g], one)
    for bad in (dict(n=0), dict(n_steps=-1), dict(batch_size=0)):
        kw = dict(n=40, n_steps=5, batch_size=7, seed=11)
        kw.update(bad)
        with pytest.raises(ValueError):
            ens.index_table(**kw)


def test_disagreement_is_the_mean_population_variance():
    from gym_cloth_amd.policies import MLPEnsemble, ensemble_disagreement
    a = np.random.RandomState(2).normal(size=(5, 9, 4))
    want = np.zeros(9)
    for i in range(9):
        for k in range(4):
            col = a[:, i, k]
            want[i] += ((col - col.mean()) ** 2).sum() / 5 / 4
    got = ensemble_disagreement(a)
    assert got.dtype == np.float64 and got.shape == (9,) and np.allclose(got, want, rtol=1e-13, atol=0)
    assert np.array_equal(got, a.var(axis=0).mean(axis=1))
    assert np.array_equal(ensemble_disagreement(np.repeat(a[:1], 4, axis=0)), np.zeros(9))      # four members that agree (their mean is exact)
    ens = _bare_ensemble(5)
    ens.actions = lambda obs: a                                # disagreement(obs) is that formula on actions(obs)
    assert np.array_equal(MLPEnsemble.disagreement(ens, None), got)
    for bad in (a[0], a[:, :, :3]):
        with pytest.raises(ValueError):
            ensemble_disagreement(bad)


class _Env(object):
    """What MLPEnsemble's constructor reads before it touches a device: P and E; set_policy would be the first device call."""
    P, E = 100, 6

    def set_policy(self, mlp):
        raise AssertionError("the argument checks come before the upload")


def _layers(widths, seed=0):
    r = np.random.RandomState(seed)
    return [(r.normal(size=(widths[l + 1], widths[l])).astype(np.float32), r.normal(size=widths[l + 1]).astype(np.float32))
            for l in range(len(widths) - 1)]


def test_ensemble_argument_checks():
    from gym_cloth_amd.policies import MLPEnsemble
    nets = [_layers([300, 5, 4], g) for g in range(3)]
    for kw in (dict(members_layers=[]),                                                       # no network
               dict(members_layers=nets[:2] + [_layers([300, 6, 4])]),                        # two shapes
               dict(members_layers=[_layers([299, 5, 4])]),                                   # not the observation's width
               dict(optimizer="rmsprop"),
               dict(lr=-1e-3), dict(lr=[1e-3, 1e-3]), dict(lr=[1e-3, float("nan"), 1e-3]), dict(beta1=1.0), dict(beta2=[0.9, 0.99, 1.5]),
               dict(eps=float("inf")), dict(momentum=-0.5), dict(lr=np.zeros((3, 1))),
               dict(member=[0, 1, 2]), dict(member=[0, 1, 2, 3, 0, 1]), dict(member=[0, 1, 2, 0, 1, -1]),
               dict(member=np.zeros(6))):                                                     # not integers
        args = dict(members_layers=nets)
        args.update(kw)
        with pytest.raises(ValueError):
            MLPEnsemble(_Env(), **args)
    with pytest.raises(AssertionError):                                                       # ... and good arguments get as far as the upload
        MLPEnsemble(_Env(), nets, lr=[1e-3, 3e-3, 1e-2], member=[2, 1, 0, 2, 1, 0])
    ens = _bare_ensemble(3)
    for bad in ([], [0, 0], [3], [-1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            ens._members(bad)
    assert ens._members(None).tolist() == [0, 1, 2] and ens._members([2, 0]).dtype == np.int32


def test_batch_refuses_bad_member_calls_before_the_library():
    """ClothBatch.fit_*_members: what the library would refuse is a ValueError first (no handle is needed to get that far)."""
    from gym_cloth_amd import _lib
    from gym_cloth_amd.batch import ClothBatch
    b = ClothBatch.__new__(ClothBatch)
    with pytest.raises(_lib.ClothHipError):
        b.fit_grad_members([0], np.zeros((1, 4), dtype=np.int32))                             # no population on this batch
    b._pop_shape = (3, 1529)
    idx = np.zeros((2, 2, 4), dtype=np.int32)
    for members, table, hyper in (([0, 0], idx, None), ([0, 3], idx, None), ([], idx, None), ([[0, 1]], idx, None), ([0.0, 1.0], idx, None),
                                  ([0, 1], idx[:, :1], None), ([0, 1], idx[0], None), ([0, 1], idx.astype(np.float64), None),
                                  ([0, 1], np.zeros((1, 2, _lib.FIT_MAX_BATCH + 1), dtype=np.int32), None),
                                  ([0, 1], idx - 1, None),
                                  ([0, 1], idx, dict(optimizer="lbfgs")), ([0, 1], idx, dict(lr=[1e-3])), ([0, 1], idx, dict(lr=-1.0)),
                                  ([0, 1], idx, dict(beta1=[0.9, 1.0])), ([0, 1], idx, dict(weight_decay=0.1))):
        with pytest.raises(ValueError):
            b.fit_members(members, table, hyper)
    with pytest.raises(ValueError):
        b.fit_grad_members([0, 1], idx)                                                       # the gradient takes [n_m, B]
    with pytest.raises(ValueError):
        b.fit_reset_members([1, 1])
