"""Host tests of PPO for a population (no GPU): the three bindings against the header's signatures; MLPEnsemble's epoch
tables against a plain loop; ppo_step's retirement rule and its NaN fill against a stub batch that returns scripted kl; the per-member
normalisation against numpy; the member_of_row demos.ppo_fit hands to the snapshot, leaves -1, against a stub; the wrappers' argument
checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.demos import member_normalize, ppo_fit
from gym_cloth_amd.policies import MLPEnsemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the bindings -------------------------------------------------------------------------------------------------------------------------
NEW = ["clothhip_fit_data_snapshot_policy_members", "clothhip_policy_fit_ppo_grad_members", "clothhip_policy_fit_ppo_members"]
_CTYPES = {"clothhip_handle *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int64_t": C.c_int64, "int32_t": C.c_int32,
           "float *": C.POINTER(C.c_float), "double *": C.POINTER(C.c_double), "const ClothFitParams *": C.POINTER(_lib.ClothFitParams),
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
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7 and re.search(r"#define CLOTHHIP_ABI_VERSION 7\b", hdr)   # the change is additive
    assert L.clothhip_fit_data_snapshot_policy_members(None, 0, 0, None) == _lib.EINVAL                 # NULL handle: a status, no device touched
    assert L.clothhip_policy_fit_ppo_grad_members(None, None, None, 1, None, 1, None, None, None) == _lib.EINVAL
    assert L.clothhip_policy_fit_ppo_members(None, None, None, None, 1, None, 0, 1, None) == _lib.EINVAL


# ---- the epoch tables -----------------------------------------------------------------------------------------------------------------------
def _tables_by_loop(rows_by_member, n_epochs, B, seed):
    r = np.random.RandomState(seed)
    steps = min(len(rows) for rows in rows_by_member) // B
    out = []
    for _ in range(n_epochs):
        epoch = [[None] * len(rows_by_member) for _ in range(steps)]
        for j, rows in enumerate(rows_by_member):
            perm = np.asarray(rows)[r.permutation(len(rows))]
            for s in range(steps):
                epoch[s][j] = perm[s * B:(s + 1) * B].tolist()
        out.append(epoch)
    return np.array(out, dtype=np.int32).reshape(n_epochs, steps, len(rows_by_member), B)


def test_epoch_tables_against_a_plain_loop():
    rows_by_member = [np.arange(100, 110), np.arange(7, 30, 2), np.array([5, 3, 200, 41, 40])]      # 10, 12 and 5 rows
    t = MLPEnsemble.ppo_epoch_tables(rows_by_member, 3, 4, seed=7)
    assert t.dtype == np.int32 and t.shape == (3, 1, 3, 4)                                           # steps = 5 // 4
    assert np.array_equal(t, _tables_by_loop(rows_by_member, 3, 4, 7))
    t = MLPEnsemble.ppo_epoch_tables(rows_by_member[:2], 4, 3, seed=1)
    assert t.shape == (4, 3, 2, 3) and np.array_equal(t, _tables_by_loop(rows_by_member[:2], 4, 3, 1))
    for e in range(4):
        for j, rows in enumerate(rows_by_member[:2]):
            seen = t[e, :, j, :].reshape(-1).tolist()
            assert set(seen) <= set(rows.tolist()) and len(set(seen)) == len(seen) == 9             # its own rows, none twice in an epoch
    assert not np.array_equal(t[0], t[1])                                                            # a new permutation per epoch
    assert np.array_equal(t, MLPEnsemble.ppo_epoch_tables(rows_by_member[:2], 4, 3, seed=1))
    assert not np.array_equal(t, MLPEnsemble.ppo_epoch_tables(rows_by_member[:2], 4, 3, seed=2))
    assert MLPEnsemble.ppo_epoch_tables(rows_by_member, 0, 4, seed=0).shape == (0, 1, 3, 4)
    with pytest.raises(ValueError, match="member 2 of the call has 5 rows"):
        MLPEnsemble.ppo_epoch_tables(rows_by_member, 1, 6, seed=0)
    for bad in ([], [np.zeros((2, 2), dtype=int)], [np.zeros(0, dtype=int)], [np.zeros(3)]):
        with pytest.raises(ValueError):
            MLPEnsemble.ppo_epoch_tables(bad, 1, 1, 0)
    with pytest.raises(ValueError):
        MLPEnsemble.ppo_epoch_tables(rows_by_member, 1, 0, 0)
    with pytest.raises(ValueError):
        MLPEnsemble.ppo_epoch_tables(rows_by_member, -1, 4, 0)


# ---- ppo_step -------------------------------------------------------------------------------------------------------------------------------
class _StubBatch(object):
    """fit_ppo_members' place: records every call; member g's kl in the epoch of the e-th call is KL[g][e] for every step."""

    def __init__(self, n, kl):
        self.n, self.kl, self.calls = n, kl, []

    def fit_size(self):
        return self.n

    def fit_ppo_members(self, members, table, sigma, clip, hyper):
        e = len(self.calls)
        self.calls.append((np.array(members), np.array(table), np.array(sigma), np.array(clip), {k: np.array(v) for k, v in hyper.items()}))
        s = np.zeros((table.shape[0], len(members), 3))
        for j, g in enumerate(members):
            s[:, j, 0], s[:, j, 1], s[:, j, 2] = 100.0 * g + e, 0.5, self.kl[int(g)][e]
        return s


class _StubEnv(object):
    pass


def _stub_ensemble(G, n, kl):
    t = MLPEnsemble.__new__(MLPEnsemble)
    t.env, t.G = _StubEnv(), G
    t.env.batch, t.env._policy_mlp = _StubBatch(n, kl), t
    t.hyper = dict(optimizer='sgd', lr=np.arange(1, G + 1) * 0.1, beta1=np.full(G, 0.9), beta2=np.full(G, 0.999), eps=np.full(G, 1e-8),
                   momentum=np.zeros(G))
    return t


def test_ppo_step_retires_members_and_fills_nan():
    kl = {0: [0.01, 0.03, 0.0, 0.0], 1: [0.05, 0.0, 0.0, 0.0], 2: [0.0, 0.0, 0.0, 0.0]}      # target 0.02: 1 retires after epoch 0, 0 after epoch 1
    rows = [np.arange(0, 8), np.arange(8, 16), np.arange(16, 28)]
    t = _stub_ensemble(3, 28, kl)
    stats, epochs = t.ppo_step(4, 4, seed=5, sigma=[0.1, 0.2, 0.3], clip=0.25, target_kl=0.02, rows_by_member=rows)
    calls = t.env.batch.calls
    tables = MLPEnsemble.ppo_epoch_tables(rows, 4, 4, 5)
    assert tables.shape == (4, 2, 3, 4) and stats.shape == (8, 3, 3) and stats.dtype == np.float64
    assert [c[0].tolist() for c in calls] == [[0, 1, 2], [0, 2], [2], [2]] and epochs.tolist() == [2, 1, 4]
    live = [[0, 1, 2], [0, 2], [2], [2]]
    for e, c in enumerate(calls):
        assert np.array_equal(c[1], tables[e][:, live[e]]) and c[1].flags['C_CONTIGUOUS']
        assert np.array_equal(c[2], np.array([0.1, 0.2, 0.3])[live[e]]) and np.array_equal(c[3], np.full(len(live[e]), 0.25))
        assert c[4]['optimizer'] == 'sgd' and np.array_equal(c[4]['lr'], (np.arange(1, 4) * 0.1)[live[e]])
    ran = np.zeros((8, 3), dtype=bool)
    ran[:4, 0] = ran[:2, 1] = ran[:, 2] = True
    assert np.array_equal(np.isnan(stats).all(axis=2), ~ran) and np.array_equal(np.isnan(stats).any(axis=2), ~ran)
    assert stats[2, 0].tolist() == [1.0, 0.5, 0.03] and stats[7, 2].tolist() == [203.0, 0.5, 0.0]
    # no target: nobody retires; a subset of the members: sigma and the hyper-parameters are the members' own
    t = _stub_ensemble(3, 28, kl)
    stats, epochs = t.ppo_step(2, 4, seed=5, sigma=0.5, members=[2, 0], rows_by_member=[rows[2], rows[0]])
    assert epochs.tolist() == [2, 2] and not np.isnan(stats).any() and stats.shape == (4, 2, 3)
    assert all(c[0].tolist() == [2, 0] and np.array_equal(c[4]['lr'], (np.arange(1, 4) * 0.1)[[2, 0]]) and c[2].tolist() == [0.5, 0.5] and c[3].tolist() == [0.2, 0.2]
               for c in t.env.batch.calls)
    # the mean over the epoch's steps decides, and every member retired ends the loop
    t = _stub_ensemble(2, 8, {0: [0.5] * 3, 1: [0.5] * 3})
    stats, epochs = t.ppo_step(3, 4, seed=0, sigma=1.0, target_kl=0.0)
    assert epochs.tolist() == [1, 1] and len(t.env.batch.calls) == 1 and np.isnan(stats[2:]).all() and not np.isnan(stats[:2]).any()
    # rows_by_member=None: every member takes all rows of the dataset
    t = _stub_ensemble(2, 8, {0: [0.0], 1: [0.0]})
    t.ppo_step(1, 4, seed=0, sigma=1.0)
    assert t.env.batch.calls[0][1].shape == (2, 2, 4) and sorted(t.env.batch.calls[0][1][:, 1].reshape(-1).tolist()) == list(range(8))
    for kw in (dict(sigma=[1.0, 2.0, 3.0]), dict(sigma=1.0, clip=[0.1, 0.2, 0.3]), dict(sigma=1.0, rows_by_member=[np.arange(8)]),
               dict(sigma=1.0, members=[0, 0]), dict(sigma=1.0, members=[2])):
        with pytest.raises(ValueError):
            _stub_ensemble(2, 8, {0: [0.0], 1: [0.0]}).ppo_step(1, 4, seed=0, **kw)
    with pytest.raises(ValueError):
        _stub_ensemble(2, 0, {}).ppo_step(1, 4, seed=0, sigma=1.0)
    other = _stub_ensemble(2, 8, {0: [0.0], 1: [0.0]})
    other.env._policy_mlp = object()                                                                  # another network was put on the env
    with pytest.raises(ValueError, match="another network"):
        other.ppo_step(1, 4, seed=0, sigma=1.0)
    assert other.env.batch.calls == []


# ---- the per-member normalisation -------------------------------------------------------------------------------------------------------------
def test_member_normalize_against_numpy():
    r = np.random.RandomState(3)
    adv = r.normal(size=50).astype(np.float32)
    mor = r.randint(-1, 3, size=50)
    mor[:3] = [2, -1, 0]
    w = member_normalize(adv, mor)
    assert w.dtype == np.float32 and w.shape == (50,) and not w[mor == -1].any() and (mor == -1).any()
    for g in range(3):
        A = adv[mor == g].astype(np.float64)
        want = ((A - A.sum() / len(A)) / (np.sqrt(((A - A.sum() / len(A)) ** 2).sum() / len(A)) + 1e-8)).astype(np.float32)
        assert np.array_equal(w[mor == g], want) and len(A) > 2
        assert abs(float(w[mor == g].astype(np.float64).mean())) < 1e-6 and abs(float(w[mor == g].astype(np.float64).std()) - 1.0) < 1e-6
    # a member's rows are normalised over ITS rows: a shift of another member's advantages changes nothing of it
    shifted = adv.copy()
    shifted[mor == 1] += 10.0
    assert np.array_equal(member_normalize(shifted, mor)[mor != 1], w[mor != 1])
    assert member_normalize(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=int)).shape == (0,)
    assert member_normalize(np.array([3.0], dtype=np.float32), np.array([0])).tolist() == [0.0]      # one row: A - mean = 0
    with pytest.raises(ValueError):
        member_normalize(adv, mor[:-1])


# ---- demos.ppo_fit with an ensemble -----------------------------------------------------------------------------------------------------------
class _FitBatch(object):
    def __init__(self, adv, nxt, log):
        self.adv, self.nxt, self.log = adv, nxt, log

    def fit_gae(self, gamma, lam, first, n, write_weights, normalize, w_scale):
        self.log.append(("gae", first, n, write_weights, normalize, w_scale))
        return self.adv, np.zeros(n, dtype=np.float32)

    def fit_get_transitions(self):
        return np.zeros(len(self.nxt), dtype=np.float32), self.nxt


class _FitEnsemble(object):
    def __init__(self, env, member, log):
        self.env, self.member, self.log = env, np.asarray(member, dtype=np.int32), log

    def set_weights(self, w, first):
        self.log.append(("set_weights", np.array(w), first))

    def snapshot_old(self, member_of_row, first=0):
        self.log.append(("snapshot_old", np.array(member_of_row), first))

    def ppo_step(self, n_epochs, batch_size, seed, sigma, clip=0.2, target_kl=None, rows_by_member=None, members=None):
        self.log.append(("ppo_step", n_epochs, batch_size, seed, sigma, clip, target_kl, [np.array(r) for r in rows_by_member], np.array(members)))
        return np.zeros((n_epochs, len(members), 3)), np.full(len(members), n_epochs)

    def size(self):
        return 107


class _FitCritic(object):
    def __init__(self, env, log):
        self.env, self.log = env, log

    def step(self, n_steps, batch_size, seed, rows=None):
        self.log.append(("critic", n_steps, np.array(rows)))
        return np.zeros(n_steps)


def test_ppo_fit_hands_the_acting_member_of_every_row_to_the_snapshot():
    log = []
    env = _StubEnv()
    ds_env = np.array([0, 1, 2, 3, 0, 1, 2, 3, 1, 3])                      # 4 envs, two slots each, then the leaves of envs 1 and 3
    leaf = np.array([False] * 8 + [True, True])
    member = [2, 0, 2, 0]                                                   # member 1 runs no env
    adv = np.array([1, 2, 3, 4, 5, 6, 7, 9, 0, 0], dtype=np.float32)
    nxt = np.concatenate([np.full(100, _lib.FIT_NEXT_TERMINAL), np.where(leaf, _lib.FIT_NEXT_NONE, _lib.FIT_NEXT_TERMINAL)]).astype(np.int32)
    env.batch = _FitBatch(adv, nxt, log)
    ens, critic = _FitEnsemble(env, member, log), _FitCritic(env, log)
    col = dict(first=100, appended=8, open_rows=2, leaf=leaf, ds_env=ds_env, nonleaf=100 + np.arange(8))
    out = ppo_fit(env, ens, critic, col, sigma=[0.1, 0.2, 0.3], gamma=0.9, lam=0.8, clip=0.1, n_value_steps=3, n_epochs=2, batch_size=4, seed=6, target_kl=0.5)
    want_mor = np.array([2, 0, 2, 0, 2, 0, 2, 0, -1, -1])
    assert [e[0] for e in log] == ["gae", "set_weights", "snapshot_old", "critic", "ppo_step"]      # one call each, the snapshot before any step
    assert log[0] == ("gae", 100, 10, True, False, 1.0)
    assert np.array_equal(log[1][1], member_normalize(adv, want_mor)) and log[1][2] == 100
    assert np.array_equal(log[2][1], want_mor) and log[2][1].dtype == np.int32 and log[2][2] == 100
    assert log[3][1] == 3 and np.array_equal(log[3][2], np.arange(108))                               # the critic: the non-leaf rows of the whole dataset
    step = log[4]
    assert step[1:7] == (2, 4, 6, [0.1, 0.2, 0.3], 0.1, 0.5) and step[8].tolist() == [0, 2]            # the members that have rows
    assert [r.tolist() for r in step[7]] == [[101, 103, 105, 107], [100, 102, 104, 106]]
    assert out['members'].tolist() == [0, 2] and np.array_equal(out['member_of_row'], want_mor) and out['epochs'].tolist() == [2, 2]
    assert out['ppo_stats'].shape == (2, 2, 3) and out['rows'] == 107 and out['adv'] is adv
    # normalize=False: the device's advantages stay, no weights are written from the host
    del log[:]
    ppo_fit(env, ens, critic, col, sigma=0.1, normalize=False)
    assert [e[0] for e in log] == ["gae", "snapshot_old", "critic", "ppo_step"]
    # a population has no learned head
    for kw in (dict(sigma=None), dict(sigma=0.1, ent_coef=0.01)):
        with pytest.raises(ValueError):
            ppo_fit(env, ens, critic, col, **kw)
    with pytest.raises(ValueError):
        ppo_fit(_StubEnv(), ens, critic, col, sigma=0.1)


# ---- the argument checks ------------------------------------------------------------------------------------------------------------------
class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s) before refusing its arguments" % name)


def test_wrappers_refuse_before_any_library_call():
    b = ClothBatch.__new__(ClothBatch)
    b._L, b._h, b.P, b.E, b._pop_shape = _NoLibrary(), None, 3, 2, (3, 10)
    for mor in (np.zeros((2, 2), dtype=int), np.zeros(3), np.array([0, 3]), np.array([-2, 0])):
        with pytest.raises(ValueError):
            b.fit_snapshot_policy_members(mor)
    with pytest.raises(ValueError):
        b.fit_snapshot_policy_members(np.array([0, -1]), first=-1)
    idx2, idx3 = np.zeros((2, 3), dtype=int), np.zeros((1, 2, 3), dtype=int)
    for kw in (dict(sigma=0.0), dict(sigma=[1.0, -1.0]), dict(sigma=np.nan), dict(sigma=[1.0, np.inf]), dict(sigma=1e-200), dict(sigma=1.0, clip=-0.1),
               dict(sigma=1.0, clip=[0.1, 1.0]), dict(sigma=1.0, clip=np.nan), dict(sigma=[1.0, 1.0, 1.0]), dict(sigma=1.0, clip=[0.1, 0.1, 0.1]),
               dict(sigma=np.ones((2, 1)))):
        with pytest.raises(ValueError):
            b.fit_ppo_grad_members([2, 0], idx2, **kw)
        with pytest.raises(ValueError):
            b.fit_ppo_members([2, 0], idx3, **kw)
    for members in ([0, 0], [3], [-1], [], [[0]], [0.5]):
        with pytest.raises(ValueError):
            b.fit_ppo_grad_members(members, idx2[:len(members)] if len(members) else idx2, sigma=1.0)
        with pytest.raises(ValueError):
            b.fit_ppo_members(members, idx3, sigma=1.0)
    for idx in (np.zeros((3, 3), dtype=int), np.zeros(3, dtype=int), np.zeros((2, 0), dtype=int), np.zeros((2, 3)), np.array([[0, -1, 0], [0, 0, 0]])):
        with pytest.raises(ValueError):
            b.fit_ppo_grad_members([2, 0], idx, sigma=1.0)
    with pytest.raises(ValueError):
        b.fit_ppo_members([2, 0], idx2, sigma=1.0)                                                    # a table of steps has three dimensions
    with pytest.raises(ValueError):
        b.fit_ppo_members([2, 0], idx3, sigma=1.0, hyper=dict(optimizer="lbfgs"))
    with pytest.raises(ValueError):
        b.fit_ppo_members([2, 0], idx3, sigma=1.0, hyper=dict(lr=[1e-3, 1e-3, 1e-3]))
    b._pop_shape = None
    with pytest.raises(_lib.ClothHipError):
        b.fit_ppo_grad_members([0], idx2[:1], sigma=1.0)
    with pytest.raises(_lib.ClothHipError):
        b.fit_ppo_members([0], idx3[:, :1], sigma=1.0)
    with pytest.raises(_lib.ClothHipError):
        b.fit_snapshot_policy_members(np.array([0]))
