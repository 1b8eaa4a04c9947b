"""GPU tests of the dataset rows appended where they lie on the device (clothhip_fit_hold, clothhip_fit_data_append_launch, k_fit_gather;
DESIGN 4.3.5): the device route stores the bytes the host route stores, on two grids and in both precisions; growth keeps the rows; a
NaN label appends nothing; every refusal of the header; a time-sliced collection stores, env by env, the rows of one whole launch; a
launch that keeps its tables on the device is otherwise the launch that downloads them; clothhip_policy_fit_loss against
clothhip_policy_fit_grad; the gradient over device-appended rows. Every comparison is array_equal or by bytes."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_dagger import CHECKER, CHOICES, E, _RECORDS, _bits, _env, _layers
from test_gpu_policy_fit import _exact_case

pytestmark = pytest.mark.gpu

T = 4


def _trainer(v, seed=21):
    from gym_cloth_amd.policies import MLPTrainer
    return MLPTrainer(v, _layers([3 * v.P, 5, 4], seed))


def _launch_rows(out):
    """(rows int32[n, 3], t, e) of the slots that ran, in [t][e] order: what slot_start_sources names, and the label row t * E + e."""
    from gym_cloth_amd.envs import slot_start_sources
    t_, e_ = np.nonzero(out["ran"])
    return np.concatenate([slot_start_sources(out)[t_, e_], (t_ * E + e_)[:, None].astype(np.int32)], axis=1), t_, e_


def _both_routes(prec, n_side, expert, choices=None, order=None):
    """hold, one armed launch with resets inside (episodes of two actions) that also downloads its tables, the device route's append
    -> (trainer, env, out, rows, what the host route would store: obs float32[n, 3P], labels float32[n, 4])."""
    from gym_cloth_amd import _lib
    from gym_cloth_amd.envs import slot_start_obs
    v = _env(prec, n_side=n_side, max_actions=2)
    v.reset()
    tr = _trainer(v)
    before = np.asarray(v.state, dtype=np.float32).reshape(E, -1)
    v.batch.fit_hold()
    out = v.step_many(policy="mlp", n_actions=T, want_obs=True, expert=expert, expert_mix=CHECKER, expert_choices=choices)
    rows, t_, e_ = _launch_rows(out)
    # a test error, not a pass, if a class of row is missing: slot 0 on the held row, slots after a reset, plain slots
    src = rows[:, 0]
    assert (src == _lib.FIT_SRC_HELD).any() and (src == _lib.FIT_SRC_RESETS).any() and (src == _lib.FIT_SRC_SLOTS).any(), src
    assert ((t_ == 0) & (src == _lib.FIT_SRC_HELD)).sum() == E and (out["reset_before"][out["ran"]] > 0).sum() == (src == _lib.FIT_SRC_RESETS).sum()
    want_obs = slot_start_obs(out, before)[t_, e_]
    want_lab = out["expert_actions"][t_, e_].astype(np.float32)
    if order is not None:
        rows, want_obs, want_lab = rows[order], want_obs[order], want_lab[order]
    assert tr.append_launch(rows) == len(rows) == tr.size()
    return tr, v, out, rows, want_obs, want_lab


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_device_route_equals_host_route(prec):
    """25x25, oracle-corner expert, a [3P, 5, 4] network: the stored rows are slot_start_obs's and the float32 labels, bit for bit."""
    tr, v, out, rows, want_obs, want_lab = _both_routes(prec, 25, "oracle_corner")
    obs, lab = tr.data()
    assert obs.dtype == lab.dtype == np.float32 and obs.shape == (len(rows), 1875) and lab.shape == (len(rows), 4)
    assert np.array_equal(obs, want_obs) and np.array_equal(lab, want_lab)
    assert len({r.tobytes() for r in obs}) == len(rows)                      # every row another state
    part = tr.data(3, 5)
    assert np.array_equal(part[0], want_obs[3:8]) and np.array_equal(part[1], want_lab[3:8])
    v.close()


def test_a_second_shape_a_repeated_row_and_another_order():
    """10x10 (3P = 300: a row is shorter than two passes of a workgroup), highest-point expert with choices from {0, 1, 4}, the row list
    shuffled and with repeats."""
    r = np.random.RandomState(4)
    tr, v, out, rows, want_obs, want_lab = _both_routes("f32", 10, "highest_point", CHOICES, order=r.randint(0, 2 * E, size=40))
    assert len(np.unique(rows, axis=0)) < len(rows) and (np.diff(rows[:, 2]) < 0).any()
    obs, lab = tr.data()
    assert obs.shape == (40, 300) and np.array_equal(obs, want_obs) and np.array_equal(lab, want_lab)
    v.close()


def test_growth_keeps_the_rows_and_a_bad_row_appends_nothing():
    from gym_cloth_amd import _lib
    tr, v, out, rows, want_obs, want_lab = _both_routes("f32", 10, "highest_point", CHOICES)
    n1 = len(rows)
    assert n1 < 64                                                           # the first allocation: 64 rows
    first = tr.data()
    assert tr.append_launch(np.tile(rows, (3, 1))) == 4 * n1 > 64            # ... so this one grows the tables
    obs, lab = tr.data()
    assert np.array_equal(obs[:n1], first[0]) and np.array_equal(lab[:n1], first[1])
    assert np.array_equal(obs, np.tile(want_obs, (4, 1))) and np.array_equal(lab, np.tile(want_lab, (4, 1)))
    L, h, b = v.batch._L, v.batch._h, v.batch
    R = out["reset_obs"].shape[1]

    def unchanged():
        assert tr.size() == 4 * n1
        o2, l2 = tr.data()
        assert np.array_equal(o2, obs) and np.array_equal(l2, lab)

    ok = rows[:1]
    bad_rows = [[3, 0, 0], [-1, 0, 0],                                       # an unknown source
                [_lib.FIT_SRC_SLOTS, T * E, 0], [_lib.FIT_SRC_SLOTS, -1, 0], [_lib.FIT_SRC_RESETS, E * R, 0], [_lib.FIT_SRC_HELD, E, 0],
                [_lib.FIT_SRC_HELD, 0, T * E], [_lib.FIT_SRC_HELD, 0, -1]]    # a label row outside the table
    for bad in bad_rows:
        with pytest.raises(ValueError):
            b.fit_append_launch(np.concatenate([ok, np.array([bad], dtype=np.int32)]))
    assert L.clothhip_fit_data_append_launch(h, _lib.i32p(ok), -1) == _lib.EINVAL
    assert L.clothhip_fit_data_append_launch(h, None, 1) == _lib.EINVAL
    assert L.clothhip_fit_data_append_launch(h, None, 0) == _lib.OK
    hold = np.stack([np.full(E, _lib.FIT_SRC_HELD), np.arange(E)], axis=1).astype(np.int32)
    for s, k in ([3, 0], [_lib.FIT_SRC_SLOTS, T * E], [_lib.FIT_SRC_RESETS, -1], [_lib.FIT_SRC_HELD, 1]):   # (HELD: only an env's own row)
        bad = hold.copy()
        bad[0] = [s, k]
        with pytest.raises(ValueError):
            b.fit_hold(bad)
    for first_, n_ in ((-1, 1), (0, 4 * n1 + 1), (4 * n1, 1), (2, -1)):
        assert L.clothhip_fit_data_get(h, first_, n_, None, None) == _lib.EINVAL
    unchanged()
    b.fit_hold(hold)                                                         # keeps every row ...
    assert b.fit_append_launch(np.array([[_lib.FIT_SRC_HELD, 2, 0]], dtype=np.int32)) == 4 * n1 + 1
    assert np.array_equal(tr.data(4 * n1)[0][0], want_obs[(rows[:, 0] == _lib.FIT_SRC_HELD) & (rows[:, 1] == 2)][0])      # ... row 2 is still env 2's slot-0 row
    # a launch in flight, then: that launch was not armed and kept no tables
    snap_n = tr.size()
    nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, E, 4)))
    assert L.clothhip_fit_data_append_launch(h, _lib.i32p(ok), 1) == _lib.ESTATE
    assert L.clothhip_fit_hold(h, None) == _lib.ESTATE
    assert L.clothhip_fit_data_get(h, 0, 1, None, None) == _lib.ESTATE
    b.run_actions_end()
    for s in (_lib.FIT_SRC_SLOTS, _lib.FIT_SRC_RESETS, _lib.FIT_SRC_HELD):   # (HELD: the row exists, the label table does not)
        with pytest.raises(_lib.ClothHipError):
            b.fit_append_launch(np.array([[s, 0, 0]], dtype=np.int32))
    for s in (_lib.FIT_SRC_SLOTS, _lib.FIT_SRC_RESETS):
        bad = hold.copy()
        bad[1] = [s, 0]
        with pytest.raises(_lib.ClothHipError):
            b.fit_hold(bad)
    assert tr.size() == snap_n
    v.close()
    # a fresh handle: HELD before any hold; episodes that end without a reset leave slots that did not run, whose label is NaN
    w = _env("f32", n_side=10, max_actions=2)
    w.reset()
    tw = _trainer(w)
    out = w.step_many(policy="mlp", n_actions=T, want_obs="device", auto_reset=False, expert="highest_point", expert_choices=CHOICES)
    assert not out["ran"][2:].any() and out["ran"][0].all()
    with pytest.raises(_lib.ClothHipError):
        tw.append_launch(np.array([[_lib.FIT_SRC_HELD, 0, 0]], dtype=np.int32))
    with pytest.raises(_lib.ClothHipError):
        tw.append_launch(np.array([[_lib.FIT_SRC_RESETS, 0, 0]], dtype=np.int32))      # no reset source, so no reset table
    good = np.array([[_lib.FIT_SRC_SLOTS, 0 * E + e, 0 * E + e] for e in range(E)], dtype=np.int32)
    assert tw.append_launch(good) == E
    kept = tw.data()
    nan_row = np.array([[_lib.FIT_SRC_SLOTS, 0 * E + 3, 2 * E + 3]], dtype=np.int32)   # slot 2 of env 3 did not run
    L, h = w.batch._L, w.batch._h
    for rows_ in (nan_row, np.concatenate([good, nan_row, good])):
        with pytest.raises(ValueError) as err:
            tw.append_launch(rows_)
        # the host entry's message for the same rows: the first NaN label, by entry and element
        obs_h = np.zeros((len(rows_), 300), dtype=np.float32)
        lab_h = np.where((rows_[:, 2] >= 2 * E)[:, None], np.nan, 0.0) * np.ones((1, 4))
        assert L.clothhip_fit_data_append(h, obs_h.ctypes.data_as(C.POINTER(C.c_float)), _lib.dp(np.ascontiguousarray(lab_h)), len(rows_)) == _lib.EINVAL
        host_msg = L.clothhip_last_error().decode()
        assert str(err.value) == host_msg and "labels[%d][0]" % (len(rows_) // 2) in host_msg, (str(err.value), host_msg)
        assert tw.size() == E
        again = tw.data()
        assert np.array_equal(again[0], kept[0]) and np.array_equal(again[1], kept[1])
    assert tw.append_launch(good[::-1]) == 2 * E                             # the spare capacity the refused call wrote into is reused
    assert np.array_equal(tw.data(E)[0], kept[0][::-1]) and np.array_equal(tw.data(0, E)[1], kept[1])
    w.close()


@pytest.mark.parametrize("max_actions", [None, 2])
def test_time_slices_store_the_rows_of_one_whole_launch_f64(max_actions):
    """N actions per env in one launch with the host route, and demos.dagger_collect in time slices that cut actions: per env, in order,
    the stored (observation row, label) pairs are the same bytes. With episodes of two actions resets run inside the launches, and at
    least one is consumed by a launch other than the first."""
    from gym_cloth_amd.demos import dagger_collect, dagger_mixture
    from gym_cloth_amd.envs import slot_start_obs
    N = 4
    noise = np.random.RandomState(13).normal(size=(N, E, 4)) * 0.05
    a, b = _env("f64", max_actions=max_actions), _env("f64", max_actions=max_actions)
    for v in (a, b):
        v.reset()
    ta, tb = _trainer(a), _trainer(b)
    before = np.asarray(a.state, dtype=np.float32).reshape(E, -1)
    whole = a.step_many(policy="mlp", n_actions=N, want_obs=True, policy_noise=noise, expert="oracle_corner",
                        expert_mix=dagger_mixture(N, E, 0.5, 7))
    assert whole["ran"].all()
    want_obs, want_lab = slot_start_obs(whole, before), whole["expert_actions"].astype(np.float32)
    res = dagger_collect(b, tb, "oracle_corner", n_actions=N, beta=0.5, seed=7, slots_per_launch=T, time_budget_ms=15.0, policy_noise=noise,
                         max_launches=60)                                    # (the loop is bounded: a collection that does not finish fails here)
    cut = sum(int((~r["ran"]).sum()) for r in res["records"])
    parked = sum(int(r["parked"].sum()) for r in res["records"])
    print("launches %d, cut %d, parked %d, resets per launch %r" % (res["launches"], cut, parked, [int(r["n_resets"].sum()) for r in res["records"]]))
    assert res["launches"] <= 60 and cut > 0 and parked > 0, (res["launches"], cut, parked)
    assert res["appended"] == N * E == tb.size() and (res["count"] >= N).all()
    if max_actions == 2:
        assert (whole["reset_before"] > 0).any()
        assert sum(int(r["n_resets"].sum()) for r in res["records"][1:]) > 0
    obs, lab = tb.data()
    seen = np.zeros((N, E), dtype=int)
    for i, (e, t) in enumerate(zip(res["row_env"], res["row_slot"])):
        seen[t, e] += 1
        assert obs[i].tobytes() == want_obs[t, e].tobytes(), (i, e, t)
        assert lab[i].tobytes() == want_lab[t, e].tobytes(), (i, e, t)
    assert (seen == 1).all()
    for e in range(E):                                                       # per env the rows come in slot order
        assert (np.diff(res["row_slot"][res["row_env"] == e]) == 1).all()
    # with an operation parked by someone else's slice the held rows would start mid-action: refused; and the bound on the loop holds
    for _ in range(60):
        b.step_many(policy="mlp", n_actions=1, time_budget_ms=15.0)
        if b.batch.in_flight().any():
            break
    assert b.batch.in_flight().any()
    with pytest.raises(ValueError):
        dagger_collect(b, tb, "oracle_corner", n_actions=1, beta=0.5, seed=7, slots_per_launch=1)
    with pytest.raises(RuntimeError):
        dagger_collect(a, ta, "oracle_corner", n_actions=N, beta=0.5, seed=7, slots_per_launch=T, time_budget_ms=15.0, max_launches=2)
    a.close(); b.close()


def test_keeping_the_tables_on_the_device_changes_nothing_else():
    a, b = _env("f32", max_actions=2), _env("f32", max_actions=2)
    for v in (a, b):
        v.reset()
        _trainer(v)
    kw = dict(policy="mlp", n_actions=T, expert="oracle_corner", expert_mix=CHECKER)
    host = a.step_many(want_obs=True, **kw)
    dev = b.step_many(want_obs="device", **kw)
    for k in _RECORDS + ("expert_actions", "expert_took", "obs"):
        assert np.array_equal(host[k], dev[k], equal_nan=True), k
    assert np.array_equal(_bits(a.batch.get_state()[0]), _bits(b.batch.get_state()[0]))
    assert "obs_t" not in dev and "reset_obs" not in dev
    assert set(dev) - set(host) == {"n_resets", "reset_capacity"} and set(host) - set(dev) == {"obs_t", "reset_obs"}
    assert dev["reset_capacity"] == host["reset_obs"].shape[1] and np.array_equal(dev["n_resets"], host["reset_before"].max(axis=0))
    # the tables are there: the device's rows are the downloaded ones
    b.batch.fit_hold(np.stack([np.zeros(E, dtype=np.int32), (T - 1) * E + np.arange(E, dtype=np.int32)], axis=1))
    rows = np.array([[2, e, 0] for e in range(E)] + [[1, e * dev["reset_capacity"], 0] for e in range(E)], dtype=np.int32)
    b.batch.fit_append_launch(rows)
    got = b.batch.fit_data()[0]
    assert np.array_equal(got[:E], host["obs_t"][T - 1]) and np.array_equal(got[E:], host["reset_obs"][:, 0])
    plain = a.step_many(policy="mlp", n_actions=1)                           # a launch without want_obs returns the keys it always did
    assert "n_resets" not in plain and "obs_t" not in plain
    a.close(); b.close()


def test_fit_loss_is_fit_grads_loss_and_sums_its_chunks_in_order():
    """Small-integer weights, rows and labels (every sum exact in any order): over B <= 4096 rows the loss is fit_grad's, bit for bit;
    over 2 * 4096 + 3 rows -- a dataset of 12 rows named again and again -- it is the chunks' sums of squares added in ascending order
    and divided by 4 n, and the float64 reference."""
    from gym_cloth_amd import _lib
    from gym_cloth_amd.batch import ClothBatch
    from gym_cloth_amd.policies import fit_reference
    from test_gpu_policy_fit import _cfg
    layers, rows, labels = _exact_case([300, 5, 4], 1.0, 0)
    b = ClothBatch(_cfg(10), n_envs=1, precision="f32")
    b.set_policy_mlp(layers)
    b.fit_append(rows, labels)
    n = 2 * _lib.FIT_MAX_BATCH + 3
    idx = np.random.RandomState(8).randint(0, len(rows), size=n).astype(np.int32)
    for B in (1, 8, 257, _lib.FIT_MAX_BATCH):
        assert b.fit_loss(idx[:B]) == b.fit_grad(idx[:B])[0], B
    sums = []
    for c in range(3):
        part = idx[c * _lib.FIT_MAX_BATCH:(c + 1) * _lib.FIT_MAX_BATCH]
        s = b.fit_grad(part)[0] * (4 * len(part))
        assert s == np.rint(s) and s > 0                                     # a sum of squares of integers
        sums.append(s)
    got = b.fit_loss(idx)
    assert got == ((sums[0] + sums[1]) + sums[2]) / (4.0 * n)
    assert got == fit_reference(layers, rows, labels, idx)[0]
    before = b.get_policy_mlp(0, b._mlp_n_params)
    assert np.array_equal(before, np.concatenate([np.concatenate([W.reshape(-1), bb]) for W, bb in layers]))   # nothing was updated
    L, h = b._L, b._h
    out = np.zeros(1)
    assert L.clothhip_policy_fit_loss(h, _lib.i32p(idx), 0, _lib.dp(out)) == _lib.EINVAL
    assert L.clothhip_policy_fit_loss(h, None, 3, _lib.dp(out)) == _lib.EINVAL
    assert L.clothhip_policy_fit_loss(h, _lib.i32p(idx), 3, None) == _lib.EINVAL
    assert L.clothhip_policy_fit_loss(h, _lib.i32p(np.array([0, 12], dtype=np.int32)), 2, _lib.dp(out)) == _lib.EINVAL
    b.fit_clear()
    assert L.clothhip_policy_fit_loss(h, _lib.i32p(idx), 3, _lib.dp(out)) == _lib.ESTATE    # an empty dataset
    b.close()


def test_the_gradient_over_device_appended_rows():
    """fit_grad on the device-appended dataset and on the host-appended twin: the same loss and gradient bits."""
    tr, v, out, rows, want_obs, want_lab = _both_routes("f32", 25, "oracle_corner")
    idx = np.random.RandomState(2).randint(0, len(rows), size=16)
    loss_d, grad_d = v.batch.fit_grad(idx)
    held_out = tr.loss(np.arange(len(rows)))
    tr.clear()
    assert tr.append(want_obs, want_lab.astype(np.float64)) == len(rows)
    loss_h, grad_h = v.batch.fit_grad(idx)
    assert loss_d == loss_h and np.isfinite(loss_d) and loss_d > 0
    assert np.array_equal(grad_d.view(np.int32), grad_h.view(np.int32)) and np.abs(grad_d).max() > 0
    assert tr.loss(np.arange(len(rows))) == held_out
    v.close()
