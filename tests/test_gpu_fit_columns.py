"""GPU test of the trainer's dataset as ONE table of columns: every column keeps its bytes across two growths. The growth
tests of test_gpu_fit_launch.py, test_gpu_actor_critic.py and test_gpu_ppo.py cross one boundary with two or three columns each; here all
seven are written before the first growth, rows arrive by the host route and by the device route, and a numpy mirror kept by the test --
what was written, and the documented defaults of a new row -- is compared by bytes after every append."""
import numpy as np
import pytest

from test_gpu_dagger import E, _env, _layers

pytestmark = pytest.mark.gpu

N = 40          # rows per append: 40 -> 64 allocated, 80 -> 128, 120 fits, 160 -> 256


def test_every_column_keeps_its_bytes_across_two_growths():
    from gym_cloth_amd import _lib
    from gym_cloth_amd.policies import gae_reference
    v = _env("f32", n_side=10)
    v.reset()
    b, r = v.batch, np.random.RandomState(7)
    L = 3 * v.P
    assert L == 300
    b.set_policy_mlp(_layers([L, 5, 4], 21))
    b.set_value_mlp(_layers([L, 5, 1], 22))
    m = dict(obs=np.zeros((0, L), np.float32), lab=np.zeros((0, 4), np.float32), w=np.zeros(0, np.float32), rew=np.zeros(0, np.float32),
             ret=np.zeros(0, np.float32), next=np.zeros(0, np.int32), old=np.zeros((0, 4), np.float32))

    def mirror_append(obs, lab, w):
        """the rows as they were given, and the defaults of the other columns: reward 0, target 0, no successor, old mean zeros"""
        n = len(obs)
        new = dict(obs=obs, lab=lab, w=w, rew=np.zeros(n), ret=np.zeros(n), next=np.full(n, _lib.FIT_NEXT_NONE), old=np.zeros((n, 4)))
        for k in m:
            m[k] = np.concatenate([m[k], np.asarray(new[k]).astype(m[k].dtype)])

    def check(where):
        n = len(m["obs"])
        assert b.fit_size() == n, where
        obs, lab = b.fit_data()
        rew, nxt = b.fit_get_transitions()
        got = dict(obs=obs, lab=lab, w=b.fit_get_weights(), rew=rew, ret=b.fit_get_returns(), next=nxt, old=b.fit_get_old_means())
        for k in m:
            assert got[k].dtype == m[k].dtype and got[k].shape == m[k].shape, (where, k)
            bad = np.nonzero((got[k] != m[k]).reshape(n, -1).any(axis=1))[0]
            assert got[k].tobytes() == m[k].tobytes(), (where, k, bad[:8])

    def host_append(weighted):
        obs = r.uniform(-1, 1, size=(N, L)).astype(np.float32)
        lab = r.uniform(-1, 1, size=(N, 4))
        w = r.uniform(-2, 2, size=N).astype(np.float32) if weighted else None
        mirror_append(obs, lab.astype(np.float32), np.ones(N, np.float32) if w is None else w)
        assert b.fit_append(obs, lab, weights=w) == len(m["obs"])

    host_append(True)
    check("the first 40 rows")
    # every other column on them: chains of three (two links, then a leaf), a terminal row, a link into the next chain; the last row ends
    i = np.arange(N)
    nxt = np.where(i % 5 == 2, _lib.FIT_NEXT_NONE, np.where(i % 5 == 3, _lib.FIT_NEXT_TERMINAL, i + 1)).astype(np.int32)
    nxt[N - 1] = _lib.FIT_NEXT_TERMINAL
    assert (nxt == _lib.FIT_NEXT_NONE).any() and (nxt == _lib.FIT_NEXT_TERMINAL).any() and (nxt > 0).any()
    m["rew"][:N] = r.uniform(-1, 1, size=N).astype(np.float32)
    m["next"][:N] = nxt
    b.fit_set_transitions(m["rew"][:N], nxt)
    m["ret"][:N] = r.uniform(-1, 1, size=N).astype(np.float32)
    b.fit_set_returns(m["ret"][:N])
    m["old"][0:10] = r.uniform(-1, 1, size=(10, 4)).astype(np.float32)
    b.fit_set_old_means(m["old"][0:10], first=0)
    m["old"][20:30] = b.fit_predict(np.arange(20, 30))      # (test_gpu_ppo.py pins the snapshot to fit_predict, and that to the reference)
    b.fit_snapshot_policy(20, 10)
    unset = np.r_[10:20, 30:N]
    assert np.abs(m["old"][20:30]).min() > 0 and not m["old"][unset].any()
    check("all seven columns written")

    host_append(False)                                      # 64 -> 128 allocated
    check("the first growth")
    held = np.asarray(v.state, dtype=np.float32).reshape(E, -1)
    b.fit_hold()
    src = np.arange(N) % E
    mirror_append(held[src], np.zeros((N, 4), np.float32), np.ones(N, np.float32))
    rows = np.stack([np.full(N, _lib.FIT_SRC_HELD), src, np.zeros(N, dtype=np.int64)], axis=1)
    assert b.fit_append_launch(rows, labels="zero") == 3 * N
    check("the device route, into spare capacity")
    host_append(True)                                       # 128 -> 256
    check("the second growth")

    # the host mirrors came along: the successor table, against which fit_gae checks its range ...
    with pytest.raises(ValueError, match="row 4: its successor 5 lies outside"):
        b.fit_gae(0.9, 0.8, first=0, n=5, write_weights=False)
    vals = b.value_predict(np.arange(N))
    adv_r, ret_r, _ = gae_reference(vals, m["rew"][:N], m["next"][:N], 0.9, 0.8)
    adv, ret = b.fit_gae(0.9, 0.8, first=0, n=N, write_weights=False)
    assert adv.tobytes() == adv_r.tobytes() and ret.tobytes() == ret_r.tobytes()
    m["ret"][:N] = ret_r
    check("after fit_gae")
    # ... and the set marks, against which PPO checks a minibatch; a snapshot row's old mean is the present mean: rho = 1 exactly
    for row in (int(unset[0]), int(unset[-1]), N, 4 * N - 1):
        with pytest.raises(_lib.ClothHipError, match="row %d has no old mean" % row):
            b.fit_ppo_grad(np.array([0, row]), 1.0)
    stats, grad, ratio = b.fit_ppo_grad(np.r_[0:10, 20:30], 1.0)
    assert np.isfinite(stats).all() and np.isfinite(grad).all() and np.array_equal(ratio[10:], np.ones(10, np.float32))
    check("after fit_ppo_grad")

    b.fit_clear()
    for k in m:
        m[k] = m[k][:0]
    obs3 = r.uniform(-1, 1, size=(3, L)).astype(np.float32)
    lab3 = r.uniform(-1, 1, size=(3, 4))
    mirror_append(obs3, lab3.astype(np.float32), np.ones(3, np.float32))
    assert b.fit_append(obs3, lab3) == 3
    check("three rows after fit_clear: every other column shows its default")
    with pytest.raises(_lib.ClothHipError, match="row 0 has no old mean"):
        b.fit_ppo_grad(np.array([0]), 1.0)
    v.close()
