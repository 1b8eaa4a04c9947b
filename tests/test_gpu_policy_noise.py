"""GPU tests of the exploration noise made on the device (clothhip_policy_noise_fill, csrc/cloth_policy_noise.hpp): the
filled table against references.policy_noise_reference by bytes over shapes, sigma forms, slot bases and seeds; a launch under a
DeviceNoise against the same launch given the downloaded table; a collection under a DeviceNoise against the same collection given the
reference's table, in two slicings; the head read where it lies; the refusals."""
import numpy as np
import pytest

from test_gpu_mlp_policy import _cfg, _env, _random_layers

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 12345                                     # above 2^32: both key words count


def _batch(E, n_side=5):
    from gym_cloth_amd import ClothBatch
    return ClothBatch(_cfg(n_side), n_envs=E, precision="f32")


def _trainer(v, seed=21):
    """A network whose last layer is scaled to short pulls near the centre: an action that ends no episode by itself."""
    from gym_cloth_amd.policies import MLPTrainer
    layers = _random_layers([3 * v.P, 5, 4], seed)
    layers[-1] = (layers[-1][0] * np.float32(0.02), np.array([0.0, 0.0, 0.05, 0.05], dtype=np.float32))
    return MLPTrainer(v, layers)


# ---- 1. the table is the reference's -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,E", [(1, 1), (3, 5), (13, 67)])      # 871 threads: three full workgroups and a tail of 103
def test_filled_table_equals_the_reference_by_bytes(T, E):
    from gym_cloth_amd.policies import exp_fixed_reference, policy_noise_reference
    b = _batch(E)
    r = np.random.RandomState(T * 100 + E)
    head = np.array([-1.25, 0.0, 0.5, -4.0], dtype=np.float32)
    b.set_policy_log_sigma(head)
    sigmas = {"scalar": 0.05, "vector": np.array([0.1, 0.0, 2.5, 1e-3]), "table": r.uniform(0.0, 2.0, size=(E, 4)), "head": None}
    bases = {"zeros": None, "ragged": r.randint(0, 50, size=E).astype(np.int64), "big": 2 ** 32 + 5 + np.arange(E, dtype=np.int64) * (2 ** 33)}
    ptrs = set()
    for sname, sg in sigmas.items():
        want_sg = exp_fixed_reference(head.astype(np.float64)) if sg is None else sg
        for bname, base in bases.items():
            for seed in (SEED, 3):
                ptr = b.policy_noise_fill(seed, T, sigma=sg, slot_base=base)
                got = b.policy_noise_get()
                want = policy_noise_reference(seed, T, E, want_sg, base)
                assert got.shape == (T, E, 4) and got.tobytes() == want.tobytes(), (sname, bname, seed)
                ptrs.add(ptr)
    assert len(ptrs) == 1 and ptr != 0                           # one table of the handle, not grown by a fill of the same size
    assert b.policy_noise_fill(SEED, T, sigma=0.05) == ptr and b.policy_noise_get().tobytes() == policy_noise_reference(SEED, T, E, 0.05).tobytes()   # two fills, the same bytes
    assert b.policy_noise_fill(SEED, T, sigma=0.05) == ptr and b.policy_noise_get().tobytes() == policy_noise_reference(SEED, T, E, 0.05).tobytes()
    assert b.last_kernel_ms > 0.0                                # the fill kernel is what clothhip_last_kernel_ms times
    # a larger table after a smaller one (the buffer grows), then the smaller again
    assert b.policy_noise_fill(7, T + 4, sigma=1.0) != 0 and b.policy_noise_get().tobytes() == policy_noise_reference(7, T + 4, E, 1.0).tobytes()
    b.policy_noise_fill(7, T, sigma=1.0)
    assert b.policy_noise_get().tobytes() == policy_noise_reference(7, T, E, 1.0).tobytes()
    b.close()


# ---- 2. a launch under a DeviceNoise -----------------------------------------------------------------------------------------------------
def _compare_launch(a, b, differ=False):
    """Every array of two step_many dicts by bytes ('op_ticks' is a clock's reading, not a result)."""
    assert set(a) == set(b)
    same = True
    for k in a:
        if k == "op_ticks":
            continue
        eq = (a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
        if not differ:
            assert eq, k
        same = same and eq
    return same


def test_step_many_under_device_noise_is_the_launch_with_the_downloaded_table():
    from gym_cloth_amd.policies import DeviceNoise, policy_noise_reference
    envs = []
    for _ in range(3):
        v = _env()
        v.reset()
        _trainer(v)
        envs.append(v)
    E = envs[0].E
    noise = DeviceNoise(SEED, sigma=[0.05, 0.05, 0.02, 0.02])
    out = envs[0].step_many(policy="mlp", n_actions=3, policy_noise=noise, want_obs=True)
    table = envs[0].batch.policy_noise_get()
    assert table.tobytes() == policy_noise_reference(SEED, 3, E, [0.05, 0.05, 0.02, 0.02]).tobytes()
    ref = envs[1].step_many(policy="mlp", n_actions=3, policy_noise=table, want_obs=True)
    assert _compare_launch(out, ref) and out["ran"].all()
    plain = envs[2].step_many(policy="mlp", n_actions=3, want_obs=True)
    assert not _compare_launch(out, plain, differ=True) and not np.array_equal(out["actions"], plain["actions"])
    # the running slot_base: the next launch goes on with every env's next slot
    assert np.array_equal(noise.slot_base, out["ran"].sum(axis=0)) and np.array_equal(noise.slot_base, [3] * E)
    out2 = envs[0].step_many(policy="mlp", n_actions=2, policy_noise=noise)
    table2 = envs[0].batch.policy_noise_get()
    assert table2.tobytes() == policy_noise_reference(SEED, 5, E, [0.05, 0.05, 0.02, 0.02])[3:].tobytes()
    ref2 = envs[1].step_many(policy="mlp", n_actions=2, policy_noise=table2)
    assert _compare_launch(out2, ref2)
    # every existing refusal keeps its place: noise of either kind goes with policy='mlp'
    with pytest.raises(ValueError):
        envs[0].step_many(np.zeros((1, E, 4)), policy_noise=noise)
    with pytest.raises(ValueError):
        envs[0].step_many(policy="mlp", n_actions=1, actions_device_ptr=1, policy_noise=noise)
    for v in envs:
        v.close()


# ---- 3. a collection does not depend on its slicing --------------------------------------------------------------------------------------
def _collected(policy_noise, slots_per_launch):
    from gym_cloth_amd.demos import reward_collect
    v = _env()
    v.reset()
    tr = _trainer(v)
    col = reward_collect(v, tr, n_actions=4, policy_noise=policy_noise(v.E), slots_per_launch=slots_per_launch, max_launches=4)
    obs, lab = tr.data()
    res = (col["launches"], obs.tobytes(), lab.tobytes(), tr.weights().tobytes(), lab)
    v.close()
    return res


def test_reward_collect_under_device_noise_is_the_collection_given_the_reference_table():
    from gym_cloth_amd.policies import DeviceNoise, policy_noise_reference
    sigma = np.array([0.05, 0.04, 0.03, 0.02])
    want = _collected(lambda E: policy_noise_reference(SEED, 4, E, sigma), 4)
    quiet = _collected(lambda E: None, 4)
    assert want[0] == 1 and want[2] != quiet[2]                  # the labels are the executed actions: the noise is in them
    for spl, launches in ((2, 2), (4, 1)):
        dn = DeviceNoise(SEED, sigma=sigma)
        got = _collected(lambda E: dn, spl)
        assert got[0] == launches
        for k in (1, 2, 3):
            assert got[k] == want[k], (spl, k)
        assert dn.slot_base is None                              # the collection numbers its slots on a copy


# ---- 4. the head, read where it lies -----------------------------------------------------------------------------------------------------
def test_the_fill_follows_the_head_and_snapshot_old_stores_what_it_read():
    from gym_cloth_amd.policies import exp_fixed_reference, policy_noise_reference
    v = _env()
    obs = v.reset()
    tr = _trainer(v)
    b, E = v.batch, v.E
    dn = tr.device_noise(SEED)
    assert dn.sigma is None
    tables = []
    for ls in (np.array([-2.0, -1.0, 0.0, 0.75], dtype=np.float32), np.float32(np.log(0.3)) * np.ones(4, dtype=np.float32)):
        tr.set_log_sigma(ls)
        dn.fill(b, 6)
        got = b.policy_noise_get()
        assert got.tobytes() == policy_noise_reference(SEED, 6, E, exp_fixed_reference(ls.astype(np.float64))).tobytes()
        tables.append(got)
    assert tables[0].tobytes() != tables[1].tobytes()
    tr.append(np.asarray(obs, dtype=np.float32).reshape(E, -1), np.zeros((E, 4)))
    tr.snapshot_old()
    old = b.fit_get_old_log_sigma()
    assert old.shape == (E, 4) and all(old[e].tobytes() == tr.log_sigma().tobytes() for e in range(E))
    assert tables[1].tobytes() == policy_noise_reference(SEED, 6, E, exp_fixed_reference(old[0].astype(np.float64))).tobytes()
    v.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    from gym_cloth_amd import _lib
    from gym_cloth_amd.policies import policy_noise_reference
    v = _env()
    v.reset()
    _trainer(v)
    b, E, L, h = v.batch, v.E, v.batch._L, v.batch._h
    snap = v.snapshot()
    dp = _lib.dp
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    one, tab = np.full(4, 0.05), np.full((E, 4), 0.05)
    out = np.zeros((2, E, 4))
    # before any fill there is no table
    assert L.clothhip_policy_noise_get(h, 2, dp(out)) == _lib.ESTATE
    # no head on the handle when the head is asked for
    assert L.clothhip_policy_noise_fill(h, 1, 2, None, None, 0, None) == _lib.ESTATE
    with pytest.raises(_lib.ClothHipError):
        b.policy_noise_fill(1, 2)
    ptr = b.policy_noise_fill(1, 2, sigma=0.05)
    want = policy_noise_reference(1, 2, E, 0.05)

    def unchanged():
        assert b.policy_noise_get().tobytes() == want.tobytes()
    # T, sigma_rows, sigma, slot_base
    for T in (0, -1):
        assert L.clothhip_policy_noise_fill(h, 1, T, None, dp(one), 1, None) == _lib.EINVAL
    assert L.clothhip_policy_noise_fill(h, 1, 2 ** 31 - 1, None, dp(one), 1, None) == _lib.EINVAL          # T E overflows
    for rows in (0, 2, E + 1, -1):
        assert L.clothhip_policy_noise_fill(h, 1, 2, None, dp(tab), rows, None) == _lib.EINVAL
    assert L.clothhip_policy_noise_fill(h, 1, 2, None, None, 1, None) == _lib.EINVAL                       # rows without a table
    for bad in (-0.05, np.nan, np.inf, -np.inf):
        s1, sE = one.copy(), tab.copy()
        s1[2] = bad
        sE[E - 1, 3] = bad
        assert L.clothhip_policy_noise_fill(h, 1, 2, None, dp(s1), 1, None) == _lib.EINVAL
        assert L.clothhip_policy_noise_fill(h, 1, 2, None, dp(sE), E, None) == _lib.EINVAL
    base = np.zeros(E, dtype=np.int64)
    base[E - 1] = -1
    assert L.clothhip_policy_noise_fill(h, 1, 2, i64(base), dp(one), 1, None) == _lib.EINVAL
    base[E - 1] = 2 ** 63 - 2
    assert L.clothhip_policy_noise_fill(h, 1, 2, i64(base), dp(one), 1, None) == _lib.EINVAL
    unchanged()
    # _get with another T than the last fill's, or without a destination
    assert L.clothhip_policy_noise_get(h, 3, dp(np.zeros((3, E, 4)))) == _lib.EINVAL and L.clothhip_policy_noise_get(h, 1, dp(out)) == _lib.EINVAL
    assert L.clothhip_policy_noise_get(h, 2, None) == _lib.EINVAL
    # a launch in flight may be reading the table: ESTATE, and the launch's result is that of an undisturbed launch
    records = []
    for disturb in (True, False):
        v.restore(snap)
        assert b.policy_noise_fill(1, 2, sigma=0.05) == ptr
        nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
        b.run_actions_begin(v._episode_params(), 2, nsteps, done, policy=_lib.POLICY_MLP, actions_device_ptr=ptr)
        if disturb:
            assert L.clothhip_policy_noise_fill(h, 99, 2, None, dp(one), 1, None) == _lib.ESTATE
            assert L.clothhip_policy_noise_fill(h, 99, 64, None, dp(one), 1, None) == _lib.ESTATE     # (one that would have grown the table)
            assert L.clothhip_policy_noise_get(h, 2, dp(out)) == _lib.ESTATE
            with pytest.raises(_lib.ClothHipError):
                b.policy_noise_fill(99, 2, sigma=0.05)
        records.append(b.run_actions_end()[0])
        unchanged()
    assert records[0].tobytes() == records[1].tobytes() and (records[0]["ran"][0] == 1).all()
    v.close()
