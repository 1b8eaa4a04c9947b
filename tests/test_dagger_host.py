"""Host-side tests of the expert beside the acting policy (clothhip_run_actions_expert / _labels, clothhip_policy_label): the ABI, the
slot-start observation rule, the DAgger mixture and the argument checks that need no device."""
import numpy as np
import pytest

from gym_cloth_amd import _lib


def test_symbols_are_exported_and_bound():
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("clothhip_run_actions_expert", "clothhip_run_actions_labels", "clothhip_policy_label"):
        assert n in names
    assert _lib.EXPERTS == {"oracle_corner": _lib.POLICY_ORACLE_CORNER, "highest_point": _lib.POLICY_HIGHEST_POINT}
    L = _lib.load()
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7
    assert L.clothhip_run_actions_expert.argtypes is not None and L.clothhip_run_actions_labels.argtypes is not None
    assert L.clothhip_policy_label.argtypes is not None


def test_library_refuses_without_touching_a_device():
    """NULL handle: the calls answer with a status."""
    L = _lib.load()
    assert L.clothhip_run_actions_expert(None, _lib.POLICY_ORACLE_CORNER, 1, None, None) == _lib.EINVAL
    assert L.clothhip_run_actions_labels(None, None, None) == _lib.EINVAL
    assert L.clothhip_policy_label(None, _lib.POLICY_ORACLE_CORNER, 1, None, 0, None, None, None) == _lib.EINVAL


def test_slot_start_obs_covers_the_three_cases():
    """T = 3, E = 3, rows of width 2. Env 0: no reset -- obs_before, obs_t[0], obs_t[1]. Env 1: a reset before slot 1 --
    obs_before, reset_obs[1, 0], obs_t[1]. Env 2: a reset before slot 0 and the env's second one before slot 2 --
    reset_obs[2, 0], obs_t[0], reset_obs[2, 1]."""
    from gym_cloth_amd.envs import slot_start_obs
    T, E, W = 3, 3, 2
    obs_t = (100 + np.arange(T * E * W, dtype=np.float32)).reshape(T, E, W)
    reset_obs = (500 + np.arange(E * 2 * W, dtype=np.float32)).reshape(E, 2, W)
    before = (900 + np.arange(E * W, dtype=np.float64)).reshape(E, W)
    rb = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 2]])
    got = slot_start_obs({"obs_t": obs_t, "reset_obs": reset_obs, "reset_before": rb}, before)
    assert got.shape == (T, E, W) and got.dtype == np.float32
    exp = np.empty((T, E, W), dtype=np.float32)
    exp[:, 0] = [before[0], obs_t[0, 0], obs_t[1, 0]]
    exp[:, 1] = [before[1], reset_obs[1, 0], obs_t[1, 1]]
    exp[:, 2] = [reset_obs[2, 0], obs_t[0, 2], reset_obs[2, 1]]
    assert np.array_equal(got, exp)
    assert np.array_equal(obs_t, (100 + np.arange(T * E * W, dtype=np.float32)).reshape(T, E, W))      # inputs untouched
    # without any reset reset_obs may be None (no reset source)
    got = slot_start_obs({"obs_t": obs_t, "reset_obs": None, "reset_before": np.zeros((T, E), dtype=np.int64)}, before)
    assert np.array_equal(got[0], before.astype(np.float32)) and np.array_equal(got[1:], obs_t[:-1])


class _FakeEnv(object):
    """What dagger_rollout touches of a ClothVecEnv."""
    E = 4

    def __init__(self):
        self.calls = []

    @property
    def state(self):
        return np.zeros((self.E, 6))

    def step_many(self, **kw):
        self.calls.append(kw)
        T = kw["n_actions"]
        return {"obs_t": np.ones((T, self.E, 6), dtype=np.float32), "reset_obs": None, "reset_before": np.zeros((T, self.E), dtype=np.int64),
                "ran": np.ones((T, self.E), dtype=bool), "expert_actions": np.zeros((T, self.E, 4)), "expert_took": kw["expert_mix"].copy()}


def test_dagger_mixture_is_seeded_and_degenerates_at_the_ends():
    from gym_cloth_amd.demos import dagger_mixture, dagger_rollout
    a, b = dagger_mixture(12, 6, 0.5, seed=7), dagger_mixture(12, 6, 0.5, seed=7)
    assert a.shape == (12, 6) and a.dtype == bool and np.array_equal(a, b)
    assert a.any() and not a.all()
    assert not np.array_equal(a, dagger_mixture(12, 6, 0.5, seed=8))
    assert not dagger_mixture(12, 6, 0.0, seed=7).any() and dagger_mixture(12, 6, 1.0, seed=7).all()
    with pytest.raises(ValueError):
        dagger_mixture(2, 2, 1.5, seed=0)
    env = _FakeEnv()
    r1 = dagger_rollout(env, n_actions=5, beta=0.5, seed=3)
    r2 = dagger_rollout(env, n_actions=5, beta=0.5, seed=3)
    kw = env.calls[0]
    assert kw["policy"] == "mlp" and kw["want_obs"] is True and kw["expert"] == "oracle_corner" and kw["n_actions"] == 5
    assert np.array_equal(kw["expert_mix"], dagger_mixture(5, 4, 0.5, seed=3)) and np.array_equal(r1["took"], r2["took"])
    assert set(r1) == {"obs", "labels", "took", "ran", "out"} and r1["obs"].shape == (5, 4, 6)
    assert not dagger_rollout(env, n_actions=5, beta=0.0, seed=3)["took"].any()
    assert dagger_rollout(env, n_actions=5, beta=1.0, seed=3)["took"].all()


def _bare_env(E=3):
    """A ClothVecEnv's host-only pieces: enough for step_many's argument checks, which come before anything touches a device.
    The order of those checks is behaviour (ClothVecEnv._parse_launch): nothing beyond what is set here may be read before the
    refusals test_step_many_rejects_bad_expert_arguments expects."""
    from gym_cloth_amd.batch import ClothBatch
    from gym_cloth_amd.envs import ClothVecEnv
    v = ClothVecEnv.__new__(ClothVecEnv)
    v.E, v._version, v._policy_mlp, v.num_points, v._delta_actions = E, 0, None, 625, True
    v.batch = ClothBatch.__new__(ClothBatch)
    v.batch.E = E
    return v


def test_step_many_rejects_bad_expert_arguments():
    v = _bare_env()
    acts = np.zeros((2, 3, 4))
    for kw in (dict(expert="oracle_corner", expert_mix=np.zeros((3, 3), dtype=bool)),            # T is 2
               dict(expert="oracle_corner", expert_mix=np.zeros((2, 4), dtype=bool)),
               dict(expert="oracle_corner", expert_mix=np.zeros(6, dtype=bool)),
               dict(expert="oracle_corner", expert_choices=np.zeros((2, 3), dtype=np.int32)),    # choices without highest_point
               dict(expert=None, expert_choices=np.zeros((2, 3), dtype=np.int32)),
               dict(expert=None, expert_mix=np.zeros((2, 3), dtype=bool)),
               dict(expert="highest_point"),                                                     # ... and highest_point without
               dict(expert="highest_point", expert_choices=np.zeros((3, 3), dtype=np.int32)),
               dict(expert="harris")):
        with pytest.raises(ValueError):
            v.step_many(acts, **kw)
    with pytest.raises(ValueError):                                                              # only a table or the network may act beside it
        v.step_many(policy="oracle_corner", n_actions=2, expert="oracle_corner")
    v.num_points = 100
    with pytest.raises(ValueError):
        v.step_many(acts, expert="oracle_corner")
