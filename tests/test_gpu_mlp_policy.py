"""GPU tests of the MLP policy (csrc/cloth_policy_mlp.hpp): the stand-alone evaluation (clothhip_policy_eval) against a float64 numpy
evaluation within an a-priori rounding bound; the evaluation inside the episode launch (step_many(policy='mlp')) against the stand-alone
one, bit for bit and whatever the number of threads per cloth; whole episodes on the device against the host loop; the noise table; time
slices; refusals and who owns the network."""
import numpy as np
import pytest

from test_gpu_env import base_cfg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                           # unit roundoff of float32


def _gamma(k):
    return k * U / (1.0 - k * U)


def _random_layers(widths, seed):
    """Weights from a seeded RandomState with scale 1 / sqrt(fan-in), rounded to float32."""
    r = np.random.RandomState(seed)
    return [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32),
             (r.normal(size=widths[l + 1]) / np.sqrt(widths[l])).astype(np.float32)) for l in range(len(widths) - 1)]


def _bound(layers, rows):
    """Higham's a-priori bound on |computed - exact| of every output, for ANY summation order with or without FMA: per layer with n
    inputs dy_j = sum_i |w_ji| dx_i + gamma_{n+1} (sum_i |w_ji| (|x_i| + dx_i) + |b_j|); ReLU is exact and 1-Lipschitz; dx = 0 at the
    input. Computed, not measured."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)
    dx = np.zeros_like(x)
    for l, (W, b) in enumerate(layers):
        W64, aW, b64 = W.astype(np.float64), np.abs(W.astype(np.float64)), b.astype(np.float64)
        n = W.shape[1]
        dy = dx @ aW.T + _gamma(n + 1) * ((np.abs(x) + dx) @ aW.T + np.abs(b64))
        y = x @ W64.T + b64
        x, dx = (np.maximum(y, 0.0) if l + 1 < len(layers) else y), dy
    return dx


def _cfg(n_side=25, tier="tier1", force_grab=False):
    cfg = base_cfg(tier, 1337)
    cfg["cloth"]["num_width_points"] = cfg["cloth"]["num_height_points"] = n_side
    cfg["env"]["force_grab"] = force_grab
    return cfg


def _env(n_side=25, prec="f32", tier="tier1", force_grab=False, E=3):
    from gym_cloth_amd.envs import ClothVecEnv
    v = ClothVecEnv(_cfg(n_side, tier, force_grab), n_envs=E, precision=prec, consume_domrand_draws=False)
    v.seed([1337 + e for e in range(E)])
    return v


_stepped = {}


@pytest.fixture(scope="module")
def stepped_env():
    """(n_side, precision) -> an env of three cloths after reset() and two random steps; shared by the cases, which only evaluate."""
    def get(n_side, prec):
        if (n_side, prec) not in _stepped:
            v = _env(n_side, prec)
            v.reset()
            r = np.random.RandomState(5)
            for _ in range(2):
                v.step(r.uniform(-1, 1, size=(3, 4)))
            _stepped[(n_side, prec)] = v
        return _stepped[(n_side, prec)]
    yield get
    for v in _stepped.values():
        v.close()
    _stepped.clear()


@pytest.mark.parametrize("hidden", [[], [5], [37, 64], [256, 256, 256]], ids=lambda h: "hidden" + "x".join(map(str, h)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n_side", [25, 10])
def test_policy_eval_against_numpy(n_side, prec, hidden, stepped_env):
    """clothhip_policy_eval on the states of three cloths after two random steps: within the a-priori bound of the float64 numpy
    evaluation of the same float32 weights, element by element; the evaluation on the handle's SoA state (obs=None, which casts the
    positions -- doubles on an fp64 handle -- as k_write_obs does) gives the bits of the evaluation on the uploaded rows."""
    from gym_cloth_amd.policies import MLPPolicy
    v = stepped_env(n_side, prec)
    P = n_side * n_side
    layers = _random_layers([3 * P] + hidden + [4], seed=100 + len(hidden))
    pol = MLPPolicy(v, layers)
    rows = v.state.astype(np.float32)
    assert rows.shape == (3, 3 * P) and np.ptp(rows[:, 2::3]) > 0            # the steps lifted something
    got = v.batch.policy_eval(rows)
    ref = pol.reference(rows)
    B = _bound(layers, rows)
    err = np.abs(got - ref)
    print("n_side %d %s hidden %r: max err %.3e, min bound %.3e, max err / bound %.3f" % (n_side, prec, hidden, err.max(), B.min(), (err / B).max()))
    assert got.shape == (3, 4) and np.isfinite(got).all() and np.abs(ref).max() > 1e-3
    assert (err <= B).all(), (err, B)
    assert np.array_equal(got, np.float32(got))                              # float32 values, widened
    from_state = v.batch.policy_eval(None)
    assert np.array_equal(from_state.view(np.int64), got.view(np.int64))
    assert np.array_equal(v.policy_actions().view(np.int64), got.view(np.int64))
    assert np.array_equal(pol.get_action(v.state).view(np.int64), got.view(np.int64))
    v.set_policy(None)


def _expected_slot_actions(v, out, pre_obs, T):
    """What the launch must have recorded: the stand-alone evaluation of the observation every slot began with."""
    exp = np.zeros((T, v.E, 4))
    for t in range(T):
        obs = pre_obs.astype(np.float32) if t == 0 else out["obs_t"][t - 1].copy()
        for e in np.nonzero(out["reset_before"][t])[0]:
            obs[e] = out["reset_obs"][e, int(out["reset_before"][t, e]) - 1]
        exp[t] = v.batch.policy_eval(obs)
    return exp


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_launch_equals_stand_alone_whatever_the_thread_count(prec, monkeypatch):
    """step_many(policy='mlp') on the default variant and on one with another number of threads per cloth: slot 0's recorded action
    is policy_eval of the pre-launch observation, slot 1's of obs_t[0] (of reset_obs where a reset came between), bit for bit -- the
    network's arithmetic has one order, whichever wave computes a neuron."""
    from gym_cloth_amd.policies import MLPPolicy
    layers = _random_layers([1875, 37, 64, 4], seed=21)
    recorded, threads = [], []
    for run in range(2):
        for k in ("CLOTHHIP_DEBUG_LEAN", "CLOTHHIP_DEBUG_W8", "CLOTHHIP_DEBUG_NOSPEC"):
            monkeypatch.delenv(k, raising=False)
        if run == 1:                                                         # the standard arithmetic's other thread layout
            monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", "0")
            monkeypatch.setenv("CLOTHHIP_DEBUG_W8", "0" if threads[0] != 256 else "1")
        v = _env(25, prec, force_grab=True)
        pre = v.reset()
        v.set_policy(MLPPolicy(v, layers))
        out = v.step_many(policy="mlp", n_actions=2, want_obs=True)
        var = v.batch.last_variant()
        assert var["fused"] == 2, var
        threads.append(var["threads"])
        assert out["ran"].all() and (out["n_grabbed"] > 0).all()
        exp = _expected_slot_actions(v, out, pre, 2)
        assert np.array_equal(out["actions"], exp), (prec, var["name"], out["actions"] - exp)
        assert not np.array_equal(out["actions"][0], out["actions"][1])      # the network reads its input
        assert (np.abs(out["actions"][0] - out["actions"][1]).max(axis=1) > 0).all()
        recorded.append(out["actions"].copy())
        v.close()
    assert threads[0] != threads[1], threads
    assert np.array_equal(recorded[0], recorded[1])


def _by_env(eps, E=3):
    return {e: [ep for ep in eps if ep["env"] == e] for e in range(E)}


def _centroid_layers(P):
    """L = 1, by hand: picks 2 mean(x) - 1 and 2 mean(y) - 1 (the cloth's centroid in clip space), the delta fixed by the bias."""
    W = np.zeros((4, 3 * P), dtype=np.float32)
    W[0, 0::3] = 2.0 / P
    W[1, 1::3] = 2.0 / P
    return [(W, np.array([-1.0, -1.0, 0.30, -0.20], dtype=np.float32))]


@pytest.mark.parametrize("case", ["tier1", "tier2", "tier1_centroid"])
def test_whole_episodes_on_the_device_equal_the_host_loop_f64(case):
    """collect_demos with the network evaluated inside the launch (policy, steps and resets in one kernel, five slots per launch)
    against the host loop step(policy.get_action(obs)): the same actions, rewards, dones, observations and infos, episode by episode.
    Random networks run with force_grab so that every action moves the cloth; the hand-built centroid network runs without, and must
    grab something in every env."""
    from gym_cloth_amd.demos import collect_demos
    from gym_cloth_amd.policies import MLPPolicy
    tier, centroid = case.split("_")[0], case.endswith("centroid")
    layers = _centroid_layers(625) if centroid else _random_layers([1875, 37, 64, 4], seed=33)
    a, b = [_env(25, "f64", tier, force_grab=not centroid) for _ in range(2)]
    grabbed = []
    step_many = a.step_many

    def spy(*args, **kw):
        out = step_many(*args, **kw)
        grabbed.append(np.where(out["ran"], out["n_grabbed"], 0).max(axis=0))
        return out
    a.step_many = spy
    dev = collect_demos(a, MLPPolicy(a, layers), max_episodes=4, slots_per_launch=5, on_device=True)
    host = collect_demos(b, MLPPolicy(b, layers), max_episodes=4)
    d, h = _by_env(dev), _by_env(host)
    compared = steps = 0
    for e in range(3):
        for ed, eh in zip(d[e], h[e]):
            assert ed["act"] == eh["act"] and ed["rew"] == eh["rew"] and ed["done"] == eh["done"], (case, e)
            assert len(ed["obs"]) == len(eh["obs"]) == len(ed["act"]) + 1
            for od, oh in zip(ed["obs"], eh["obs"]):
                assert np.array_equal(od, oh.astype(np.float32))
            assert ed["info"] == eh["info"]
            compared += 1; steps += len(ed["act"])
    assert compared >= 3 and steps >= 6
    if centroid:
        assert (np.max(grabbed, axis=0) > 0).all(), grabbed                   # no env sat idle through the test
    a.close(); b.close()


def test_noise_table_is_added_as_a_double_and_zero_noise_is_no_noise():
    """With a seeded [T, E, 4] table the recorded action is policy_eval(obs) + noise[t, e], one double addition; a table of zeros
    gives the bits of no table -- actions, rewards, final particles."""
    from gym_cloth_amd.policies import MLPPolicy
    T, E = 2, 3
    layers = _random_layers([300, 5, 4], seed=44)
    noise = np.random.RandomState(9).normal(size=(T, E, 4)) * 0.05
    res = []
    for tbl in (None, np.zeros((T, E, 4)), noise):
        v = _env(10, "f32", force_grab=True)
        pre = v.reset()
        v.set_policy(MLPPolicy(v, layers))
        out = v.step_many(policy="mlp", n_actions=T, want_obs=True, policy_noise=tbl)
        assert out["ran"].all()
        exp = _expected_slot_actions(v, out, pre, T)
        if tbl is not None:
            exp = exp + tbl
        assert np.array_equal(out["actions"], exp), out["actions"] - exp
        res.append((out["actions"].copy(), out["rew"].copy(), v.batch.get_state()[0].copy()))
        v.close()
    for x, y in zip(res[0], res[1]):
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
    assert not np.array_equal(res[0][0], res[2][0])
    with pytest.raises(ValueError):
        v2 = _env(10, "f32")
        try:
            v2.reset()
            v2.set_policy(MLPPolicy(v2, layers))
            v2.step_many(policy="mlp", n_actions=T, policy_noise=np.zeros((T + 1, E, 4)))
        finally:
            v2.close()


def test_time_sliced_launches_equal_unsliced_f64():
    """collect_demos over time-sliced launches with a noisy MLP policy: an action a slice cuts is not evaluated again, the noise rows
    a slice leaves unused go to the next launch, a slice may end right after a reset. The episodes equal those of unsliced launches."""
    from gym_cloth_amd.demos import collect_demos
    from gym_cloth_amd.policies import MLPPolicy
    layers = _random_layers([1875, 37, 64, 4], seed=55)
    a, b = [_env(25, "f64", force_grab=True) for _ in range(2)]
    whole = collect_demos(a, MLPPolicy(a, layers, noise_std=0.05, seed=3), max_episodes=6, slots_per_launch=6, on_device=True)
    idle = []
    step_many = b.step_many

    def spy(*args, **kw):
        out = step_many(*args, **kw)
        idle.append(int((~out["ran"]).sum()))
        return out
    b.step_many = spy
    sliced = collect_demos(b, MLPPolicy(b, layers, noise_std=0.05, seed=3), max_episodes=6, slots_per_launch=6, on_device=True,
                           time_budget_ms=20.0)
    assert sum(idle) > 0, "no launch was cut by its time slice"
    w, s_ = _by_env(whole), _by_env(sliced)
    compared = 0
    for e in range(3):
        for ew, es in zip(w[e], s_[e]):
            assert ew["act"] == es["act"] and ew["rew"] == es["rew"] and ew["done"] == es["done"], e
            assert len(es["obs"]) == len(es["act"]) + 1
            for ow, os_ in zip(ew["obs"], es["obs"]):
                assert np.array_equal(ow, os_)
            compared += 1
    assert compared >= 3
    a.close(); b.close()


def test_refusals_and_who_owns_the_network():
    """No network: the launch and the evaluation refuse. Bad widths: refused by the library itself. The network is the handle's: a
    new one changes the next launch's actions; snapshot / restore and a masked reset leave it alone; set_policy(None) clears it."""
    import ctypes as C
    from gym_cloth_amd import _lib
    from gym_cloth_amd.policies import MLPPolicy
    v = _env(10, "f32", force_grab=True)
    pre = v.reset()
    P = 100
    with pytest.raises(ValueError):
        v.step_many(policy="mlp", n_actions=1)
    with pytest.raises(_lib.ClothHipError):
        v.batch.policy_eval(None)
    nsteps, done = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.uint8)
    with pytest.raises(_lib.ClothHipError):                                  # the library's own check (CLOTHHIP_ESTATE)
        v.batch.run_actions_begin(v._episode_params(), 1, nsteps, done, policy=_lib.POLICY_MLP)

    def raw_set(widths):
        w = np.asarray(widths, dtype=np.int32)
        n = sum(int(w[l + 1]) * int(w[l]) + int(w[l + 1]) for l in range(len(w) - 1))
        blob = np.zeros(max(n, 1), dtype=np.float32)
        return v.batch._L.clothhip_set_policy_mlp(v.batch._h, len(w) - 1, _lib.i32p(w), blob.ctypes.data_as(C.POINTER(C.c_float)), n)
    assert raw_set([3 * P, 8, 4]) == _lib.OK
    for bad in ([3 * P + 3, 8, 4], [3 * P, 257, 4], [3 * P, 0, 4], [3 * P, 8, 5], [3 * P, 2, 2, 2, 2, 4]):
        assert raw_set(bad) == _lib.EINVAL, bad
    w = np.asarray([3 * P, 8, 4], dtype=np.int32)
    blob = np.zeros(3 * P * 8 + 8 + 8 * 4 + 4 + 1, dtype=np.float32)
    assert v.batch._L.clothhip_set_policy_mlp(v.batch._h, 2, _lib.i32p(w), blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size) == _lib.EINVAL
    for bad in ([3 * P + 3, 8, 4], [3 * P, 257, 4]):
        with pytest.raises(ValueError):
            v.batch.set_policy_mlp(_random_layers(bad, seed=1))
    assert np.array_equal(v.batch.policy_eval(None), np.zeros((3, 4)))      # a refused call leaves the earlier (all-zero) network

    A, Bn = _random_layers([3 * P, 16, 4], seed=61), _random_layers([3 * P, 16, 4], seed=62)
    obs = pre.astype(np.float32)
    v.set_policy(MLPPolicy(v, A))
    act_a = v.policy_actions(obs)
    snap = v.snapshot()
    out_a = v.step_many(policy="mlp", n_actions=1)
    assert np.array_equal(out_a["actions"][0], act_a)
    v.restore(snap)
    assert np.array_equal(v.policy_actions(obs).view(np.int64), act_a.view(np.int64))     # restore leaves the network alone
    v.set_policy(MLPPolicy(v, Bn))                                          # replaced: the next launch runs the new one
    act_b = v.policy_actions(obs)
    out_b = v.step_many(policy="mlp", n_actions=1)
    assert np.array_equal(out_b["actions"][0], act_b) and not np.array_equal(act_a, act_b)
    v.reset(mask=np.array([True, False, True]))
    assert np.array_equal(v.policy_actions(obs).view(np.int64), act_b.view(np.int64))     # ... and so does a masked reset
    v.set_policy(None)
    with pytest.raises(ValueError):
        v.step_many(policy="mlp", n_actions=1)
    with pytest.raises(_lib.ClothHipError):
        v.batch.policy_eval(obs)
    v.close()
