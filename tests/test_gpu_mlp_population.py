"""GPU tests of the MLP population (csrc/cloth_policy_population.hpp, MlpDesc::member): the perturbed rows and their weighted sum
against the numpy restatement of tests/test_mlp_population_host.py, bit for bit; a member of a population against the same network as
a handle's shared one, bit for bit -- stand-alone and inside the episode launch, on two thread layouts; the network as the env slot's
across in-kernel resets and a new map; time slices; the library's own refusals."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mlp_policy import _by_env, _cfg, _random_layers
from test_mlp_population_host import eps, reference_combine, reference_rows

pytestmark = pytest.mark.gpu

E, G = 6, 4
MEMBER = np.array([0, 1, 2, 3, 4, 0], dtype=np.int32)
SEEDS = (20261018, 2 ** 32 * 77 + 5)                      # the second: the key's high half is not zero


def _env(n_side=25, prec="f32", tier="tier1", force_grab=False, max_actions=None, same_seed=False):
    from gym_cloth_amd.envs import ClothVecEnv
    cfg = _cfg(n_side, tier, force_grab)
    if max_actions is not None:
        cfg["env"]["max_actions"] = max_actions
    v = ClothVecEnv(cfg, n_envs=E, precision=prec, consume_domrand_draws=False)
    v.seed([1337] * E if same_seed else [1337 + e for e in range(E)])
    return v


_cache = {}


@pytest.fixture(scope="module")
def envs():
    """(n_side, precision, which) -> an env of six cloths after reset() and two random steps; shared by the cases, which only upload
    networks and evaluate."""
    def get(n_side, prec, which=0):
        key = (n_side, prec, which)
        if key not in _cache:
            v = _env(n_side, prec)
            v.reset()
            r = np.random.RandomState(5)
            for _ in range(2):
                v.step(r.uniform(-1, 1, size=(E, 4)))
            _cache[key] = v
        return _cache[key]
    yield get
    for v in _cache.values():
        v.close()
    _cache.clear()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.int64) if a.dtype == np.float64 else a)


def _download(batch, n, rows=G + 1, with_pad=True):
    from gym_cloth_amd.policies import population_stride
    return np.stack([batch.get_policy_mlp(g, population_stride(n) if with_pad else n) for g in range(rows)])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("anti", [True, False], ids=["antithetic", "plain"])
@pytest.mark.parametrize("n_side,hidden", [(10, [5]), (25, [37, 64])], ids=["10-hidden5", "25-hidden37x64"])
def test_perturb_equals_numpy_bit_for_bit(n_side, hidden, anti, seed, envs):
    """All five rows after population_perturb, downloaded with their pad, against the numpy restatement: the same bits, the pad zeros,
    row G the centre. Hidden [5] at n_side 10 has 1 529 parameters: the last vector of four straddles the end of the blob."""
    from gym_cloth_amd.policies import pack_mlp
    v = envs(n_side, "f32")
    layers = _random_layers([3 * n_side * n_side] + hidden + [4], seed=7)
    widths, theta = pack_mlp(layers)
    if hidden == [5]:
        assert theta.size == 1529
    sigma = 0.05
    w2, n = v.batch.population_perturb(layers, G, sigma, seed, antithetic=anti, member=MEMBER)
    assert n == theta.size and np.array_equal(w2, widths)
    got = _download(v.batch, n)
    ref = reference_rows(theta, G, sigma, seed, anti)
    assert got.shape == ref.shape == (G + 1, (n + 63) // 64 * 64)
    assert not got[:, n:].any()
    assert np.array_equal(got[G, :n], theta)
    bad = np.nonzero(_bits(got) != _bits(ref))
    assert len(bad[0]) == 0, (len(bad[0]), bad[0][:5], bad[1][:5])
    assert (np.abs(got[:G, :n] - theta).max(axis=1) > 0).all()               # every member moved
    assert np.array_equal(_download(v.batch, n, with_pad=False), ref[:, :n])
    v.set_policy(None)


@pytest.mark.parametrize("n_side,hidden", [(10, [5]), (25, [37, 64])], ids=["10-hidden5", "25-hidden37x64"])
def test_combine_equals_the_float64_loop_bit_for_bit(n_side, hidden, envs):
    """sum_k coef[k] eps_k for K = 1 (a unit coefficient: eps itself), K = 2 (G = 4, antithetic) and K = G = 4 without the flag,
    coefficients of mixed sign and magnitude, against a sequential float64 loop."""
    v = envs(n_side, "f32")
    layers = _random_layers([3 * n_side * n_side] + hidden + [4], seed=8)
    for g, anti, coef, seed in ((2, True, [1.0], SEEDS[1]), (4, True, [1e-3, -7.5], SEEDS[0]), (4, False, [0.3, -2e4, 1e-6, 5.0], SEEDS[1])):
        _, n = v.batch.population_perturb(layers, g, 0.1, seed, antithetic=anti, member=np.zeros(E, dtype=np.int32))
        got = v.batch.population_combine(coef)
        ref = reference_combine(coef, seed, n)
        assert got.dtype == np.float32 and got.shape == (n,)
        assert np.array_equal(_bits(got), _bits(ref)), (g, anti, np.nonzero(_bits(got) != _bits(ref))[0][:5])
        if coef == [1.0]:
            assert np.array_equal(got, eps(seed, 0, np.arange(n)))
        assert np.abs(got).max() > 0
    v.set_policy(None)


@pytest.mark.parametrize("hidden", [[], [5], [256, 256, 256]], ids=lambda h: "hidden" + "x".join(map(str, h)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n_side", [25, 10])
def test_a_member_computes_the_shared_networks_bits(n_side, prec, hidden, envs):
    """Each of the five rows, downloaded and uploaded as the SHARED network of a second handle: policy_eval_members of the population
    handle equals that handle's policy_eval, row by row, bit for bit -- on uploaded rows and on the handle's own state."""
    from gym_cloth_amd.policies import unpack_mlp
    a, b = envs(n_side, prec, 0), envs(n_side, prec, 1)
    layers = _random_layers([3 * n_side * n_side] + hidden + [4], seed=200 + len(hidden))
    widths, n = a.batch.population_perturb(layers, G, 0.05, SEEDS[1], antithetic=True, member=MEMBER)
    rows = a.state.astype(np.float32)
    assert np.array_equal(rows, b.state.astype(np.float32)) and np.ptp(rows[:, 2::3]) > 0
    mixed = a.batch.policy_eval_members(rows, MEMBER)
    from_state = a.batch.policy_eval_members(None, MEMBER)
    assert np.array_equal(_bits(mixed), _bits(from_state))
    per_row = []
    for g in range(G + 1):
        b.batch.set_policy_mlp(unpack_mlp(widths, a.batch.get_policy_mlp(g, n)))
        shared = b.batch.policy_eval(rows)
        assert np.isfinite(shared).all() and np.abs(shared).max() > 1e-4
        assert np.array_equal(_bits(a.batch.policy_eval_members(rows, np.full(E, g, dtype=np.int32))), _bits(shared)), g
        assert np.array_equal(_bits(b.batch.policy_eval_members(rows, np.zeros(E, dtype=np.int32))), _bits(shared))      # a shared network is blob 0
        assert np.array_equal(_bits(b.batch.policy_eval(None)), _bits(shared))
        per_row.append(shared)
    for e in range(E):
        assert np.array_equal(_bits(mixed[e]), _bits(per_row[MEMBER[e]][e])), e
    assert not np.array_equal(per_row[0], per_row[1]) and not np.array_equal(per_row[0], per_row[G])
    a.set_policy(None); b.set_policy(None)


_RECORDS = ("actions", "rew", "done", "ran", "executed", "n_grabbed", "num_steps", "num_sim_steps", "actual_coverage", "variance_inv",
            "have_tear", "out_of_bounds", "reset_before")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_launch_equals_per_network_launches(prec, monkeypatch):
    """Six identically seeded envs under the map [0, 1, 2, 3, 4, 0], three slots with a noise table, in one launch: env e's actions,
    records and final particles equal env e of a launch that runs network member[e] as the handle's shared network -- array_equal in
    both precisions, it is the same kernel on the same inputs. Envs 0 and 5 share network and seed and equal each other. Once on the
    512-thread and once on the 256-thread layout."""
    from gym_cloth_amd.policies import MLPPopulation, unpack_mlp
    layers = _random_layers([1875, 37, 64, 4], seed=21)
    T = 3
    noise = np.repeat(np.random.RandomState(9).normal(size=(T, 1, 4)) * 0.05, E, axis=1)
    threads = []
    for run in range(2):
        for k in ("CLOTHHIP_DEBUG_LEAN", "CLOTHHIP_DEBUG_W8", "CLOTHHIP_DEBUG_NOSPEC"):
            monkeypatch.delenv(k, raising=False)
        if run == 1:                                                         # the standard arithmetic's other thread layout
            monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", "0")
            monkeypatch.setenv("CLOTHHIP_DEBUG_W8", "0" if threads[0] != 256 else "1")
        v = _env(25, prec, force_grab=True, same_seed=True)

        def launch():
            v.seed([1337] * E)
            v.reset()
            out = v.step_many(policy="mlp", n_actions=T, policy_noise=noise)
            return out, v.batch.get_state()[0].copy()
        v.reset()
        pop = MLPPopulation(v, layers, G, 0.05, SEEDS[1], member=MEMBER)
        nets = pop.members()
        out, state = launch()
        var = v.batch.last_variant()
        assert var["fused"] == 2, var
        threads.append(var["threads"])
        assert out["ran"].all() and (out["n_grabbed"] > 0).all()
        for k in _RECORDS:
            assert np.array_equal(out[k][:, 0], out[k][:, 5]), k
        assert np.array_equal(state[0], state[5])
        assert len({out["actions"][0, e].tobytes() for e in range(5)}) == 5   # five networks, five first actions
        for g in range(G + 1):
            v.set_policy(nets[g])
            ref, ref_state = launch()
            assert v.batch.last_variant()["threads"] == threads[-1]
            for e in np.nonzero(MEMBER == g)[0]:
                for k in _RECORDS:
                    assert np.array_equal(out[k][:, e], ref[k][:, e]), (prec, threads[-1], g, e, k)
                assert np.array_equal(_bits(state[e]), _bits(ref_state[e])), (prec, threads[-1], g, e)
        v.close()
    assert sorted(threads) == [256, 512], threads


def test_the_network_is_the_slots_across_resets_and_a_new_map():
    """Episodes of two actions, five slots, auto_reset: every env is reset inside the launch, and the first action after the reset is
    its own member's network on the new episode's first state (policy_eval_members on reset_obs). Then set_policy_members between two
    launches from the same start: only the remapped envs' actions change."""
    from gym_cloth_amd.policies import MLPPopulation
    v = _env(10, "f32", force_grab=True, max_actions=2)
    pre = v.reset()
    pop = MLPPopulation(v, _random_layers([300, 16, 4], seed=31), G, 0.1, SEEDS[0], member=MEMBER)
    T = 5
    out = v.step_many(policy="mlp", n_actions=T, want_obs=True, auto_reset=True)
    assert (out["reset_before"].max(axis=0) > 0).all(), out["reset_before"]  # every env met an in-kernel reset
    for t in range(T):
        obs = pre.astype(np.float32) if t == 0 else out["obs_t"][t - 1].copy()
        for e in np.nonzero(out["reset_before"][t])[0]:
            obs[e] = out["reset_obs"][e, int(out["reset_before"][t, e]) - 1]
        exp = pop.get_action(obs)
        ran = out["ran"][t]
        assert ran.any() and np.array_equal(out["actions"][t][ran], exp[ran]), t
    v.close()

    v = _env(10, "f32", force_grab=True)
    new_map = np.array([3, 1, 2, 0, 4, 0], dtype=np.int32)                   # envs 0 and 3 swap networks, the others keep theirs
    acts = []
    for m in (MEMBER, new_map):
        v.seed([1337 + e for e in range(E)])
        pre = v.reset()
        if m is MEMBER:
            pop = MLPPopulation(v, _random_layers([300, 16, 4], seed=31), G, 0.1, SEEDS[0], member=MEMBER)
        else:
            pop.set_members(m)
        out = v.step_many(policy="mlp", n_actions=1)
        assert np.array_equal(out["actions"][0], v.batch.policy_eval_members(pre.astype(np.float32), m))
        acts.append(out["actions"][0].copy())
    same = MEMBER == new_map
    assert np.array_equal(acts[0][same], acts[1][same])
    assert (np.abs(acts[0][~same] - acts[1][~same]).max(axis=1) > 0).all()
    v.close()


def test_time_sliced_population_launches_equal_unsliced_f64():
    """collect_demos with a population inside the launch, over time-sliced launches and over whole ones: the same episodes."""
    from gym_cloth_amd.demos import collect_demos
    from gym_cloth_amd.policies import MLPPopulation
    layers = _random_layers([1875, 37, 64, 4], seed=55)
    a, b = [_env(25, "f64", force_grab=True) for _ in range(2)]
    whole = collect_demos(a, MLPPopulation(a, layers, G, 0.05, 3, member=MEMBER), max_episodes=12, slots_per_launch=6, on_device=True)
    idle = []
    step_many = b.step_many

    def spy(*args, **kw):
        out = step_many(*args, **kw)
        idle.append(int((~out["ran"]).sum()))
        return out
    b.step_many = spy
    sliced = collect_demos(b, MLPPopulation(b, layers, G, 0.05, 3, member=MEMBER), max_episodes=12, slots_per_launch=6, on_device=True,
                           time_budget_ms=20.0)
    assert sum(idle) > 0, "no launch was cut by its time slice"
    w, s_ = _by_env(whole, E), _by_env(sliced, E)
    compared = 0
    for e in range(E):
        for ew, es in zip(w[e], s_[e]):
            assert ew["act"] == es["act"] and ew["rew"] == es["rew"] and ew["done"] == es["done"], e
            for ow, os_ in zip(ew["obs"], es["obs"]):
                assert np.array_equal(ow, os_)
            compared += 1
    assert compared >= 6                                                     # (both runs stop at the first twelve episodes, whichever envs they come from)
    a.close(); b.close()


def test_refusals_by_the_library_itself():
    """Raw ctypes: every refusal returns its code and leaves the handle usable -- with its earlier network where the arguments were
    refused."""
    from gym_cloth_amd import _lib
    v = _env(10, "f32", force_grab=True)
    pre = v.reset().astype(np.float32)
    L, h, P = v.batch._L, v.batch._h, 100
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    w = np.asarray([3 * P, 8, 4], dtype=np.int32)
    n = 3 * P * 8 + 8 + 8 * 4 + 4
    zeros2, ones = np.zeros((2, n), dtype=np.float32), np.ones(n, dtype=np.float32)
    ok_map, bad_map = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32), np.array([0, 1, 2, 1, 0, 1], dtype=np.int32)
    out = np.zeros((E, 4))

    assert L.clothhip_set_policy_members(h, _lib.i32p(ok_map)) == _lib.ESTATE                      # nothing to map yet
    assert L.clothhip_set_policy_mlp(h, 2, _lib.i32p(w), fp(ones), n) == _lib.OK                    # the earlier network: all ones
    earlier = v.batch.policy_eval(pre)
    assert np.abs(earlier).max() > 0

    def earlier_network_stays():
        assert np.array_equal(v.batch.policy_eval(pre), earlier)
    assert L.clothhip_set_policy_population(h, 2, _lib.i32p(w), fp(zeros2), 2, _lib.i32p(bad_map)) == _lib.EINVAL      # member >= G
    earlier_network_stays()
    assert L.clothhip_set_policy_population(h, 2, _lib.i32p(w), fp(zeros2), 0, _lib.i32p(ok_map)) == _lib.EINVAL       # G < 1
    earlier_network_stays()
    assert L.clothhip_set_policy_population(h, 2, _lib.i32p(np.asarray([3 * P, 257, 4], dtype=np.int32)), fp(zeros2), 2, _lib.i32p(ok_map)) == _lib.EINVAL
    assert L.clothhip_policy_population_perturb(h, 2, _lib.i32p(w), fp(ones), 3, 0.1, 1, _lib.POP_ANTITHETIC, _lib.i32p(ok_map)) == _lib.EINVAL   # odd G
    assert L.clothhip_policy_population_perturb(h, 2, _lib.i32p(w), fp(ones), 0, 0.1, 1, 0, _lib.i32p(ok_map)) == _lib.EINVAL                       # G < 1
    assert L.clothhip_policy_population_perturb(h, 2, _lib.i32p(w), fp(ones), 2, 0.1, 1, 2, _lib.i32p(ok_map)) == _lib.EINVAL                       # unknown flag
    assert L.clothhip_policy_population_perturb(h, 2, _lib.i32p(w), fp(ones), 2, 0.1, 1, 0, _lib.i32p(np.full(E, 3, dtype=np.int32))) == _lib.EINVAL  # member > G
    earlier_network_stays()
    coef, blob = np.ones(4, dtype=np.float32), np.zeros(n, dtype=np.float32)
    assert L.clothhip_policy_population_combine(h, fp(coef), 1, fp(blob)) == _lib.ESTATE            # a shared network has no perturbations

    # an uploaded population: evaluated through its map; no plain evaluation, nothing to sum
    two = np.stack([ones, 2 * ones]).astype(np.float32)
    assert L.clothhip_set_policy_population(h, 2, _lib.i32p(w), fp(two), 2, _lib.i32p(ok_map)) == _lib.OK
    assert L.clothhip_policy_eval(h, fp(pre), E, _lib.dp(out)) == _lib.ESTATE
    assert b"clothhip_policy_eval_members" in L.clothhip_last_error()
    assert L.clothhip_policy_population_combine(h, fp(coef), 2, fp(blob)) == _lib.ESTATE
    assert L.clothhip_policy_eval_members(h, fp(pre), E, _lib.i32p(bad_map), _lib.dp(out)) == _lib.EINVAL
    assert L.clothhip_set_policy_members(h, _lib.i32p(bad_map)) == _lib.EINVAL
    got = v.batch.policy_eval_members(pre, ok_map)
    assert np.array_equal(got[ok_map == 0], earlier[ok_map == 0]) and not np.array_equal(got[1], earlier[1])
    assert np.array_equal(v.batch.get_policy_mlp(1, n), two[1])
    with pytest.raises(ValueError):
        v.batch.get_policy_mlp(2, n)
    with pytest.raises(ValueError):
        v.batch.get_policy_mlp(0, n + 1)

    # a generated one: K must be the number of perturbations
    assert L.clothhip_policy_population_perturb(h, 2, _lib.i32p(w), fp(ones), 4, 0.1, 1, _lib.POP_ANTITHETIC, _lib.i32p(ok_map)) == _lib.OK
    for K in (4, 1, 0):
        assert L.clothhip_policy_population_combine(h, fp(coef), K, fp(blob)) == _lib.EINVAL, K
    assert L.clothhip_policy_population_combine(h, fp(coef), 2, fp(blob)) == _lib.OK and np.abs(blob).max() > 0
    assert L.clothhip_set_policy_members(h, _lib.i32p(np.full(E, 4, dtype=np.int32))) == _lib.OK    # row G, the centre: the all-ones network
    assert np.array_equal(v.batch.policy_eval_members(pre, np.full(E, 4, dtype=np.int32)), earlier)

    # the relaxed-order companion has no policy code: the launch is refused, the handle stays usable
    nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
    v.batch.set_relaxed_order(True)
    with pytest.raises(_lib.ClothHipError) as ei:
        v.batch.run_actions_begin(v._episode_params(), 1, nsteps, done, policy=_lib.POLICY_MLP)
    assert "[%d]" % _lib.ESTATE in str(ei.value)
    v.batch.set_relaxed_order(False)
    assert np.array_equal(v.batch.policy_eval_members(pre, np.full(E, 4, dtype=np.int32)), earlier)

    # n_layers == 0 drops the population as it drops a shared network
    assert L.clothhip_set_policy_population(h, 0, None, None, 0, None) == _lib.OK
    assert L.clothhip_policy_eval_members(h, fp(pre), E, _lib.i32p(ok_map), _lib.dp(out)) == _lib.ESTATE
    with pytest.raises(_lib.ClothHipError):
        v.batch.run_actions_begin(v._episode_params(), 1, nsteps, done, policy=_lib.POLICY_MLP)
    v.close()
