"""CPU tests of the MLP population's host side. The numpy restatement of Philox4x32-10 and of the perturbation eps below is written from
the definition's text (csrc/cloth_policy_population.hpp states the same), not from the device code; tests/test_gpu_mlp_population.py
compares the device against it bit for bit. Here: the generator's published known-answer vectors, the symmetry of eps and of an
antithetic pair, the moments of a fixed-seed sample, the layout of the rows, the evolution-strategies coefficients on a hand-made
fitness vector, and every refusal of the Python side. No GPU."""
import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.policies import MLPPopulation, es_coefficients, pack_mlp, pack_population, population_stride, unpack_mlp

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
EPS_SCALE = np.float32(np.sqrt(3.0) / 2.0 ** 24)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars) of one shape, key: two Python ints. Returns the four output words as uint64 arrays < 2^32."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = M0 * c[0], M1 * c[2]                                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
    return c


def eps_int(seed, k, i):
    """D of perturbation k at blob indices i (int64 array): the centred sum of the four words' top 24 bits."""
    i = np.asarray(i, dtype=np.uint64)
    r = philox4x32_10((i & MASK, i >> np.uint64(32), np.uint64(k), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))
    S = sum(x >> np.uint64(8) for x in r)
    return S.astype(np.int64) - (2 ** 25 - 2)


def eps_from_int(D):
    return np.asarray(D).astype(np.int32).astype(np.float32) * EPS_SCALE


def eps(seed, k, i):
    return eps_from_int(eps_int(seed, k, i))


def weight(theta, signed_sigma, e):
    """(float)((double)theta + (double)(+-sigma) * (double)eps)"""
    return (np.asarray(theta, dtype=np.float32).astype(np.float64) + np.float64(np.float32(signed_sigma)) * e.astype(np.float64)).astype(np.float32)


def reference_rows(theta, G, sigma, seed, antithetic):
    """The G + 1 rows as the device must hold them: float32 [G + 1, stride], stride = n rounded up to 64, pad zeros, row G = theta."""
    theta = np.asarray(theta, dtype=np.float32)
    n = theta.size
    rows = np.zeros((G + 1, (n + 63) // 64 * 64), dtype=np.float32)
    idx = np.arange(n)
    for g in range(G):
        k, sign = (g // 2, 1.0 if g % 2 == 0 else -1.0) if antithetic else (g, 1.0)
        rows[g, :n] = weight(theta, sign * np.float32(sigma), eps(seed, k, idx))
    rows[G, :n] = theta
    return rows


def reference_combine(coef, seed, n):
    """(float) sum_{k ascending} (double)coef[k] * (double)eps_k[i]: a sequential float64 loop."""
    acc = np.zeros(n, dtype=np.float64)
    idx = np.arange(n)
    for k, c in enumerate(np.asarray(coef, dtype=np.float32)):
        acc = acc + np.float64(c) * eps(seed, k, idx).astype(np.float64)
    return acc.astype(np.float32)


class FakeEnv(object):
    """What MLPPopulation reads of an env: the grid size, the batch size, and where it uploads itself."""

    def __init__(self, P=4, E=6):
        self.P, self.E, self.uploaded, self._policy_mlp = P, E, [], None

    def set_policy(self, pop):
        self.uploaded.append((pop, pop.generation, pop.generation_seed(pop.generation)))
        self._policy_mlp = pop


def _layers(widths, seed=0):
    r = np.random.RandomState(seed)
    return [(r.normal(size=(widths[l + 1], widths[l])), r.normal(size=widths[l + 1])) for l in range(len(widths) - 1)]


def _words(c):
    return ["%08x" % int(x) for x in c]


def test_philox_known_answer_vectors():
    assert _words(philox4x32_10((0, 0, 0, 0), (0, 0))) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert _words(philox4x32_10((f, f, f, f), (f, f))) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _words(philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    # vectorised over the counter as the scalar calls
    c = philox4x32_10((np.array([0, f, 0x243F6A88]), np.array([0, f, 0x85A308D3]), np.array([0, f, 0x13198A2E]), np.array([0, f, 0x03707344])),
                      (0, 0))
    assert _words([x[0] for x in c]) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]


def test_eps_scale_and_range():
    assert "%.7e" % EPS_SCALE == "1.0323827e-07" and EPS_SCALE.view(np.uint32) == 0x33DDB3D7
    # S lies in [0, 4 (2^24 - 1)], so D in [-(2^25 - 2), 2^25 - 2]
    top = eps_from_int(np.array([2 ** 25 - 2, -(2 ** 25 - 2), 0]))
    assert top[0] == -top[1] and 3.46 < top[0] <= 3.47 and top[2] == 0.0


def test_eps_is_odd_in_d_and_an_antithetic_pair_is_symmetric_about_theta():
    D = eps_int(0x1234567890, 3, np.arange(4096))
    assert np.array_equal(eps_from_int(-D), -eps_from_int(D))
    big = np.array([2 ** 24 + 1, 2 ** 25 - 3, 2 ** 24 + 3, 33554429])       # not representable in float32: the rounding is symmetric too
    assert np.array_equal(eps_from_int(-big), -eps_from_int(big))
    theta = np.random.RandomState(1).normal(size=4096).astype(np.float32)
    e = eps_from_int(D)
    sigma = np.float32(0.05)
    e64 = e.astype(np.float64)
    step = np.float64(sigma) * e64                                           # float32 x float32: exact in float64
    assert np.array_equal(step, (np.float32(sigma).astype(np.float64) * e64)) and np.array_equal(np.float64(-sigma) * e64, -step)
    from fractions import Fraction
    for j in (0, 17, 4095):                                                  # in exact arithmetic the pair mirrors about theta
        th, d = Fraction(float(theta[j])), Fraction(float(sigma)) * Fraction(float(e[j]))
        assert Fraction(float(step[j])) == d and (th + d) - th == -((th - d) - th)
    # after the rounding to float32 the two displacements differ by at most one ulp of the weight
    d_plus, d_minus = weight(theta, sigma, e).astype(np.float64) - theta, weight(theta, -sigma, e).astype(np.float64) - theta
    ulp = np.spacing(np.maximum(np.abs(weight(theta, sigma, e)), np.abs(weight(theta, -sigma, e)))).astype(np.float64)
    assert (np.abs(d_plus + d_minus) <= ulp).all()


def test_moments_of_a_fixed_seed_sample():
    n = 2 ** 20
    e = eps(20261018, 0, np.arange(n)).astype(np.float64)
    mean, std = e.mean(), e.std()
    print("n = 2^20: mean %.3e (bound %.3e), std - 1 %.3e (bound %.3e), max |eps| %.4f" % (mean, 4 / np.sqrt(n), std - 1, 4 / np.sqrt(2 * n), np.abs(e).max()))
    assert abs(mean) <= 4.0 / np.sqrt(n)
    assert abs(std - 1.0) <= 4.0 / np.sqrt(2.0 * n)
    assert np.abs(e).max() <= 3.47
    # another perturbation index and another index range are other numbers
    assert not np.array_equal(eps(20261018, 1, np.arange(64)), eps(20261018, 0, np.arange(64)))
    assert not np.array_equal(eps(20261018 + 2 ** 32, 0, np.arange(64)), eps(20261018, 0, np.arange(64)))      # the key's high half counts
    assert not np.array_equal(eps(7, 0, np.arange(64) + 2 ** 32), eps(7, 0, np.arange(64)))                    # ... and the counter's


def test_row_layout_stride_pad_and_centre_row():
    assert [population_stride(n) for n in (1, 63, 64, 65, 1529, 124484)] == [64, 64, 64, 128, 1536, 124544]
    assert _lib.POP_ROW_ALIGN == 64 and _lib.POP_ANTITHETIC == 1
    widths, theta = pack_mlp(_layers([300, 5, 4], seed=2), n_in=300)
    assert theta.size == 1529
    for anti in (True, False):
        rows = reference_rows(theta, 4, 0.1, 99, anti)
        assert rows.shape == (5, 1536) and rows.dtype == np.float32
        assert not rows[:, 1529:].any()                                      # the pad
        assert np.array_equal(rows[4, :1529], theta)                         # row G = theta
        e0 = eps(99, 0, np.arange(1529))
        assert np.array_equal(rows[0, :1529], weight(theta, np.float32(0.1), e0))
        if anti:
            assert np.array_equal(rows[1, :1529], weight(theta, -np.float32(0.1), e0))
            assert np.array_equal(rows[2, :1529], weight(theta, np.float32(0.1), eps(99, 1, np.arange(1529))))
        else:
            assert np.array_equal(rows[1, :1529], weight(theta, np.float32(0.1), eps(99, 1, np.arange(1529))))
            assert np.array_equal(rows[3, :1529], weight(theta, np.float32(0.1), eps(99, 3, np.arange(1529))))
    # K = 1 with a unit coefficient: the sum is eps itself
    assert np.array_equal(reference_combine([1.0], 99, 1529), eps(99, 0, np.arange(1529)))


def test_pack_population_and_unpack_round_trip():
    nets = [_layers([12, 5, 4], seed=s) for s in range(3)]
    widths, blob = pack_population(nets, n_in=12)
    assert widths.tolist() == [12, 5, 4] and blob.shape == (3, 12 * 5 + 5 + 5 * 4 + 4) and blob.dtype == np.float32
    for g in range(3):
        assert np.array_equal(blob[g], pack_mlp(nets[g])[1])
        for (W, b), (W2, b2) in zip(nets[g], unpack_mlp(widths, blob[g])):
            assert np.array_equal(W.astype(np.float32), W2) and np.array_equal(b.astype(np.float32), b2)
    with pytest.raises(ValueError):
        pack_population([], n_in=12)
    with pytest.raises(ValueError):                                          # one shape
        pack_population([_layers([12, 5, 4]), _layers([12, 6, 4])], n_in=12)
    with pytest.raises(ValueError):
        pack_population([_layers([12, 257, 4])], n_in=12)
    with pytest.raises(ValueError):
        unpack_mlp(widths, blob[0][:-1])


def test_es_coefficients_on_a_hand_made_fitness_vector():
    f = [3.0, -1.0, 10.0, 0.5]                                               # ranks 2, 0, 3, 1 -> u = 2/3 - 1/2, -1/2, 1/2, 1/3 - 1/2
    sigma = 0.25
    u = np.array([2.0 / 3 - 0.5, -0.5, 0.5, 1.0 / 3 - 0.5])
    w = es_coefficients(f, sigma, antithetic=False, shaping="centered_rank")
    assert w.dtype == np.float32 and np.array_equal(w, (u / (4 * sigma)).astype(np.float32))
    w = es_coefficients(f, sigma, antithetic=True, shaping="centered_rank")
    assert np.array_equal(w, (np.array([u[0] - u[1], u[2] - u[3]]) / (4 * sigma)).astype(np.float32))
    assert np.array_equal(es_coefficients(f, sigma, antithetic=False, shaping="raw"), (np.array(f) / 1.0).astype(np.float32))
    assert np.array_equal(es_coefficients(f, sigma, antithetic=True, shaping="raw"), np.array([4.0, 9.5], dtype=np.float32))
    assert np.array_equal(es_coefficients([5.0, 5.0], 1.0, antithetic=False), np.array([-0.25, 0.25], dtype=np.float32))   # ties: member order
    assert np.array_equal(es_coefficients([7.0], 1.0, antithetic=False), np.zeros(1, dtype=np.float32))
    for bad in (dict(fitness=[1.0, 2.0, 3.0], sigma=1.0, antithetic=True), dict(fitness=[1.0, np.nan], sigma=1.0),
                dict(fitness=[], sigma=1.0, antithetic=False), dict(fitness=[1.0, 2.0], sigma=0.0),
                dict(fitness=[1.0, 2.0], sigma=1.0, shaping="softmax")):
        with pytest.raises(ValueError):
            es_coefficients(**bad)


def test_population_object_seeds_generations_and_fitness():
    env = FakeEnv(P=4, E=6)
    pop = MLPPopulation(env, _layers([12, 5, 4], seed=4), n_members=4, sigma=0.1, seed=2 ** 64 - 1)
    assert env.uploaded == [(pop, 0, 2 ** 64 - 1)]
    assert pop.member.tolist() == [0, 1, 2, 3, 4, 0] and pop.member.dtype == np.int32       # e % (G + 1)
    assert pop.sigma == float(np.float32(0.1)) and pop.n_params == 12 * 5 + 5 + 5 * 4 + 4
    pop.perturb(3)
    assert env.uploaded[-1] == (pop, 3, 2)                                   # seed + generation, mod 2^64
    out = {"rew": np.array([[1.0, 2, 3, 4, 5, 6], [10.0, 20, 30, 40, 50, 60]]),
           "ran": np.array([[True] * 6, [True, True, False, True, True, True]])}
    assert np.array_equal(pop.fitness(out), [(11.0 + 66.0) / 2, 22.0, 3.0, 44.0, 55.0])
    w = pop.coefficients([1.0, 0.0, 0.0, 1.0, 123.0])                        # the centre's entry is left out
    assert np.array_equal(w, es_coefficients([1.0, 0.0, 0.0, 1.0], pop.sigma, True))
    with pytest.raises(ValueError):
        pop.coefficients([1.0, 2.0, 3.0])
    lone = MLPPopulation(FakeEnv(E=3), _layers([12, 4]), n_members=2, sigma=1.0, seed=0, member=[2, 2, 2])
    assert np.isnan(lone.fitness({"rew": np.ones((1, 3)), "ran": np.ones((1, 3), dtype=bool)})[:2]).all()


@pytest.mark.parametrize("name,kw", [
    ("odd G with antithetic", dict(n_members=3)),
    ("G < 1", dict(n_members=0)),
    ("member out of range", dict(member=[0, 1, 2, 3, 4, 5])),
    ("negative member", dict(member=[0, 1, 2, 3, 4, -1])),
    ("wrong map length", dict(member=[0, 1, 2])),
    ("a map of floats", dict(member=[0.0, 1.0, 2.0, 3.0, 4.0, 0.0])),
    ("sigma 0", dict(sigma=0.0)),
    ("sigma not finite", dict(sigma=np.inf)),
    ("negative seed", dict(seed=-1)),
    ("seed of 65 bits", dict(seed=2 ** 64)),
    ("wrong input width", dict(center_layers=_layers([11, 5, 4]))),
    ("hidden width 257", dict(center_layers=_layers([12, 257, 4]))),
    ("five layers", dict(center_layers=_layers([12, 3, 3, 3, 3, 4]))),
    ("last width not 4", dict(center_layers=_layers([12, 5, 3]))),
])
def test_every_python_side_refusal(name, kw):
    env = FakeEnv(P=4, E=6)
    args = dict(center_layers=_layers([12, 5, 4]), n_members=4, sigma=0.1, seed=1)
    args.update(kw)
    with pytest.raises(ValueError):
        MLPPopulation(env, **args)
    assert env.uploaded == []                                                # refused before anything reaches the device


def test_odd_g_without_antithetic_is_accepted():
    env = FakeEnv(P=4, E=6)
    pop = MLPPopulation(env, _layers([12, 5, 4]), n_members=3, sigma=0.1, seed=1, antithetic=False)
    assert pop.member.tolist() == [0, 1, 2, 3, 0, 1] and len(env.uploaded) == 1


def test_library_symbols():
    names = [s[0] for s in _lib.SYMBOLS]
    new = ["clothhip_set_policy_population", "clothhip_set_policy_members", "clothhip_get_policy_mlp", "clothhip_policy_eval_members",
           "clothhip_policy_population_perturb", "clothhip_policy_population_combine"]
    assert all(n in names for n in new)
    L = _lib.load()
    assert L.clothhip_abi_version() == _lib.ABI_VERSION
    # NULL handle: the calls answer with a status instead of touching a device
    assert L.clothhip_set_policy_population(None, 0, None, None, 0, None) == _lib.EINVAL
    assert L.clothhip_set_policy_members(None, None) == _lib.EINVAL
    assert L.clothhip_get_policy_mlp(None, 0, None, 0) == _lib.EINVAL
    assert L.clothhip_policy_eval_members(None, None, 0, None, None) == _lib.EINVAL
    assert L.clothhip_policy_population_perturb(None, 0, None, None, 0, 0.0, 0, 0, None) == _lib.EINVAL
    assert L.clothhip_policy_population_combine(None, None, 0, None) == _lib.EINVAL
