"""Host tests of the exploration noise made on the device (no GPU: clothhip_selftest_normal_fixed runs the device's inline
function on the host): references.normal_fixed_reference against it by bytes; its accuracy against numpy's own Box-Muller on the same
uniforms, under the bound DESIGN derives; the distribution of the reference (Kolmogorov-Smirnov against Phi, four moments, the
correlation of the components, the tail beyond population_eps' support); the key (seed, env, slot) and nothing else; the bindings against
the header's signatures and the wrappers' refusals before any library call."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.policies import DeviceNoise, exp_fixed_reference, log_fixed_reference, normal_fixed_reference, policy_noise_reference
from gym_cloth_amd.references import normal_uniforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# DESIGN 4.3.13, in units of rad * 2^-52 (u = 2^-53 is half of it), all absolute:
#   normal_fixed against the exact value on the same uniforms: 8.2 u = 4.1 units (log_fixed 6.2 u relative -> rad 4.1 u; the angle's
#   product and constant 1.06 u, the two Horner series 1.96 u; the last product 1 u)
#   numpy's own rad * cos/sin(x) turned exactly by the quadrant: log, sqrt, cos/sin within one ulp each and the same angle error:
#   (2 + 2 + 1.06 + 1) u = 3.1 units
#   numpy's own rad * cos/sin(q pi/2 + x): as above with the rounding of q (pi/2) (<= 4 u), of the sum (<= 4 u) and q times the error of
#   the constant pi/2 (<= 1.65 u) in the angle: (2 + 2 + 10.71 + 1) u = 7.9 units
BOUND_TURNED = 4.1 + 3.1
BOUND_SUMMED = 4.1 + 7.9
LOG_BOUND = (6.2 + 2.0) * 2.0 ** -53          # log_fixed's 6.2 u plus one ulp of numpy's log, relative


def _c_normal(seed, env, slot):
    L = _lib.load()
    env = np.ascontiguousarray(env, dtype=np.uint32)
    slot = np.ascontiguousarray(slot, dtype=np.uint64)
    out = np.zeros((env.size, 4))
    rc = L.clothhip_selftest_normal_fixed(int(seed), env.ctypes.data_as(C.POINTER(C.c_uint32)), slot.ctypes.data_as(C.POINTER(C.c_uint64)), env.size, _lib.dp(out))
    assert rc == _lib.OK
    return out


def _triples(n=2500):
    """n (env, slot) pairs for each of four seeds, 10^4 triples in all: envs 0 and 2^32 - 1, slot 0, slots and seeds above 2^32."""
    r = np.random.RandomState(5)
    env = r.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    slot = r.randint(0, 2 ** 63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    env[:4] = [0, 2 ** 32 - 1, 0, 2 ** 32 - 1]
    slot[:4] = [0, 0, 2 ** 64 - 1, 2 ** 32]
    slot[4:n // 2] = np.arange(4, n // 2)                       # and the small slot numbers a collection uses
    return [(seed, env, slot) for seed in (0, 1, 12345, 2 ** 63 + 2 ** 32 + 7)]


# ---- 1. the reference is the C function --------------------------------------------------------------------------------------------------
def test_normal_fixed_reference_equals_the_c_function_by_bytes():
    total = 0
    for seed, env, slot in _triples():
        got = _c_normal(seed, env, slot)
        want = normal_fixed_reference(seed, env, slot)
        assert want.dtype == np.float64 and want.shape == (env.size, 4) and np.isfinite(want).all()
        assert got.tobytes() == want.tobytes(), seed
        total += env.size
    assert total == 10 ** 4
    L = _lib.load()
    assert L.clothhip_selftest_normal_fixed(0, None, None, 0, None) == _lib.OK
    assert L.clothhip_selftest_normal_fixed(0, None, None, 1, None) == _lib.EINVAL and L.clothhip_selftest_normal_fixed(0, None, None, -1, None) == _lib.EINVAL


# ---- 2. accuracy -------------------------------------------------------------------------------------------------------------------------
def test_normal_fixed_reference_against_numpys_own_box_muller():
    worst_t = worst_s = worst_l = 0.0
    for seed in (3, 2 ** 40 + 1):
        env, slot = np.meshgrid(np.arange(512), np.arange(256), indexing="ij")
        z = normal_fixed_reference(seed, env, slot).reshape(-1, 2, 2)                      # [..., pair, (cos, sin)]
        n1, n2 = (a.reshape(-1, 2) for a in normal_uniforms(seed, env, slot))
        u1 = (n1.astype(np.float64) + 0.5) * 2.0 ** -52
        q = (n2 >> np.uint64(50)).astype(np.int64)
        x = (((n2 & np.uint64(2 ** 50 - 1)).astype(np.float64) + 0.5) * 2.0 ** -50 - 0.5) * (np.pi / 2)
        assert (u1 > 0.0).all() and (u1 < 1.0).all() and (np.abs(x) < np.pi / 4).all()
        rad = np.sqrt(-2.0 * np.log(u1))
        unit = rad * 2.0 ** -52
        summed = np.stack([rad * np.cos(q * (np.pi / 2) + x), rad * np.sin(q * (np.pi / 2) + x)], axis=-1)
        c, s = np.cos(x), np.sin(x)
        turned = np.stack([rad * np.choose(q, [c, -s, -c, s]), rad * np.choose(q, [s, c, -s, -c])], axis=-1)
        worst_s = max(worst_s, float((np.abs(z - summed) / unit[..., None]).max()))
        worst_t = max(worst_t, float((np.abs(z - turned) / unit[..., None]).max()))
        worst_l = max(worst_l, float(np.abs(log_fixed_reference(u1.reshape(-1)) / np.log(u1.reshape(-1)) - 1.0).max()))
    print("normal_fixed_reference against numpy, in rad 2^-52: %.3f (quadrant in the angle; bound %.1f), %.3f (quadrant by signs; bound %.1f); "
          "log_fixed relative %.3e (bound %.3e)" % (worst_s, BOUND_SUMMED, worst_t, BOUND_TURNED, worst_l, LOG_BOUND))
    assert worst_s <= BOUND_SUMMED and worst_t <= BOUND_TURNED and worst_l <= LOG_BOUND
    # log_fixed at the ends of its domain here and at the mantissa's switch
    for u in (2.0 ** -53, 1.0 - 2.0 ** -53, 0.5, float(np.nextafter(np.sqrt(0.5), 1.0)), float(np.nextafter(np.sqrt(0.5), 0.0)), 0.75):
        assert abs(float(log_fixed_reference(u)[0]) - math.log(u)) <= LOG_BOUND * abs(math.log(u)), u


# ---- 3. the distribution -----------------------------------------------------------------------------------------------------------------
_PHI = np.vectorize(lambda v: 0.5 * (1.0 + math.erf(v / math.sqrt(2.0))), otypes=[np.float64])


@pytest.mark.parametrize("seed", [1, 12345])
def test_distribution_of_the_reference(seed):
    E, S = 1024, 256
    tab = policy_noise_reference(seed, S, E, 1.0)                       # [S, E, 4]: envs 0 .. 1023, slots 0 .. 255
    z = tab.reshape(-1)
    N, n = z.size, z.size // 4
    assert N == 2 ** 20
    zs = np.sort(z)
    F = _PHI(zs)
    i = np.arange(1, N + 1, dtype=np.float64)
    D = max(float((i / N - F).max()), float((F - (i - 1.0) / N).max()))
    mean, var = float(z.mean()), float(z.var())
    m4 = float(((z - mean) ** 4).mean())
    cols = tab.reshape(-1, 4)
    corr = np.corrcoef(cols.T)
    off = float(np.abs(corr - np.eye(4)).max())
    fig = (math.sqrt(N) * D, abs(mean) * math.sqrt(N), abs(var - 1.0) * math.sqrt(N / 2.0), abs(m4 - 3.0) * math.sqrt(N / 96.0), off * math.sqrt(n))
    print("seed %d: sqrt(N) D_KS %.3f, |mean| sqrt(N) %.3f, |var - 1| sqrt(N/2) %.3f, |m4 - 3| sqrt(N/96) %.3f, max corr sqrt(n) %.3f, max |z| %.3f"
          % ((seed,) + fig + (float(np.abs(z).max()),)))
    assert fig[0] < 1.95 and all(f < 4.0 for f in fig[1:])
    assert np.abs(z).max() > 3.47                                        # beyond the support of population_eps


# ---- 4. the key --------------------------------------------------------------------------------------------------------------------------
def test_the_noise_is_keyed_by_seed_env_and_slot_alone():
    seed, T, E = 2 ** 35 + 9, 5, 7
    sigma = np.random.RandomState(2).uniform(0.1, 2.0, size=(E, 4))
    base = np.array([0, 3, 2 ** 33, 1, 0, 17, 2], dtype=np.int64)
    tab = policy_noise_reference(seed, T, E, sigma, base)
    assert tab.shape == (T, E, 4) and tab.dtype == np.float64
    for t in range(T):
        for e in range(E):
            E2 = e + 3                                                   # another T (1) and another E
            sg = np.ones((E2, 4))
            sg[e] = sigma[e]
            b2 = np.zeros(E2, dtype=np.int64)
            b2[e] = base[e] + t
            assert policy_noise_reference(seed, 1, E2, sg, b2)[0, e].tobytes() == tab[t, e].tobytes()
    assert policy_noise_reference(seed, T, E, sigma).tobytes() == policy_noise_reference(seed, T, E, sigma, np.zeros(E, dtype=np.int64)).tobytes()
    # scalar and [4] sigma are the [E, 4] table of equal rows; the multiplication is the only use of sigma
    assert policy_noise_reference(seed, T, E, 0.3).tobytes() == policy_noise_reference(seed, T, E, np.full((E, 4), 0.3)).tobytes()
    v = np.array([0.1, 0.2, 0.0, 4.0])
    assert policy_noise_reference(seed, T, E, v).tobytes() == (v * policy_noise_reference(seed, T, E, 1.0)).tobytes()
    # one step in the seed, the env or the slot changes all four values
    env, slot = np.meshgrid(np.arange(50), np.arange(40), indexing="ij")
    z = normal_fixed_reference(seed, env, slot)
    assert (z != normal_fixed_reference(seed + 1, env, slot)).all()
    assert (z != normal_fixed_reference(seed, env + 1, slot)).all() and (z != normal_fixed_reference(seed, env, slot + 1)).all()
    assert (z[:-1] != z[1:]).all() and (z[:, :-1] != z[:, 1:]).all()
    # the head's sigma is exp_fixed of the float32 values
    ls = np.array([-1.5, 0.0, 0.25, -3.0], dtype=np.float32)
    sg = exp_fixed_reference(ls.astype(np.float64))
    assert sg[1] == 1.0 and policy_noise_reference(1, 2, 3, sg)[:, :, 1].tobytes() == policy_noise_reference(1, 2, 3, 1.0)[:, :, 1].tobytes()


# ---- 5. the bindings ---------------------------------------------------------------------------------------------------------------------
NEW = ["clothhip_policy_noise_fill", "clothhip_policy_noise_get", "clothhip_selftest_normal_fixed"]
_CTYPES = {"clothhip_handle *": C.c_void_p, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "int64_t": C.c_int64, "const int64_t *": C.POINTER(C.c_int64),
           "const double *": C.POINTER(C.c_double), "double *": C.POINTER(C.c_double), "void **": C.POINTER(C.c_void_p),
           "const uint32_t *": C.POINTER(C.c_uint32), "const uint64_t *": C.POINTER(C.c_uint64)}


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
    assert L.clothhip_policy_noise_fill(None, 0, 1, None, None, 0, None) == _lib.EINVAL                # NULL handle: a status, no device touched
    assert L.clothhip_policy_noise_get(None, 1, None) == _lib.EINVAL


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s) before refusing its arguments" % name)


def test_wrappers_refuse_before_any_library_call():
    b = ClothBatch.__new__(ClothBatch)
    b._L, b._h, b.P, b.E = _NoLibrary(), None, 3, 2
    bad = [dict(seed=-1, n_actions=1), dict(seed=2 ** 64, n_actions=1), dict(seed=0, n_actions=0), dict(seed=0, n_actions=2 ** 30),
           dict(seed=0, n_actions=1, sigma=-0.1), dict(seed=0, n_actions=1, sigma=np.nan), dict(seed=0, n_actions=1, sigma=np.inf),
           dict(seed=0, n_actions=1, sigma=np.ones(3)), dict(seed=0, n_actions=1, sigma=np.ones((3, 4))), dict(seed=0, n_actions=1, sigma=np.ones((2, 4, 1))),
           dict(seed=0, n_actions=1, sigma=[1.0, 1.0, -1.0, 1.0]), dict(seed=0, n_actions=1, sigma=1.0, slot_base=np.array([0, -1])),
           dict(seed=0, n_actions=1, sigma=1.0, slot_base=np.array([0, 1, 2])), dict(seed=0, n_actions=1, sigma=1.0, slot_base=np.array([0.0, 1.0])),
           dict(seed=0, n_actions=2, sigma=1.0, slot_base=np.array([0, 2 ** 63 - 2], dtype=np.int64))]
    for kw in bad:
        with pytest.raises(ValueError):
            b.policy_noise_fill(**kw)
    with pytest.raises(ValueError):
        b.policy_noise_get()                                             # before any fill
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(seed=0, sigma=-1.0), dict(seed=0, sigma=np.nan), dict(seed=0, sigma=np.ones(3)),
               dict(seed=0, sigma=np.ones((2, 3))), dict(seed=0, sigma=np.ones((2, 2, 4)))):
        with pytest.raises(ValueError):
            DeviceNoise(**kw)
    d = DeviceNoise(7, sigma=0.5)
    assert d.slot_base is None and np.array_equal(d.base(2), np.zeros(2, dtype=np.int64)) and d.base(2).dtype == np.int64
    d.advance(np.array([[True, True], [True, False], [False, False]]))
    assert np.array_equal(d.slot_base, [2, 1])
    with pytest.raises(ValueError):
        d.base(3)
    with pytest.raises(ValueError):
        d.fill(b, 0)                                                     # the batch's wrapper refuses, still without the library
    assert DeviceNoise(1).sigma is None and DeviceNoise(1, sigma=[1, 2, 3, 4]).sigma.shape == (4,)
