"""CPU tests of the per-env material interface (clothhip_set_material / _get_material / _selftest_material): the symbols exist on every
layer, and the seven stepper constants a material turns into are the reference's expressions (cloth.pyx:175-186, :240-241, :368) evaluated
by the library's one derivation -- bit for bit in fp64, their float32 rounding in fp32."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("clothhip_set_material", "clothhip_get_material", "clothhip_selftest_material")
FIELDS = ("density", "ks", "damping", "plane_friction", "tear_thresh", "gravity")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "gym_cloth_amd", "libclothhip.so")):
        ge.build()
    from gym_cloth_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def goldens():
    from oracle import pyoracle
    return {n: pyoracle.load_golden("g_traj_%s_25.npz" % n)["cfg"] for n in ("lift_pull", "friction")}


def params_of(lib, c):
    return lib.params_from_cfg({"cloth": {"num_width_points": c["n_side"], "num_height_points": c["n_side"], "width": c["width"],
                                          "height": c["height"], "density": c["density"], "ks": c["ks"], "damping": c["damping"],
                                          "thickness": c["thickness"], "plane_friction": c["plane_friction"],
                                          "tear_thresh": c["tear_thresh"]},
                                "frames_per_sec": c["frames_per_sec"], "simulation_steps": c["simulation_steps"],
                                "env": {"grip_radius": c["grip_radius"]}}, gravity=c["gravity"], minimum_z=c["minimum_z"])


def material_of(lib, c):
    m = lib.ClothMaterial()
    for k in FIELDS:
        setattr(m, k, float(c[k]))
    return m


def selftest(lib, p, m, precision):
    out = np.full(7, np.nan)
    lib.check(lib.load().clothhip_selftest_material(C.byref(p), None if m is None else C.byref(m), precision, lib.dp(out)))
    return out


def reference_constants(c, n_side, frames_per_sec, simulation_steps):
    """The reference's own expressions in numpy float64, in its order of operations."""
    f = np.float64
    N = f(n_side)
    mass = f(c["density"]) / N / N                                       # cloth.pyx:178
    dt = f(1.0) / f(frames_per_sec) / f(simulation_steps)                # cloth.pyx:177
    return np.array([mass * f(c["gravity"]),                             # :179
                     f(c["ks"]) * f(1.0), f(c["ks"]) * f(0.2),           # :225-232
                     (dt * dt) / mass,                                   # :240
                     f(1) - f(c["damping"]) / f(100),                    # :241
                     f(1.) - f(c["plane_friction"]),                     # :368
                     f(c["tear_thresh"])], dtype=np.float64)             # :272


def test_material_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "clothhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(clothhip_[a-z0-9_]+)\s*\(", hdr))
    bound = {n for n, _, _ in lib.SYMBOLS}
    L = lib.load()
    for name in NAMES:
        assert name in declared and name in bound, name
        assert getattr(L, name) is not None
    assert re.search(r"typedef struct ClothMaterial \{ double density, ks, damping, plane_friction, tear_thresh, gravity; \} ClothMaterial;", hdr)
    assert C.sizeof(lib.ClothMaterial) == 48 == lib.MATERIAL_DTYPE.itemsize
    assert tuple(n for n, _ in lib.ClothMaterial._fields_) == FIELDS == lib.MATERIAL_DTYPE.names
    # purely additive: the ABI version and ClothParams stay what they were
    assert L.clothhip_abi_version() == 7 and C.sizeof(lib.ClothParams) == 104


@pytest.mark.parametrize("which", ["lift_pull", "friction"])
def test_selftest_material_is_the_references_arithmetic(lib, goldens, which):
    """On a handle of the default cfg, the default material and the friction fixture's (ks 7000, damping 1.2, friction 0.5): fp64 bit for
    bit the reference's float64 expressions, fp32 their float32 rounding."""
    base, c = goldens["lift_pull"], goldens[which]
    if which == "friction":
        changed = {k for k in base if base[k] != c[k]}
        assert changed == {"ks", "damping", "plane_friction"}, changed          # the fixture differs from the default in material fields only
    p = params_of(lib, base)
    ref = reference_constants(c, base["n_side"], base["frames_per_sec"], base["simulation_steps"])
    got64 = selftest(lib, p, material_of(lib, c), lib.F64)
    assert got64.tobytes() == ref.tobytes(), (got64, ref)
    got32 = selftest(lib, p, material_of(lib, c), lib.F32)
    assert got32.tobytes() == ref.astype(np.float32).astype(np.float64).tobytes(), (got32, ref)


@pytest.mark.parametrize("which", ["lift_pull", "friction"])
@pytest.mark.parametrize("precision", [0, 1])
def test_handles_own_values_give_the_handles_constants(lib, goldens, which, precision):
    """A material equal to the handle's parameters yields what the derivation yields for the handle itself (m = NULL), and what a
    handle created from the material's cfg gets: the same constants from either source."""
    c = goldens[which]
    p = params_of(lib, c)
    own = selftest(lib, p, None, precision)
    assert selftest(lib, p, material_of(lib, c), precision).tobytes() == own.tobytes()
    assert selftest(lib, params_of(lib, goldens["lift_pull"]), material_of(lib, c), precision).tobytes() == own.tobytes()
    assert np.isfinite(own).all()


def test_selftest_material_validates_like_check_params(lib, goldens):
    p = params_of(lib, goldens["lift_pull"])
    for bad in (0.0, -1.0, float("nan")):
        m = material_of(lib, goldens["lift_pull"])
        m.density = bad
        out = np.zeros(7)
        assert lib.load().clothhip_selftest_material(C.byref(p), C.byref(m), 0, lib.dp(out)) == lib.EINVAL
    out = np.zeros(7)
    assert lib.load().clothhip_selftest_material(C.byref(p), None, 2, lib.dp(out)) == lib.EINVAL
    # without a handle the setters fail loudly instead of crashing
    assert lib.load().clothhip_set_material(None, 0, 1, None) == lib.EINVAL
    assert lib.load().clothhip_get_material(None, 0, 1, None) == lib.EINVAL
