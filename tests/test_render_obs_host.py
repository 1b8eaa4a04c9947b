"""CPU tests of the two host-side self-tests of clothhip_render_obs: the 8-bit depth rule (the inline function the finishing
kernel runs) against the numpy lines of ClothVecEnv.image_obs, byte for byte, and the band plan's invariants. No device."""
import ctypes as C

import numpy as np
import pytest

from gym_cloth_amd import _lib as lib


def _numpy_depth8(dep):
    """The finishing lines of ClothVecEnv.image_obs (gym_cloth_amd/envs.py), dep float32 [n, npx]."""
    dep = dep[:, :, None]                                  # [n, H, W] with W = 1: the same per-image min / max
    lo = dep.min(axis=(1, 2), keepdims=True); hi = dep.max(axis=(1, 2), keepdims=True)
    nz = np.where(hi > lo, (dep - lo) / np.where(hi > lo, hi - lo, 1.0), 0.0)
    d8 = np.uint8(np.maximum(0.0, np.rint(nz * 255.0) - 50.0))
    assert nz.dtype == np.float32
    return d8[:, :, 0]


def _lib_depth8(dep):
    L = lib.load()
    dep = np.ascontiguousarray(dep, dtype=np.float32)
    out = np.full(dep.shape, 0xAB, dtype=np.uint8)
    lib.check(L.clothhip_selftest_depth8(dep.ctypes.data_as(C.POINTER(C.c_float)), dep.shape[0], dep.shape[1], lib.u8p(out)))
    return out


def _ulp_walk(x, k):
    """float32 values x - k ulp .. x + k ulp"""
    out = [np.float32(x)]
    lo = hi = np.float32(x)
    for _ in range(k):
        lo = np.nextafter(lo, np.float32(-np.inf), dtype=np.float32); hi = np.nextafter(hi, np.float32(np.inf), dtype=np.float32)
        out += [lo, hi]
    return np.sort(np.array(out, dtype=np.float32))


def test_depth8_random_images():
    rng = np.random.RandomState(11)
    dep = rng.uniform(1.15, 1.45, size=(7, 29 * 37)).astype(np.float32)
    dep[3] = rng.uniform(0.0, 1000.0, size=dep.shape[1]).astype(np.float32)
    assert np.array_equal(_lib_depth8(dep), _numpy_depth8(dep))


def test_depth8_constant_and_two_valued_images():
    dep = np.zeros((3, 64), dtype=np.float32)                # all 0: hi == lo, every pixel 0
    dep[1] = 1.45                                            # constant, non-zero
    dep[2, ::3] = 1.45; dep[2, 1::3] = 1.45; dep[2, 2::3] = np.float32(1.2)   # two distinct values: 0 and 255 - 50
    got = _lib_depth8(dep)
    assert np.array_equal(got, _numpy_depth8(dep))
    assert (got[:2] == 0).all() and set(got[2].tolist()) == {0, 205}


def test_depth8_halves_round_to_even():
    """lo = 0, hi = 255 makes nz * 255 the depth itself up to the division's rounding: values on k + .5 and one ulp to either
    side of it, for even and odd k."""
    vals = [np.float32(0.0), np.float32(255.0)]
    for k in (49, 50, 51, 52, 100, 101, 203, 204, 253, 254):
        vals += list(_ulp_walk(k + 0.5, 2))
    dep = np.array(vals, dtype=np.float32)[None, :]
    got, ref = _lib_depth8(dep), _numpy_depth8(dep)
    assert np.array_equal(got, ref)
    # the ties themselves are in the image: nz * 255 of the .5 values must be exactly .5 for the test to mean anything
    nz = (dep - dep.min()) / (dep.max() - dep.min()) * np.float32(255.0)
    frac = nz - np.floor(nz)
    assert (frac == 0.5).sum() >= 8 and ((frac > 0.49) & (frac < 0.5)).any() and ((frac > 0.5) & (frac < 0.51)).any()
    # half to even: 50.5 -> 50 -> 0, 51.5 -> 52 -> 2 (half away from zero would give 1 and 2)
    i50, i51 = vals.index(np.float32(50.5)), vals.index(np.float32(51.5))
    assert nz[0, i50] == 50.5 and got[0, i50] == 0 and nz[0, i51] == 51.5 and got[0, i51] == 2


def test_depth8_camera_range_ulp_by_ulp():
    """Depths of a cloth under the default camera: the bed at 1.45, the cloth up to 0.3 nearer; every float32 within 40 ulps of a
    few values of that range, in one image whose extremes are the range's ends."""
    lo, hi = np.float32(1.45 - 0.3), np.float32(1.45)
    walks = [_ulp_walk(v, 40) for v in (1.45 - 0.3 + 1e-4, 1.2, 1.3, 1.3005882, 1.37, 1.45 - 1e-4)]
    for v in np.linspace(float(lo), float(hi), 511, dtype=np.float64)[1:-1]:      # and around every .5 boundary of the 8-bit scale
        walks.append(_ulp_walk(np.float32(v), 3))
    dep = np.concatenate([[lo, hi]] + walks).astype(np.float32)[None, :]
    assert dep.min() == lo and dep.max() == hi
    assert np.array_equal(_lib_depth8(dep), _numpy_depth8(dep))


def _params(n_side):
    return lib.params_from_cfg({"cloth": {"num_width_points": n_side, "num_height_points": n_side, "width": 1, "height": 1,
                                          "density": 200.0, "ks": 1e4, "damping": 2.0, "thickness": 0.02, "plane_friction": 1.0,
                                          "tear_thresh": 2.0},
                                "frames_per_sec": 30, "simulation_steps": 30, "env": {"grip_radius": 0.003}})


def _plan(n_side, w, h):
    out = np.full(4, -7, dtype=np.int32)
    p = _params(n_side)
    lib.check(lib.load().clothhip_selftest_render_plan(C.byref(p), w, h, lib.i32p(out)))
    return [int(v) for v in out]


@pytest.mark.parametrize("n_side", [3, 25, 50, 64])
@pytest.mark.parametrize("size", [(1, 1), (37, 29), (224, 224), (4096, 8)])
def test_render_plan_covers_the_image_within_lds(n_side, size):
    w, h = size
    rows, bands, lds, fits = _plan(n_side, w, h)
    assert fits == 1                                          # every grid up to 64 x 64 leaves room for a row of 4096 keys
    assert lds <= 163840
    assert rows >= 1 and bands >= 1
    assert rows * bands >= h > rows * (bands - 1)
    ppad = (n_side * n_side + 63) // 64 * 64
    assert lds == 7 * ppad * 4 + rows * w * 8                 # seven per-vertex float arrays + the band's 64-bit keys


def test_render_plan_rejects_a_row_that_cannot_fit():
    # 64 x 64: 114 688 B of vertex arrays leave 49 152 B = 6 144 keys
    assert _plan(64, 6144, 3)[3] == 1 and _plan(64, 6144, 3)[:2] == [1, 3]
    rows, bands, lds, fits = _plan(64, 6145, 3)
    assert fits == 0 and lds > 163840
    assert _plan(3, 30000, 1)[3] == 0
    p = _params(25)
    out = np.zeros(4, dtype=np.int32)
    assert lib.load().clothhip_selftest_render_plan(C.byref(p), 0, 5, lib.i32p(out)) == lib.EINVAL
