"""CPU tests of the exact render reference (oracle/render_exact.py) and of the cases the GPU file renders (render_states.py): the reference
against closed forms, the conditions every case must meet (at most 1 % ambiguous pixels, none in an exact state, each state's non-vacuity
facts), and oracle/render_oracle.py -- the float32 restatement of the kernels -- against the reference through the comparison function the
GPU tests use: the early warning available without a device."""
from fractions import Fraction

import numpy as np
import pytest

import render_states as rs
from oracle import render_exact, render_oracle


def _case(N, name):
    (c,) = [c for c in rs.cases(N) if c.name == name]
    return c


def _ex(c, N):
    return rs.exact(c.pos, N, c.view, c.swap, c.exact)


def _solve3(R, k):
    """Cramer's rule in Fractions: w with R w = k (R row major)."""
    det = lambda m: (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]))
    D = det(R)
    out = []
    for j in range(3):
        m = list(R)
        m[j], m[3 + j], m[6 + j] = k
        out.append(det(m) / D)
    return out


# ---- the reference against closed forms ---------------------------------------------------------------------------------------------
def test_tie_rule_on_the_3x3_grid_of_the_outline_centres():
    """Vertices on the centres {1.5, 3.5, 5.5}^2 of an 8 x 8 image: the square [1.5, 5.5]^2 owns the centres on its left and top outline and
    not those on its right and bottom outline: columns 1..4, rows 2..5 (y up in the world is row 6 down to row 2 in the image)."""
    q = np.array([0.1875, 0.4375, 0.6875])
    pos = rs._grid(3, q, q)
    v = rs.view(8, 8, cam_pos=(0.5, 0.5, 1.0), lens_mm=36.0)
    ex = rs.exact(pos, 3, v, exact=True)
    want = np.zeros((8, 8), dtype=bool)
    want[2:6, 1:5] = True
    assert np.array_equal(ex.covered, want)
    assert ex.on_outline.sum() == 16 and (ex.depth[want] == 1.0).all() and (ex.depth[~want] == 1.0).all()
    assert not ex.front[want].any()                                   # rows run up the image: the other winding


@pytest.mark.parametrize("N", [3, 5, 9, 17, 33])
def test_flat_square_pixel_set_and_depth(N):
    for name in ("flat_on_centres", "flat_between_centres", "turned_over"):
        ex = _ex(_case(N, name), N)
        want = np.zeros((48, 64), dtype=bool)
        want[5:37, 10:42] = True                                      # [10.5, 42.5) x [5.5, 37.5) on centres, (10, 42) x (5, 37) between them
        assert np.array_equal(ex.covered, want), name
        assert all(q == 1 for q in ex.inv_d[want]) and (ex.depth == 1.0).all(), name
        assert len({tuple(b) for b in ex.byte[want]}) == 1, name      # one normal, one intensity: every cloth byte equal


@pytest.mark.parametrize("N", [3, 9, 33])
def test_turned_over_is_the_mirror_image_with_ownership_moved(N):
    """The mirrored cloth has the same outline, so the same pixels -- NOT the mirror image of the pixels: mirrored about the square's axis
    u = 26.5, flat_on_centres' columns 10..41 become 11..42, and ownership moves from the (new) right edge back to the left one."""
    flat, turned, sw = (_ex(_case(N, n), N) for n in ("flat_on_centres", "turned_over", "turned_over_swapped"))
    assert np.array_equal(turned.covered, flat.covered)
    mirrored = np.zeros_like(flat.covered)
    mirrored[:, 52 - np.arange(53)] = flat.covered[:, :53]                                # column ix -> 52 - ix
    assert np.array_equal(mirrored[:, 1:], flat.covered[:, :-1]) and not np.array_equal(mirrored, flat.covered)
    assert flat.front[flat.covered].all() and not turned.front[turned.covered].any() and sw.front[sw.covered].all()
    assert np.array_equal(sw.byte, flat.byte) and not np.array_equal(turned.byte, flat.byte)


@pytest.mark.parametrize("N,name", [(3, "tilted_plane_ex"), (3, "tilted_plane_tilted"), (12, "tilted_plane_tilted"), (25, "tilted_plane_ex")])
def test_tilted_plane_depth_is_the_ray_plane_depth(N, name):
    """z = x / 4 + y / 8 + 1 / 16: the depth at a pixel is where its ray meets the plane, whatever the triangulation -- exactly."""
    c = _case(N, name)
    ex = _ex(c, N)
    sc = rs.scene_of(c.view)
    fr = lambda v: Fraction(float(v))
    R = [fr(v) for v in sc.R]
    cam = [fr(v) for v in sc.cam]
    n = (Fraction(-1, 4), Fraction(-1, 8), Fraction(1))
    ys, xs = np.nonzero(ex.covered)
    assert len(ys) > 100
    for iy, ix in zip(ys[::7], xs[::7]):
        k = ((Fraction(2 * int(ix) + 1, 2) - fr(sc.cx)) / fr(sc.fx), (fr(sc.cy) - Fraction(2 * int(iy) + 1, 2)) / fr(sc.fy), Fraction(-1))
        ray = _solve3(R, k)                                   # R^-1 k (the float32 R is not exactly orthogonal): the world direction per unit depth
        d = (Fraction(1, 16) - sum(a * b for a, b in zip(n, cam))) / sum(a * b for a, b in zip(n, ray))
        assert ex.inv_d[iy, ix] == 1 / d, (ix, iy)


def test_all_background_images():
    for N in (3, 12):
        for name in ("one_point", "one_point_tilted", "collinear", "outside"):
            c = _case(N, name)
            ex = _ex(c, N)
            assert not ex.covered.any() and (ex.byte == 255).all() and (ex.depth == float(np.float32(c.view.cam_pos[2]))).all(), name


def test_the_reference_refuses_what_it_cannot_prove():
    c = _case(5, "tilted_plane_ex")
    with pytest.raises(render_exact.NotExact):
        render_exact.render(c.pos, 5, rs.scene_of(c.view), exact=True)


# ---- the conditions of every case the GPU file uses ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", rs.GRIDS)
def test_conditions_of_every_hand_made_case(N):
    names = set()
    for c in rs.cases(N):
        rs.check_non_vacuity(c, _ex(c, N), N)
        names.add(c.name)
    assert {"flat_on_centres", "flat_between_centres", "turned_over", "tilted_plane_tilted", "coincident_rows", "one_point", "collinear",
            "straddles_left", "straddles_right", "straddles_top", "straddles_bottom", "outside", "behind_camera", "one_pixel", "one_column",
            "one_row"} <= names
    assert (N < 5) or "fold_gap_tilted" in names
    assert (N < 50) or "sub_pixel_top" in names
    assert (N != 3) or "huge_faces_top" in names
    if rs._pow2(N):
        assert sum(c.exact for c in rs.cases(N)) >= 12
        assert (N < 5) or _case(N, "fold_gap_ex").exact


@pytest.mark.parametrize("plan", rs.BAND_PLANS, ids=[p[0] for p in rs.BAND_PLANS])
def test_conditions_of_the_band_plan_cases(plan):
    _, N, v, _, _, (rows, bands) = plan
    cs = rs.band_cases(N, v)
    assert len(cs) >= 4 and rows * bands >= v.height > rows * (bands - 1)
    for c in cs:
        rs.check_non_vacuity(c, _ex(c, N), N)


def test_conditions_of_the_golden_cases(oracle_lib):
    _, cs = rs.golden_cases(oracle_lib)
    for c in cs:
        rs.check_non_vacuity(c, _ex(c, 25), 25)


# ---- the float32 restatement against the reference -------------------------------------------------------------------------------------
def _oracle_images(c, N):
    from gym_cloth_amd import ClothBatch
    d, v = dict(ClothBatch.RENDER_DEFAULTS), c.view
    return render_oracle.render(c.pos, N, v.width, v.height, v.cam_pos, ClothBatch.camera_matrix(v.cam_deg), v.lens_mm, v.sensor_mm, d["front"],
                                d["back"], d["background"], d["light_dir"], d["ambient"], d["energy"], swap=c.swap)


@pytest.mark.parametrize("N", [3, 5, 9, 12, 17])
def test_render_oracle_meets_the_exact_reference(N):
    """oracle/render_oracle.py computes what the kernels compute, in numpy: through the GPU tests' comparison it must meet the reference on
    every case -- in the exact states to the bit, on the outline centres too."""
    stats = {}
    for c in rs.cases(N):
        rgb, dep = _oracle_images(c, N)
        render_exact.compare(_ex(c, N), rgb, dep, rs.BG_BYTE, tag="%dx%d %s" % (N, N, c.name), stats=stats)
    assert stats["cloth"] > 0 and stats["ambiguous"] <= rs.CAP * stats["pixels"]


def test_render_oracle_meets_the_exact_reference_on_golden_states(oracle_lib):
    _, cs = rs.golden_cases(oracle_lib)
    for c in cs[:4]:
        rgb, dep = _oracle_images(c, 25)
        render_exact.compare(_ex(c, 25), rgb, dep, rs.BG_BYTE, tag=c.name)
