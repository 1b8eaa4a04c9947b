"""Both rasterisers (csrc/cloth_render.hpp: k_render; csrc/cloth_render_obs.hpp: k_render_obs) against the exact reference
(oracle/render_exact.py) computed from the positions READ BACK from the handle and cast to float32, as the kernels cast them: every hand-made
state of render_states.py at every grid in both precisions, the golden 25x25 states, crumpled states taken from the device, and k_render_obs
from every source, in every format and under one-band, one-row-band and walked band plans -- against the reference and byte for byte
against k_render. oracle/render_oracle.py keeps pinning the kernels' bits (test_gpu_render.py); this file pins the rules.

Bounds, derived (oracle/render_exact.py's docstring), never measured; u = 2^-24, SAFETY = 2:
  coverage  a pixel is compared unless a (face, centre) pair lies within tau = SAFETY de of an edge, de the float32 error of that edge
            function from the vertices' projection errors; at most 1 % of an image's pixels may be excused so, none in an exact state
  depth     relative rho = SAFETY d(1/d) d + 2 u per pixel (at most 3.1e-5 on 3x3, 4.7e-3 on 64x64 in these cases: the quotient e / area
            carries the edge error over a small area)
  colour    the byte lies in floor(t -+ dt), never more than 1 from the reference's
  exact states: coverage, every byte and every depth bit, zero tolerance

MEASURED on an MI355X (every test prints its own line, `pytest -s`); the bounds above stay as derived, they are not tightened to these:
  k_render      3x3, 5x5, 9x9, 17x17 (15 exact states each, 13 at 3x3; fp32 and fp64 handles give the same images): relative depth error
                <= 2.7e-7 against bounds up to 3.1e-5 (3x3) .. 3.1e-4 (17x17), at most 2.5 % of the bound (3x3); <= 1 ambiguous pixel of
                67 700; one byte off by one (17x17), inside its window
                12x12: depth <= 5.1e-7 (fp32), 1.2e-6 (fp64), at most 0.78 % of the bound; 9 / 4 ambiguous pixels of 92 200
                25x25 (with the golden states, one at 224 x 224): depth <= 4.2e-7, 0.69 % of the bound; 434 ambiguous pixels of 176 000
                (0.25 %: the straight-down views of the flat start grid's diagonals)
                33x33: depth <= 4.4e-7, 0.53 % of the bound; 34 / 30 ambiguous of 98 400. 50x50: depth <= 9.1e-7, 0.33 %; 48 / 65 ambiguous of
                92 600, one byte off by one. 64x64 (fp32): depth <= 7.1e-7, 0.22 % of a bound of up to 4.7e-3; 24 ambiguous
  k_render_obs  equal to k_render byte for byte from all three sources in all three formats under every plan; against the reference no byte
                off by one; ambiguous 0 (33x33, exact camera, 111 000 pixels), 3 of 9 660 (25x25, one-row bands), 6 of 45 000 (64x64)
  Every exact state held with zero tolerance -- coverage, every byte, every depth bit -- in both kernels, once the tie rule was top-left:
  before, both kernels differed from the reference on 126 outline centres of a flat 32 x 32 pixel square: those on its left and top outline
  uncovered, those on its right and bottom outline covered.
"""
import ctypes as C

import numpy as np
import pytest

import render_states as rs
from oracle import render_exact
from test_gpu_metrics_exact import _SEEDS, _THICKNESS, _actions, _seeded_env
from test_gpu_render_obs import FORMATS, _finish

pytestmark = pytest.mark.gpu

_KNOBS = ("CLOTHHIP_DEBUG_RENDER_LDS", "CLOTHHIP_DEBUG_RENDER_WALK")


def _cfg(n_side):
    import bench
    return bench.bench_cfg(n_side, _THICKNESS.get(n_side, 0.02), "tier1")


# Which two of test_gpu_metrics_exact.py's six env seeds per grid give the crumpled states: those whose state after reset + one action shows
# both sides of the cloth to both cameras and keeps well under the cap of ambiguous pixels (layers in contact lie within the derived depth bound of
# each other; some seeds' states exceed 1 % so). The test asserts both conditions itself, on the reference of the state it reads back.
_CRUMPLED_PICK = {12: (1, 2), 33: (0, 3), 50: (1, 5), 64: (2, 3)}


def _crumpled(n_side, prec):
    """Two states taken from the device: tier-1 reset plus one action, env seeds as in test_gpu_metrics_exact.py."""
    six = _SEEDS.get((n_side, prec), _SEEDS.get((n_side, "f32"), _SEEDS.get((n_side, "f64"))))
    seeds = tuple(six[k] for k in _CRUMPLED_PICK[n_side])
    env = _seeded_env(n_side, prec, seeds)
    env.reset()
    env.step_many(_actions(seeds), auto_reset=False)
    pos = env.batch.positions()
    env.close()
    out = []
    for i, p in enumerate(pos):
        assert np.isfinite(p).all() and np.abs(p).max() <= 64.0
        out.append(rs.RenderCase("crumpled%d_top" % i, p, rs.view(128, 96), i == 0, False, False, {"sides": "both"}))
        out.append(rs.RenderCase("crumpled%d_tilted" % i, p, rs.TILTED, i == 1, False, False, {"sides": "both"}))
    return out


def _batch_of(cases, n_side, prec):
    """One ClothBatch with every case as one env -> (batch, float32 positions as the kernels see them [E, P, 3])."""
    from gym_cloth_amd import ClothBatch
    P = n_side * n_side
    b = ClothBatch(_cfg(n_side), n_envs=len(cases), precision=prec)
    allpos = np.stack([c.pos for c in cases])
    b.set_state(allpos, allpos, np.zeros((len(cases), P), dtype=np.uint8))
    return b, b.positions().astype(np.float32)


def _compare(failures, *args, **kw):
    """render_exact.compare, but a case that fails does not hide the next one: every failing case is reported (a mutant's log names them all)."""
    try:
        render_exact.compare(*args, **kw)
    except AssertionError as e:
        failures.append(str(e))


def _views(cases):
    out = []
    for c in cases:
        if c.view not in out:
            out.append(c.view)
    return out


def test_there_is_no_64x64_fp64_handle():
    """Why (64, 'f64') is missing from render_states.GRID_PRECISIONS: the stepper's fp64 state of 4096 particles does not fit the LDS, so no
    such handle can be created and there is nothing to render from."""
    from gym_cloth_amd import ClothBatch
    with pytest.raises(ValueError, match="LDS"):
        ClothBatch(_cfg(64), n_envs=1, precision="f64")


@pytest.mark.parametrize("n_side,prec", rs.GRID_PRECISIONS, ids=["%d-%s" % gp for gp in rs.GRID_PRECISIONS])
def test_k_render_meets_the_exact_reference(n_side, prec, oracle_lib):
    """k_render: one ClothBatch per (grid, precision), every case one env, one render() per distinct view with the cases' swap flags mixed."""
    cases = list(rs.cases(n_side))
    if n_side == 25:
        cases += rs.golden_cases(oracle_lib)[1]
    if n_side in (12, 33, 50, 64):
        cases += _crumpled(n_side, prec)
    b, pos = _batch_of(cases, n_side, prec)
    swap = np.array([c.swap for c in cases], dtype=np.uint8)
    assert swap.any() and not swap.all()
    stats, n_exact, failures = {}, 0, []
    for v in _views(cases):
        rgb, dep = b.render(swap_sides=swap, **rs.view_kw(v))
        for i, c in enumerate(cases):
            if c.view != v:
                continue
            if not c.name.startswith("crumpled"):
                assert np.array_equal(pos[i].astype(np.float64), c.pos), c.name        # a hand-made state is held as made, in either precision
            ex = rs.exact(pos[i], n_side, v, c.swap, c.exact)
            rs.check_non_vacuity(c, ex, n_side)
            _compare(failures, ex, rgb[i], dep[i], rs.BG_BYTE, tag="%dx%d %s %s" % (n_side, n_side, prec, c.name), stats=stats)
            n_exact += c.exact
    b.close()
    assert not failures, "\n".join(failures)
    assert n_exact >= (12 if rs._pow2(n_side) else 1) and stats["cloth"] > 1000
    assert stats["ambiguous"] <= rs.CAP * stats["pixels"]
    print("MEASURED k_render %dx%d %s: %d cases (%d exact) %s" % (n_side, n_side, prec, len(cases), n_exact,
                                                                 " ".join("%s=%.3g" % kv for kv in sorted(stats.items()))))


@pytest.mark.parametrize("plan", rs.BAND_PLANS, ids=[p[0] for p in rs.BAND_PLANS])
def test_k_render_obs_meets_the_exact_reference_under_every_band_plan(plan, monkeypatch):
    """k_render_obs from a float32 '1d' table, from an fp32 handle's state and from an fp64 handle's state, in all three formats, under the
    band plan of the case: the RGB bytes against the exact reference, every format byte for byte against k_render finished on the host."""
    from gym_cloth_amd import _lib
    _, n_side, v, lds_kib, walk, (rows, bands) = plan
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    cases = list(rs.band_cases(n_side, v))
    E = len(cases)
    kw = rs.view_kw(v)
    swap = np.array([c.swap for c in cases], dtype=np.uint8)
    valid = np.ones(E, dtype=np.uint8)
    valid[1] = 0
    assert swap.any() and not swap.all()
    # the pinned path first, without the knobs: k_render, finished with the numpy lines of ClothVecEnv.image_obs
    b, pos = _batch_of(cases, n_side, "f32")
    rgb, dep = b.render(swap_sides=swap, **kw)
    b.close()
    want = {f: _finish(rgb, dep, f) for f in FORMATS}
    exs = [rs.exact(pos[i], n_side, v, c.swap, c.exact) for i, c in enumerate(cases)]
    if lds_kib is not None:
        monkeypatch.setenv("CLOTHHIP_DEBUG_RENDER_LDS", lds_kib)                   # read when the handle is created
    if walk is not None:
        monkeypatch.setenv("CLOTHHIP_DEBUG_RENDER_WALK", walk)
    got_plan = np.zeros(4, dtype=np.int32)
    p = _lib.params_from_cfg(_cfg(n_side))
    _lib.check(_lib.load().clothhip_selftest_render_plan(C.byref(p), v.width, v.height, _lib.i32p(got_plan)))
    assert got_plan.tolist()[:2] == [rows, bands] and got_plan[3] == 1, got_plan
    # the plan cuts where it matters: a face drawn on both sides of a band border, and (exact camera) a centre exactly on an outline
    # edge in a band's first row
    firsts = np.arange(rows, v.height, rows)
    if bands > 1:
        assert any(((ex.face_v[:, 0] <= r - 0.5) & (ex.face_v[:, 1] >= r + 0.5)).any() for ex in exs for r in firsts)   # spans the centres of rows r - 1 and r
        if v == rs.EX:
            assert any(ex.on_outline[firsts].any() for ex in exs)
    stats, failures = {}, []
    rows32 = pos.reshape(E, -1)
    for src, prec in (("host", "f32"), ("state", "f32"), ("state", "f64")):
        if (n_side, prec) not in rs.GRID_PRECISIONS:
            continue
        h, hpos = _batch_of(cases if src == "state" else cases[:1], n_side, prec)
        assert src == "host" or np.array_equal(hpos, pos)
        for fmt in FORMATS:
            got = h.render_obs(src, obs=rows32 if src == "host" else None, valid=valid, swap_sides=swap, fmt=fmt, **kw)
            assert not got[1].any(), (src, prec, fmt)                                       # valid = 0: all bytes zero
            for i in range(E):
                if valid[i]:
                    assert np.array_equal(got[i], want[fmt][i]), (src, prec, fmt, cases[i].name, int((got[i] != want[fmt][i]).sum()))
            if fmt == "rgb":
                for i, c in enumerate(cases):
                    if valid[i]:
                        rs.check_non_vacuity(c, exs[i], n_side)
                        _compare(failures, exs[i], got[i], None, rs.BG_BYTE, tag="%s %s %s %s" % (plan[0], src, prec, c.name), stats=stats)
        h.close()
    assert not failures, "\n".join(failures)
    assert stats["cloth"] > 300
    print("MEASURED k_render_obs %s (%d rows x %d bands): %s" % (plan[0], rows, bands, " ".join("%s=%.3g" % kv for kv in sorted(stats.items()))))
