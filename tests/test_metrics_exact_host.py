"""The exact-rational metrics reference (oracle/metrics_exact.py) against the reference's own numbers, the host routine
clothhip_hull_area against it on every hand-made state of the GPU tests, and the conditions that make those states mean something --
all without a device, so they are known true before any GPU run.

Bounds (derived, oracle/metrics_exact.py): |coverage - exact| <= 8 (k + 1) 2^-53 for a hull of k vertices; equality where the coordinates
are dyadic or the hull is degenerate by construction. Largest deviation of clothhip_hull_area seen: 1.74e-15 (bound 2.2e-12) on the fp64
circle of 2500 points, every one a hull vertex (0.0 on every fp32 grid); at most 1.27e-16 between the exact area and the golden's Qhull
coverage."""
import numpy as np
import pytest

from metrics_states import GRIDS, check_non_vacuity, exact, held, host_hull_area, states, thickness_of
from oracle import metrics_exact


def test_exact_area_matches_qhull_golden(oracle_lib):
    """All 16 states of g_metrics.npz (25x25; flat / folded / clipped / out-of-bounds / blob; hulls of 4 to 18 vertices): the exact area
    agrees with the coverage scipy / Qhull gave the reference within 2e-16, and out-of-bounds is equal."""
    g = oracle_lib.load_golden("g_metrics.npz")
    assert len(g["pos"]) == 16
    ks = []
    for i, pos in enumerate(g["pos"]):
        ex = exact(pos, 0.02)
        ks.append(ex.k)
        dev = abs(float(ex.area - metrics_exact.Fraction(float(g["coverage"][i]))))
        print("state %d: k %d, |exact - qhull| %.3e" % (i, ex.k, dev))
        assert dev <= 2e-16, (i, dev)
        assert ex.oob == bool(g["oob"][i]), i
    assert min(ks) == 4 and max(ks) == 18, ks            # (what the 25x25 GPU test reaches: no deeper hull stack than 18)


def test_exact_reference_on_known_shapes():
    """The reference itself on shapes whose answers are known in closed form."""
    F = metrics_exact.Fraction
    sq = np.array([[0, 0, 0.5], [1, 0, 0.5], [1, 1, 0.5], [0, 1, 0.5], [0.5, 0.5, 0.5], [0.5, 0, 0.5], [2.0, 0.5, 0.5]])
    ex = metrics_exact.metrics(sq, 0.02)
    assert ex.area == 1 and ex.k == 4 and ex.var == 0 and ex.variance_inv == 1000 and ex.oob and ex.n_below == 0
    tri = np.array([[0.25, 0.25, 0.0], [0.75, 0.25, 0.002], [0.25, 0.75, 0.004]])
    ex = metrics_exact.metrics(tri, 0.004)
    assert ex.area == F(1, 8) and ex.k == 3 and not ex.oob and ex.n_below == 1
    assert ex.var == (F(0.002) ** 2 + F(0.004) ** 2) / 3 - ((F(0.002) + F(0.004)) / 3) ** 2
    assert ex.variance_inv == F(0.001) / ex.var
    for deg in (np.zeros((5, 3)), np.array([[0, 0, 0], [1, 1, 0], [0.5, 0.5, 0], [0.25, 0.25, 0]], dtype=float)):
        ex = metrics_exact.metrics(deg, 0.02)
        assert ex.area == 0 and ex.k == 0


@pytest.mark.parametrize("n_side,prec", GRIDS)
def test_host_hull_area_and_state_conditions(n_side, prec):
    """Every hand-made state as a handle of that precision holds it: the non-vacuity conditions, and clothhip_hull_area within the derived
    bound of the exact area (equal where the state is dyadic or degenerate)."""
    worst = 0.0
    for st in states(n_side, prec):
        pos = held(st.pos, prec)
        ex = exact(pos, thickness_of(prec))
        check_non_vacuity(st, pos, ex, prec)
        area = host_hull_area(pos)
        dev = abs(float(metrics_exact.Fraction(area) - ex.area))
        worst = max(worst, dev)
        assert dev <= metrics_exact.coverage_bound(ex.k), (st.name, dev, ex.k)
        if st.dyadic:
            assert area == float(ex.area), (st.name, area)
        if st.zero_area:
            assert area == 0.0, (st.name, area)
    print("%dx%d %s: max |clothhip_hull_area - exact| = %.3e" % (n_side, n_side, prec, worst))
