"""The early walk's rule, without a GPU (csrc/phase_strain.hpp: strain_sweep_lean, EARLY): the strain sweep enters the window table
at window 0 while the pre-pass is still testing the springs, and takes the pre-pass's result -- first and last flagged window -- only where its
own reach is used up. The pre-pass therefore reads particle records the walk is correcting: a spring may be tested before, between or after
the corrections of its particles, or on a record mixed word by word from before and after one. The argument says none of that matters, because
the pre-pass's only output is where the walk may stop. This file restates the numpy model of tests/test_sweep_rule.py (same exported tables,
same 24 stretched states) with such a pre-pass and holds it, over seeded interleavings, to the reference's sequential loop (cloth.pyx:258-296)
bit for bit."""
import numpy as np
import pytest

from test_host_logic import golden_cfg, lib  # noqa: F401  (fixture)
from test_sweep_rule import C11, window_table, _sequential

GRANT = 4                   # windows the walk grants itself while the pre-pass's count is short (phase_strain.hpp: EARLY_GRANT)
INTERLEAVINGS = 300         # per state


def _states():
    """The 24 stretched states of tests/test_sweep_rule.py::test_pass_rule_equals_sequential_sweep, in its order (same generator, same draws)."""
    from oracle.pyoracle import load_golden
    rng = np.random.RandomState(7)
    for name, cps in (("g_traj_lift_pull_25.npz", (4, 9, 12)), ("g_traj_fold_25.npz", (3, 6)), ("g_traj_tear_25.npz", (2,))):
        g = load_golden(name)
        rest = np.asarray(g["rest"], dtype=np.float64)
        tt = float(g["cfg"]["tear_thresh"])
        for cp in cps:
            if cp >= len(g["cp_pos"]):
                continue
            base = np.asarray(g["cp_pos"][cp], dtype=np.float64)
            pin = np.asarray(g["cp_pinned"][cp]).astype(np.uint8).copy()
            for variant in range(4):
                pos = base.copy()
                if variant == 0:
                    pos = pos.mean(axis=0) + (pos - pos.mean(axis=0)) * 1.13
                elif variant == 1:
                    idx = np.nonzero(pin)[0] if pin.any() else np.array([0, 1, 25])
                    pos[idx] += np.array([0.03, 0.02, 0.05])
                elif variant == 2:
                    pos += rng.normal(scale=0.004, size=pos.shape)
                else:
                    pin[[100, 101, 126, 300, 325]] = 1
                    pos[[100, 126, 300]] += np.array([0.0, 0.06, 0.1])
                    pos[350:360] += np.array([0.2, 0.0, 0.3])
                yield (name, cp, variant), pos, pin.copy(), rest, tt, g


class _Tables:
    """Per window: lanes in use, their springs, particles, dependency words, reach -- taken apart once."""
    def __init__(self, W):
        A, B, sa = W["A"], W["B"], W["spring_at"]
        self.nW = W["nW"]
        self.win = []
        for w in range(self.nW):
            lanes = np.nonzero(sa[w * 64:(w + 1) * 64] >= 0)[0]
            sw = sa[w * 64 + lanes].astype(np.int64)
            self.win.append((lanes.astype(np.uint64), sw, A[sw], B[sw], W["dep"][w * 64 + lanes].astype(np.uint64),
                             (int(W["ent"][w * 64]) >> 28) << W["rshift"]))
        valid = np.nonzero(sa >= 0)[0]
        self.slot = valid                                         # table slots in use, ascending
        self.spring = sa[valid].astype(np.int64)                  # their springs
        self.a, self.b = A[self.spring], B[self.spring]


def _early_walk(pos0, pin, rest, Tb, tear_thresh, rng, take_published_end=True):
    """The walk from window 0 beside a pre-pass whose spring tests happen at random moments of it.
    Moments are counted in passes. Spring k (in table order) is tested at moment when[k] <= done_at; the count of the pre-pass is complete at
    done_at. A test at a moment right behind a correcting pass reads, word by word at random, the record from before or from after that pass."""
    pos = pos0.copy()
    tear = False
    n = len(Tb.slot)
    done_at = int(rng.randint(0, 150))
    when = rng.randint(0, done_at + 1, size=n)
    order = np.argsort(when, kind="stable")
    when_sorted = when[order]
    nxt = 0                                                       # springs order[:nxt] have been tested
    both = (pin[Tb.a] != 0) & (pin[Tb.b] != 0)
    flagged = np.zeros(n, dtype=bool)
    moment = 0
    prev = pos.copy()                                             # the state before the last pass's corrections

    def test_until(m):
        nonlocal nxt
        hi = int(np.searchsorted(when_sorted, m, side="right"))
        if hi <= nxt:
            return
        k = order[nxt:hi]
        mix = rng.randint(0, 2, size=(len(k), 2, 3)).astype(bool)  # per word: the record from before (prev) or after (pos) the last pass
        pa = np.where(mix[:, 0], prev[Tb.a[k]], pos[Tb.a[k]])
        pb = np.where(mix[:, 1], prev[Tb.b[k]], pos[Tb.b[k]])
        d = pa - pb
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        r = rest[Tb.spring[k]]
        flagged[k] = (~both[k]) & ((ln > r * C11) | (ln > r * tear_thresh))
        nxt = hi

    t11 = [rest[x[1]] * C11 for x in Tb.win]                      # per window: the limits and the both-pinned springs of this state
    ttr = [rest[x[1]] * tear_thresh for x in Tb.win]
    bothws = [(pin[x[2]] != 0) & (pin[x[3]] != 0) for x in Tb.win]
    test_until(0)
    w, w_end, known = 0, min(GRANT, Tb.nW) - 1, False
    while True:
        while w <= w_end:
            lanes, sw, a, b, dep, reach = Tb.win[w]
            bothw, lim, limt = bothws[w], t11[w], ttr[w]
            pend = np.ones(len(lanes), dtype=bool)
            while True:
                d = pos[a] - pos[b]
                ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                trig = (ln > lim) & ~bothw & pend
                tb = np.bitwise_or.reduce(np.uint64(1) << lanes[trig]) if trig.any() else np.uint64(0)
                bad = ((dep & tb) != 0) & pend
                fin = pend & ~bad
                if ((ln > limt) & fin & ~bothw).any():
                    tear = True
                prev = pos                                        # (a quiet pass: before == after)
                if tb != 0:
                    prev = pos.copy()
                    w_end = max(w_end, w + reach)
                    i = np.nonzero(trig & ~bad)[0]                 # they share no particle: one numpy statement per branch of :281-296
                    u = d[i] / ln[i][:, None]
                    e = (ln[i] - lim[i])[:, None]
                    pa_, pb_ = pin[a[i]] != 0, pin[b[i]] != 0
                    ia, ib, ih = i[pa_], i[~pa_ & pb_], i[~pa_ & ~pb_]
                    pos[b[ia]] = pos[b[ia]] + u[pa_] * e[pa_]
                    pos[a[ib]] = pos[a[ib]] - u[~pa_ & pb_] * e[~pa_ & pb_]
                    uh, eh = u[~pa_ & ~pb_], e[~pa_ & ~pb_] * 0.5
                    pos[a[ih]] = pos[a[ih]] - uh * eh
                    pos[b[ih]] = pos[b[ih]] + uh * eh
                moment += 1
                test_until(moment)                                # the pre-pass's tests of this moment: on records mixed across this pass
                if tb == 0:
                    break
                pend = bad
                if not pend.any():
                    break
            w += 1
        # the cold edge: the walk's reach is used up
        if known:
            break
        if moment < done_at:
            if w < Tb.nW:
                w_end = min(w + GRANT, Tb.nW) - 1                 # a quiet window is always exact: walk on
                continue
            prev = pos                                            # the table's end: wait (nothing moves any more)
            moment = done_at
            test_until(moment)
        assert nxt == n
        known = True
        if take_published_end and flagged.any():
            fl = Tb.slot[flagged]
            w_end = max(w_end, int(fl.max()) >> 6)
            w = max(w, int(fl.min()) >> 6)
        if w > w_end:
            break
    return pos, tear


@pytest.fixture(scope="module")
def tables(lib):
    W = window_table(lib, 25)
    return W, _Tables(W)


def test_early_walk_equals_sequential_sweep_under_any_interleaving(tables):
    W, Tb = tables
    cases = 0
    for key, pos, pin, rest, tt, g in _states():
        assert np.array_equal(g["spring_a"], W["A"]) and np.array_equal(g["spring_b"], W["B"])
        p_seq, t_seq = _sequential(pos, pin, rest, W["A"], W["B"], tt)
        for it in range(INTERLEAVINGS):
            rng = np.random.RandomState(1000 * cases + it)
            p_w, t_w = _early_walk(pos, pin, rest, Tb, tt, rng)
            assert np.array_equal(p_seq, p_w), (key, it, float(np.abs(p_seq - p_w).max()))
            assert t_seq == t_w, (key, it)
        cases += 1
    assert cases >= 20


def test_a_walk_that_ignores_the_published_end_is_caught(tables):
    """The model of mutant 5 (csrc: CLOTHHIP_MUTATE == 5): the walk stops at its own reach without taking the pre-pass's last flagged window.
    The states above tell it from the sequential loop -- so the comparison above does pin the rule."""
    W, Tb = tables
    wrong = 0
    for n_case, (key, pos, pin, rest, tt, g) in enumerate(_states()):
        p_seq, _ = _sequential(pos, pin, rest, W["A"], W["B"], tt)
        p_w, _ = _early_walk(pos, pin, rest, Tb, tt, np.random.RandomState(n_case), take_published_end=False)
        wrong += 0 if np.array_equal(p_seq, p_w) else 1
    assert wrong >= 1
