"""The rule of the early walk with per-window flags, without a GPU (csrc/phase_strain.hpp: strain_sweep_lean, EARLY;
csrc/substep_strain_early.inc.hpp): while the walk runs, the other waves test whole WINDOWS of the table with the walk's own quiet-window test
and publish per window a bit in the flag mask F and then a bit in the tested mask D. Where its reach is used up (w > w_end) the walk reads D, then
F, and continues at the first window w' >= w that is untested or flagged; everything in between is jumped over; no such window: the sweep is over.
A window is therefore tested before, between or after corrections of its particles, on records mixed word by word from before and after one, or
never. This file restates the numpy model of tests/test_early_walk_rule.py (same exported tables, same 24 stretched states) with such a pre-pass
and holds it, over seeded interleavings, to the reference's sequential loop (cloth.pyx:258-296) bit for bit."""
import numpy as np
import pytest

from test_host_logic import golden_cfg, lib  # noqa: F401  (fixture)
from test_sweep_rule import C11, window_table, _sequential
from test_early_walk_rule import _states, _Tables

GRANT_FIRST, GRANT = 2, 4   # phase_strain.hpp: EARLY_GRANT_FIRST, EARLY_GRANT
INTERLEAVINGS = 300         # per state
NEVER = 1 << 30


def _flag_walk(pos0, pin, rest, Tb, tear_thresh, rng, look_at_flags=True, log=None):
    """The walk from window 0 beside a pre-pass that tests window v at moment when[v] (counted in passes of the walk) or never. The F bit of a
    tested window is visible from that moment on, its D bit from a moment not earlier. A test right behind a correcting pass reads, word by
    word at random, the record from before or from after that pass."""
    assert tear_thresh >= C11                                     # (the early order is not taken otherwise)
    pos = pos0.copy()
    tear = False
    nW = Tb.nW
    horizon = int(rng.randint(0, 150))
    when = rng.randint(0, horizon + 1, size=nW)
    when[rng.rand(nW) < 0.15] = NEVER                             # never tested in this sweep's lifetime
    d_at = np.where(when == NEVER, NEVER, when + rng.randint(0, 3, size=nW))      # the D bit is set after the F bit
    order = np.argsort(when, kind="stable")
    when_sorted = when[order]
    nxt = 0
    F = np.zeros(nW, dtype=bool)
    bothws = [(pin[x[2]] != 0) & (pin[x[3]] != 0) for x in Tb.win]
    t11 = [rest[x[1]] * C11 for x in Tb.win]
    ttr = [rest[x[1]] * tear_thresh for x in Tb.win]
    moment = 0
    prev = pos.copy()                                             # the state before the last pass's corrections

    def test_until(m):
        nonlocal nxt
        hi = int(np.searchsorted(when_sorted, m, side="right"))
        for v in order[nxt:hi]:
            lanes, sw, a, b, dep, reach = Tb.win[v]
            mix = rng.randint(0, 2, size=(len(a), 2, 3)).astype(bool)
            pa = np.where(mix[:, 0], prev[a], pos[a])
            pb = np.where(mix[:, 1], prev[b], pos[b])
            d = pa - pb
            ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            F[v] = bool(((ln > t11[v]) & ~bothws[v]).any())       # a test writes nothing but its two bits
        nxt = max(nxt, hi)

    test_until(0)
    w, w_end = 0, min(GRANT_FIRST, nW) - 1
    corrected = False
    while True:
        while w <= w_end:
            lanes, sw, a, b, dep, reach = Tb.win[w]
            bothw, lim, limt = bothws[w], t11[w], ttr[w]
            pend = np.ones(len(lanes), dtype=bool)
            if log is not None:
                log.append(w)
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
                    corrected = True
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
        # ---- the cold edge: the walk's reach is used up ----
        if w >= nW:
            break                                                 # exact whatever D says
        Dm = d_at <= moment                                       # D first ...
        Fm = F & (when <= moment)                                 # ... then F: at least as new
        assert not (Dm & ~(when <= moment)).any()
        if not look_at_flags:
            Fm = np.zeros(nW, dtype=bool)                         # the mutant
        cand = np.nonzero((~Dm | Fm)[w:])[0]
        if len(cand) == 0:
            break                                                 # nothing left: the sweep is over
        w = w + int(cand[0])
        if not Dm[w]:
            w_end = min(w + GRANT, nW) - 1                        # untested: a grant from there
        else:
            run = np.nonzero(~Fm[w:])[0]
            w_end = min(w + (int(run[0]) if len(run) else nW - w), nW) - 1
    return pos, tear, corrected, bool(F.any())


@pytest.fixture(scope="module")
def tables(lib):
    W = window_table(lib, 25)
    return W, _Tables(W)


def test_flag_walk_equals_sequential_sweep_under_any_interleaving(tables):
    W, Tb = tables
    cases = jumped = 0
    for key, pos, pin, rest, tt, g in _states():
        assert np.array_equal(g["spring_a"], W["A"]) and np.array_equal(g["spring_b"], W["B"])
        p_seq, t_seq = _sequential(pos, pin, rest, W["A"], W["B"], tt)
        moved = not np.array_equal(p_seq, pos)
        for it in range(INTERLEAVINGS):
            rng = np.random.RandomState(1000 * cases + it)
            log = []
            p_w, t_w, corrected, any_flag = _flag_walk(pos, pin, rest, Tb, tt, rng, log=log)
            assert np.array_equal(p_seq, p_w), (key, it, float(np.abs(p_seq - p_w).max()))
            assert t_seq == t_w, (key, it)
            assert (corrected or any_flag) == moved, (key, it)     # "sweeps run" counts what the barriered order counts
            assert log == sorted(set(log))                         # every window at most once, ascending
            jumped += 1 if len(log) < Tb.nW and (np.diff(log) > 1).any() else 0
        cases += 1
    assert cases >= 20 and jumped > 100                            # the jump is exercised, not only the grants


def test_a_walk_that_jumps_without_looking_at_the_flags_is_caught(tables):
    """The model of mutant 5 (csrc: CLOTHHIP_MUTATE == 5): the walk jumps over a tested window without looking at its F bit. The states above
    tell it from the sequential loop -- so the comparison above does pin the rule."""
    W, Tb = tables
    wrong = 0
    for n_case, (key, pos, pin, rest, tt, g) in enumerate(_states()):
        p_seq, _ = _sequential(pos, pin, rest, W["A"], W["B"], tt)
        p_w = _flag_walk(pos, pin, rest, Tb, tt, np.random.RandomState(n_case), look_at_flags=False)[0]
        wrong += 0 if np.array_equal(p_seq, p_w) else 1
    assert wrong >= 1
