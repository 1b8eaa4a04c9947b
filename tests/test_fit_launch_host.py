"""CPU tests of the dataset rows named by where they lie on the device (clothhip_fit_hold, clothhip_fit_data_append_launch):
envs.slot_start_sources is slot_start_obs stated as indices; envs.hold_sources carries the rule across launches, however a synthetic
episode is cut; the new entries are declared, exported and bound with the header's signatures; the wrappers refuse before any library
call. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.envs import hold_sources, slot_start_obs, slot_start_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["clothhip_fit_hold", "clothhip_fit_data_append_launch", "clothhip_fit_data_get", "clothhip_policy_fit_loss"]
T, E, R, W = 4, 6, 3, 9                     # slots, envs, reset capacity, floats per row (3P of a 3-point cloth)
SLOTS, RESETS, HELD = _lib.FIT_SRC_SLOTS, _lib.FIT_SRC_RESETS, _lib.FIT_SRC_HELD

# reset_before of the unsplit launch: env 1 resets before slot 2, env 2 twice (before slots 1 and 3), env 4 before slot 0, env 5 before slot 3
RB = np.zeros((T, E), dtype=np.int64)
RB[2, 1] = 1
RB[1, 2], RB[3, 2] = 1, 2
RB[0, 4] = 1
RB[3, 5] = 1


def _whole(seed=5):
    """The unsplit launch: every slot ran; every row a different random vector."""
    r = np.random.RandomState(seed)
    out = {'obs_t': r.normal(size=(T, E, W)).astype(np.float32), 'reset_obs': r.normal(size=(E, R, W)).astype(np.float32),
           'reset_before': RB.copy(), 'ran': np.ones((T, E), dtype=bool), 'n_resets': RB.max(axis=0)}
    return out, r.normal(size=(E, W)).astype(np.float32)


def _gather(src, out, held):
    """What k_fit_gather reads for the (source, row) pairs src[..., 2]: numpy tables in the device's layout."""
    tables = {SLOTS: out['obs_t'].reshape(-1, W), RESETS: out['reset_obs'].reshape(-1, W), HELD: held}
    flat = src.reshape(-1, 2)
    rows = np.stack([tables[int(s)][int(k)] for s, k in flat])
    return rows.reshape(src.shape[:-1] + (W,))


def test_sources_are_slot_start_obs_as_indices():
    out, before = _whole()
    src = slot_start_sources(out, True)
    assert src.dtype == np.int32 and src.shape == (T, E, 2)
    assert np.array_equal(_gather(src, out, before), slot_start_obs(out, before))
    # all three classes occur, each where the rule says
    assert np.array_equal(src[..., 0] == RESETS, RB > 0) and (src[0, RB[0] == 0, 0] == HELD).all() and (src[1:][RB[1:] == 0][:, 0] == SLOTS).all()
    assert src[3, 2].tolist() == [RESETS, 2 * R + 1] and src[0, 3].tolist() == [HELD, 3] and src[2, 0].tolist() == [SLOTS, 1 * E + 0]
    # without the table itself the capacity comes from the key a want_obs='device' launch carries
    dev = {k: v for k, v in out.items() if k not in ('obs_t', 'reset_obs')}
    dev['reset_capacity'] = R
    assert np.array_equal(slot_start_sources(dev), src)
    # an env without a held row has no source for slot 0 (the library refuses -1), unless a reset precedes the slot
    none = slot_start_sources(out, False)
    assert (none[0, RB[0] == 0] == -1).all() and np.array_equal(none[0, 4], src[0, 4]) and np.array_equal(none[1:], src[1:])
    some = slot_start_sources(out, np.arange(E) != 3)
    assert (some[0, 3] == -1).all() and np.array_equal(np.delete(some, 3, axis=1), np.delete(src, 3, axis=1))


def _split(whole, cuts):
    """The unsplit launch cut into len(cuts) + 1 launches. A cut (t, after_reset) ends a launch in front of slot t -- with after_reset
    behind the reset that precedes slot t, where there is one (a time slice that ended right after a reset: consumed, no record carries
    it). Each launch numbers its slots and resets anew and fills its own tables, as the device does."""
    launches = []
    for j in range(len(cuts) + 1):
        launches.append({'obs_t': np.full((T, E, W), np.nan, dtype=np.float32), 'reset_obs': np.full((E, R, W), np.nan, dtype=np.float32),
                         'reset_before': np.zeros((T, E), dtype=np.int64), 'ran': np.zeros((T, E), dtype=bool),
                         'n_resets': np.zeros(E, dtype=np.int64)})
    for e in range(E):
        slot = [0] * len(launches)
        pending = [0] * len(launches)
        for t in range(T):
            ja = sum(1 for tc, _ in cuts if t >= tc)                              # the launch of the action
            jr = sum(1 for tc, after in cuts if t > tc or (t == tc and not after))   # ... and of the reset in front of it
            if RB[t, e]:
                L = launches[jr]
                L['n_resets'][e] += 1
                L['reset_obs'][e, L['n_resets'][e] - 1] = whole['reset_obs'][e, RB[t, e] - 1]
                pending[jr] = L['n_resets'][e]
            L = launches[ja]
            s = slot[ja]
            slot[ja] += 1
            L['ran'][s, e] = True
            L['obs_t'][s, e] = whole['obs_t'][t, e]
            L['reset_before'][s, e] = pending[ja]                                 # (0 when the reset was consumed by the launch before)
            pending[ja] = 0
    return launches


def _collect(launches, before):
    """dagger_collect's loop on numpy tables: per launch the rows that ran, gathered by slot_start_sources, then the hold-over."""
    held = before.copy()
    rows = [[] for _ in range(E)]
    for L in launches:
        src = slot_start_sources(L, True)
        got = _gather(src, L, held)
        for t, e in zip(*np.nonzero(L['ran'])):
            rows[e].append(got[t, e])
        hs = hold_sources(L)
        assert hs.dtype == np.int32 and hs.shape == (E, 2)
        held = _gather(hs, L, held)
    return rows


ALL_CUTS = [(t, False) for t in range(1, T)] + [(t, True) for t in range(T) if RB[t].any()]


@pytest.mark.parametrize("cuts", [[(t, False) for t in range(1, T)],             # at every slot boundary: one slot per launch
                                  [(t, True) for t in range(T)],                 # right after every reset (and at plain boundaries elsewhere)
                                  [(0, False)], [(T, False)]]                    # an empty launch in front, one behind
                         + [[c] for c in ALL_CUTS]
                         + [[(1, True), (3, True)], [(2, True), (3, False)], [(3, False), (3, True)]])
def test_hold_over_carries_the_rule_across_launches(cuts):
    whole, before = _whole()
    want = slot_start_obs(whole, before)
    cuts = sorted(cuts)
    launches = _split(whole, cuts)
    assert sum(int(L['ran'].sum()) for L in launches) == T * E
    rows = _collect(launches, before)
    for e in range(E):
        assert len(rows[e]) == T
        for t in range(T):
            assert rows[e][t].tobytes() == want[t, e].tobytes(), (cuts, e, t)


def test_the_split_makes_the_cases_it_is_meant_to():
    """The cut right after a reset leaves a consumed reset no record carries; hold_sources then names its row, else the last slot's, else
    the held row."""
    whole, _ = _whole()
    A, B = _split(whole, [(2, True)])
    assert A['n_resets'][1] == 1 and A['reset_before'][:, 1].max() == 0 and B['reset_before'][0, 1] == 0 and B['n_resets'][1] == 0
    assert A['n_resets'][2] == 1 and A['reset_before'][1, 2] == 1                # env 2's first reset has its record in A
    hs = hold_sources(A)
    assert hs[1].tolist() == [RESETS, 1 * R + 0] and hs[2].tolist() == [SLOTS, 1 * E + 2] and hs[0].tolist() == [SLOTS, 1 * E + 0]
    empty, _ = _split(whole, [(0, False)])
    assert np.array_equal(hold_sources(empty), np.stack([np.full(E, HELD), np.arange(E)], axis=1))
    first, _ = _split(whole, [(0, True)])                                        # only env 4's reset ran
    assert hold_sources(first)[4].tolist() == [RESETS, 4 * R + 0] and (np.delete(hold_sources(first), 4, axis=0)[:, 0] == HELD).all()


_CTYPES = {"clothhip_handle *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int64_t": C.c_int64, "float *": C.POINTER(C.c_float),
           "double *": C.POINTER(C.c_double)}


def test_symbols_declared_exported_bound_with_the_headers_signatures():
    hdr = open(os.path.join(ROOT, "include", "clothhip.h")).read()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    L = _lib.load()
    for name in NEW:
        m = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        types = [re.sub(r"\s*\w+$", "", p.strip()).strip() for p in m.group(1).split(",")]
        assert name in bound and bound[name][0] is C.c_int, name
        assert bound[name][1] == [_CTYPES[t] for t in types], (name, types)
        assert getattr(L, name) is not None
    assert re.search(r"CLOTHHIP_FIT_SRC_SLOTS = 0, CLOTHHIP_FIT_SRC_RESETS = 1, CLOTHHIP_FIT_SRC_HELD = 2", hdr)
    assert (SLOTS, RESETS, HELD) == (0, 1, 2)
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7                     # the change is additive
    assert L.clothhip_fit_hold(None, None) == _lib.EINVAL                        # NULL handle: a status, no device touched
    assert L.clothhip_fit_data_append_launch(None, None, 0) == _lib.EINVAL
    assert L.clothhip_fit_data_get(None, 0, 0, None, None) == _lib.EINVAL
    assert L.clothhip_policy_fit_loss(None, None, 1, None) == _lib.EINVAL


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s) before refusing its arguments" % name)


def test_wrappers_refuse_before_any_library_call():
    b = ClothBatch.__new__(ClothBatch)
    b._L, b._h, b.P, b.E, b._mlp_n_params = _NoLibrary(), None, 3, E, 10
    for src in [np.zeros((E, 3), dtype=int), np.zeros((E + 1, 2), dtype=int), np.zeros((E, 2))]:
        with pytest.raises(ValueError):
            b.fit_hold(src)
    for rows in [np.zeros((2, 2), dtype=int), np.zeros(3, dtype=int), np.zeros((2, 3))]:
        with pytest.raises(ValueError):
            b.fit_append_launch(rows)
    for idx in [np.zeros((2, 2), dtype=int), np.zeros(0, dtype=int), np.zeros(3), np.array([0, -1])]:
        with pytest.raises(ValueError):
            b.fit_loss(idx)
    nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
    with pytest.raises(ValueError):
        b.run_actions_begin(None, 1, nsteps, done, actions=np.zeros((1, E, 4)), want_obs='host')
