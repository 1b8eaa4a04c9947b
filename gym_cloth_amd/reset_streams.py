"""Where an env's reset draws come from: the draw order of the reference's resets as plain functions of a numpy RandomState
(cloth.pyx:75; cloth_env.py:786-789, :824-840, :851-877, :959-978), one env's chain of resets pre-drawn for an episode launch
(ScriptChain, step_many(device_rng=False)), and the hand-over of every env's MT19937 stream to the device and back (export_mt /
import_mt, device_rng=True). Nothing here touches a device."""
import collections
import ctypes

import numpy as np

from ._lib import MT_WORDS, RESET_SCRIPT_DTYPE


def randval_minabs(rng, low, high, minabs=None):                      # cloth_env.py:824-832
    val = rng.uniform(low=low, high=high)
    if minabs is not None:
        assert minabs > 0, minabs
        assert low < -minabs or high > minabs
        while np.abs(val) < minabs:
            val = rng.uniform(low=low, high=high)
    return val


def prevent_oob(val, dval, lower=0.0, upper=1.0):                     # cloth_env.py:834-840
    if val + dval < lower:
        dval = lower - val
    elif val + dval > upper:
        dval = upper - val
    return dval


def domrand_draws(rng, wd, hd):
    """cloth_env.py:786-789: the draws every reset makes after the scripted actions."""
    rng.uniform(low=40, high=50)
    rng.uniform(low=0.7, high=1.3)
    lim = rng.uniform(low=-15.0, high=15.0)
    rng.uniform(low=-lim, high=lim, size=(wd, hd, 3))


def draw_script(rng, tier, out, P, iters_up):
    """Draw ONE reset from `rng` in the reference's order (cloth.pyx:75; cloth_env.py:851-877 / :959-978) into the
    script record `out`. Returns (init_side, rng state if the reset runs 2 pulls, rng state if it runs 3 (tier 1))."""
    init_side = bool(rng.rand() > 0.5)                                               # cloth.pyx:75
    out['valid'], out['_pad'] = 1, 0
    if tier == 1:
        lim = 0.20
        out['n_pulls'], out['settle_after'] = 3, 0
        s2 = None
        for k in range(3):
            if k == 2:
                s2 = rng.get_state()                          # the third pull's draws happen only if coverage >= 0.90
            pl = out['pull'][k]
            pl['point'] = rng.randint(P)
            pl['dx'] = randval_minabs(rng, -lim, lim, 0.08)
            pl['dy'] = randval_minabs(rng, -lim, lim, 0.08)
            pl['x'] = pl['y'] = 0.0
            pl['need_coverage'], pl['coverage_min'] = int(k == 2), 0.90
            pl['iters_up'] = float(iters_up)
        return init_side, s2, rng.get_state()
    assert tier == 3, tier                                                           # tier 2 is drawn on the device only
    lim = 0.25
    out['n_pulls'], out['settle_after'] = 1, 800
    pl = out['pull'][0]
    pl['iters_up'] = rng.uniform(low=200, high=280)
    pl['x'] = randval_minabs(rng, 0.30, 0.70)
    pl['y'] = randval_minabs(rng, 0.30, 0.70)
    pl['dx'] = randval_minabs(rng, -lim, lim, 0.10)
    pl['dy'] = randval_minabs(rng, -lim, lim, 0.10)
    pl['point'], pl['need_coverage'], pl['coverage_min'] = -1, 0, 0.0
    st = rng.get_state()
    return init_side, st, st


# `before`: the stream where the script's draws start; `after`: (state after the unconditional pulls, state after all pulls)
ScriptNode = collections.namedtuple('ScriptNode', 'before after')


class ScriptChain(object):
    """One env's next resets, pre-drawn: nodes[k] / recs[k] (RESET_SCRIPT_DTYPE) / sides[k] (Cloth.init_side, cloth.pyx:75) of the
    k-th. Script k+1 is drawn from the state script k leaves when only its unconditional pulls run (tier 1: two pulls; the third,
    coverage-conditional one draws further numbers and forks the stream, cloth_env.py:866-877), after the domain-randomisation draws
    where `domrand` = (wd, hd) is given. The env's RandomState stays parked where script 0 starts, so a host-side reset() simply
    re-draws and dropping the chain gives every draw back."""

    def __init__(self, tier, P, iters_up, domrand=None):
        self.tier, self.P, self.iters_up, self.domrand = tier, P, iters_up, domrand
        self._void()

    def _void(self):
        self.nodes, self.recs, self.sides = [], np.zeros(0, dtype=RESET_SCRIPT_DTYPE), np.zeros(0, dtype=bool)

    def _after_reset(self, rng):
        if self.domrand is not None:
            domrand_draws(rng, *self.domrand)

    def extend(self, rng, n):
        """Make the chain at least n scripts long; `rng` is left where it was."""
        k0 = len(self.nodes)
        if k0 >= n:
            return
        s_start = rng.get_state()
        if k0:
            rng.set_state(self.nodes[-1].after[0])
            self._after_reset(rng)
        recs = np.zeros(n, dtype=RESET_SCRIPT_DTYPE)
        sides = np.zeros(n, dtype=bool)
        recs[:k0], sides[:k0] = self.recs, self.sides
        for k in range(k0, n):
            before = rng.get_state()
            sides[k], s2, s3 = draw_script(rng, self.tier, recs[k], self.P, self.iters_up)
            self.nodes.append(ScriptNode(before, (s2, s3)))
            rng.set_state(s2)                                     # the chain continues as if only the unconditional pulls ran
            self._after_reset(rng)
        self.recs, self.sides = recs, sides
        rng.set_state(s_start)

    def take(self, R):
        """(records, sides) of the first R scripts, as a launch takes them."""
        return self.recs[:R], self.sides[:R]

    def commit(self, rng, n_consumed, pulls_run_of_last):
        """A launch ran the first n_consumed >= 1 scripts, the last of them with that many pulls: move `rng` past them. Where the
        conditional pull ran the stream forked and the later scripts are void; so they are when none is left. Otherwise the rest of
        the chain stays and `rng` parks where its first script starts."""
        c = int(n_consumed)
        last = self.recs[c - 1]
        n_uncond = int((last['pull']['need_coverage'][:int(last['n_pulls'])] == 0).sum())
        forked = int(pulls_run_of_last) > n_uncond
        if forked or c >= len(self.nodes):
            rng.set_state(self.nodes[c - 1].after[1 if forked else 0])
            self._after_reset(rng)
            self._void()
        else:
            rng.set_state(self.nodes[c].before)
            self.nodes, self.recs, self.sides = self.nodes[c:], self.recs[c:], self.sides[c:]


def _mt_state_address(rng):
    """Address of numpy's `mt19937_state { uint32 key[624]; int pos; }` behind a RandomState (its MT19937 bit generator exports
    it for exactly this kind of access), or None: then get_state() / set_state() are used. Copying 2 500 bytes per env this way
    instead of building state tuples takes the per-launch RNG hand-over of 512 envs from ~30 ms to ~1 ms."""
    try:
        bg = rng._bit_generator
        if type(bg).__name__ != 'MT19937':
            return None
        return int(bg.ctypes.state_address)
    except Exception:
        return None


def export_mt(np_randoms):
    """Every env's numpy stream as RandomState.get_state() has it: (mt uint32[E, MT_WORDS] = key[624], pos, pad per row; token for
    import_mt)."""
    E = len(np_randoms)
    mt = np.zeros((E, MT_WORDS), dtype=np.uint32)
    addr, gauss = [_mt_state_address(r) for r in np_randoms], [None] * E
    row0, row_bytes = mt.ctypes.data, mt.strides[0]
    for e in range(E):
        if addr[e]:                                               # key[624] + pos, straight out of numpy's generator state
            ctypes.memmove(row0 + e * row_bytes, addr[e], 625 * 4)
        else:
            st = np_randoms[e].get_state()
            mt[e, :624], mt[e, 624], gauss[e] = st[1], st[2], st[3:]
    return mt, (addr, gauss)


def import_mt(np_randoms, mt, mt_before, token):
    """The streams as the device left them in `mt`: only the rows that differ from mt_before are written back (the cached
    gaussian of RandomState is not the device's business and stays)."""
    addr, gauss = token
    row0, row_bytes = mt.ctypes.data, mt.strides[0]
    for e in np.nonzero((mt != mt_before).any(axis=1))[0]:
        if addr[e]:
            ctypes.memmove(addr[e], row0 + int(e) * row_bytes, 625 * 4)
        else:
            np_randoms[e].set_state(('MT19937', mt[e, :624], int(mt[e, 624])) + tuple(gauss[e]))
