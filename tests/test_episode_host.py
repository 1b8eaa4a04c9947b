"""CPU tests of the host side of an episode launch (ClothVecEnv.step_many), stage by stage, without a device: the chain of pre-drawn
reset scripts and the MT19937 hand-over (gym_cloth_amd/reset_streams.py), the accounting of a launch's records, and the order of the
argument checks. Expected values come from numpy's RandomState and from the sequential semantics written out here."""
import copy

import numpy as np
import pytest

from gym_cloth_amd import _lib, reset_streams
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.envs import Box, ClothVecEnv, compute_terminal


class _NoDevice(object):
    """Stands where an env's ClothBatch would: whatever is asked of it, the test fails."""

    def __getattr__(self, name):
        raise AssertionError("the host stage reached for batch.%s" % name)


# ---- reset scripts ------------------------------------------------------------------------------------------------------------
def _minabs(ref, lo, hi, minabs=None):                         # cloth_env.py:824-832, written out again
    val = ref.uniform(low=lo, high=hi)
    while minabs is not None and abs(val) < minabs:
        val = ref.uniform(low=lo, high=hi)
    return val


def _ref_domrand(ref):                                         # cloth_env.py:786-789
    ref.uniform(low=40, high=50)
    ref.uniform(low=0.7, high=1.3)
    lim = ref.uniform(low=-15.0, high=15.0)
    ref.uniform(low=-lim, high=lim, size=(224, 224, 3))


def _ref_tier1_pulls(ref, n):
    return [(ref.randint(625), _minabs(ref, -0.2, 0.2, 0.08), _minabs(ref, -0.2, 0.2, 0.08)) for _ in range(n)]


def _same_stream(rng, ref):
    a, b = rng.get_state(), ref.get_state()
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _script_env(tier, domrand, E=3):
    v = ClothVecEnv.__new__(ClothVecEnv)                       # host-only pieces: no device needed
    v.E, v.P, v._init_type, v._consume_domrand, v.iters_up, v._wd, v._hd = E, 625, tier, domrand, 50, 224, 224
    v.np_randoms = [np.random.RandomState(40 + e) for e in range(E)]
    v._pending = [None] * E
    v.batch = _NoDevice()
    return v


@pytest.mark.parametrize("domrand", [False, True])
def test_chain_commit_not_forked_keeps_the_tail(domrand):
    """Four scripts drawn, two consumed with their two unconditional pulls: the RandomState stands after two resets' draws and the
    next launch gets the former scripts 2 and 3."""
    v = _script_env("tier1", domrand)
    sc = v._prepare_scripts(4)
    for e in range(3):
        v._pending[e].commit(v.np_randoms[e], 2, 2)
        ref = np.random.RandomState(40 + e)
        for s in range(2):
            ref.rand()                                         # init_side
            pulls = _ref_tier1_pulls(ref, 2)
            for k, (pt, dx, dy) in enumerate(pulls):
                assert (sc[e, s]["pull"][k]["point"], sc[e, s]["pull"][k]["dx"], sc[e, s]["pull"][k]["dy"]) == (pt, dx, dy)
            if domrand:
                _ref_domrand(ref)
        assert _same_stream(v.np_randoms[e], ref), e
        assert len(v._pending[e].nodes) == 2
    nxt = v._prepare_scripts(2)
    assert nxt.tobytes() == np.ascontiguousarray(sc[:, 2:4]).tobytes()


@pytest.mark.parametrize("domrand", [False, True])
def test_chain_commit_forked_voids_the_chain(domrand):
    """... the second of them with its coverage-conditional third pull: the stream forked there, the chain is void and the next
    script is drawn fresh from the state after three pulls."""
    v = _script_env("tier1", domrand)
    sc = v._prepare_scripts(4)
    for e in range(3):
        v._pending[e].commit(v.np_randoms[e], 2, 3)
        ref = np.random.RandomState(40 + e)
        ref.rand(); _ref_tier1_pulls(ref, 2)
        if domrand:
            _ref_domrand(ref)
        ref.rand()
        third = _ref_tier1_pulls(ref, 3)[2]
        assert (sc[e, 1]["pull"][2]["point"], sc[e, 1]["pull"][2]["dx"], sc[e, 1]["pull"][2]["dy"]) == third
        if domrand:
            _ref_domrand(ref)
        assert _same_stream(v.np_randoms[e], ref), e
        assert len(v._pending[e].nodes) == 0 and len(v._pending[e].recs) == 0
    fresh = v._prepare_scripts(1)
    for e in range(3):
        ref = np.random.RandomState(40 + e)
        ref.rand(); _ref_tier1_pulls(ref, 2)
        if domrand:
            _ref_domrand(ref)
        ref.rand(); _ref_tier1_pulls(ref, 3)
        if domrand:
            _ref_domrand(ref)
        assert _same_stream(v.np_randoms[e], ref)              # parked where the fresh script starts
        side = ref.rand() > 0.5
        for k, (pt, dx, dy) in enumerate(_ref_tier1_pulls(ref, 3)):
            assert (fresh[e, 0]["pull"][k]["point"], fresh[e, 0]["pull"][k]["dx"], fresh[e, 0]["pull"][k]["dy"]) == (pt, dx, dy)
        assert v._script_sides[e, 0] == side


@pytest.mark.parametrize("n_drawn", [1, 2])
def test_chain_commit_tier3(n_drawn):
    """Tier 3 has no conditional pull: both `after` states of a node coincide, and a commit leaves the stream after the script's
    draws (cloth.pyx:75, then iters_up, x, y, dx, dy of cloth_env.py:959-972), with the chain exhausted or not."""
    v = _script_env("tier3", False, E=2)
    sc = v._prepare_scripts(n_drawn)
    for e in range(2):
        chain = v._pending[e]
        for node in chain.nodes:
            assert node.after[0][0] == node.after[1][0] and np.array_equal(node.after[0][1], node.after[1][1])
            assert node.after[0][2:] == node.after[1][2:]
        chain.commit(v.np_randoms[e], 1, 1)
        ref = np.random.RandomState(40 + e)
        ref.rand()
        want = (ref.uniform(low=200, high=280), _minabs(ref, 0.30, 0.70), _minabs(ref, 0.30, 0.70),
                _minabs(ref, -0.25, 0.25, 0.10), _minabs(ref, -0.25, 0.25, 0.10))
        pl = sc[e, 0]["pull"][0]
        assert (pl["iters_up"], pl["x"], pl["y"], pl["dx"], pl["dy"]) == want
        assert _same_stream(v.np_randoms[e], ref)
        assert len(chain.nodes) == n_drawn - 1


# ---- the MT19937 hand-over ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_mt_hand_over_round_trip(fast, monkeypatch):
    """export_mt then import_mt: unchanged rows leave every RandomState as it was, cached gaussian included; a changed row makes
    that env continue like the stream the row is the image of, and only that env. On numpy's state memory and through
    get_state() / set_state()."""
    if fast:
        assert reset_streams._mt_state_address(np.random.RandomState(0)) is not None
    else:
        monkeypatch.setattr(reset_streams, "_mt_state_address", lambda rng: None)
    rngs = [np.random.RandomState(7 + e) for e in range(3)]
    for r in rngs:
        r.rand(11)
        r.normal()                                             # leaves has_gauss = 1 and a cached gaussian behind
    before = [r.get_state() for r in rngs]
    assert all(st[3] == 1 for st in before)

    def unchanged(e):
        st = rngs[e].get_state()
        return st[0] == before[e][0] and np.array_equal(st[1], before[e][1]) and st[2:] == before[e][2:]
    mt, token = reset_streams.export_mt(rngs)
    assert mt.shape == (3, _lib.MT_WORDS) and mt.dtype == np.uint32
    for e in range(3):
        assert np.array_equal(mt[e, :624], before[e][1]) and mt[e, 624] == before[e][2]
    reset_streams.import_mt(rngs, mt, mt.copy(), token)
    assert all(unchanged(e) for e in range(3))
    twin = np.random.RandomState()
    twin.set_state(before[1])
    twin.rand(700)
    mt_before = mt.copy()
    mt[1, :624], mt[1, 624] = twin.get_state()[1], twin.get_state()[2]
    reset_streams.import_mt(rngs, mt, mt_before, token)
    assert unchanged(0) and unchanged(2)
    assert rngs[1].get_state()[3:] == before[1][3:]            # the cached gaussian stays
    assert np.array_equal(rngs[1].randint(0, 2 ** 32, size=1500, dtype=np.uint64), twin.randint(0, 2 ** 32, size=1500, dtype=np.uint64))
    assert _same_stream(rngs[1], twin)


# ---- accounting ---------------------------------------------------------------------------------------------------------------
def bare_accounting_env(E, P=625, reward_type="coverage", max_actions=3, clip_act_space=True):
    """A ClothVecEnv's host arrays and nothing else: what the accounting stage of step_many works on. Its batch refuses every access."""
    v = ClothVecEnv.__new__(ClothVecEnv)
    v.E, v.P, v.num_points, v.reward_type, v.max_actions, v._clip_act_space = E, P, P, reward_type, max_actions, clip_act_space
    v.action_space = Box([-1., -1., -1., -1.], [1., 1., 1., 1.])
    v._neg_living_rew, v._nogrip_penalty, v._tear_penalty, v._oob_penalty = 0.0, -0.01, 0.0, 0.0
    v._cover_success, v._act_bound_factor, v._act_pen_limit = 5., 1.0, 3.0
    for k in ClothVecEnv._SNAP_ARRAYS:
        v.__dict__[k] = np.zeros(E, dtype={"have_tear": bool, "init_side": bool, "_ep_done": bool}.get(
            k, np.int64 if k.startswith(("num_", "last_")) else np.float64))
    v.total_substeps = 0
    v.batch = _NoDevice()
    return v


T_, E_, R_ = 5, 4, 2
# The launch, written out slot by slot (max_actions = 3). Env 0 never runs. Env 1 enters with its episode over: reset 1, an action that
# tears (done), reset 2, an action that grabs nothing, two more actions, the second its third (done by max_actions); it has no
# reset left and idles. Env 2 enters at num_steps 1: out of bounds (done), reset 1, three actions (done by max_actions), and the time
# slice ends right after its reset 2 (a tail reset). Env 3 enters at num_steps 2: one action (done by max_actions), then the slice cuts
# its reset in the middle (consumed == 2: the device has zeroed its counters, the host has not heard of the reset).
_RAN = np.array([[0, 1, 1, 1], [0, 1, 1, 0], [0, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]], dtype=np.uint8)
_RESET_BEFORE = np.array([[0, 1, 0, 0], [0, 2, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.uint8)
_TEAR = np.array([[0, 1, 0, 0]] + [[0, 0, 0, 0]] * 4, dtype=np.uint8)
_OOB = np.array([[0, 0, 1, 0]] + [[0, 0, 0, 0]] * 4, dtype=np.uint8)
_GRABBED = np.array([[0, 3, 2, 4], [0, 0, 5, 0], [0, 1, 1, 0], [0, 2, 6, 0], [0, 0, 0, 0]], dtype=np.int32)
_DONE = np.array([[0, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0]], dtype=np.uint8)
_NUM_STEPS0 = np.array([1, 3, 1, 2])
_EP_DONE0 = np.array([False, True, False, False])
# num_steps / have_tear / episode-over as the host holds them after each slot, by the sequential semantics
_NUM_STEPS = np.array([[1, 1, 2, 3], [1, 1, 1, 3], [1, 2, 2, 3], [1, 3, 3, 3], [1, 3, 3, 3]])
_HAVE_TEAR = np.array([[0, 1, 0, 0]] + [[0, 0, 0, 0]] * 4, dtype=bool)
_EP_DONE = np.array([[0, 1, 1, 1], [0, 0, 0, 1], [0, 0, 0, 1], [0, 1, 1, 1], [0, 1, 1, 1]], dtype=bool)
# ... and as the device reports them when the launch ends: env 2's tail reset and env 3's cut reset have zeroed theirs
_NSTEPS_END, _DONE_END = np.array([1, 3, 0, 0], dtype=np.int32), np.array([0, 1, 0, 0], dtype=np.uint8)


def _records():
    g = np.random.RandomState(5)
    rec = np.zeros((T_, E_), dtype=_lib.STEP_RECORD_DTYPE)
    rec["ran"], rec["reset_before"], rec["tear"], rec["oob"], rec["n_grabbed"], rec["done"] = _RAN, _RESET_BEFORE, _TEAR, _OOB, _GRABBED, _DONE
    rec["action"] = g.uniform(-1, 1, size=(T_, E_, 4))
    rec["coverage"] = g.uniform(0.3, 0.9, size=(T_, E_))          # below the 0.92 that ends an episode
    rec["variance_inv"] = g.uniform(1, 9, size=(T_, E_))
    rec["executed"] = np.where(_GRABBED > 0, g.randint(100, 400, size=(T_, E_)), 0)
    rec["iters_pull"] = g.randint(1, 90, size=(T_, E_))
    rec["n_below_half_thickness"] = g.randint(0, 625, size=(T_, E_))
    rst = np.zeros((E_, R_), dtype=_lib.RESET_RECORD_DTYPE)
    rst["consumed"] = [[0, 0], [1, 1], [1, 1], [2, 0]]
    done_ = rst["consumed"] == 1
    rst["pulls_run"] = np.where(done_, 2, 0)
    rst["executed"] = np.where(done_[:, :, None], g.randint(50, 300, size=(E_, R_, 3)), 0)
    rst["settle_executed"] = np.where(done_, g.randint(0, 800, size=(E_, R_)), 0)
    rst["init_side"] = np.where(done_, g.randint(0, 2, size=(E_, R_)), 0)
    rst["start_coverage"] = np.where(done_, g.uniform(0.3, 0.8, size=(E_, R_)), 0.0)
    rst["start_variance_inv"] = np.where(done_, g.uniform(1, 9, size=(E_, R_)), 0.0)
    return rec, rst


def _launch_env():
    g = np.random.RandomState(6)
    v = bare_accounting_env(E_)
    v.num_steps[:], v._ep_done[:] = _NUM_STEPS0, _EP_DONE0
    v.num_sim_steps[:] = g.randint(0, 900, size=E_)
    v._prev_reward[:] = v._start_coverage[:] = g.uniform(0.3, 0.8, size=E_)
    v._start_variance_inv[:], v._current_coverage[:] = g.uniform(1, 9, size=E_), g.uniform(0.3, 0.8, size=E_)
    v.init_side[:] = [True, False, True, False]
    return v


_OP = (np.zeros((E_, 4), dtype=np.uint64), np.zeros((E_, 4), dtype=np.uint64))


def test_accounting_records_cover_every_case():
    rec, rst = _records()
    ran, rb = rec["ran"] == 1, rec["reset_before"]
    assert (~ran[:, 0]).all()                                                        # an env that never runs
    assert list(rb[:, 1][rb[:, 1] > 0]) == [1, 2]                                    # reset 1 then reset 2
    over = _NUM_STEPS >= 3
    assert (ran & over & (rec["tear"] == 0) & (rec["oob"] == 0) & (rec["done"] == 1)).any()      # ended by max_actions
    assert (ran & ~over & (rec["oob"] == 1) & (rec["done"] == 1)).any()              # ended out of bounds
    assert (ran & ~over & (rec["tear"] == 1) & (rec["done"] == 1)).any()             # ended by a tear
    assert (ran & (rec["n_grabbed"] == 0)).any()                                     # a slot that grabbed nothing
    assert ((rst["consumed"] == 1).sum(axis=1) > rb.max(axis=0)).any()               # a tail reset
    assert (rst["consumed"] == 2).any()                                              # a cut reset
    for t in range(T_):                                                              # the done bytes are _terminal's
        want = compute_terminal("coverage", 3, _NUM_STEPS[t], _HAVE_TEAR[t], rec["oob"][t] != 0, rec["coverage"][t], ran[t])
        assert np.array_equal(want, rec["done"][t] != 0), t


def _slot_launch(rec, rst, t):
    """Slot t as a launch of its own: its record, and the reset records that belong to it, re-indexed from 1."""
    rec_t, rst_t = rec[t:t + 1].copy(), np.zeros((E_, R_), dtype=_lib.RESET_RECORD_DTYPE)
    for e in np.nonzero(rec[t]["reset_before"])[0]:
        rst_t[e, 0] = rst[e, rec[t, e]["reset_before"] - 1]
        rec_t[0, e]["reset_before"] = 1
    if t == T_ - 1:                                               # what the slice left after the last slot: the tail and the cut reset
        rst_t[2, 0], rst_t[3, 0] = rst[2, 1], rst[3, 0]
        return rec_t, rst_t, _NSTEPS_END, _DONE_END
    return rec_t, rst_t, _NUM_STEPS[t].astype(np.int32), _EP_DONE[t].astype(np.uint8)


def test_accounting_needs_no_device_and_is_split_invariant():
    """_account_launch on a bare env whose batch refuses every access: the launch in one call, and on a twin as T launches of one
    slot each. Same `out` rows, same host arrays, same counters; and both are what the sequential semantics give."""
    rec, rst = _records()
    a, b = _launch_env(), _launch_env()
    out, n_consumed, side_t = a._account_launch(rec, rst, _NSTEPS_END, _DONE_END, True, True, _OP)
    parts, n_parts = [], np.zeros(E_, dtype=np.int64)
    for t in range(T_):
        o, n, s = b._account_launch(*_slot_launch(rec, rst, t), True, True, _OP)
        o["side_t"] = s
        parts.append(o)
        n_parts += n
    out["side_t"] = side_t
    slot_keys = [k for k in out if out[k].shape[:2] == (T_, E_)]
    assert {"rew", "done", "ran", "executed", "n_grabbed", "reset_before", "reset_substeps", "num_steps", "num_sim_steps", "have_tear",
            "out_of_bounds", "actual_coverage", "start_coverage", "variance_inv", "start_variance_inv", "actions", "side_t"} <= set(slot_keys)
    for k in slot_keys:
        whole, joined = out[k], np.concatenate([p[k] for p in parts], axis=0)
        if k == "reset_before":                                   # counts the resets of its own launch: the second of the whole
            assert np.array_equal(whole, _RESET_BEFORE)           # launch is the first of slot 1's
            whole, joined = whole > 0, joined > 0
        assert np.array_equal(whole, joined), k
    assert np.array_equal(out["tail_reset_substeps"], parts[-1]["tail_reset_substeps"])
    assert all("tail_reset_substeps" not in p for p in parts[:-1])
    for k in ClothVecEnv._SNAP_ARRAYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.total_substeps == b.total_substeps and np.array_equal(n_consumed, n_parts)
    # ... and the sequential semantics
    ran = _RAN == 1
    assert np.array_equal(n_consumed, [0, 2, 2, 0]) and np.array_equal(out["tail_reset_index"], [0, 0, 2, 0])
    assert np.array_equal(out["ran"], ran) and np.array_equal(out["done"], _DONE != 0)
    assert np.array_equal(out["num_steps"], _NUM_STEPS) and np.array_equal(out["have_tear"], _HAVE_TEAR)
    assert np.array_equal(a.num_steps, [1, 3, 0, 3]) and np.array_equal(a._ep_done, [False, True, False, True])
    assert np.array_equal(out["rew"], np.where(ran, rec["coverage"] + np.where(_GRABBED == 0, -0.01, 0.0), 0.0))
    resets = rst["executed"].sum(axis=2) + rst["settle_executed"]
    assert a.total_substeps == int(rec["executed"][ran].sum() + resets[rst["consumed"] == 1].sum())
    assert np.array_equal(out["reset_substeps"][1], [0, resets[1, 1], resets[2, 0], 0]) and out["tail_reset_substeps"][2] == resets[2, 1]
    assert np.array_equal(a.init_side, [True, rst["init_side"][1, 1] != 0, rst["init_side"][2, 1] != 0, False])
    assert np.array_equal(a._start_coverage[1:3], [rst["start_coverage"][1, 1], rst["start_coverage"][2, 1]])
    assert np.array_equal(a._current_coverage[1:], [rec["coverage"][3, 1], 0.0, rec["coverage"][0, 3]])


def test_accounting_raises_where_device_and_host_disagree_on_done():
    rec, rst = _records()
    rec["done"][2, 1] ^= 1
    with pytest.raises(RuntimeError, match="terminal test"):
        _launch_env()._account_launch(rec, rst, _NSTEPS_END, _DONE_END, True, True, _OP)


# ---- the order of the argument checks -----------------------------------------------------------------------------------------
class _ArgumentBatch(_NoDevice):
    """What the argument checks may use of a batch: E and the expert tables' own checks."""
    _expert_tables = ClothBatch._expert_tables

    def __init__(self, E):
        self.E = E


def _bare_env(E=3):
    """tests/test_dagger_host.py's _bare_env on a batch that refuses everything else, plus the init type: the checks that follow
    batch._expert_tables decide from it whether the launch resets envs at all."""
    v = ClothVecEnv.__new__(ClothVecEnv)
    v.E, v._version, v._policy_mlp, v.num_points, v._delta_actions = E, 0, None, 625, True
    v._init_type = "tier1"
    v.batch = _ArgumentBatch(E)
    return v


def test_step_many_refuses_bad_arguments_before_it_touches_a_device():
    acts = np.zeros((2, 3, 4))
    for kw in (dict(actions=acts, policy_noise=np.zeros((2, 3, 4))),                             # noise without the network policy
               dict(policy="mlp", n_actions=2),                                                  # ... which needs a network
               dict(actions=acts, images="png"),
               dict(actions=acts, max_resets=0, auto_reset=True),
               dict(actions=acts, max_resets=256, auto_reset=True),
               dict(actions=acts, policy="harris"),
               dict(actions=acts, expert="harris"),                                              # (the expert checks, on this batch)
               dict(actions=acts, expert="oracle_corner", expert_mix=np.zeros((3, 3), dtype=bool))):
        with pytest.raises(ValueError):
            _bare_env().step_many(**kw)
    v = _bare_env()
    v._policy_mlp = object()
    for kw in (dict(actions=acts, policy="mlp", n_actions=2),                                    # the network gives the actions
               dict(policy="mlp", n_actions=2, policy_noise=np.zeros((2, 2, 4)))):
        with pytest.raises(ValueError):
            v.step_many(**kw)
    a = _bare_env()._parse_launch(acts, None, None, False, False, None, 0, 0.0, True, None, "rgbd", None, None, None, None, None)
    assert (a.pol, a.T, a.R, a.dev_reset, a.use_rng, a.want_obs) == (_lib.POLICY_TABLE, 2, 0, False, False, True)   # no resets: any R
