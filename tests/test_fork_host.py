"""CPU tests of the host logic behind snapshot / lookahead: the reward arithmetic as a pure function (so that the branches of a lookahead
can be rewarded without touching the env) and LookaheadPolicy's candidate streams and arg-max rule. No GPU, no library load."""
import numpy as np
import pytest

from gym_cloth_amd.envs import compute_reward, compute_terminal, _REWARD_THRESHOLDS
from gym_cloth_amd.policies import LookaheadPolicy

REWARD_TYPES = ("coverage", "coverage-delta")        # what ClothEnv accepts (`assert 'coverage' in self.reward_type`, cloth_env.py:130)
CONSTS = dict(neg_living_rew=-0.05, nogrip_penalty=-0.01, tear_penalty=-10.0, oob_penalty=-3.0, cover_success=5.,
              act_bound_factor=1.5, act_pen_limit=3.0)
LOW, HIGH = np.array([-0.25, -0.25, 0.0, -np.pi]), np.array([1.25, 1.25, 1.0, np.pi])


def reference_reward(rt, clip, action, exit_early, cov, vinv, oob, have_tear, prev, height, c):
    """cloth_env.py:536-683 for ONE cloth, statement by statement: (reward, _prev_reward afterwards)."""
    rew = 0
    if have_tear:                                    # :558-563: tear OR out of bounds, never both
        rew += c["tear_penalty"]
    elif oob:
        rew += c["oob_penalty"]
    if exit_early:                                   # :564-566
        rew += c["nogrip_penalty"]

    def penalize_action(aval, low, high):            # :569-578
        if low <= aval <= high:
            return 0.0
        diff = low - aval if aval < low else aval - high
        return -min(diff ** 2, c["act_pen_limit"]) * c["act_bound_factor"]
    if not clip:                                     # :580-591 (the four penalties are summed first, as the vectorised env does)
        pens = [penalize_action(action[k], LOW[k], HIGH[k]) for k in range(4)]
        rew += ((pens[0] + pens[1]) + pens[2]) + pens[3]
    if cov > 0.92:                                   # :648-650
        rew += c["cover_success"]
    rew += c["neg_living_rew"]                       # :653
    val = {"coverage": cov, "coverage-delta": cov, "height": height, "height-delta": height, "variance": vinv,
           "variance-delta": vinv}[rt]
    if rt.endswith("-delta"):                        # :640-643
        rew += val - prev
        prev = val
    else:
        rew += val
    return rew, prev


def random_inputs(n, seed):
    r = np.random.RandomState(seed)
    d = dict(actions=r.uniform(-4.0, 4.0, size=(n, 4)),                  # well outside the action space on both sides
             exit_early=r.rand(n) < 0.3, cov=r.uniform(0.0, 1.0, n), vinv=r.uniform(0.0, 3.0, n), oob=r.rand(n) < 0.4,
             have_tear=r.rand(n) < 0.3, prev=r.uniform(0.0, 1.0, n), height=r.uniform(0.0, 1.0, n), mask=r.rand(n) < 0.8)
    d["actions"][::5] = r.uniform(0.0, 1.0, size=d["actions"][::5].shape)  # ... and inside
    d["actions"][1, 0] = LOW[0]; d["actions"][2, 3] = HIGH[3]              # on the bounds: no penalty
    d["cov"][:4] = [0.92, np.nextafter(0.92, 1), 0.95, 0.0]                # around the success threshold (strictly greater)
    return d


@pytest.mark.parametrize("rt", REWARD_TYPES + ("height", "height-delta", "variance", "variance-delta"))
@pytest.mark.parametrize("clip", [True, False])
def test_pure_reward_equals_the_reference_rules(rt, clip):
    n = 64
    d = random_inputs(n, 5)
    assert (d["have_tear"] & d["oob"]).any() and (d["exit_early"] & ~d["have_tear"]).any() and (~d["mask"]).any()
    snapshot = {k: v.copy() for k, v in d.items()}
    rew, tracked = compute_reward(rt, d["actions"], d["exit_early"], d["cov"], d["vinv"], d["oob"], d["mask"], d["have_tear"],
                                  d["prev"], height=d["height"], clip_act_space=clip, act_low=LOW, act_high=HIGH, consts=CONSTS)
    assert all(np.array_equal(d[k], snapshot[k]) for k in d), "the function must not write to its inputs"
    for e in range(n):
        want, prev_after = reference_reward(rt, clip, d["actions"][e], d["exit_early"][e], d["cov"][e], d["vinv"][e], d["oob"][e],
                                            d["have_tear"][e], d["prev"][e], d["height"][e], CONSTS)
        assert rew[e] == (want if d["mask"][e] else 0.0), (e, rew[e], want)
        if rt.endswith("-delta"):
            assert tracked[e] == prev_after
    assert (tracked is None) == (not rt.endswith("-delta"))
    if not clip:
        assert (rew[d["mask"]] < -1.0).any()                               # the action penalties were exercised


def test_pure_reward_rejects_what_the_reference_rejects():
    d = random_inputs(4, 1)
    args = (d["actions"], d["exit_early"], d["cov"], d["vinv"], d["oob"], d["mask"], d["have_tear"], d["prev"])
    with pytest.raises(NotImplementedError):
        compute_reward("folding-number", *args)
    with pytest.raises(ValueError):
        compute_reward("nonsense", *args)


def test_pure_terminal_equals_the_reference_rules():
    r = np.random.RandomState(2)
    n = 64
    steps = r.randint(0, 12, n); tear = r.rand(n) < 0.2; oob = r.rand(n) < 0.2; cov = r.uniform(0.8, 1.0, n); mask = r.rand(n) < 0.8
    cov[:2] = [0.92, np.nextafter(0.92, 1)]
    for rt in REWARD_TYPES:
        got = compute_terminal(rt, 10, steps, tear, oob, cov, mask)
        want = [bool(mask[e] and (steps[e] >= 10 or tear[e] or oob[e] or cov[e] > _REWARD_THRESHOLDS[rt])) for e in range(n)]   # :692-710
        assert got.tolist() == want


# ---- LookaheadPolicy on a stub env ------------------------------------------------------------------------------------------------------------
class StubSpace(object):
    low, high = np.array([-1.0, -1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0, 1.0])


class StubEnv(object):
    """What LookaheadPolicy touches of a ClothVecEnv: E, action_space, np_randoms (must stay untouched), lookahead."""

    def __init__(self, E, table):
        self.E, self.action_space, self.table = E, StubSpace(), np.asarray(table, dtype=np.float64)
        self.np_randoms = [np.random.RandomState(100 + e) for e in range(E)]
        self.seen = []

    def lookahead(self, actions):
        self.seen.append(np.array(actions, copy=True))
        return {"rew": self.table}


class ConstantPolicy(object):
    def get_action(self, obs, t=0):
        return np.full((3, 4), 0.125)


TABLE = [[0.0, 2.0, 2.0, 1.0],        # a tie: the lowest index (1) wins
         [3.0, 3.0, 3.0, 3.0],        # all equal: candidate 0
         [-1.0, -2.0, -0.5, -0.5]]    # a tie at the end: 2


def test_lookahead_policy_streams_are_reproducible_and_leave_the_env_streams_alone():
    envs = [StubEnv(3, TABLE) for _ in range(3)]
    before = [r.get_state()[1].copy() for r in envs[0].np_randoms]
    pols = [LookaheadPolicy(envs[0], n_candidates=4, seed=7), LookaheadPolicy(envs[1], n_candidates=4, seed=7),
            LookaheadPolicy(envs[2], n_candidates=4, seed=8)]
    acts = [[p.get_action(None, t) for t in range(3)] for p in pols]
    for t in range(3):
        assert np.array_equal(envs[0].seen[t], envs[1].seen[t]) and np.array_equal(acts[0][t], acts[1][t])
        assert not np.array_equal(envs[0].seen[t], envs[2].seen[t])
        c = envs[0].seen[t]
        assert c.shape == (3, 4, 4) and (c >= -1.0).all() and (c < 1.0).all()
    assert not np.array_equal(envs[0].seen[0], envs[0].seen[1])             # the stream advances from call to call
    assert all(np.array_equal(r.get_state()[1], s) for r, s in zip(envs[0].np_randoms, before))
    # the candidate table is the plain uniform stream of RandomState(seed)
    assert np.array_equal(envs[0].seen[0], np.random.RandomState(7).uniform(StubSpace.low, StubSpace.high, size=(3, 4, 4)))


def test_lookahead_policy_takes_the_arg_max_with_ties_to_the_lowest_index():
    env = StubEnv(3, TABLE)
    p = LookaheadPolicy(env, n_candidates=4, seed=0)
    act = p.get_action(None, 0)
    assert p.last_choice.tolist() == [1, 0, 2]
    assert np.array_equal(act, env.seen[0][np.arange(3), [1, 0, 2]])
    assert np.array_equal(p.last_candidates, env.seen[0]) and p.last_lookahead["rew"] is env.table
    assert LookaheadPolicy.choose([[1.0, 1.0], [0.0, 1.0]]).tolist() == [0, 1]


def test_lookahead_policy_include_is_candidate_zero():
    env = StubEnv(3, TABLE)
    p = LookaheadPolicy(env, n_candidates=4, seed=0, include=ConstantPolicy())
    plain = np.random.RandomState(0).uniform(StubSpace.low, StubSpace.high, size=(3, 4, 4))
    act = p.get_action(None, 0)
    assert np.array_equal(env.seen[0][:, 0], np.full((3, 4), 0.125)) and np.array_equal(env.seen[0][:, 1:], plain[:, 1:])
    assert np.array_equal(act[1], np.full(4, 0.125))                         # env 1: all equal, candidate 0 = the included proposal
    with pytest.raises(ValueError):
        LookaheadPolicy(env, n_candidates=0)
