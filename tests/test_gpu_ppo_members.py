"""GPU tests of PPO for a population (clothhip_fit_data_snapshot_policy_members, clothhip_policy_fit_ppo_grad_members,
clothhip_policy_fit_ppo_members; k_fit_scatter_y, and k_fit_loss_ppo reading member j's constants from row j of the call's table, the
kernel of the shared-network entries too, which send one row). Every comparison is array_equal or by bytes, and the twin is
always a SECOND handle that carries the member as its shared network, stores the same dataset, weights and old means and is driven by
the shared-network entries (fit_ppo_grad, fit_ppo, fit), which tests/test_gpu_ppo.py pins to the numpy restatement of the arithmetic.
Shapes and helpers are those of tests/test_gpu_ppo.py and tests/test_gpu_fit_members.py."""
import numpy as np
import pytest

from test_gpu_dagger import _layers
from test_gpu_env import base_cfg
from test_gpu_fit_members import OPTIMIZERS, _n_params, _same, _stride
from test_gpu_policy_fit import _blob, _flat, _new_batch, _random_case, _random_layers
from test_gpu_ppo import FREEZE_LR, _forward, _freeze_case, _reference_steps_to_freeze

pytestmark = pytest.mark.gpu

G, N_ROWS = 3, 40
Q = [(1.0, 0.25), (0.5, 0.1)]          # (sigma, clip) of the first and the second member of a call
_made = {}


@pytest.fixture(scope="module")
def handle():
    """which -> ONE ClothBatch of one 10x10 cloth with an empty dataset; the cases put their own networks and rows on it."""
    def get(which="pop"):
        if which not in _made:
            _made[which] = _new_batch(10)
        _made[which].fit_clear()
        return _made[which]
    yield get
    for b in _made.values():
        b.close()
    _made.clear()


def _case(widths, n_rows=N_ROWS):
    """test_gpu_ppo._gauss_case with the spread of the LARGER sigma of Q: _random_case's network and rows, actions around network 0's
    mean at standard deviation 1, old means around it at 0.3, Gaussian advantages with every fifth one 0 -- so that the ratios lie on
    both sides of both bounds under sigma = 1 and (further out) under sigma = 0.5; and G networks of one shape: network 0 and two
    neighbours of it, every weight moved by 2 % of the layer's scale. -> (nets, rows, act, old, adv)."""
    layers, rows, _, _ = _random_case(widths, 1, 4, n_rows=n_rows)
    r = np.random.RandomState(7004)
    mu = _forward(layers, rows)
    act = (mu + r.normal(size=mu.shape)).astype(np.float32)
    old = (mu + 0.3 * r.normal(size=mu.shape)).astype(np.float32)
    adv = r.normal(size=n_rows).astype(np.float32)
    adv[::5] = 0.0
    nets = [layers]
    for g in range(1, G):
        r = np.random.RandomState(80 + g)
        nets.append([((W + 0.02 * r.normal(size=W.shape) / np.sqrt(W.shape[1])).astype(np.float32),
                      (c + 0.02 * r.normal(size=c.shape) / np.sqrt(W.shape[1])).astype(np.float32)) for W, c in layers])
    return nets, rows, act, old, adv


def _population(b, nets, rows, act, adv, old=None):
    b.set_policy_population(nets, np.zeros(b.E, dtype=np.int32))
    b.fit_clear()
    b.fit_append(rows, act.astype(np.float64), weights=adv)
    if old is not None:
        b.fit_set_old_means(old)
    return b


def _twin(t, layers, rows, act, adv, old):
    """The twin: `layers` as the shared network of handle t (a fresh optimizer), the same dataset, weights and old means."""
    t.set_policy_mlp(layers)
    t.fit_clear()
    t.fit_append(rows, act.astype(np.float64), weights=adv)
    t.fit_set_old_means(old)
    return t


def _row(b, g, n, pad=False):
    return b.get_policy_mlp(g, _stride(n) if pad else n)


# ---- 1. the snapshot ------------------------------------------------------------------------------------------------------------------------
def _check_snapshot(b, mor, first, before):
    """Every named row of the column holds fit_predict([row], [g]); every other row of the dataset its bytes of `before`."""
    got = b.fit_get_old_means()
    want = before.copy()
    for g in np.unique(mor[mor >= 0]):
        mine = first + np.nonzero(mor == g)[0]
        want[mine] = b.fit_predict(mine, [int(g)])[0]
        assert np.abs(want[mine]).min() > 0
    assert got.tobytes() == want.tobytes()
    return got


def test_snapshot_stores_the_acting_members_mean(handle):
    from gym_cloth_amd import _lib
    widths = [300, 37, 64, 4]
    nets, rows, act, old, adv = _case(widths)
    b = _population(handle(), nets, rows, act, adv)
    mor = np.full(N_ROWS, 2, dtype=np.int32)                                 # member 0 has one row, member 1 none, the rest are member 2's
    mor[5] = 0
    skipped = [0, 17, 39]
    mor[skipped] = -1
    assert not b.fit_get_old_means().any()
    b.fit_snapshot_policy_members(mor)
    assert b.last_kernel_ms > 0.0
    col = _check_snapshot(b, mor, 0, np.zeros((N_ROWS, 4), dtype=np.float32))
    assert not col[skipped].any() and col[5].tobytes() != b.fit_predict(np.array([5]), [2])[0, 0].tobytes()
    # the skipped rows stay without an old mean: a PPO call that names one is refused, one that names the others is not
    named = np.nonzero(mor >= 0)[0]
    assert b.fit_ppo_grad_members([2, 0], np.stack([named[:6], named[6:12]]), 1.0)[0].shape == (2, 3)
    for row in skipped:
        with pytest.raises(_lib.ClothHipError, match="row %d of member 1 has no old mean.*clothhip_fit_data_snapshot_policy_members.*clothhip_fit_data_set_old_means" % row):
            b.fit_ppo_grad_members([2, 1], np.array([[1, 2], [3, row]]), 1.0)
    # five group PPO steps move the rows and leave the column alone
    table = np.random.RandomState(3).choice(named, size=(5, 2, 9))
    b.fit_ppo_members([2, 0], table, [s for s, _ in Q], [c for _, c in Q], dict(OPTIMIZERS["adam"], lr=1e-2))
    assert b.fit_get_old_means().tobytes() == col.tobytes()
    assert b.fit_predict(named, [2])[0].tobytes() != col[named].tobytes()
    # a sub-range with a first: one row is written anew (under the moved member 0), every other row keeps its bytes, -1 or outside
    again = np.array([-1, 0, -1], dtype=np.int32)
    b.fit_snapshot_policy_members(again, first=15)                           # rows 15 and 17 are skipped, 16 is member 0's now
    col2 = _check_snapshot(b, again, 15, col)
    assert not col2[17].any() and col2[15].tobytes() == col[15].tobytes() and col2[16].tobytes() != col[16].tobytes()
    with pytest.raises(_lib.ClothHipError, match="row 17 of member 0 has no old mean"):
        b.fit_ppo_grad_members([0], np.array([[16, 17]]), 1.0)
    # all -1, and no rows at all: nothing happens
    b.fit_snapshot_policy_members(np.full(N_ROWS, -1, dtype=np.int32))
    b.fit_snapshot_policy_members(np.zeros(0, dtype=np.int32), first=N_ROWS)
    assert b.fit_get_old_means().tobytes() == col2.tobytes()
    # growth keeps the column and the marks; the new rows have no old mean; clear empties both
    b.fit_append(rows, act.astype(np.float64), weights=adv)                  # 80 rows: past the first capacity of 64
    got = b.fit_get_old_means()
    assert b.fit_size() == 2 * N_ROWS and got[:N_ROWS].tobytes() == col2.tobytes() and not got[N_ROWS:].any()
    assert b.fit_ppo_grad_members([0], named[None, :4], 1.0)[0].shape == (1, 3)
    with pytest.raises(_lib.ClothHipError, match="row %d of member 0 has no old mean" % N_ROWS):
        b.fit_ppo_grad_members([0], np.array([[1, N_ROWS]]), 1.0)
    b.fit_snapshot_policy_members(np.array([1, 1], dtype=np.int32), first=2 * N_ROWS - 2)
    _check_snapshot(b, np.array([1, 1]), 2 * N_ROWS - 2, got)
    b.fit_clear()
    b.fit_append(rows[:8], act[:8].astype(np.float64), weights=adv[:8])
    assert not b.fit_get_old_means().any()
    with pytest.raises(_lib.ClothHipError, match="row 1 of member 0 has no old mean"):
        b.fit_ppo_grad_members([0], np.array([[1]]), 1.0)


def test_snapshot_cuts_a_long_member_into_chunks(handle):
    """4 200 rows, 4 097 of them under member 1: one row more than a chunk holds, so its list is cut in two; member 0 has 100 rows
    (padded to the long member's length in the first launch), member 2 none, three rows are skipped."""
    from gym_cloth_amd import _lib
    widths = [300, 5, 4]
    n = 4200
    assert _lib.FIT_MAX_BATCH == 4096
    r = np.random.RandomState(23)
    rows, act = r.uniform(-1, 1, size=(n, 300)).astype(np.float32), r.uniform(-1, 1, size=(n, 4))
    nets = [_random_layers(widths, 70 + g) for g in range(G)]
    b = handle()
    b.set_policy_population(nets, np.zeros(b.E, dtype=np.int32))
    b.fit_append(rows, act)
    mor = np.full(n, 1, dtype=np.int32)
    mor[r.permutation(n)[:103]] = np.concatenate([np.zeros(100, dtype=np.int32), np.full(3, -1, dtype=np.int32)])
    assert (mor == 1).sum() == 4097 and (mor == 0).sum() == 100 and (mor == -1).sum() == 3
    b.fit_snapshot_policy_members(mor)
    every = b.fit_predict(np.arange(n), [0, 1, 2])
    want = np.where((mor == 0)[:, None], every[0], np.where((mor == 1)[:, None], every[1], np.float32(0)))
    got = b.fit_get_old_means()
    assert got.tobytes() == want.tobytes() and not got[mor == -1].any() and np.abs(got[mor >= 0]).min() > 0
    assert not np.array_equal(every[0], every[1])


# ---- 2. the gradient ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 33, 300], ids=["B5", "B33", "B300-two-ranges"])
@pytest.mark.parametrize("widths", [[300, 5, 4], [300, 37, 64, 4]], ids=lambda w: "x".join(map(str, w)))
def test_gradient_equals_each_twins(widths, B, handle):
    """fit_ppo_grad_members(members=[2, 0]) under q = Q with other index rows per member, and members=[1] alone (n_m = 1 on a row other
    than 0): gradient, statistics and ratios of every member are its twin's fit_ppo_grad. B = 300: two ranges of the split batch sum
    and a thread's second row."""
    from gym_cloth_amd.policies import ppo_reference
    nets, rows, act, old, adv = _case(widths)
    b = _population(handle(), nets, rows, act, adv, old)
    t = handle("twin")
    n = _n_params(widths)
    for members, q in (([2, 0], Q), ([1], Q[1:])):
        idx = np.random.RandomState(11 + len(members)).randint(0, N_ROWS, size=(len(members), B)).astype(np.int32)
        stats, grad, ratio = b.fit_ppo_grad_members(members, idx, [s for s, _ in q], [c for _, c in q])
        assert stats.shape == (len(members), 3) and grad.shape == (len(members), n) and ratio.shape == (len(members), B) and grad.dtype == ratio.dtype == np.float32
        for j, g in enumerate(members):
            if B >= 33:                                                     # what the comparison must meet, from the float64 reference alone
                _, _, rho, active = ppo_reference(nets[g], rows, act, old, adv, idx[j], q[j][0], q[j][1])
                a = adv[idx[j]]
                assert (a == 0).any() and (a > 0).any() and (a < 0).any() and active.any() and (~active).any()
                assert (rho > 1.0 + q[j][1]).any() and (rho < 1.0 - q[j][1]).any()                  # both sides of both bounds
                assert B < 300 or ((rho > 1.0 - q[j][1]) & (rho < 1.0 + q[j][1])).any()
            want = _twin(t, nets[g], rows, act, adv, old).fit_ppo_grad(idx[j], q[j][0], q[j][1])
            print("%r B %d member %d: stats %r (twin %r), max |grad| %.3e" % (widths, B, g, stats[j].tolist(), want[0].tolist(), np.abs(grad[j]).max()))
            assert stats[j].tobytes() == want[0].tobytes() and np.isfinite(want[0]).all()
            assert _same(grad[j], want[1]) and np.abs(want[1]).max() > 0
            assert _same(ratio[j], want[2])
        if len(members) == 2:
            assert not _same(grad[0], grad[1]) and not _same(ratio[0], ratio[1])
    for g in range(G):                                                       # nothing was updated
        assert _same(_row(b, g, n), _flat(nets[g]))
    # every output is optional
    L = b._L
    from gym_cloth_amd import _lib
    q1 = (_lib.ClothPpoParams * 1)(_lib.ClothPpoParams(1.0, 0.2))
    assert L.clothhip_policy_fit_ppo_grad_members(b._h, q1, _lib.i32p(np.array([1], dtype=np.int32)), 1, _lib.i32p(idx[:1].copy()), B, None, None, None) == _lib.OK


# ---- 3. steps -------------------------------------------------------------------------------------------------------------------------------
def _steps(b, t, opt, split, case):
    """Five group PPO steps of members [2, 0] under Q and per-member learning rates, as the calls `split` cuts them; then two steps of
    members [0, 1]. -> every returned statistic and every row's whole stride, after checking them against the twins."""
    widths = [300, 5, 4]
    nets, rows, act, old, adv = case
    n, B = _n_params(widths), 7
    _population(b, nets, rows, act, adv, old)
    uploaded = [_row(b, g, n, pad=True) for g in range(G)]
    assert _stride(n) > n and all((u[n:] == 0).all() for u in uploaded)
    members, lr = [2, 0], [3e-3, 1e-2]
    table = np.random.RandomState(12).randint(0, N_ROWS, size=(5, 2, B)).astype(np.int32)
    later = np.random.RandomState(13).randint(0, N_ROWS, size=(2, 2, B)).astype(np.int32)
    sig, clp = [s for s, _ in Q], [c for _, c in Q]
    hyper = dict(OPTIMIZERS[opt], lr=lr)
    cuts = np.cumsum([0] + list(split))
    stats = np.concatenate([b.fit_ppo_members(members, table[lo:hi], sig, clp, hyper) for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert stats.shape == (5, 2, 3)
    for j, g in enumerate(members):
        _twin(t, nets[g], rows, act, adv, old)
        kw = dict(OPTIMIZERS[opt], lr=lr[j])
        want = np.concatenate([t.fit_ppo(table[lo:hi, j], sig[j], clp[j], **kw) for lo, hi in zip(cuts[:-1], cuts[1:])])
        print("%s member %d: kl %r, twin %r" % (opt, g, stats[:, j, 2].tolist(), want[:, 2].tolist()))
        assert stats[:, j].tobytes() == want.tobytes() and (want[1:, 2] > 0).all()
        got = _row(b, g, n, pad=True)
        assert _same(got[:n], t.get_policy_mlp(0, n)) and not _same(got, uploaded[g])
        assert not got[n:].any() and got[n:].tobytes() == uploaded[g][n:].tobytes()      # the pad stays zeros
        if g == 0:                                                          # the twin of row 0 goes on: its step count is 6 and 7 below
            want0 = t.fit_ppo(later[:, 0], 0.7, 0.3, **dict(OPTIMIZERS[opt], lr=2e-3))
    assert _same(_row(b, 1, n, pad=True), uploaded[1])                       # the row not named keeps its whole stride
    # the per-row step count: row 1 joins at t = 1 while row 0 continues
    s2 = b.fit_ppo_members([0, 1], later, [0.7, 0.9], [0.3, 0.15], dict(OPTIMIZERS[opt], lr=[2e-3, 5e-3]))
    assert s2[:, 0].tobytes() == want0.tobytes() and _same(_row(b, 0, n), t.get_policy_mlp(0, n))
    _twin(t, nets[1], rows, act, adv, old)
    want1 = t.fit_ppo(later[:, 1], 0.9, 0.15, **dict(OPTIMIZERS[opt], lr=5e-3))
    assert s2[:, 1].tobytes() == want1.tobytes() and _same(_row(b, 1, n), t.get_policy_mlp(0, n))
    return stats.tobytes() + s2.tobytes() + b"".join(_row(b, g, n, pad=True).tobytes() for g in range(G))


@pytest.mark.parametrize("opt", sorted(OPTIMIZERS))
def test_steps_equal_each_twins(opt, handle):
    """3 + 2 steps with per-member sigma, clip and learning rate: the rows, the statistics and the per-row step count are the twins'
    after the same calls of fit_ppo; the unnamed row's whole stride is what was uploaded; every pad is zeros."""
    _steps(handle(), handle("twin"), opt, (3, 2), _case([300, 5, 4]))


def test_two_and_three_steps_are_five_and_two_runs_give_the_same_bytes(handle):
    case = _case([300, 5, 4])
    one = _steps(handle(), handle("twin"), "adam", (2, 3), case)
    assert one == _steps(handle("other"), handle("twin"), "adam", (5,), case)
    assert one == _steps(handle(), handle("twin"), "adam", (2, 3), case)


def test_a_squared_error_step_and_a_ppo_step_share_the_rows_optimizer(handle):
    """fit_members, then fit_ppo_members, then fit_members again on rows [2, 0]: the twins' fit, fit_ppo, fit -- one set of moments and
    one step count per row. After fit_reset_members([2]) row 2 equals a twin that was reset, row 0 one that was not."""
    widths = [300, 37, 64, 4]
    nets, rows, act, old, adv = _case(widths)
    n = _n_params(widths)
    b, t = _population(handle(), nets, rows, act, adv, old), handle("twin")
    r = np.random.RandomState(14)
    ta, tb, tc, td = (r.randint(0, N_ROWS, size=(2, 2, 9)).astype(np.int32) for _ in range(4))
    members, lr = [2, 0], [3e-3, 1e-2]
    hyper = dict(OPTIMIZERS["adam"], lr=lr)
    sig, clp = [s for s, _ in Q], [c for _, c in Q]
    la = b.fit_members(members, ta, hyper)
    sb = b.fit_ppo_members(members, tb, sig, clp, hyper)
    lc = b.fit_members(members, tc, hyper)
    b.fit_reset_members([2])
    sd = b.fit_ppo_members(members, td, sig, clp, hyper)
    for j, g in enumerate(members):
        _twin(t, nets[g], rows, act, adv, old)
        kw = dict(OPTIMIZERS["adam"], lr=lr[j])
        assert _same(la[:, j], t.fit(ta[:, j], **kw)) and sb[:, j].tobytes() == t.fit_ppo(tb[:, j], sig[j], clp[j], **kw).tobytes()
        assert _same(lc[:, j], t.fit(tc[:, j], **kw))
        if g == 2:
            t.fit_reset()
        assert sd[:, j].tobytes() == t.fit_ppo(td[:, j], sig[j], clp[j], **kw).tobytes()
        assert _same(_row(b, g, n), t.get_policy_mlp(0, n))


# ---- 4. the freeze --------------------------------------------------------------------------------------------------------------------------
def _reference_clip_fractions(widths, layers, rows, act, adv, lr, n_steps):
    """Plain SGD on ppo_reference's gradient from the old means = the first means (test_gpu_ppo._reference_steps_to_freeze's loop):
    the clip fraction before each of n_steps steps."""
    from gym_cloth_amd.policies import ppo_reference, sgd_reference, unpack_mlp
    old = _forward(layers, rows).astype(np.float32)
    theta, u = _flat(layers).astype(np.float32), np.zeros(_flat(layers).size, dtype=np.float32)
    out = []
    for s in range(n_steps):
        stats, grads, _, _ = ppo_reference(unpack_mlp(np.array(widths, dtype=np.int32), theta), rows, act, old, adv, np.arange(len(rows)), 1.0, 0.2)
        out.append(stats[1])
        theta, u = sgd_reference(theta, u, _flat(grads).astype(np.float32), lr=lr, momentum=0.0)
    return np.array(out)


def test_one_member_freezes_while_the_other_keeps_moving(handle):
    """G = 2 under plain SGD on full batches. Member 0 has test_gpu_ppo's freeze case: every advantage -1, so each row is clipped once
    its ratio has fallen below 1 - eps; from the step at which policies.ppo_reference reaches clip_fraction == 1 its gradient is ALL
    zeros and its row stands still, byte for byte, for ten more steps. Member 1 has the same observations under mixed advantages and
    keeps moving through those ten steps."""
    widths, layers, rows, act, adv = _freeze_case()
    at = _reference_steps_to_freeze()
    assert at is not None and 2 <= at < 100, at
    other = _layers(widths, 77)
    r = np.random.RandomState(78)
    act1 = (_forward(other, rows) + r.normal(size=(12, 4))).astype(np.float32)
    adv1 = r.normal(size=12).astype(np.float32)
    assert (adv1 > 0).any() and (adv1 < 0).any()
    n = _n_params(widths)
    b = handle()
    b.set_policy_population([layers, other], np.zeros(b.E, dtype=np.int32))
    b.fit_append(np.concatenate([rows, rows]), np.concatenate([act, act1]).astype(np.float64), weights=np.concatenate([adv, adv1]))
    b.fit_snapshot_policy_members(np.repeat(np.array([0, 1], dtype=np.int32), 12))
    idx = np.arange(24).reshape(2, 12)
    sgd = dict(optimizer="sgd", lr=[FREEZE_LR, FREEZE_LR / 20.0], momentum=0.0)
    assert _reference_clip_fractions(widths, other, rows, act1, adv1, FREEZE_LR / 20.0, at + 11).max() < 0.75      # member 1 is far from frozen then
    before = b.fit_ppo_members([0, 1], np.tile(idx, (at, 1, 1)), 1.0, 0.2, sgd)
    print("the reference freezes at step %d; member 0's clip fractions %r" % (at, before[:, 0, 1].tolist()))
    assert before[0, 0, 1] == 0.0 and (before[:, 0, 1] < 1.0).all()          # not before that step
    stats, grad, ratio = b.fit_ppo_grad_members([0, 1], idx, 1.0, 0.2)
    assert stats[0, 1] == 1.0 and not grad[0].any() and (ratio[0] <= np.float32(0.8)).all()
    assert stats[1, 1] < 1.0 and grad[1].any()
    frozen, moving = _row(b, 0, n).tobytes(), _row(b, 1, n).tobytes()
    assert frozen != _flat(layers).tobytes()
    for s in range(10):
        later = b.fit_ppo_members([0, 1], idx[None], 1.0, 0.2, sgd)
        assert later[0, 0, 1] == 1.0 and _row(b, 0, n).tobytes() == frozen
        now = _row(b, 1, n).tobytes()
        assert now != moving, s
        moving = now


# ---- 5. what the new entries leave alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [9, 300], ids=["B9", "B300-two-ranges"])
def test_the_shared_entries_keep_their_bytes(B, handle):
    """Two handles with one shared network and the same rows. One is asked for every new entry between the existing calls -- each is
    refused, a shared network is no population --; the other never is. Every existing entry of the trainer returns the same bytes:
    the fixed-sigma and the learned-sigma PPO gradient and steps, the snapshot, the squared-error gradient, steps, loss and predict,
    the critic's steps and predict, GAE."""
    from gym_cloth_amd import _lib
    widths = [300, 37, 64, 4]
    nets, rows, act, old, adv = _case(widths)
    r = np.random.RandomState(B)
    idx, table = r.randint(0, N_ROWS, size=B).astype(np.int32), r.randint(0, N_ROWS, size=(3, B)).astype(np.int32)
    critic = _layers([300, 6, 1], 22)
    rew = r.normal(size=N_ROWS).astype(np.float32)
    nxt = np.where(np.arange(N_ROWS) % 4 == 3, -1, np.arange(N_ROWS) + 1).astype(np.int32)
    new, twin = handle("shared-new"), handle("shared-twin")
    for b in (new, twin):
        _twin(b, nets[0], rows, act, adv, old)
        b.set_value_mlp(critic)
        b.fit_set_transitions(rew, nxt)
        b.set_policy_log_sigma(np.full(4, np.log(0.5)))
    L, h = new._L, new._h
    q1 = (_lib.ClothPpoParams * 1)(_lib.ClothPpoParams(0.5, 0.2))
    p1 = (_lib.ClothFitParams * 1)(_lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0))
    zero = np.zeros(1, dtype=np.int32)
    mor = np.zeros(N_ROWS, dtype=np.int32)

    def refused():
        for rc in (L.clothhip_fit_data_snapshot_policy_members(h, 0, N_ROWS, _lib.i32p(mor)),
                   L.clothhip_policy_fit_ppo_grad_members(h, q1, _lib.i32p(zero), 1, _lib.i32p(idx), B, None, None, None),
                   L.clothhip_policy_fit_ppo_members(h, p1, q1, _lib.i32p(zero), 1, _lib.i32p(idx), 1, B, None)):
            assert rc == _lib.ESTATE and "ONE shared network, not a population" in L.clothhip_last_error().decode()

    adam = dict(OPTIMIZERS["adam"], lr=1e-2)
    refused()
    ga, gb = new.fit_ppo_grad(idx, 0.5, 0.2), twin.fit_ppo_grad(idx, 0.5, 0.2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ga, gb))
    refused()
    assert new.fit_ppo(table, 0.5, 0.2, **adam).tobytes() == twin.fit_ppo(table, 0.5, 0.2, **adam).tobytes() and _blob(new).tobytes() == _blob(twin).tobytes()
    refused()
    fa, fb = new.fit_grad(idx), twin.fit_grad(idx)
    assert fa[0] == fb[0] and fa[1].tobytes() == fb[1].tobytes()
    assert new.fit(table, **adam).tobytes() == twin.fit(table, **adam).tobytes() and _blob(new).tobytes() == _blob(twin).tobytes()
    refused()
    new.fit_snapshot_policy(3, 20); twin.fit_snapshot_policy(3, 20)
    assert new.fit_get_old_means().tobytes() == twin.fit_get_old_means().tobytes() and new.fit_predict(idx).tobytes() == twin.fit_predict(idx).tobytes()
    assert new.fit_ppo(table, 1.0, 0.1, **adam).tobytes() == twin.fit_ppo(table, 1.0, 0.1, **adam).tobytes() and _blob(new).tobytes() == _blob(twin).tobytes()
    refused()
    # the learned-sigma entries (the snapshots above stored the head as the old log sigma of rows 3 .. 22), the loss, the critic and GAE
    sub = 3 + idx % 20
    sa, sb = new.fit_ppo_sigma_grad(sub, 0.2, 0.01), twin.fit_ppo_sigma_grad(sub, 0.2, 0.01)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(sa, sb))
    sa, sb = new.fit_ppo_sigma(3 + table % 20, 0.2, 0.01, **adam), twin.fit_ppo_sigma(3 + table % 20, 0.2, 0.01, **adam)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(sa, sb)) and _blob(new).tobytes() == _blob(twin).tobytes()
    assert new.get_policy_log_sigma().tobytes() == twin.get_policy_log_sigma().tobytes()
    refused()
    assert new.fit_loss(idx) == twin.fit_loss(idx)
    assert new.value_fit(table, **adam).tobytes() == twin.value_fit(table, **adam).tobytes() and new.get_value_mlp().tobytes() == twin.get_value_mlp().tobytes()
    assert new.value_predict(idx).tobytes() == twin.value_predict(idx).tobytes()
    refused()
    ga, gb = new.fit_gae(0.9, 0.8, normalize=True), twin.fit_gae(0.9, 0.8, normalize=True)
    assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes() and new.fit_get_weights().tobytes() == twin.fit_get_weights().tobytes()
    for b in (new, twin):
        b.set_policy_log_sigma(None)
        b.set_value_mlp(None)


def test_fit_members_keeps_its_bytes_beside_the_new_entries(handle):
    """Two population handles: one runs fit_members, then the new entries' gradient and snapshot (which update no row), then fit_members
    again; the other only the two fit_members calls. Losses and rows are equal."""
    widths = [300, 37, 64, 4]
    nets, rows, act, old, adv = _case(widths)
    n = _n_params(widths)
    r = np.random.RandomState(15)
    ta, tb = (r.randint(0, N_ROWS, size=(2, 3, 9)).astype(np.int32) for _ in range(2))
    hyper = dict(OPTIMIZERS["adam"], lr=[1e-2, 3e-3, 1e-3])
    new, twin = _population(handle(), nets, rows, act, adv, old), _population(handle("other"), nets, rows, act, adv, old)
    a1, b1 = new.fit_members([0, 1, 2], ta, hyper), twin.fit_members([0, 1, 2], ta, hyper)
    new.fit_ppo_grad_members([2, 0], tb[0, :2], 0.5)
    new.fit_snapshot_policy_members(np.arange(N_ROWS, dtype=np.int32) % 4 - 1)
    new.fit_ppo_grad_members([1], tb[0, :1], 0.5)
    a2, b2 = new.fit_members([0, 1, 2], tb, hyper), twin.fit_members([0, 1, 2], tb, hyper)
    assert _same(a1, b1) and _same(a2, b2)
    for g in range(G):
        assert _same(_row(new, g, n, pad=True), _row(twin, g, n, pad=True))
    assert new.fit_get_old_means().tobytes() != twin.fit_get_old_means().tobytes()


def test_a_shared_call_after_a_grouped_call_reads_its_own_row_of_constants():
    """ONE handle, the file's 40 rows, Adam. The shared network's constants are row 0 of the table every fixed-sigma call uploads, and a
    grouped call leaves that table longer and different: a shared network at sigma 0.5, gradient and 2 steps at B = 5; a population of
    3, a snapshot by member and 2 steps of members [2, 0] under sigma (0.7, 0.3), clip (0.1, 0.3); a new shared network, a snapshot, the
    gradient and 3 steps at sigma 1.0, B = 300 (two 256-row ranges). Every stage's statistics, gradients, ratios and final weights are,
    byte for byte, those of a FRESH handle given that stage's calls alone (test_gpu_fit_members.py has the squared-error walk)."""
    widths = [300, 5, 4]
    n = _n_params(widths)
    nets, rows, act, old, adv = _case(widths)
    first, last = nets[0], _random_layers(widths, 51)
    r = np.random.RandomState(17)
    i1, t1, t2, i3, t3 = (r.randint(0, N_ROWS, size=s).astype(np.int32) for s in [(5,), (2, 5), (2, 2, 5), (300,), (3, 300)])
    adam = dict(OPTIMIZERS["adam"], lr=1e-2)

    def shared(layers, idx, table, sigma, snapshot):
        def stage(x):
            x.set_policy_mlp(layers)
            if snapshot:
                x.fit_snapshot_policy()
            grad = x.fit_ppo_grad(idx, sigma, 0.2)                         # (statistics, gradient, ratios)
            return [x.fit_ppo(table, sigma, 0.2, **adam)] + list(grad), [x.get_policy_mlp(0, n)]
        return stage

    def population(x):
        x.set_policy_population(nets, np.zeros(x.E, dtype=np.int32))
        x.fit_snapshot_policy_members(np.arange(N_ROWS, dtype=np.int32) % G)
        got = [x.fit_ppo_members([2, 0], t2, [0.7, 0.3], [0.1, 0.3], adam), x.fit_get_old_means()]
        return got, [_row(x, g, n, pad=True) for g in range(G)]

    def dataset(x):
        x.fit_append(rows, act.astype(np.float64), weights=adv)
        x.fit_set_old_means(old)
        return x

    b = dataset(_new_batch(10))
    stages = [("shared, sigma 0.5, B = 5", shared(first, i1, t1, 0.5, False)), ("population", population), ("shared, sigma 1.0, B = 300", shared(last, i3, t3, 1.0, True))]
    for name, stage in stages:
        got, got_w = stage(b)
        fresh = dataset(_new_batch(10))
        want, want_w = stage(fresh)
        fresh.close()
        print("%s: the steps' statistics %r, fresh handle %r" % (name, got[0].tolist(), want[0].tolist()))
        assert len(got) == len(want) and len(got_w) == len(want_w)
        assert all(np.isfinite(w).all() for w in want) and all(np.isfinite(w).all() for w in want_w)
        assert all(_same(g, w) for g, w in zip(got, want)), name
        assert all(_same(g, w) for g, w in zip(got_w, want_w)), name
        assert (want[0][1:, ..., 2] > 0).all()                              # the steps moved off the old means
        if name != "population":
            assert np.abs(want[2]).max() > 0 and want[3].shape == (len(want[3]),) and want[3].dtype == np.float32
    assert not _same(got_w[0], _flat(last))                                  # (the last stage did train)
    b.close()


# ---- 6. every refusal -----------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from gym_cloth_amd import _lib
    from gym_cloth_amd.envs import ClothVecEnv
    cfg = base_cfg("tier1", 1337)
    cfg["cloth"]["num_width_points"] = cfg["cloth"]["num_height_points"] = 10
    cfg["env"]["force_grab"] = True
    v = ClothVecEnv(cfg, n_envs=2, precision="f32", consume_domrand_draws=False)
    v.seed([1337, 1338])
    v.reset()
    b, L, h = v.batch, v.batch._L, v.batch._h
    widths = [300, 5, 4]
    nets = [_layers(widths, 1 + g) for g in range(G)]
    npar = _n_params(widths)
    b.set_policy_population(nets, np.zeros(2, dtype=np.int32))
    r = np.random.RandomState(0)
    n = 10
    rows, labels = r.uniform(-1, 1, size=(n, 300)).astype(np.float32), r.uniform(-1, 1, size=(n, 4))
    w, old = r.normal(size=n).astype(np.float32), r.uniform(-1, 1, size=(n, 4)).astype(np.float32)
    b.fit_append(rows, labels, weights=w)
    b.fit_set_old_means(old[:8])                                               # rows 8 and 9 have no old mean
    old[8:] = 0.0
    members = np.array([2, 0], dtype=np.int32)
    idx = np.ascontiguousarray(np.arange(8, dtype=np.int32).reshape(2, 4))
    adam = dict(OPTIMIZERS["adam"], lr=1e-3)
    b.fit_ppo_members(members, idx[None], 0.5, 0.2, adam)                      # one step, so that the moments and the step counts exist
    state = lambda: [_row(b, g, npar, pad=True) for g in range(G)]
    snap = (b.fit_ppo_grad_members(members, idx, 0.5), state())
    after_one = (b.fit_ppo_members(members, idx[None], 0.5, 0.2, adam), state())   # what the NEXT step gives from this state ...
    b.set_policy_population(nets, np.zeros(2, dtype=np.int32))                # ... which is rebuilt: the same rows, one step
    b.fit_ppo_members(members, idx[None], 0.5, 0.2, adam)
    assert all(_same(x, y) for x, y in zip(state(), snap[1]))
    ip, dp, fp = _lib.i32p, _lib.dp, _lib.fp
    QA = _lib.ClothPpoParams * 2
    PA = _lib.ClothFitParams * 2
    ok = QA(_lib.ClothPpoParams(0.5, 0.2), _lib.ClothPpoParams(0.5, 0.2))
    pa = PA(_lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0), _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0))
    g, st, ra = np.zeros((2, npar), dtype=np.float32), np.zeros((2, 3)), np.zeros((2, 4), dtype=np.float32)
    mor = np.zeros(n, dtype=np.int32)

    def unchanged():
        assert b.fit_size() == n and b.fit_get_weights().tobytes() == w.tobytes() and b.fit_get_old_means().tobytes() == old.tobytes()
        o, l = b.fit_data()
        assert np.array_equal(o, rows) and np.array_equal(l, labels.astype(np.float32))
        now = (b.fit_ppo_grad_members(members, idx, 0.5), state())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(now[0], snap[0])) and all(_same(x, y) for x, y in zip(now[1], snap[1]))
        for row in (8, 9):                                                    # the marks
            with pytest.raises(_lib.ClothHipError, match="row %d of member 0 has no old mean" % row):
                b.fit_ppo_grad_members([0], np.array([[0, row]]), 0.5)

    def grad(q=ok, m=members, n_m=2, ix=idx, B=4):
        return L.clothhip_policy_fit_ppo_grad_members(h, q, ip(m), n_m, ip(ix), B, fp(g), dp(st), fp(ra))

    def step(p=pa, q=ok, m=members, n_m=2, ix=idx, n_steps=1, B=4):
        return L.clothhip_policy_fit_ppo_members(h, p, q, ip(m), n_m, ip(ix), n_steps, B, None)

    def snapshot(first=0, k=n, m=mor):
        return L.clothhip_fit_data_snapshot_policy_members(h, first, k, ip(m))

    err = lambda: L.clothhip_last_error().decode()
    # the snapshot: a range outside the dataset, a NULL table, an entry outside [-1, rows) by its position
    for first, k in ((n - 1, 2), (n, 1), (-1, 1), (0, n + 1), (2, -1)):
        assert snapshot(first, k) == _lib.EINVAL
    assert snapshot(0, n, None) == _lib.EINVAL and "member_of_row is NULL" in err()
    for bad in (G, -2, 1 << 20):
        m = mor.copy()
        m[7] = bad
        assert snapshot(0, n, m) == _lib.EINVAL and "member_of_row[7] = %d" % bad in err()
    assert snapshot(3, 1, np.array([G], dtype=np.int32)) == _lib.EINVAL and "member_of_row[0]" in err()
    assert snapshot(4, 0, None) == _lib.OK and snapshot(n, 0, None) == _lib.OK and snapshot(0, n, np.full(n, -1, dtype=np.int32)) == _lib.OK
    unchanged()
    # no old mean: rows 8, 9, by row and member
    assert grad(ix=np.array([[0, 1, 2, 3], [4, 9, 6, 7]], dtype=np.int32)) == _lib.ESTATE
    assert "idx[5] = row 9 of member 0" in err() and "clothhip_fit_data_snapshot_policy_members" in err() and "clothhip_fit_data_set_old_means" in err()
    assert step(ix=np.array([[[0, 1, 2, 3], [4, 5, 6, 7]], [[0, 8, 2, 3], [4, 5, 6, 7]]], dtype=np.int32), n_steps=2) == _lib.ESTATE and "row 8 of member 2" in err()
    # sigma and clip of member j, by j
    for bad in ((0.0, 0.2), (-1.0, 0.2), (np.nan, 0.2), (np.inf, 0.2), (1e-200, 0.2), (0.5, -0.01), (0.5, 1.0), (0.5, np.nan), (0.5, np.inf)):
        for j in (0, 1):
            q = QA(_lib.ClothPpoParams(0.5, 0.2), _lib.ClothPpoParams(0.5, 0.2))
            q[j] = _lib.ClothPpoParams(*bad)
            assert grad(q=q) == _lib.EINVAL and ("q[%d]: " % j) in err(), (bad, j)
            assert step(q=q) == _lib.EINVAL and ("q[%d]: " % j) in err(), (bad, j)
    # q == NULL, and everything clothhip_policy_fit_members refuses
    assert grad(q=None) == _lib.EINVAL and step(q=None) == _lib.EINVAL and step(p=None) == _lib.EINVAL
    assert grad(m=None) == _lib.EINVAL and grad(ix=None) == _lib.EINVAL and step(m=None) == _lib.EINVAL and step(ix=None) == _lib.EINVAL
    assert grad(n_m=0) == _lib.EINVAL and step(n_m=-1) == _lib.EINVAL and step(n_steps=-1) == _lib.EINVAL
    for m in ([2, 2], [0, G], [-1, 0]):
        assert grad(m=np.array(m, dtype=np.int32)) == _lib.EINVAL and step(m=np.array(m, dtype=np.int32)) == _lib.EINVAL, m
    assert grad(B=0) == _lib.EINVAL and grad(B=_lib.FIT_MAX_BATCH + 1) == _lib.EINVAL and step(B=0) == _lib.EINVAL
    many = np.zeros(17, dtype=np.int32)                                        # (refused by B before idx is read)
    assert L.clothhip_policy_fit_ppo_grad_members(h, ok, ip(np.arange(3, dtype=np.int32)), 3, ip(many), _lib.FIT_MAX_MEMBER_ROWS // 2, None, None, None) == _lib.EINVAL
    for ix in ([[0, 1, 2, 3], [4, 5, 6, n]], [[0, -1, 2, 3], [4, 5, 6, 7]]):
        assert grad(ix=np.array(ix, dtype=np.int32)) == _lib.EINVAL and step(ix=np.array(ix, dtype=np.int32)) == _lib.EINVAL
    for field, bad in (("optimizer", 2.0), ("lr", -1.0), ("lr", np.nan), ("beta1", 1.0), ("beta2", 1.5), ("eps", np.inf), ("momentum", -0.1)):
        p = PA(_lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0), _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0))
        setattr(p[1], field, bad)
        assert step(p=p) == _lib.EINVAL and "p[1]" in err(), field
    p = PA(_lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0), _lib.ClothFitParams(1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0))
    assert step(p=p) == _lib.EINVAL and "one optimizer per call" in err()
    assert step(n_steps=0) == _lib.OK                                          # no steps: nothing changes
    assert L.clothhip_policy_fit_ppo_grad_members(h, ok, ip(members), 2, ip(idx), 4, None, None, None) == _lib.OK   # every output is optional
    unchanged()
    # a launch in flight
    nsteps, done = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, 2, 4)))
    assert grad() == _lib.ESTATE and step() == _lib.ESTATE and snapshot() == _lib.ESTATE
    b.run_actions_end()
    unchanged()
    # the moments and the step counts are untouched too: the next step is the one that followed the snapshot
    nxt = b.fit_ppo_members(members, idx[None], 0.5, 0.2, adam)
    assert nxt.tobytes() == after_one[0].tobytes() and all(_same(x, y) for x, y in zip(state(), after_one[1]))
    # an empty dataset, a shared network, no network (these change the handle, so they come last)
    b.fit_clear()
    assert grad() == _lib.ESTATE and "empty" in err() and step() == _lib.ESTATE and snapshot(0, 0) == _lib.ESTATE
    b.set_policy_mlp(nets[0])
    b.fit_append(rows, labels, weights=w)
    for rc in (grad(m=np.zeros(1, dtype=np.int32), n_m=1), step(m=np.zeros(1, dtype=np.int32), n_m=1), snapshot()):
        assert rc == _lib.ESTATE and "ONE shared network, not a population" in err()
    v.close()
    bare = _new_batch(10)
    assert L.clothhip_policy_fit_ppo_grad_members(bare._h, ok, ip(members), 2, ip(idx), 4, None, None, None) == _lib.ESTATE and "no network" in err()
    assert L.clothhip_fit_data_snapshot_policy_members(bare._h, 0, 0, None) == _lib.ESTATE
    bare.close()


# ---- 7. demos.ppo_fit with an ensemble ------------------------------------------------------------------------------------------------------
def _ppo_run(target_kl):
    from gym_cloth_amd.demos import actor_critic_collect, ppo_fit
    from gym_cloth_amd.envs import ClothVecEnv
    from gym_cloth_amd.policies import MLPEnsemble, ValueTrainer
    cfg = base_cfg("tier1", 1337)
    cfg["cloth"]["num_width_points"] = cfg["cloth"]["num_height_points"] = 10
    cfg["env"]["force_grab"] = True
    cfg["env"]["max_actions"] = 2
    v = ClothVecEnv(cfg, n_envs=4, precision="f32", consume_domrand_draws=False)
    v.seed([1337 + e for e in range(4)])
    v.reset()
    ens = MLPEnsemble(v, [_layers([3 * v.P, 5, 4], 21), _layers([3 * v.P, 5, 4], 23)], lr=[1e-2, 3e-3])
    critic = ValueTrainer(v, _layers([3 * v.P, 6, 1], 22), lr=1e-2)
    sigma = np.array([0.05, 0.1])
    noise = np.random.RandomState(14).normal(size=(4, 4, 4)) * sigma[ens.member][None, :, None]
    col = actor_critic_collect(v, ens, n_actions=4, policy_noise=noise, slots_per_launch=4)
    n = col["appended"] + col["open_rows"]
    before = ens.predict(np.arange(n))
    fit = ppo_fit(v, ens, critic, col, sigma=sigma, gamma=0.9, lam=0.8, clip=[0.2, 0.1], n_value_steps=3, n_epochs=3, batch_size=4, seed=0, target_kl=target_kl)
    res = (fit, col, before, v.batch.fit_get_old_means(), ens.weights(), [v.batch.get_policy_mlp(g, ens.n_params) for g in range(2)], v.batch.get_value_mlp(), ens.member.copy())
    v.close()
    return res


def test_ppo_fit_with_an_ensemble_is_deterministic_and_retires_on_target_kl():
    from gym_cloth_amd.demos import member_normalize
    one, again = _ppo_run(None), _ppo_run(None)
    fit, col, before, old, w, blobs, vblob, member = one
    assert all(x.tobytes() == y.tobytes() for x, y in zip(blobs, again[5])) and vblob.tobytes() == again[6].tobytes()
    assert fit["ppo_stats"].tobytes() == again[0]["ppo_stats"].tobytes() and old.tobytes() == again[3].tobytes()
    mor = fit["member_of_row"]
    assert col["appended"] == 16 and np.array_equal(mor, np.where(col["leaf"], -1, member[col["ds_env"]])) and member.tolist() == [0, 1, 0, 1]
    assert fit["members"].tolist() == [0, 1] and (mor == 0).sum() == (mor == 1).sum() == 8
    assert fit["epochs"].tolist() == [3, 3] and fit["ppo_stats"].shape == (6, 2, 3) and np.isfinite(fit["ppo_stats"]).all()
    # ONE snapshot before any policy step: every non-leaf row holds the mean of the member that acted there, a leaf nothing
    want_old = np.where((mor == 0)[:, None], before[0], np.where((mor == 1)[:, None], before[1], np.float32(0)))
    assert old.tobytes() == want_old.tobytes()
    assert (fit["ppo_stats"][0, :, 1] == 0.0).all() and (fit["ppo_stats"][0, :, 2] == 0.0).all() and (fit["ppo_stats"][1:, :, 2] > 0.0).all()
    assert w.tobytes() == member_normalize(fit["adv"], mor).tobytes() and np.count_nonzero(w) == 16      # normalised per member, a leaf 0
    assert fit["value_losses"].shape == (3,)
    assert blobs[0].tobytes() != _flat(_layers([300, 5, 4], 21)).tobytes() and blobs[1].tobytes() != _flat(_layers([300, 5, 4], 23)).tobytes()
    stopped = _ppo_run(0.0)
    assert stopped[0]["epochs"].tolist() == [1, 1] and np.isnan(stopped[0]["ppo_stats"][2:]).all()      # two minibatches per epoch: the second has kl > 0
    assert stopped[0]["ppo_stats"][:2].tobytes() == fit["ppo_stats"][:2].tobytes()
