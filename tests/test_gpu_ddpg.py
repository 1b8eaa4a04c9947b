"""GPU tests of DDPG on the device (csrc/cloth_fit_ddpg.hpp, clothhip_q_fit*, clothhip_policy_fit_dpg*, clothhip_ddpg_*): the
critic's and the actor's gradients on exactly representable data, EQUAL to the float64 references; the four new kernels by bytes
against their numpy restatements; Gaussian data within the a-priori bound; the critic pinned to the value network's trainer; a fit of
n steps against the same steps one call at a time, optimizers restated; the gate's freeze; independence from everything else on the
handle; every refusal; demos.ddpg_fit over two collections. tests/ddpg_cases.py holds the cases, tests/test_ddpg_host.py checks their
preconditions on the CPU. Every comparison is array_equal or by bytes unless it says otherwise."""
import ctypes as C

import numpy as np
import pytest

import ddpg_cases as D
from test_gpu_dagger import E, _env, _layers
from test_gpu_policy_fit import ADAM, OPTIMIZERS, _blob, _flat, _new_batch, _random_layers, _restated_step

pytestmark = pytest.mark.gpu

INF = float("inf")


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b):
    return np.array_equal(_i32(np.asarray(a, dtype=np.float32)), _i32(np.asarray(b, dtype=np.float32)))


@pytest.fixture(scope="module")
def batch_of():
    """n_side -> ONE ClothBatch of one cloth for the cases that only need a handle to train on (each sets its own networks and data)."""
    made = {}

    def get(n_side):
        if n_side not in made:
            made[n_side] = _new_batch(n_side)
        b = made[n_side]
        b.fit_clear()
        b.set_policy_mlp(None)
        b.set_value_mlp(None)
        b.set_q_mlp(None)
        b.set_policy_log_sigma(None)
        return b
    yield get
    for b in made.values():
        b.close()


def _load(b, c):
    """The case on b: its dataset with the transitions, its policy and Q network, and its target networks by upload."""
    n = len(c['rows'])
    assert b.fit_append(c['rows'], c['labels']) == n
    b.fit_set_transitions(c['rew'], c['next'])
    b.set_policy_mlp(c['pol'])
    b.set_q_mlp(c['q'])
    b.ddpg_set_targets(c['tpol'], c['tq'])
    pol, q = b.ddpg_targets()
    assert _same(pol, _flat(c['tpol'])) and _same(q, _flat(c['tq']))
    return b


def _states(b):
    """Every network and target of b, by download."""
    return (_blob(b), b.get_q_mlp()) + b.ddpg_targets()


# ---- 1. exact data ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_side,pw,qw,dens,seed", D.EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_exact_data_equals_the_references(n_side, pw, qw, dens, seed, batch_of):
    """Small-integer networks, rows, labels and rewards, gamma = tau = 1/2, act_bound = 1, the twelve rows of chain_case; B = 8, B = 1
    and a repeated row: the statistics, y, q, dA and every gradient element of q_grad and dpg_grad EQUAL the float64 references'
    (ddpg_cases.exact_asserts has the preconditions); ddpg_polyak equals polyak_reference. Nothing else moves."""
    from gym_cloth_amd.policies import dpg_reference, polyak_reference, q_fit_reference
    c = D.exact_asserts(pw, qw, dens, seed)
    b = _load(batch_of(n_side), c)
    for idx in (D.IDX8, D.IDX1, D.IDXR):
        B = len(idx)
        loss, gq, y, q = q_fit_reference(c['q'], c['tq'], c['tpol'], c['rows'], c['labels'], c['rew'], c['next'], idx, D.GAMMA, D.BOUND)
        stats, grad, y_d, q_d = b.q_grad(idx, D.GAMMA, D.BOUND)
        assert np.array_equal(stats, [loss, q.sum() / B, y.sum() / B]), (stats, loss)
        assert np.array_equal(y_d.astype(np.float64), y) and np.array_equal(q_d.astype(np.float64), q)
        bad = np.nonzero(grad.astype(np.float64) != _flat(gq))[0]
        assert bad.size == 0, (qw, B, bad[:8], grad[bad[:8]], _flat(gq)[bad[:8]])
        st, gp, dA = dpg_reference(c['pol'], c['q'], c['rows'], idx, D.BOUND)
        stats, grad, dA_d = b.dpg_grad(idx, D.BOUND)
        assert np.array_equal(stats, st), (stats, st)
        assert np.array_equal(dA_d.astype(np.float64), dA)
        bad = np.nonzero(grad.astype(np.float64) != _flat(gp))[0]
        assert bad.size == 0, (pw, B, bad[:8], grad[bad[:8]], _flat(gp)[bad[:8]])
    g0 = b.q_grad(D.IDX8, 0.0, D.BOUND)
    assert np.array_equal(g0[2], c['rew'][D.IDX8]) and not np.array_equal(g0[1], b.q_grad(D.IDX8, D.GAMMA, D.BOUND)[1])
    before = _states(b)
    assert _same(before[0], _flat(c['pol'])) and _same(before[1], _flat(c['q'])) and _same(before[2], _flat(c['tpol'])) and _same(before[3], _flat(c['tq']))
    b.ddpg_polyak(D.TAU)
    after = _states(b)
    assert _same(after[0], before[0]) and _same(after[1], before[1])
    assert _same(after[2], polyak_reference(before[2], before[0], D.TAU)) and _same(after[3], polyak_reference(before[3], before[1], D.TAU))
    assert np.array_equal(after[2].astype(np.float64), 0.5 * before[2].astype(np.float64) + 0.5 * before[0].astype(np.float64)) and not _same(after[2], before[2])


# ---- 2. the elementwise kernels by bytes on Gaussian data ---------------------------------------------------------------------------------
def _colsum32(dz):
    """k_fit_colsum: a float32 sum over the rows in ascending order, per column."""
    s = np.zeros(dz.shape[1:], dtype=np.float32)
    for r in range(len(dz)):
        s = (s + dz[r]).astype(np.float32)
    return s


@pytest.mark.parametrize("n_side,B", [(10, 8), (10, 1), (10, 257), (25, 8)], ids=lambda v: str(v))
def test_elementwise_kernels_by_bytes(n_side, B, batch_of):
    """k_fit_concat through the downloaded X (both action sources, with and without a clamp, the 16-byte aligned rows of 10 x 10 and
    the unaligned ones of 25 x 25); k_fit_loss_td's y, statistics and -- through the last layer's bias gradient, a float32 sum of dz in
    row order -- dz against td_loss_reference fed the downloaded q and qn; k_fit_dpg_dz through da_out, the statistics and the last
    bias gradient against dpg_dz_reference. B = 257: two rows for thread 0, the split batch sum of two ranges behind it."""
    from gym_cloth_amd.policies import concat_reference, dpg_dz_reference, td_loss_reference
    P3 = 3 * n_side * n_side
    pw, qw = [P3, 37, 64, 4], [P3 + 4, 37, 64, 1]
    c, idx = D.gaussian_case(pw, qw, B, seed=4, n_rows=48 if B <= 48 else 300)
    if B == 8:
        idx[1] = idx[5]                                                        # a repeated row
    b = _load(batch_of(n_side), c)
    nx = np.asarray(c['next'])[idx]
    for bound in (D.G_BOUND, INF):
        stats, grad, y, q = b.q_grad(idx, D.G_GAMMA, bound)
        X, qn, q_again = b.ddpg_last_tables(B)
        want_X = concat_reference(c['rows'], c['labels'][idx], idx, bound)
        assert X.tobytes() == want_X.tobytes() and _same(q, q_again)
        if B > 1:
            assert (bound == INF) == _same(X[:, -4:], c['labels'][idx]) and (bound == INF or np.abs(X[:, -4:]).max() == bound)
        y_r, dz_r, st_r = td_loss_reference(q, qn, c['rew'][idx], nx, D.G_GAMMA)
        assert y.tobytes() == y_r.tobytes() and stats.tobytes() == st_r.tobytes() and np.isfinite(stats).all()
        assert _same(grad[-1:], _colsum32(dz_r[:, None]))
        assert _same(y[nx == D.TERMINAL], c['rew'][idx][nx == D.TERMINAL]) and (B == 1 or (nx == D.TERMINAL).any()) and not _same(y, c['rew'][idx])
        mu = b.fit_predict(idx)
        stats, grad, dA = b.dpg_grad(idx, bound)
        X, _, q = b.ddpg_last_tables(B, want_qn=False)
        assert X.tobytes() == concat_reference(c['rows'], mu, idx, bound).tobytes()
        dz_r, st_r = dpg_dz_reference(dA, mu, q, bound)
        assert stats.tobytes() == st_r.tobytes() and (B == 1 or (bound == INF) == (stats[1] == 0.0))
        assert _same(grad[-4:], _colsum32(dz_r))
    # the target pass's concat, the network source over the SUCCESSOR rows: a target Q network that reads one input column
    succ = np.where(nx >= 0, nx, idx)
    b.set_policy_mlp(c['tpol'])
    mu_n = b.fit_predict(succ)                                                  # the target policy's output, by the trainer's own forward
    b.set_policy_mlp(c['pol'])
    for col in (0, P3 - 1, P3, P3 + 1, P3 + 2, P3 + 3):
        W = np.zeros((1, P3 + 4), dtype=np.float32)
        W[0, col] = 1.0
        b.set_q_mlp([(W, np.zeros(1, dtype=np.float32))])
        b.ddpg_set_targets(c['tpol'], [(W, np.zeros(1, dtype=np.float32))])
        b.q_grad(idx, 1.0, D.G_BOUND)
        _, qn, _ = b.ddpg_last_tables(B)
        assert _same(qn, concat_reference(c['rows'], mu_n, succ, D.G_BOUND)[:, col]), col


@pytest.mark.parametrize("tau", [0.0, 0.005, 1.0])
def test_polyak_by_bytes(tau, batch_of):
    """k_fit_polyak over both targets of a 25 x 25 pair (n_params no multiple of 256) against polyak_reference: by bytes at
    tau = 0.005; as VALUES at tau = 0 and tau = 1, where a product by 0 may turn a -0 into a +0. Twice: the update reads what it wrote."""
    from gym_cloth_amd.policies import polyak_reference
    pw, qw = [1875, 37, 64, 4], [1879, 37, 64, 1]
    c = dict(pol=_random_layers(pw, 1), tpol=_random_layers(pw, 2), q=_random_layers(qw, 3), tq=_random_layers(qw, 4))
    b = batch_of(25)
    b.set_policy_mlp(c['pol'])
    b.set_q_mlp(c['q'])
    b.ddpg_set_targets(c['tpol'], c['tq'])
    want = [_flat(c['tpol']), _flat(c['tq'])]
    assert want[0].size % 256 and want[1].size % 256
    for _ in range(2):
        b.ddpg_polyak(tau)
        want = [polyak_reference(want[0], _flat(c['pol']), tau), polyak_reference(want[1], _flat(c['q']), tau)]
        got = b.ddpg_targets()
        for g, w, live, old in zip(got, want, (c['pol'], c['q']), (c['tpol'], c['tq'])):
            if tau == 0.005:
                assert g.tobytes() == w.tobytes() and not _same(g, _flat(old)) and not _same(g, _flat(live))
            else:
                assert np.array_equal(g, w) and np.array_equal(g, _flat(live) if tau == 1.0 else _flat(old))
    assert _same(_blob(b), _flat(c['pol'])) and _same(b.get_q_mlp(), _flat(c['q']))


# ---- 3. Gaussian data within the a-priori bound -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 257])
def test_gaussian_data_within_the_a_priori_bound(B, batch_of):
    """Gaussian networks, uniform rows and labels: the critic's loss, y, q and every gradient element, and the actor's statistics, dA
    and every gradient element, lie within the computed bound of the float64 references (ddpg_cases.critic_bound / actor_bound: the
    trainer's Higham bound extended by the TD target's roundings and by the input-gradient chain), with the ReLU margins and the
    gate's margin asserted > 0. B = 257 is past FIT_SPLIT_ROWS: the batch sums go through two slabs and k_fit_reduce."""
    pw, qw = [300, 37, 64, 4], [304, 37, 64, 1]
    c, idx = D.gaussian_case(pw, qw, B, seed=4, n_rows=48 if B == 8 else 300)
    cb, ab = D.critic_bound(c, idx, D.G_GAMMA, D.G_BOUND), D.actor_bound(c, idx, D.G_BOUND)
    assert cb['margin'] > 0.0 and ab['margin'] > 0.0 and ab['gate_margin'] > 0.0, (cb['margin'], ab['margin'], ab['gate_margin'])
    b = _load(batch_of(10), c)
    stats, grad, y, q = b.q_grad(idx, D.G_GAMMA, D.G_BOUND)
    err = np.abs(grad.astype(np.float64) - _flat(cb['grads']))
    print("critic %r B %d: margin %.3e, loss err %.3e (bound %.3e), max grad err %.3e, max err / bound %.3f, max |grad| %.3e" % (
        qw, B, cb['margin'], abs(stats[0] - cb['loss']), cb['dloss'], err.max(), (err[cb['bound'] > 0] / cb['bound'][cb['bound'] > 0]).max(), np.abs(grad).max()))
    assert np.isfinite(grad).all() and np.abs(_flat(cb['grads'])).max() > 1e-4
    assert abs(stats[0] - cb['loss']) <= cb['dloss']
    assert (np.abs(y.astype(np.float64) - cb['y']) <= cb['dy']).all() and (np.abs(q.astype(np.float64) - cb['q']) <= cb['dq']).all()
    assert abs(stats[1] - cb['q'].mean()) <= cb['dq'].mean() + 1e-14 and abs(stats[2] - cb['y'].mean()) <= cb['dy'].mean() + 1e-14
    assert (err <= cb['bound']).all(), (np.nonzero(err > cb['bound'])[0][:8], err.max())
    stats, grad, dA = b.dpg_grad(idx, D.G_BOUND)
    err = np.abs(grad.astype(np.float64) - _flat(ab['grads']))
    print("actor %r B %d: margin %.3e, gate margin %.3e, gated %d of %d, max dA err %.3e, max grad err %.3e, max err / bound %.3f, max |grad| %.3e" % (
        pw, B, ab['margin'], ab['gate_margin'], ab['gated'], 4 * B, np.abs(dA - ab['dA']).max(), err.max(), (err[ab['bound'] > 0] / ab['bound'][ab['bound'] > 0]).max(),
        np.abs(grad).max()))
    assert np.isfinite(grad).all() and np.abs(_flat(ab['grads'])).max() > 1e-5 and 0 < ab['gated'] < 4 * B
    assert stats[1] == ab['stats'][1] and (np.abs(stats - ab['stats']) <= ab['dstats']).all(), (stats, ab['stats'], ab['dstats'])
    assert (np.abs(dA.astype(np.float64) - ab['dA']) <= ab['ddA']).all()
    assert (err <= ab['bound']).all(), (np.nonzero(err > ab['bound'])[0][:8], err.max())


# ---- 4. a pin to the existing trainer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 257])
def test_zero_action_columns_reproduce_the_value_trainer(B, batch_of):
    """A Q network whose layer-0 action columns are zero is the value network of its other columns: with gamma = 0 and rew == ret the
    critic's loss and gradient reproduce clothhip_value_fit_grad's BYTES on every shared block -- the four zero products leave a
    finite accumulator's bits alone, and X's observation columns are the dataset's. The action columns' own gradient, dZ_0^T a, is
    non-zero and lies within the computed bound of the reference."""
    pw, qw = [300, 37, 64, 4], [304, 37, 64, 1]
    c, idx = D.gaussian_case(pw, qw, B, seed=6, n_rows=48 if B == 8 else 300, zero_action_columns=True)
    W0 = c['q'][0][0]
    assert not W0[:, -4:].any() and W0[:, :-4].all()
    val = [(np.ascontiguousarray(W0[:, :-4]), c['q'][0][1])] + c['q'][1:]
    b = _load(batch_of(10), c)
    b.set_value_mlp(val)
    b.fit_set_returns(c['rew'])
    v_loss, v_grad = b.value_grad(idx)
    stats, grad, y, q = b.q_grad(idx, 0.0, D.G_BOUND)
    assert stats[0] == v_loss and _same(y, c['rew'][idx]) and _same(q, b.value_predict(idx))
    n0 = 37 * 304
    g0 = grad[:n0].reshape(37, 304)
    assert _same(g0[:, :-4], v_grad[:37 * 300].reshape(37, 300)) and _same(grad[n0:], v_grad[37 * 300:])
    cb = D.critic_bound(c, idx, 0.0, D.G_BOUND)
    assert cb['margin'] > 0.0
    ref, bound = cb['grads'][0][0][:, -4:], cb['bound'][:n0].reshape(37, 304)[:, -4:]
    err = np.abs(g0[:, -4:].astype(np.float64) - ref)
    assert np.abs(ref).max() > 1e-4 and (err <= bound).all() and bound.max() < 0.05 * np.abs(ref).max(), (err.max(), bound.max())


# ---- 5. composition: n steps in one call, the same steps one call at a time, the optimizers restated ---------------------------------------
@pytest.mark.parametrize("name,hyper", [OPTIMIZERS[0], OPTIMIZERS[2]], ids=["adam", "sgd_momentum"])
def test_a_fit_is_its_steps_one_call_at_a_time(name, hyper):
    """Three ddpg_fit steps on one handle; on a second the same steps as q_fit (1 step), dpg_fit (1 step), ddpg_polyak -- where every
    optimizer step is also the numpy restatement of the header's update applied to the gradient q_grad / dpg_grad return just before
    it (so the moments and the 1-based step counts are the restatement's), the actor's gradient is taken against the UPDATED critic,
    and the soft update is polyak_reference's. Both handles then hold the same bytes in the policy, the Q network and both targets,
    and return the same statistics; a fourth step on both (the moments and step counts continue) leaves them equal again."""
    from gym_cloth_amd.policies import polyak_reference
    pw, qw = [300, 37, 64, 4], [304, 37, 64, 1]
    c, _ = D.gaussian_case(pw, qw, 8, seed=7, n_rows=48)
    r = np.random.RandomState(3)
    table = r.randint(0, 47, size=(4, 9)).astype(np.int32)                      # (row 47 is the leaf)
    q_hyper = dict(hyper, lr=2.0 * hyper['lr'])
    one, steps = _load(_new_batch(10), c), _load(_new_batch(10), c)
    whole = one.ddpg_fit(table[:3], D.G_GAMMA, 0.25, D.G_BOUND, policy_hyper=hyper, q_hyper=q_hyper)
    th_p, th_q, tg_p, tg_q = _states(steps)
    mom = {k: (np.zeros_like(t), np.zeros_like(t)) for k, t in (('p', th_p), ('q', th_q))}
    for s in range(3):
        st_q, g_q, _, _ = steps.q_grad(table[s], D.G_GAMMA, D.G_BOUND)
        assert np.array_equal(steps.q_fit(table[s:s + 1], D.G_GAMMA, D.G_BOUND, **q_hyper), st_q[None])
        th_q, m, v = _restated_step(q_hyper, th_q, mom['q'][0], mom['q'][1], g_q, s + 1)
        mom['q'] = (m, v)
        assert _same(steps.get_q_mlp(), th_q), (name, s)
        st_p, g_p, _ = steps.dpg_grad(table[s], D.G_BOUND)
        assert np.array_equal(steps.dpg_fit(table[s:s + 1], D.G_BOUND, **hyper), st_p[None])
        th_p, m, v = _restated_step(hyper, th_p, mom['p'][0], mom['p'][1], g_p, s + 1)
        mom['p'] = (m, v)
        assert _same(_blob(steps), th_p), (name, s)
        steps.ddpg_polyak(0.25)
        tg_p, tg_q = polyak_reference(tg_p, th_p, 0.25), polyak_reference(tg_q, th_q, 0.25)
        assert np.array_equal(whole[s], np.concatenate([st_q, st_p])), (name, s)
    for a, w in zip(_states(steps), (th_p, th_q, tg_p, tg_q)):
        assert _same(a, w)
    for a, w in zip(_states(one), _states(steps)):
        assert a.tobytes() == w.tobytes()
    assert np.abs(th_p - _flat(c['pol'])).max() > 1e-4 and np.abs(th_q - _flat(c['q'])).max() > 1e-4 and np.isfinite(whole).all()
    more = one.ddpg_fit(table[3:], D.G_GAMMA, 0.25, D.G_BOUND, policy_hyper=hyper, q_hyper=q_hyper)
    again = np.concatenate([steps.q_fit(table[3:], D.G_GAMMA, D.G_BOUND, **q_hyper), steps.dpg_fit(table[3:], D.G_BOUND, **hyper)], axis=1)
    steps.ddpg_polyak(0.25)
    assert np.array_equal(more, again)
    for a, w in zip(_states(one), _states(steps)):
        assert a.tobytes() == w.tobytes()
    # q_fit_reset restarts the critic's moments and step count, and nothing of the policy's
    one.q_fit_reset()
    _, g_q, _, _ = one.q_grad(table[0], D.G_GAMMA, D.G_BOUND)
    th = one.get_q_mlp()
    one.q_fit(table[:1], D.G_GAMMA, D.G_BOUND, **q_hyper)
    assert _same(one.get_q_mlp(), _restated_step(q_hyper, th, np.zeros_like(th), np.zeros_like(th), g_q, 1)[0])
    one.close(); steps.close()


def _layers_of(blob, widths):
    """_flat's inverse: the blob as [(W, b)] of a network of these widths."""
    layers, at = [], 0
    for n_in, n_out in zip(widths[:-1], widths[1:]):
        layers.append((blob[at:at + n_out * n_in].reshape(n_out, n_in).copy(), blob[at + n_out * n_in:at + n_out * n_in + n_out].copy()))
        at += n_out * n_in + n_out
    assert at == blob.size
    return layers


@pytest.mark.parametrize("name,hyper", [OPTIMIZERS[0], OPTIMIZERS[2]], ids=["adam", "sgd_momentum"])
def test_different_losses_continue_one_optimizers_step_count(name, hyper):
    """On ONE handle: fit (2 steps), dpg_fit (1 step), fit_ppo (1 step, fixed sigma, after a snapshot), ddpg_fit (2 steps). Before every
    step a second handle, a probe with the same dataset, is given the restated networks and targets and returns the corresponding
    *_grad entry's gradient on the step's rows; after each call the policy's blob equals by bytes the restated optimizer step of that
    gradient with t = 1 .. 6 and the moments carried over from loss to loss, and the Q blob the restated steps t = 1, 2 of its own
    optimizer. After fit_reset the next DPG step is the t = 1 step from zero moments."""
    from gym_cloth_amd.policies import polyak_reference
    pw, qw, B, sigma, tau = [300, 5, 4], [304, 5, 1], 8, 0.3, 0.25
    c, _ = D.gaussian_case(pw, qw, B, seed=7, n_rows=48)
    table = np.random.RandomState(3).randint(0, 47, size=(7, B)).astype(np.int32)      # (row 47 is the leaf)
    w = np.random.RandomState(1).normal(size=48).astype(np.float32)
    q_hyper = dict(hyper, lr=2.0 * hyper['lr'])
    b, probe = _load(_new_batch(10), c), _load(_new_batch(10), c)
    for x in (b, probe):
        x.fit_set_weights(w)
    th = dict(zip(('p', 'q', 'tp', 'tq'), _states(b)))
    mom = {k: (np.zeros_like(th[k]), np.zeros_like(th[k])) for k in ('p', 'q')}
    t = {'p': 0, 'q': 0}

    def put():
        """the restated state on the probe (a new network drops its target: all four, in this order)"""
        probe.set_policy_mlp(_layers_of(th['p'], pw))
        probe.set_q_mlp(_layers_of(th['q'], qw))
        probe.ddpg_set_targets(_layers_of(th['tp'], pw), _layers_of(th['tq'], qw))

    def restate(k, hyp, g):
        assert g.any()
        t[k] += 1
        before = th[k]
        th[k], m, v = _restated_step(hyp, th[k], mom[k][0], mom[k][1], g, t[k])
        mom[k] = (m, v)
        assert not _same(th[k], before)

    # 1. the squared error, two steps in one call: t = 1, 2
    for s in (0, 1):
        put()
        restate('p', hyper, probe.fit_grad(table[s])[1])
    b.fit(table[0:2], **hyper)
    assert _same(_blob(b), th['p']), (name, "fit")
    # 2. the deterministic policy gradient: t = 3
    put()
    restate('p', hyper, probe.dpg_grad(table[2], D.G_BOUND)[1])
    b.dpg_fit(table[2:3], D.G_BOUND, **hyper)
    assert _same(_blob(b), th['p']), (name, "dpg_fit")
    # 3. PPO's clipped surrogate under a fixed sigma, after a snapshot of the present means: t = 4
    put()
    probe.fit_snapshot_policy()
    b.fit_snapshot_policy()
    assert b.fit_get_old_means().tobytes() == probe.fit_get_old_means().tobytes()
    restate('p', hyper, probe.fit_ppo_grad(table[2], sigma)[1])
    b.fit_ppo(table[2:3], sigma, **hyper)
    assert _same(_blob(b), th['p']), (name, "fit_ppo")
    # 4. DDPG, two steps in one call: the critic's t = 1, 2, the actor's t = 5, 6 against the updated critic, then the soft update
    for s in (3, 4):
        put()
        restate('q', q_hyper, probe.q_grad(table[s], D.G_GAMMA, D.G_BOUND)[1])
        put()
        restate('p', hyper, probe.dpg_grad(table[s], D.G_BOUND)[1])
        th['tp'], th['tq'] = polyak_reference(th['tp'], th['p'], tau), polyak_reference(th['tq'], th['q'], tau)
    b.ddpg_fit(table[3:5], D.G_GAMMA, tau, D.G_BOUND, policy_hyper=hyper, q_hyper=q_hyper)
    assert t == {'p': 6, 'q': 2}
    for a, k in zip(_states(b), ('p', 'q', 'tp', 'tq')):
        assert _same(a, th[k]), (name, "ddpg_fit", k)
    # fit_reset: the next DPG step is the first step of a fresh optimizer
    b.fit_reset()
    put()
    g = probe.dpg_grad(table[5], D.G_BOUND)[1]
    b.dpg_fit(table[5:6], D.G_BOUND, **hyper)
    fresh = _restated_step(hyper, th['p'], np.zeros_like(th['p']), np.zeros_like(th['p']), g, 1)[0]
    assert _same(_blob(b), fresh)
    restate('p', hyper, g)                                                       # ... and not the seventh of the old one
    assert not _same(fresh, th['p'])
    b.close(); probe.close()


# ---- 6. the gate freezes ------------------------------------------------------------------------------------------------------------------
def test_the_gate_freezes_a_policy_pushed_further_out(batch_of):
    """Twelve rows whose means lie beyond +bound under a critic that is linear in the action with positive coefficients: the step up
    the critic's gradient would push every component further out, the gate holds all of them, the gradient is zero and ten actor steps
    leave the policy's blob byte-identical -- and its moments zero: a squared-error step afterwards equals, under SGD with momentum,
    the same step on a handle that never ran an actor step. With the critic's sign flipped the same ten steps move the policy inward."""
    r = np.random.RandomState(2)
    rows, labels = r.uniform(-1, 1, size=(12, 300)).astype(np.float32), r.uniform(-1, 1, size=(12, 4))
    pol = [((0.01 * r.normal(size=(4, 300))).astype(np.float32), np.array([1.5, 2.0, 1.25, 3.0], dtype=np.float32))]
    W = np.zeros((1, 304), dtype=np.float32)
    W[0, -4:] = [1.0, 0.5, 2.0, 0.25]
    sgd, table = OPTIMIZERS[2][1], np.tile(np.arange(12, dtype=np.int32), (10, 1))
    b, twin = batch_of(10), _new_batch(10)
    for x in (b, twin):
        x.fit_append(rows, labels)
        x.fit_set_transitions(np.zeros(12, dtype=np.float32), np.full(12, D.TERMINAL))
        x.set_policy_mlp(pol)
    assert (b.fit_predict(np.arange(12)) > 1.0).all()
    for name, hyper in (OPTIMIZERS[0], OPTIMIZERS[2]):
        b.set_policy_mlp(pol)
        b.set_q_mlp([(W, np.zeros(1, dtype=np.float32))])
        stats, grad, dA = b.dpg_grad(np.arange(12), 1.0)
        assert stats[1] == 1.0 and not grad.any() and (dA < 0).all() and stats[0] == -float(W.sum())      # Q saw the clamped action (1, 1, 1, 1)
        out = b.dpg_fit(table, 1.0, **hyper)
        assert (out[:, 1] == 1.0).all() and _same(_blob(b), _flat(pol)), name
    assert b.fit(table[:1], **sgd).tobytes() == twin.fit(table[:1], **sgd).tobytes() and _blob(b).tobytes() == _blob(twin).tobytes()
    b.set_policy_mlp(pol)
    b.set_q_mlp([(-W, np.zeros(1, dtype=np.float32))])
    out = b.dpg_fit(table, 1.0, **ADAM)
    assert out[0, 1] == 0.0 and (b.dpg_grad(np.arange(12), 1.0)[2] > 0).all()
    moved = b.get_policy_mlp(0, b._mlp_n_params)[-4:]
    assert (moved < pol[0][1]).all() and not _same(_blob(b), _flat(pol))
    twin.close()


# ---- 7. independence ----------------------------------------------------------------------------------------------------------------------
def test_ddpg_touches_nothing_else_and_invalidates_exactly_its_targets():
    from gym_cloth_amd import _lib
    pw, qw = [300, 37, 64, 4], [304, 37, 64, 1]
    c, idx = D.gaussian_case(pw, qw, 8, seed=8, n_rows=48)
    b = _load(_new_batch(10), c)
    val, ls = _random_layers([300, 6, 1], 9), np.array([-1.0, -0.5, 0.25, 0.0], dtype=np.float32)
    b.set_value_mlp(val)
    b.set_policy_log_sigma(ls)
    w = np.random.RandomState(1).normal(size=48).astype(np.float32)
    b.fit_set_weights(w)
    b.fit_set_returns(c['rew'])
    b.fit_snapshot_policy()
    table = np.random.RandomState(5).randint(0, 47, size=(3, 8)).astype(np.int32)

    def others():
        """the value network, the head, every dataset column, and what a squared-error, a value and a PPO step return from a reset"""
        cols = (b.fit_data(), b.fit_get_weights(), b.fit_get_transitions(), b.fit_get_returns(), b.fit_get_old_means(), b.fit_get_old_log_sigma())
        return [b.get_value_mlp(), b.get_policy_log_sigma(), b.fit_grad(idx), b.value_grad(idx), b.fit_ppo_grad(idx, 0.3), b.fit_ppo_sigma_grad(idx)] + [cols]

    def flat(o):
        return b"".join(np.ascontiguousarray(x).tobytes() for x in _leaves(o))
    before = flat(others())
    pol0 = _blob(b)
    b.q_grad(idx, D.G_GAMMA, D.G_BOUND); b.q_fit(table, D.G_GAMMA, D.G_BOUND, **ADAM); b.ddpg_polyak(0.1); b.ddpg_last_tables(8)
    b.q_fit_reset(); b.ddpg_sync_targets(); b.dpg_grad(idx, D.G_BOUND)
    assert _same(_blob(b), pol0) and flat(others()) == before                  # critic steps, polyak, sync: no bit of anything else, the policy among it
    # the policy's steps under another loss continue from a reset as if DDPG had not been: twin handles
    twin = _new_batch(10)
    twin.fit_append(c['rows'], c['labels'], weights=w)
    twin.set_policy_mlp(c['pol'])
    b.fit_reset(); b.set_policy_mlp(c['pol']); b.ddpg_sync_targets()
    b.ddpg_fit(table, D.G_GAMMA, 0.1, D.G_BOUND, policy_hyper=ADAM, q_hyper=ADAM)
    assert not _same(_blob(b), _flat(c['pol']))
    b.set_policy_mlp(c['pol'])                                                 # (restarts the policy's optimizer)
    assert b.fit(table, **ADAM).tobytes() == twin.fit(table, **ADAM).tobytes() and _blob(b).tobytes() == _blob(twin).tobytes()
    assert _same(b.get_value_mlp(), _flat(val)) and _same(b.get_policy_log_sigma(), ls)
    # invalidation: a new policy drops the target policy alone, a new Q network the target Q alone, a population refuses everything
    L, h = b._L, b._h
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    tp, tq = np.zeros(b._mlp_n_params, dtype=np.float32), np.zeros(b._q_n_params, dtype=np.float32)
    b.ddpg_sync_targets()
    kept_q = b.ddpg_targets()[1]
    b.set_policy_mlp(c['tpol'])
    assert L.clothhip_ddpg_get_targets(h, fp(tp), None) == _lib.ESTATE and L.clothhip_ddpg_get_targets(h, None, fp(tq)) == _lib.OK and _same(tq, kept_q)
    with pytest.raises(_lib.ClothHipError):
        b.q_grad(idx, D.G_GAMMA, D.G_BOUND)
    with pytest.raises(_lib.ClothHipError):
        b.ddpg_polyak(0.1)
    b.dpg_grad(idx, D.G_BOUND)                                                 # the actor reads no target
    b.ddpg_sync_targets()
    kept_p = b.ddpg_targets()[0]
    assert _same(kept_p, _flat(c['tpol']))
    b.set_q_mlp(c['tq'])
    assert L.clothhip_ddpg_get_targets(h, None, fp(tq)) == _lib.ESTATE and L.clothhip_ddpg_get_targets(h, fp(tp), None) == _lib.OK and _same(tp, kept_p)
    with pytest.raises(_lib.ClothHipError):
        b.ddpg_fit(table, D.G_GAMMA, 0.1, D.G_BOUND)
    b.ddpg_set_targets(None, c['q'])
    assert _same(b.ddpg_targets()[1], _flat(c['q'])) and np.isfinite(b.q_grad(idx, D.G_GAMMA, D.G_BOUND)[0]).all()
    b.set_value_mlp(None); b.set_policy_log_sigma(None)                        # neither is DDPG's business
    assert np.isfinite(b.q_grad(idx, D.G_GAMMA, D.G_BOUND)[0]).all()
    b.set_policy_population([c['pol'], c['tpol']], np.zeros(1, dtype=np.int32))
    p = _lib.ClothDdpgParams(0.9, 0.1, 1.0, 0)
    adam = _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    ip, st = _lib.i32p(np.ascontiguousarray(idx, dtype=np.int32)), np.zeros(6)
    for rc in (L.clothhip_ddpg_sync_targets(h), L.clothhip_ddpg_set_targets(h, fp(tp), fp(tq)), L.clothhip_ddpg_polyak(h, 0.1),
               L.clothhip_q_fit_grad(h, C.byref(p), ip, 8, None, _lib.dp(st), None, None), L.clothhip_q_fit(h, C.byref(adam), C.byref(p), ip, 1, 8, None),
               L.clothhip_policy_fit_dpg_grad(h, C.byref(p), ip, 8, None, _lib.dp(st), None), L.clothhip_policy_fit_dpg(h, C.byref(adam), C.byref(p), ip, 1, 8, None),
               L.clothhip_ddpg_fit(h, C.byref(adam), C.byref(adam), C.byref(p), ip, 1, 8, None), L.clothhip_ddpg_get_targets(h, fp(tp), None)):
        assert rc == _lib.ESTATE
    assert _same(b.get_q_mlp(), _flat(c['tq']))                                # the Q network itself stays, as the value network does
    b.close(); twin.close()


def _leaves(o):
    if isinstance(o, (list, tuple)):
        for x in o:
            for y in _leaves(x):
                yield y
    else:
        yield np.asarray(o)


# ---- 8. every refusal ---------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from gym_cloth_amd import _lib
    v = _env("f32", n_side=10, max_actions=2)
    v.reset()
    b, L, h = v.batch, v.batch._L, v.batch._h
    pw, qw = [300, 5, 4], [304, 5, 1]
    c = D.exact_case(pw, qw, 1.0, 0)
    _load(b, c)
    idx = np.ascontiguousarray(D.IDX8, dtype=np.int32)
    table = np.tile(idx, (2, 1))
    b.q_fit(table, 0.9, 1.0, **ADAM); b.dpg_fit(table, 1.0, **ADAM)            # moments and step counts exist
    twin = _load(_new_batch(10), c)
    twin.q_fit(table, 0.9, 1.0, **ADAM); twin.dpg_fit(table, 1.0, **ADAM)
    snap = [x.copy() for x in _states(b)]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = _lib.i32p
    P_ = _lib.ClothDdpgParams
    ok, adam = P_(0.9, 0.1, 1.0, 0), _lib.ClothFitParams(0.0, ADAM['lr'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], 0.0)
    g_q, g_p, st, y8 = np.zeros(b._q_n_params, dtype=np.float32), np.zeros(b._mlp_n_params, dtype=np.float32), np.zeros(12), np.zeros(32, dtype=np.float32)

    def every(p=ok, ix=idx, B=8, n_steps=1, fit=adam, grads_only=False):
        """the status of every entry that takes a minibatch (grads_only: of the two that update nothing), for one set of arguments"""
        pp, ff, ii = (C.byref(p) if p is not None else None), (C.byref(fit) if fit is not None else None), (ip(ix) if ix is not None else None)
        calls = [lambda: L.clothhip_q_fit_grad(h, pp, ii, B, fp(g_q), _lib.dp(st), fp(y8), fp(y8)), lambda: L.clothhip_policy_fit_dpg_grad(h, pp, ii, B, fp(g_p), _lib.dp(st), fp(y8)),
                 lambda: L.clothhip_q_fit(h, ff, pp, ii, n_steps, B, _lib.dp(st)), lambda: L.clothhip_policy_fit_dpg(h, ff, pp, ii, n_steps, B, _lib.dp(st)),
                 lambda: L.clothhip_ddpg_fit(h, ff, ff, pp, ii, n_steps, B, _lib.dp(st))]
        return [call() for call in (calls[:2] if grads_only else calls)]

    def unchanged():
        for a, w in zip(_states(b), snap):
            assert a.tobytes() == w.tobytes()

    assert every() == [0] * 5
    snap = [x.copy() for x in _states(b)]
    twin.q_fit(table[:1], 0.9, 1.0, **ADAM); twin.dpg_fit(table[:1], 1.0, **ADAM)
    twin.q_fit(table[:1], 0.9, 1.0, **ADAM); twin.dpg_fit(table[:1], 1.0, **ADAM); twin.ddpg_polyak(0.1)
    for a, w in zip(_states(b), _states(twin)):
        assert a.tobytes() == w.tobytes()
    # B, the indices, a leaf, NULL tables
    assert every(B=0) == [_lib.EINVAL] * 5 and every(B=_lib.FIT_MAX_BATCH + 1) == [_lib.EINVAL] * 5
    assert every(ix=None) == [_lib.EINVAL] * 5 and every(p=None) == [_lib.EINVAL] * 5
    assert every(fit=None)[2:] == [_lib.EINVAL] * 3
    for bad in (12, -1):
        assert every(ix=np.array([0, 1, 2, 3, 4, 5, 6, bad], dtype=np.int32)) == [_lib.EINVAL] * 5
    assert every(ix=np.array([0, 1, 2, 3, 4, 5, 6, 10], dtype=np.int32)) == [_lib.EINVAL] * 5          # row 10 is the leaf
    assert b"leaf" in L.clothhip_last_error()
    assert every(n_steps=-1)[2:] == [_lib.EINVAL] * 3 and every(n_steps=0)[2:] == [0] * 3
    # gamma, tau, act_bound, flags
    for p in (P_(np.nan, 0.1, 1.0, 0), P_(1.5, 0.1, 1.0, 0), P_(-0.1, 0.1, 1.0, 0), P_(np.inf, 0.1, 1.0, 0), P_(0.9, np.nan, 1.0, 0), P_(0.9, 1.5, 1.0, 0), P_(0.9, -1e-9, 1.0, 0),
              P_(0.9, 0.1, 0.0, 0), P_(0.9, 0.1, -1.0, 0), P_(0.9, 0.1, np.nan, 0), P_(0.9, 0.1, 1.0, 1), P_(0.9, 0.1, 1.0, -1)):
        assert every(p=p) == [_lib.EINVAL] * 5, (p.gamma, p.tau, p.act_bound, p.flags)
    assert every(p=P_(0.0, 0.0, INF, 0), grads_only=True) == [0, 0] and every(p=P_(1.0, 1.0, 1e-3, 0), n_steps=0) == [0] * 5      # the ends of the ranges are inside
    for tau in (np.nan, np.inf, -0.1, 1.5):
        assert L.clothhip_ddpg_polyak(h, tau) == _lib.EINVAL
    for field, bad in (("optimizer", 2.0), ("lr", -1.0), ("lr", np.nan), ("beta1", 1.0), ("beta2", 1.5), ("eps", np.inf), ("momentum", -0.1)):
        f = _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
        setattr(f, field, bad)
        assert every(fit=f, n_steps=1)[2:] == [_lib.EINVAL] * 3, field
    # the Q network's shape rules: a refused call keeps the earlier one
    wd, blob = np.array(qw, dtype=np.int32), _flat(c['q'])
    for widths, n_par in ((np.array([304, 5, 4], dtype=np.int32), blob.size), (np.array([300, 5, 1], dtype=np.int32), blob.size), (np.array([304, 257, 1], dtype=np.int32), blob.size),
                          (wd, blob.size - 1)):
        assert L.clothhip_set_q_mlp(h, 2, ip(widths), fp(blob), n_par) == _lib.EINVAL
    assert L.clothhip_set_q_mlp(h, 5, ip(np.array([304, 5, 5, 5, 5, 1], dtype=np.int32)), fp(blob), blob.size) == _lib.EINVAL
    assert L.clothhip_set_q_mlp(h, 2, ip(wd), None, blob.size) == _lib.EINVAL and L.clothhip_set_q_mlp(h, 2, None, fp(blob), blob.size) == _lib.EINVAL
    assert L.clothhip_get_q_mlp(h, fp(g_q), g_q.size + 1) == _lib.EINVAL and L.clothhip_get_q_mlp(h, None, g_q.size) == _lib.EINVAL
    assert L.clothhip_ddpg_last_tables(h, 9, None, None, None) == _lib.EINVAL
    unchanged()
    # a launch in flight
    nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, E, 4)))
    assert every() == [_lib.ESTATE] * 5
    for rc in (L.clothhip_ddpg_polyak(h, 0.1), L.clothhip_ddpg_sync_targets(h), L.clothhip_ddpg_get_targets(h, fp(g_p), fp(g_q)), L.clothhip_ddpg_set_targets(h, fp(g_p), fp(g_q)),
               L.clothhip_q_fit_reset(h), L.clothhip_set_q_mlp(h, 2, ip(wd), fp(blob), blob.size), L.clothhip_set_q_mlp(h, 0, None, None, 0), L.clothhip_get_q_mlp(h, fp(g_q), g_q.size),
               L.clothhip_ddpg_last_tables(h, 8, None, None, None)):
        assert rc == _lib.ESTATE
    b.run_actions_end()
    unchanged()
    # the moments and step counts too: the next step on both handles gives the same bytes
    out = b.ddpg_fit(table[:1], 0.9, 0.1, 1.0, policy_hyper=ADAM, q_hyper=ADAM)
    want = twin.ddpg_fit(table[:1], 0.9, 0.1, 1.0, policy_hyper=ADAM, q_hyper=ADAM)
    assert out.tobytes() == want.tobytes()
    for a, w in zip(_states(b), _states(twin)):
        assert a.tobytes() == w.tobytes()
    # no targets, no Q network, no policy network, an empty dataset (these change the handle, so they come last)
    b.set_q_mlp(c['q'])
    assert every() == [_lib.ESTATE, 0, _lib.ESTATE, 0, _lib.ESTATE] and L.clothhip_ddpg_polyak(h, 0.1) == _lib.ESTATE
    b.set_q_mlp(None)
    assert every() == [_lib.ESTATE] * 5 and L.clothhip_ddpg_sync_targets(h) == _lib.ESTATE and L.clothhip_get_q_mlp(h, fp(g_q), g_q.size) == _lib.ESTATE
    assert L.clothhip_ddpg_set_targets(h, None, fp(g_q)) == _lib.ESTATE and L.clothhip_ddpg_last_tables(h, 8, None, None, None) == _lib.ESTATE and L.clothhip_q_fit_reset(h) == _lib.OK
    b.set_q_mlp(c['q']); b.set_policy_mlp(None)
    assert every() == [_lib.ESTATE] * 5 and L.clothhip_ddpg_sync_targets(h) == _lib.ESTATE and L.clothhip_ddpg_set_targets(h, fp(g_p), None) == _lib.ESTATE
    b.set_policy_mlp(c['pol']); b.ddpg_sync_targets(); b.fit_clear()
    assert every() == [_lib.ESTATE] * 5 and L.clothhip_ddpg_polyak(h, 0.1) == _lib.OK
    twin.close()
    v.close()


# ---- 9. demos.ddpg_fit ----------------------------------------------------------------------------------------------------------------------
def _env8():
    """test_gpu_dagger's _env with 8 cloths of 10 x 10, episodes of two actions."""
    from gym_cloth_amd.envs import ClothVecEnv
    from test_gpu_env import base_cfg
    cfg = base_cfg("tier1", 1337)
    cfg["cloth"]["num_width_points"] = cfg["cloth"]["num_height_points"] = 10
    cfg["env"]["force_grab"] = True
    cfg["env"]["max_actions"] = 2
    v = ClothVecEnv(cfg, n_envs=8, precision="f32", consume_domrand_draws=False)
    v.seed([1337 + e for e in range(8)])
    return v


def _ddpg_run():
    from gym_cloth_amd.demos import actor_critic_collect, ddpg_fit
    from gym_cloth_amd.policies import DeviceNoise, MLPTrainer, QTrainer
    v = _env8()
    v.reset()
    tr = MLPTrainer(v, _layers([3 * v.P, 5, 4], 21), lr=1e-3)
    qc = QTrainer(v, _layers([3 * v.P + 4, 6, 1], 22), lr=1e-2)
    cols = [actor_critic_collect(v, tr, n_actions=3, policy_noise=DeviceNoise(13 + i, sigma=0.05), slots_per_launch=3) for i in range(2)]
    fit = ddpg_fit(v, tr, qc, cols[1], gamma=0.9, tau=0.05, n_steps=6, batch_size=8, seed=0, act_bound=1.0)
    again = ddpg_fit(v, tr, qc, cols[1], gamma=0.9, tau=0.05, n_steps=2, batch_size=8, seed=1, act_bound=1.0)
    res = (cols, fit, again, _states(v.batch), v.batch.fit_get_transitions()[1])
    v.close()
    return res


def test_ddpg_fit_samples_the_whole_replay_buffer():
    """Two collections of 8 cloths of 10 x 10, then ONE fit: its minibatches come from both collections, hold no leaf, its statistics
    are finite, the first call synced the targets and the second did not; two runs give the same bytes."""
    from gym_cloth_amd import _lib
    cols, fit, again, states, nxt = _ddpg_run()
    first2 = cols[1]['first']
    assert first2 == cols[0]['appended'] + cols[0]['open_rows'] and fit['collected'] == cols[1]['appended']
    assert fit['stats'].shape == (6, 6) and np.isfinite(fit['stats']).all() and fit['rows'].shape == (6, 8)
    assert (fit['rows'] < first2).any() and (fit['rows'] >= first2).any()
    assert not (nxt[fit['rows']] == _lib.FIT_NEXT_NONE).any() and (nxt == _lib.FIT_NEXT_NONE).any() and np.array_equal(fit['replay'], np.nonzero(nxt != _lib.FIT_NEXT_NONE)[0])
    assert fit['synced'] and not again['synced'] and not np.array_equal(states[0], states[2]) and not np.array_equal(states[1], states[3])
    cols_b, fit_b, again_b, states_b, nxt_b = _ddpg_run()
    assert fit_b['stats'].tobytes() == fit['stats'].tobytes() and again_b['stats'].tobytes() == again['stats'].tobytes() and np.array_equal(nxt, nxt_b)
    for a, w in zip(states, states_b):
        assert a.tobytes() == w.tobytes()
