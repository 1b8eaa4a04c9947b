"""GPU tests of DDPG from demonstrations (k_fit_dpg_bc and k_fit_concat's expert mode in csrc/cloth_fit_ddpg.hpp, the expert
column of the dataset, clothhip_policy_fit_dpg_bc*, clothhip_ddpg_fit_bc): the column and its append source; the anchor to plain DDPG by
bytes; the kernel by bytes against its numpy restatement; exact data EQUAL to the float64 reference, a tie among it; Gaussian data
within the a-priori bound; pure cloning against the squared-error trainer; isolation and the one-call-at-a-time decomposition; every
refusal; demos over 8 cloths. tests/ddpg_bc_cases.py holds the cases, tests/test_ddpg_bc_host.py checks their preconditions on the CPU.
Every comparison is array_equal or by bytes unless it says otherwise."""
import ctypes as C

import numpy as np
import pytest

import ddpg_bc_cases as K
import ddpg_cases as D
from test_gpu_dagger import _layers
from test_gpu_ddpg import _env8, _leaves, _load, _same, _states, batch_of      # noqa: F401  (batch_of: the module's fixture)
from test_gpu_policy_fit import ADAM, OPTIMIZERS, _blob, _flat, _new_batch

pytestmark = pytest.mark.gpu

INF = float("inf")
FILL = np.uint32(0x7fc00000)


def _load_bc(b, c):
    """test_gpu_ddpg's _load, then the case's expert column."""
    _load(b, c)
    b.fit_set_expert(c['expert'])
    assert b.fit_expert().tobytes() == c['expert'].tobytes()
    return b


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ---- 1. the column and its append source ---------------------------------------------------------------------------------------------------
def _armed_launch(v, armed=True):
    """One launch of 3 slots over the 8 cloths from reset, every table on the device; armed: the highest-point expert beside the policy
    (the oracle-corner expert is defined for 25 x 25 cloths only), taking the action over on a checkerboard. -> (rows int32[n, 3] of the slots that ran, out)."""
    from gym_cloth_amd.envs import slot_start_sources
    from gym_cloth_amd.policies import MLPTrainer
    v.reset()
    tr = MLPTrainer(v, _layers([3 * v.P, 5, 4], 21))
    v.batch.fit_hold()
    mix = (np.add.outer(np.arange(3), np.arange(8)) % 2).astype(bool)
    kw = dict(expert="highest_point", expert_mix=mix, expert_choices=(np.add.outer(np.arange(3), np.arange(8)) % 3).astype(np.int32)) if armed else {}
    out = v.step_many(policy="mlp", n_actions=3, want_obs="device", **kw)
    t_, e_ = np.nonzero(out["ran"])
    rows = np.concatenate([slot_start_sources(out)[t_, e_], (t_ * 8 + e_)[:, None].astype(np.int32)], axis=1)
    return tr, rows, out


def test_the_expert_column_and_its_append_source():
    from gym_cloth_amd import _lib
    a, twin = _env8(), _env8()
    tr_a, rows, out = _armed_launch(a)
    tr_t, rows_t, out_t = _armed_launch(twin)
    assert np.array_equal(rows, rows_t) and len(rows) >= 16 and out["expert_took"].any() and not out["expert_took"].all()
    b, t = a.batch, twin.batch
    n = len(rows)
    # the new source on a; the two existing ones on the twin, one behind the other
    assert tr_a.append_launch(rows, labels="action+expert") == n
    assert tr_t.append_launch(rows, labels="action") == n and tr_t.append_launch(rows, labels="expert") == 2 * n
    obs_a, lab_a = b.fit_data()
    obs_t, lab_t = t.fit_data()
    assert obs_a.tobytes() == obs_t[:n].tobytes() and lab_a.tobytes() == lab_t[:n].tobytes()
    assert b.fit_expert().tobytes() == lab_t[n:].tobytes() and K.expert_mask(b.fit_expert()).all()
    assert lab_a.tobytes() != b.fit_expert().tobytes()                         # the learner acted on half the slots: two different columns
    took = out["expert_took"][np.nonzero(out["ran"])]
    assert np.array_equal(lab_a[took], b.fit_expert()[took])                   # where the expert acted, the executed action IS its action
    assert b.fit_get_weights().tobytes() == t.fit_get_weights()[:n].tobytes()
    # defaults after every existing source: the device routes, a leaf, the host route
    assert (t.fit_expert().view(np.uint32) == FILL).all()
    t.fit_append_launch(np.array([[_lib.FIT_SRC_SLOTS, 0, 0]]), labels="zero")
    t.fit_append(obs_t[:3], lab_t[:3].astype(np.float64))
    ex = t.fit_expert()
    assert ex.shape == (2 * n + 4, 4) and (ex.view(np.uint32) == FILL).all() and not K.expert_mask(ex).any()
    # the same rows again on a, under the old sources: behind the labelled rows the column holds the fill
    assert tr_a.append_launch(rows, labels="action") == 2 * n
    assert (b.fit_expert(n).view(np.uint32) == FILL).all() and K.expert_mask(b.fit_expert(0, n)).all()
    # set / get: a round trip, clearing rows, any NaN stored as the fill
    r = np.random.RandomState(3)
    vals = r.normal(size=(n, 4)).astype(np.float32)
    vals[2] = np.array([0xffc00001] * 4, dtype=np.uint32).view(np.float32)
    vals[5] = np.nan
    b.fit_set_expert(vals, first=n)
    got = b.fit_expert(n)
    want = vals.copy()
    want[[2, 5]] = K.NO_EXPERT
    assert got.tobytes() == want.tobytes() and b.fit_expert(0, n).tobytes() == lab_t[n:].tobytes()
    raw = vals.copy()                                                          # ... and by the C entry itself, which stores the fill whatever NaN it is given
    assert b._L.clothhip_fit_data_set_expert(b._h, n, n, _fp(raw)) == _lib.OK and b.fit_expert(n).tobytes() == want.tobytes()
    # a mixed row, an infinity, a range outside: refused, the dataset byte-identical
    before = [x.tobytes() for x in _leaves([b.fit_data(), b.fit_expert(), b.fit_get_weights(), b.fit_get_transitions()])]
    for bad in ([1.0, np.nan, 0.0, 0.0], [np.nan, 1.0, 1.0, 1.0], [np.inf, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, -np.inf], [np.nan, np.nan, np.nan, np.inf]):
        tab = np.zeros((3, 4), dtype=np.float32)
        tab[1] = bad
        assert b._L.clothhip_fit_data_set_expert(b._h, 1, 3, _fp(tab)) == _lib.EINVAL, bad
        with pytest.raises(ValueError):
            b.fit_set_expert(tab, first=1)
    ok = np.zeros((3, 4), dtype=np.float32)
    assert b._L.clothhip_fit_data_set_expert(b._h, 2 * n - 2, 3, _fp(ok)) == _lib.EINVAL and b._L.clothhip_fit_data_set_expert(b._h, 0, 3, None) == _lib.EINVAL
    assert b._L.clothhip_fit_data_get_expert(b._h, 2 * n - 2, 3, _fp(ok)) == _lib.EINVAL and b._L.clothhip_fit_data_set_expert(b._h, 0, 0, None) == _lib.OK
    assert [x.tobytes() for x in _leaves([b.fit_data(), b.fit_expert(), b.fit_get_weights(), b.fit_get_transitions()])] == before
    # label source 2 stays refused; a label row outside; a launch that was not armed
    i32 = np.ascontiguousarray(rows, dtype=np.int32)
    assert b._L.clothhip_fit_data_append_launch_ex(b._h, _lib.i32p(i32), n, 2, None) == _lib.EINVAL
    far = i32.copy()
    far[0, 2] = 24
    assert b._L.clothhip_fit_data_append_launch_ex(b._h, _lib.i32p(far), n, _lib.FIT_LABEL_ACTION_EXPERT, None) == _lib.EINVAL
    tr_a2, rows2, _ = _armed_launch(a, armed=False)
    size = b.fit_size()
    assert b._L.clothhip_fit_data_append_launch_ex(b._h, _lib.i32p(np.ascontiguousarray(rows2, dtype=np.int32)), len(rows2), _lib.FIT_LABEL_ACTION_EXPERT, None) == _lib.ESTATE
    with pytest.raises(_lib.ClothHipError):
        tr_a2.append_launch(rows2, labels="action+expert")
    assert b.fit_size() == size and tr_a2.append_launch(rows2, labels="action") == size + len(rows2)
    a.close(); twin.close()


# ---- 2. the anchor to plain DDPG -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_side,B", [(10, 8), (10, 1), (10, 257), (25, 8)], ids=lambda v: str(v))
def test_unit_q_coef_and_no_cloning_is_the_parent_by_bytes(n_side, B, batch_of):
    """q_coef = 1, bc_coef = 0: dz, stats[0 .. 3) and the gradient are clothhip_policy_fit_dpg_grad's by bytes, filter on and off,
    with labelled rows and with none; three dpg_bc steps leave the policy and its moments where three policy_fit_dpg steps leave them
    (a fourth, plain, step on both handles gives the same bytes: the moments and the step count are equal too)."""
    P3 = 3 * n_side * n_side
    pw, qw = [P3, 37, 64, 4], [P3 + 4, 37, 64, 1]
    c, idx = D.gaussian_case(pw, qw, B, seed=4, n_rows=48 if B <= 48 else 300)
    c = K.with_expert(c, 4)
    b = _load(batch_of(n_side), c)
    stats, grad, dA = b.dpg_grad(idx, D.G_BOUND)
    mu = b.fit_predict(idx)
    want_dz = np.where(((mu >= D.G_BOUND) & (dA < 0)) | ((mu <= -D.G_BOUND) & (dA > 0)), np.float32(0.0), dA).astype(np.float32)
    for labelled in (False, True):
        if labelled:
            b.fit_set_expert(c['expert'])
        for q_filter in (True, False):
            got = b.dpg_bc_grad(idx, D.G_BOUND, 1.0, 0.0, q_filter)
            assert got['dz'].tobytes() == want_dz.tobytes() and got['stats'][:3].tobytes() == stats.tobytes() and got['grad'].tobytes() == grad.tobytes()
            assert got['da'].tobytes() == dA.tobytes() and (got['qe'] is None) == (not q_filter)
            m = K.expert_mask(c['expert'][idx]) if labelled else np.zeros(B, dtype=bool)
            assert got['stats'][4] == m.sum() / float(B) and (got['stats'][5] <= got['stats'][4]) and (q_filter or got['stats'][5] == got['stats'][4])
            assert (got['stats'][3] > 0) == bool(got['stats'][5] > 0)          # the loss is reported whatever bc_coef is
    if B != 8 or n_side != 10:
        return
    table = np.random.RandomState(5).randint(0, 47, size=(4, 8)).astype(np.int32)
    for name, hyper in (OPTIMIZERS[0], OPTIMIZERS[2]):
        one, two = _load_bc(_new_batch(10), c), _load_bc(_new_batch(10), c)
        s1 = one.dpg_bc_fit(table[:3], D.G_BOUND, 1.0, 0.0, True, **hyper)
        s2 = two.dpg_fit(table[:3], D.G_BOUND, **hyper)
        assert s1[:, :3].tobytes() == s2.tobytes() and _blob(one).tobytes() == _blob(two).tobytes() and not _same(_blob(one), _flat(c['pol'])), name
        assert one.dpg_fit(table[3:], D.G_BOUND, **hyper).tobytes() == two.dpg_fit(table[3:], D.G_BOUND, **hyper).tobytes()
        assert _blob(one).tobytes() == _blob(two).tobytes(), name
        one.close(); two.close()


# ---- 3. the kernel by bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_side,B", [(10, 8), (10, 1), (10, 257), (25, 8)], ids=lambda v: str(v))
def test_the_kernel_and_the_expert_concat_by_bytes(n_side, B, batch_of):
    """Gaussian data, a quarter of the rows without an expert action: dz_out, the six statistics and -- through clothhip_ddpg_last_tables
    after a filter-on call -- X of the expert concat equal dpg_bc_dz_reference and concat_reference's expert mode fed the kernel's own
    q, qe, dA and y. The policy's outputs lie outside the box of bound 1/4 on both sides and so do the expert's actions; the rows of
    10 x 10 are 16-byte aligned and those of 25 x 25 are not; at B = 257 thread 0 owns two rows."""
    from gym_cloth_amd.references import concat_reference, dpg_bc_dz_reference
    P3 = 3 * n_side * n_side
    pw, qw = [P3, 37, 64, 4], [P3 + 4, 37, 64, 1]
    c, idx = D.gaussian_case(pw, qw, B, seed=4, n_rows=48 if B <= 48 else 300)
    c = K.with_expert(c, 4)
    if B == 8:
        idx[1] = idx[5]                                                        # a repeated row
        c['expert'][idx[2]] = K.NO_EXPERT                                      # at least one row of each kind
        c['expert'][idx[3]] = [0.1, -0.6, 0.7, -0.05]
    b = _load_bc(batch_of(n_side), c)
    mu = b.fit_predict(idx)
    ae = c['expert'][idx]
    m = K.expert_mask(ae)
    if B > 1:
        assert (mu > D.G_BOUND).any() and (mu < -D.G_BOUND).any() and (ae[m] > D.G_BOUND).any() and (ae[m] < -D.G_BOUND).any() and m.any() and not m.all()
    for bound in (D.G_BOUND, INF):
        for qc, bc in ((K.G_QC, K.G_BC), (1.0, 0.5), (0.0, 1.0), (2.0, 0.0)):
            for q_filter in (True, False):
                got = b.dpg_bc_grad(idx, bound, qc, bc, q_filter)
                dz, stats = dpg_bc_dz_reference(got['da'], mu, got['q'], got['qe'], ae, bound, qc, bc)
                assert got['dz'].tobytes() == dz.tobytes() and got['stats'].tobytes() == stats.tobytes(), (bound, qc, bc, q_filter)
                assert np.isfinite(got['grad']).all() and np.isfinite(got['stats']).all()
                X, _, q_again = b.ddpg_last_tables(B, want_qn=False)
                if q_filter:
                    assert X.tobytes() == concat_reference(c['rows'], ae, idx, bound, expert=True).tobytes() and not X[~m, -4:].any()
                    assert np.isfinite(got['qe']).all() and _same(got['q'], q_again)
                    f = m & (got['qe'] > got['q'])
                    assert stats[5] == f.sum() / float(B) and (B != 257 or 0 < f.sum() < m.sum())
                else:
                    assert X.tobytes() == concat_reference(c['rows'], mu, idx, bound).tobytes()
        with pytest.raises(Exception):
            b.ddpg_last_tables(B, want_qn=True)                                # an actor's call: no target critic's values


# ---- 4. exact data -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_side,pw,qw,dens,seed,eseed", K.EXACT_BC_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_exact_data_equals_the_reference(n_side, pw, qw, dens, seed, eseed, batch_of):
    """Small-integer networks, rows and expert actions, bc_coef = 1/2, q_coef = 1 and 2, act_bound = 1; B = 8, B = 1 and a repeated
    row: the six statistics, dA, dz, q, qe and every gradient element EQUAL dpg_bc_reference's, filter on and off. The minibatch of
    eight has rows that pass the filter, rows that fail it, one exact tie and a row without an expert action
    (ddpg_bc_cases.exact_bc_asserts has the preconditions, asserted again here)."""
    from gym_cloth_amd.references import dpg_bc_reference
    c = K.exact_bc_asserts(pw, qw, dens, seed, eseed)
    b = _load_bc(batch_of(n_side), c)
    for idx in (D.IDX8, D.IDX1, D.IDXR):
        for qc in K.QCS:
            for q_filter in (True, False):
                ref = dpg_bc_reference(c['pol'], c['q'], c['rows'], c['expert'], idx, D.BOUND, qc, K.BC, q_filter)
                got = b.dpg_bc_grad(idx, D.BOUND, qc, K.BC, q_filter)
                assert np.array_equal(got['stats'], ref['stats']), (got['stats'], ref['stats'])
                assert np.array_equal(got['da'].astype(np.float64), ref['dA']) and np.array_equal(got['dz'].astype(np.float64), ref['dz'])
                assert np.array_equal(got['q'].astype(np.float64), ref['q']) and (not q_filter or np.array_equal(got['qe'].astype(np.float64), ref['qe']))
                bad = np.nonzero(got['grad'].astype(np.float64) != _flat(ref['grads']))[0]
                assert bad.size == 0, (pw, len(idx), qc, q_filter, bad[:8], got['grad'][bad[:8]], _flat(ref['grads'])[bad[:8]])
                if idx is D.IDX8 and q_filter:
                    assert got['qe'][0] == got['q'][0] and ref['m'][0] and not ref['f'][0] and got['stats'][5] == ref['f'].sum() / 8.0
                    assert got['stats'][5] >= 2.0 / 8.0 and got['stats'][4] == 7.0 / 8.0
    assert _same(_blob(b), _flat(c['pol'])) and _same(b.get_q_mlp(), _flat(c['q']))


# ---- 5. Gaussian data within the a-priori bound ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 257])
def test_gaussian_data_within_the_a_priori_bound(B, batch_of):
    """Gaussian networks, uniform rows and expert actions, q_coef = 3/4, bc_coef = 3/2, the filter on: the six statistics, dA, dz, q,
    qe and every gradient element lie within ddpg_cases.actor_bound extended by the cloning term's roundings
    (ddpg_bc_cases.actor_bc_bound states the extension), with the ReLU margins, the gate's margin and the FILTER's margin -- over every
    row of the minibatch -- asserted > 0: the labelled share and the filter-pass share are then exact, and no row is left out."""
    ok, c, idx, ab = K.gaussian_bc_ok(B, K.GAUSSIAN_BC_SEEDS[B])
    assert ok and ab['margin'] > 0.0 and ab['gate_margin'] > 0.0 and ab['filter_margin'] > 0.0, (ab['margin'], ab['gate_margin'], ab['filter_margin'])
    assert (np.abs(ab['qe'] - ab['q']) > ab['dqe'] + ab['dq']).all() and len(ab['q']) == B
    b = _load_bc(batch_of(10), c)
    got = b.dpg_bc_grad(idx, D.G_BOUND, K.G_QC, K.G_BC, True)
    err = np.abs(got['grad'].astype(np.float64) - _flat(ab['grads']))
    print("B %d: margin %.3e, gate margin %.3e, filter margin %.3e, labelled %d, passing %d of %d, max dz err %.3e, max grad err %.3e, max err / bound %.3f, max |grad| %.3e" % (
        B, ab['margin'], ab['gate_margin'], ab['filter_margin'], ab['m'].sum(), ab['f'].sum(), B, np.abs(got['dz'] - ab['dz']).max(), err.max(),
        (err[ab['bound'] > 0] / ab['bound'][ab['bound'] > 0]).max(), np.abs(got['grad']).max()))
    assert np.isfinite(got['grad']).all() and np.abs(_flat(ab['grads'])).max() > 1e-5 and 0 < ab['gated'] < 4 * B
    assert got['stats'][1] == ab['stats'][1] and got['stats'][4] == ab['stats'][4] and got['stats'][5] == ab['stats'][5], (got['stats'], ab['stats'])
    assert (np.abs(got['stats'] - ab['stats']) <= ab['dstats']).all(), (got['stats'], ab['stats'], ab['dstats'])
    assert (np.abs(got['q'].astype(np.float64) - ab['q']) <= ab['dq']).all() and (np.abs(got['qe'].astype(np.float64) - ab['qe']) <= ab['dqe']).all()
    assert np.array_equal(got['qe'] > got['q'], ab['qe'] > ab['q'])           # every row's filter decision, the unlabelled rows' among them
    assert (np.abs(got['da'].astype(np.float64) - ab['dA']) <= ab['ddA']).all() and (np.abs(got['dz'].astype(np.float64) - ab['dz']) <= ab['ddz']).all()
    assert (err <= ab['bound']).all(), (np.nonzero(err > ab['bound'])[0][:8], err.max())
    assert ab['bound'].max() < 0.05 * np.abs(_flat(ab['grads'])).max()           # the bound binds


# ---- 6. pure cloning ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 257])
def test_pure_cloning_is_the_squared_error_trainer(B, batch_of):
    """q_coef = 0, bc_coef = 1, no filter, every row labelled: the gradient equals clothhip_policy_fit_grad's on a twin handle whose
    labels are the clamped expert actions with weights 1 -- np.array_equal, not bytes: 0 g may be -0, and x + (-0) differs from x only
    in the sign of a zero -- and the reported BC loss is its loss to within the two kernels' different summation orders."""
    c, idx = D.gaussian_case(K.PW, K.QW, B, seed=4, n_rows=48 if B <= 48 else 300)
    c = K.with_expert(c, 4, unlabelled=0.0)
    assert K.expert_mask(c['expert']).all()
    b = _load_bc(batch_of(10), c)
    got = b.dpg_bc_grad(idx, D.G_BOUND, 0.0, 1.0, False)
    twin = _new_batch(10)
    twin.fit_append(c['rows'], D.clamp(c['expert'], np.float32(D.G_BOUND)).astype(np.float64))
    twin.set_policy_mlp(c['pol'])
    loss, grad = twin.fit_grad(idx)
    assert np.array_equal(got['grad'], grad) and np.abs(grad).max() > 1e-4 and got['stats'][4] == got['stats'][5] == 1.0
    assert abs(got['stats'][3] - loss) <= 2.0 * (4 * B) * 2.0 ** -53 * loss and loss > 0      # (two double sums of 4 B terms, each within 4 B 2^-53 of exact)
    twin.close()


# ---- 7. isolation; a fit is its steps one call at a time ----------------------------------------------------------------------------------------
def test_the_new_entries_touch_nothing_else():
    pw, qw = [300, 37, 64, 4], [304, 37, 64, 1]
    c, idx = D.gaussian_case(pw, qw, 8, seed=8, n_rows=48)
    c = K.with_expert(c, 8)
    b = _load_bc(_new_batch(10), c)
    from test_gpu_policy_fit import _random_layers
    val, ls = _random_layers([300, 6, 1], 9), np.array([-1.0, -0.5, 0.25, 0.0], dtype=np.float32)
    b.set_value_mlp(val)
    b.set_policy_log_sigma(ls)
    b.fit_set_weights(np.random.RandomState(1).normal(size=48).astype(np.float32))
    b.fit_set_returns(c['rew'])
    b.fit_snapshot_policy()
    table = np.random.RandomState(5).randint(0, 47, size=(3, 8)).astype(np.int32)

    def others(policy):
        cols = (b.fit_data(), b.fit_get_weights(), b.fit_get_transitions(), b.fit_get_returns(), b.fit_get_old_means(), b.fit_get_old_log_sigma(), b.fit_expert())
        nets = [b.get_q_mlp(), b.get_value_mlp(), b.get_policy_log_sigma()] + list(b.ddpg_targets()) + ([_blob(b)] if policy else [])
        return b"".join(np.ascontiguousarray(x).tobytes() for x in _leaves([nets, cols]))
    before = others(True)
    for q_filter in (True, False):
        b.dpg_bc_grad(idx, D.G_BOUND, K.G_QC, K.G_BC, q_filter)
    assert others(True) == before                                              # the gradient entry: nothing at all
    before = others(False)
    pol0 = _blob(b)
    for q_filter in (True, False):
        b.dpg_bc_fit(table, D.G_BOUND, K.G_QC, K.G_BC, q_filter, **ADAM)
    assert others(False) == before and not _same(_blob(b), pol0)              # the step entry: the policy alone (the Q network, both targets, the value network, the head, every column stay)
    val_before = b"".join(np.ascontiguousarray(x).tobytes() for x in _leaves([b.get_value_mlp(), b.get_policy_log_sigma(), b.fit_data(), b.fit_expert(), b.fit_get_weights()]))
    b.ddpg_fit(table, D.G_GAMMA, 0.1, D.G_BOUND, policy_hyper=ADAM, q_hyper=ADAM, bc=dict(q_coef=K.G_QC, bc_coef=K.G_BC, q_filter=True))
    assert val_before == b"".join(np.ascontiguousarray(x).tobytes() for x in _leaves([b.get_value_mlp(), b.get_policy_log_sigma(), b.fit_data(), b.fit_expert(), b.fit_get_weights()]))
    b.close()


@pytest.mark.parametrize("name,hyper", [OPTIMIZERS[0], OPTIMIZERS[2]], ids=["adam", "sgd_momentum"])
@pytest.mark.parametrize("q_filter", [True, False], ids=["filter", "nofilter"])
def test_a_bc_fit_is_its_steps_one_call_at_a_time(name, hyper, q_filter):
    """Three clothhip_ddpg_fit_bc steps on one handle; on a second the same steps as q_fit (1 step), dpg_bc_fit (1 step), ddpg_polyak:
    the same statistics, and the same bytes in the policy, the Q network and both targets; a fourth step on both leaves them equal
    again (the moments and the step counts continue). The cloning term changes the outcome: plain ddpg_fit ends elsewhere."""
    c, _ = D.gaussian_case(K.PW, K.QW, 8, seed=7, n_rows=48)
    c = K.with_expert(c, 7)
    table = np.random.RandomState(3).randint(0, 47, size=(4, 9)).astype(np.int32)      # (row 47 is the leaf)
    q_hyper = dict(hyper, lr=2.0 * hyper['lr'])
    bc = dict(q_coef=K.G_QC, bc_coef=K.G_BC, q_filter=q_filter)
    one, steps, plain = _load_bc(_new_batch(10), c), _load_bc(_new_batch(10), c), _load_bc(_new_batch(10), c)
    whole = one.ddpg_fit(table[:3], D.G_GAMMA, 0.25, D.G_BOUND, policy_hyper=hyper, q_hyper=q_hyper, bc=bc)
    assert whole.shape == (3, 9) and np.isfinite(whole).all() and (whole[:, 7] > 0).all() and (not q_filter or (whole[:, 8] < whole[:, 7]).any())
    for s in range(3):
        st_q = steps.q_fit(table[s:s + 1], D.G_GAMMA, D.G_BOUND, **q_hyper)
        st_p = steps.dpg_bc_fit(table[s:s + 1], D.G_BOUND, K.G_QC, K.G_BC, q_filter, **hyper)
        steps.ddpg_polyak(0.25)
        assert whole[s].tobytes() == np.concatenate([st_q[0], st_p[0]]).tobytes(), (name, s)
    for a, w in zip(_states(one), _states(steps)):
        assert a.tobytes() == w.tobytes()
    more = one.ddpg_fit(table[3:], D.G_GAMMA, 0.25, D.G_BOUND, policy_hyper=hyper, q_hyper=q_hyper, bc=bc)
    again = np.concatenate([steps.q_fit(table[3:], D.G_GAMMA, D.G_BOUND, **q_hyper), steps.dpg_bc_fit(table[3:], D.G_BOUND, K.G_QC, K.G_BC, q_filter, **hyper)], axis=1)
    steps.ddpg_polyak(0.25)
    assert more.tobytes() == again.tobytes()
    for a, w in zip(_states(one), _states(steps)):
        assert a.tobytes() == w.tobytes()
    plain.ddpg_fit(table, D.G_GAMMA, 0.25, D.G_BOUND, policy_hyper=hyper, q_hyper=q_hyper)
    assert not _same(_states(plain)[0], _states(one)[0])
    one.close(); steps.close(); plain.close()


# ---- 8. every refusal ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from gym_cloth_amd import _lib
    from test_gpu_dagger import E, _env
    v = _env("f32", n_side=10, max_actions=2)
    v.reset()
    b, L, h = v.batch, v.batch._L, v.batch._h
    pw, qw = [300, 5, 4], [304, 5, 1]
    c = K.exact_bc_case(pw, qw, 1.0, 0, 2)
    _load_bc(b, c)
    idx = np.ascontiguousarray(D.IDX8, dtype=np.int32)
    table = np.tile(idx, (2, 1))
    bc_kw = dict(q_coef=1.0, bc_coef=0.5, q_filter=True)
    b.ddpg_fit(table, 0.9, 0.1, 1.0, policy_hyper=ADAM, q_hyper=ADAM, bc=bc_kw)      # moments and step counts exist
    twin = _load_bc(_new_batch(10), c)
    twin.ddpg_fit(table, 0.9, 0.1, 1.0, policy_hyper=ADAM, q_hyper=ADAM, bc=bc_kw)
    ip, P_, B_ = _lib.i32p, _lib.ClothDdpgParams, _lib.ClothBcParams
    ok, okb, adam = P_(0.9, 0.1, 1.0, 0), B_(1.0, 0.5, 1, 0), _lib.ClothFitParams(0.0, ADAM['lr'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], 0.0)
    g_p, st, y8 = np.zeros(b._mlp_n_params, dtype=np.float32), np.zeros(18), np.zeros(32, dtype=np.float32)

    def every(p=ok, bc=okb, ix=idx, B=8, n_steps=1, fit=adam, grads_only=False, qe=True):
        pp, bb, ff, ii = (C.byref(p) if p is not None else None), (C.byref(bc) if bc is not None else None), (C.byref(fit) if fit is not None else None), (ip(ix) if ix is not None else None)
        calls = [lambda: L.clothhip_policy_fit_dpg_bc_grad(h, pp, bb, ii, B, _fp(g_p), _lib.dp(st), _fp(y8), _fp(y8), _fp(y8), _fp(y8) if qe else None),
                 lambda: L.clothhip_policy_fit_dpg_bc(h, ff, pp, bb, ii, n_steps, B, _lib.dp(st)), lambda: L.clothhip_ddpg_fit_bc(h, ff, ff, pp, bb, ii, n_steps, B, _lib.dp(st))]
        return [call() for call in (calls[:1] if grads_only else calls)]

    def state():
        return [x.tobytes() for x in _leaves([list(_states(b)), b.fit_expert(), b.fit_data()])]
    assert every(grads_only=True) == [0]
    snap = state()
    EI, ES = _lib.EINVAL, _lib.ESTATE
    # the coefficients, the flags, reserved
    for bad in (B_(np.nan, 0.5, 1, 0), B_(1.0, np.nan, 1, 0), B_(np.inf, 0.5, 1, 0), B_(1.0, np.inf, 0, 0), B_(-1e-9, 0.5, 1, 0), B_(1.0, -0.5, 0, 0), B_(0.0, 0.0, 1, 0), B_(-0.0, 0.0, 0, 0),
                B_(1.0, 0.5, 2, 0), B_(1.0, 0.5, 3, 0), B_(1.0, 0.5, -1, 0), B_(1.0, 0.5, 1, 1), B_(1.0, 0.5, 0, -1)):
        assert every(bc=bad) == [EI] * 3, (bad.q_coef, bad.bc_coef, bad.flags, bad.reserved)
    assert every(bc=None) == [EI] * 3 and every(p=None) == [EI] * 3 and every(ix=None) == [EI] * 3 and every(fit=None)[1:] == [EI] * 2
    assert every(bc=B_(1.0, 0.5, 0, 0), grads_only=True) == [EI] and b"qe_out" in L.clothhip_last_error()      # qe_out with the filter off
    assert every(bc=B_(1.0, 0.5, 0, 0), grads_only=True, qe=False) == [0] and every(bc=B_(0.0, 1e-3, 0, 0), n_steps=0)[1:] == [0, 0] and every(bc=B_(1e-3, 0.0, 1, 0), n_steps=0)[1:] == [0, 0]
    # DDPG's own refusals
    assert every(B=0) == [EI] * 3 and every(B=_lib.FIT_MAX_BATCH + 1) == [EI] * 3 and every(n_steps=-1)[1:] == [EI] * 2
    for bad in (12, -1, 10):                                                   # outside the dataset; row 10 is the leaf
        assert every(ix=np.array([0, 1, 2, 3, 4, 5, 6, bad], dtype=np.int32)) == [EI] * 3
    for p in (P_(np.nan, 0.1, 1.0, 0), P_(0.9, 1.5, 1.0, 0), P_(0.9, 0.1, 0.0, 0), P_(0.9, 0.1, np.nan, 0), P_(0.9, 0.1, 1.0, 1)):
        assert every(p=p) == [EI] * 3
    f = _lib.ClothFitParams(2.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert every(fit=f)[1:] == [EI] * 2
    assert state() == snap
    # a launch in flight
    nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, E, 4)))
    assert every() == [ES] * 3 and L.clothhip_fit_data_set_expert(h, 0, 1, _fp(y8)) == ES and L.clothhip_fit_data_get_expert(h, 0, 1, _fp(y8)) == ES
    b.run_actions_end()
    assert state() == snap
    # the moments and step counts too: the next step on both handles gives the same bytes
    out = b.ddpg_fit(table[:1], 0.9, 0.1, 1.0, policy_hyper=ADAM, q_hyper=ADAM, bc=bc_kw)
    want = twin.ddpg_fit(table[:1], 0.9, 0.1, 1.0, policy_hyper=ADAM, q_hyper=ADAM, bc=bc_kw)
    assert out.tobytes() == want.tobytes()
    for a, w in zip(_states(b), _states(twin)):
        assert a.tobytes() == w.tobytes()
    # no targets (the fused entry alone reads them), a population, no Q network, no policy, an empty dataset
    b.set_q_mlp(c['q'])
    assert every() == [0, 0, ES]
    b.set_q_mlp(None)
    assert every() == [ES] * 3
    b.set_q_mlp(c['q']); b.set_policy_mlp(None)
    assert every() == [ES] * 3
    b.set_policy_population([c['pol'], c['tpol']], np.zeros(E, dtype=np.int32))
    assert every() == [ES] * 3
    b.set_policy_mlp(c['pol']); b.ddpg_sync_targets(); b.fit_clear()
    assert every() == [ES] * 3
    twin.close()
    v.close()


# ---- 9. demos over 8 cloths ----------------------------------------------------------------------------------------------------------------------
def test_demos_collect_with_an_expert_and_fit_with_demonstrations():
    """One collection of pure demonstrations (beta = 1) and one of the learner's own states under an armed expert (beta = 0): every
    non-leaf row carries an expert action, the leaves carry none; where the expert acted the label is its action; ddpg_fit with a
    cloning term and demo_fraction = 1/2 runs, returns statistics [n, 9], draws half of every minibatch from the labelled rows, and the
    plain call on the same dataset still returns [n, 6]."""
    from gym_cloth_amd import _lib
    from gym_cloth_amd.batch_fit import has_expert
    from gym_cloth_amd.demos import actor_critic_collect, ddpg_fit
    from gym_cloth_amd.policies import DeviceNoise, MLPTrainer, QTrainer
    v = _env8()
    v.reset()
    tr = MLPTrainer(v, _layers([3 * v.P, 5, 4], 21), lr=1e-3)
    qc = QTrainer(v, _layers([3 * v.P + 4, 6, 1], 22), lr=1e-2)
    cols = [actor_critic_collect(v, tr, n_actions=3, policy_noise=DeviceNoise(13 + i, sigma=0.05), slots_per_launch=3, expert="highest_point", beta=beta, seed=i,
                                 expert_choices=np.zeros((3, 8), dtype=np.int32))
            for i, beta in enumerate((1.0, 0.0))]
    ex, (_, lab), nxt = v.batch.fit_expert(), v.batch.fit_data(), v.batch.fit_get_transitions()[1]
    leaf = nxt == _lib.FIT_NEXT_NONE
    assert leaf.any() and (~leaf).sum() == cols[0]['appended'] + cols[1]['appended']
    assert has_expert(ex)[~leaf].all() and not has_expert(ex)[leaf].any() and (ex[leaf].view(np.uint32) == FILL).all()
    first2 = cols[1]['first']
    demo = ~leaf & (np.arange(len(leaf)) < first2)
    assert np.array_equal(lab[demo], ex[demo]) and not np.array_equal(lab[~leaf & ~demo], ex[~leaf & ~demo])      # beta = 1: the expert drove; beta = 0: the learner (plus noise) did
    took = np.concatenate([r['expert_took'][r['ran']] for r in cols[0]['records']])
    assert took.all() and not np.concatenate([r['expert_took'][r['ran']] for r in cols[1]['records']]).any()
    fit = ddpg_fit(v, tr, qc, cols[1], gamma=0.9, tau=0.05, n_steps=6, batch_size=8, seed=0, act_bound=1.0, q_coef=1.0, bc_coef=2.0, q_filter=True, demo_fraction=0.5)
    assert fit['stats'].shape == (6, 9) and np.isfinite(fit['stats']).all() and fit['rows'].shape == (6, 8) and fit['synced']
    assert np.array_equal(fit['labelled'], np.nonzero(~leaf)[0]) and not leaf[fit['rows']].any() and (fit['stats'][:, 7] == 1.0).all() and (fit['stats'][:, 8] <= 1.0).all()
    off = ddpg_fit(v, tr, qc, cols[1], gamma=0.9, tau=0.05, n_steps=2, batch_size=8, seed=1, act_bound=1.0, q_coef=0.5, bc_coef=1.0, q_filter=False)
    assert off['stats'].shape == (2, 9) and (off['stats'][:, 8] == 1.0).all() and (off['stats'][:, 6] > 0).all() and 'labelled' not in off
    plain = ddpg_fit(v, tr, qc, cols[1], gamma=0.9, tau=0.05, n_steps=2, batch_size=8, seed=1, act_bound=1.0)
    assert plain['stats'].shape == (2, 6) and np.array_equal(plain['rows'], off['rows'])
    v.batch.fit_set_expert(np.full((len(leaf), 4), np.nan))
    with pytest.raises(ValueError):
        ddpg_fit(v, tr, qc, cols[1], n_steps=2, batch_size=8, bc_coef=1.0, demo_fraction=0.5)
    v.close()
