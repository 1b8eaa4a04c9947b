"""GPU tests of fitting from reward: the per-row weight in the trainer's loss (k_fit_loss, k_fit_sqsum) on exactly
representable data, as exact scalings and zero rows, within an a-priori bound on Gaussian data, and through the grouped trainer; a
dataset of all-ones weights gives the unweighted bits; clothhip_policy_fit_predict is the y of the loss; the executed action as the label
(k_fit_gather reading the launch's records) with the row's weight; the refusals of the header; growth; demos.reward_collect. Every
comparison is array_equal or by bytes unless it says otherwise."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_dagger import E, _env, _layers
from test_gpu_policy_fit import ADAM, _blob, _exact_case, _exact_facts, _flat, _gamma, _new_batch, _random_case, _random_layers

pytestmark = pytest.mark.gpu

T = 4


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 1. exact data ------------------------------------------------------------------------------------------------------------------------
IDX8, IDX1, IDXR = np.array([7, 2, 11, 0, 5, 9, 4, 1]), np.array([3]), np.array([6, 2, 6, 10, 8, 2, 6, 0])


def _exact_weights(seed, n_rows=12):
    """Integer weights from {-2 .. 3}, from a stream of their own beside _exact_case's."""
    return np.random.RandomState(5000 + seed).randint(-2, 4, size=n_rows).astype(np.float32)


EXACT_CASES = [  # (n_side, widths, dens, seed): the first seed from 0 for which the asserts of the test hold (checked on the CPU)
    (10, [300, 5, 4], 1.0, 0),
    (10, [300, 37, 64, 4], 0.3, 0),
    (25, [1875, 37, 64, 4], 0.3, 0),
]


def _exact_asserts(widths, dens, seed):
    """The preconditions of the exact test, from the float64 reference alone: -> (layers, rows, labels, w)."""
    from gym_cloth_amd.policies import fit_reference
    layers, rows, labels = _exact_case(widths, dens, seed)
    w = _exact_weights(seed)
    wb = w[IDX8]
    assert (wb < 0).any() and (wb > 0).any() and (wb == 0).any(), wb       # both signs and a zero among the batch's rows
    for idx in (IDX8, IDX1, IDXR):
        worst, frac, _ = _exact_facts(layers, rows, labels, idx)
        # every quantity is a multiple of 1/16 (2 B = 16, integer weights); |g| grows by at most max |w|, so every inner product of
        # both passes stays below 2^24 / 16 in magnitude: every partial sum in ANY order is a float32
        assert 16.0 * float(np.abs(w).max()) * worst < 2.0 ** 24, (worst, w)
        if len(idx) == 8:
            assert frac is None or 0.45 <= frac <= 0.57, frac
        plain = _flat(fit_reference(layers, rows, labels, idx)[1])
        weighted = _flat(fit_reference(layers, rows, labels, idx, weights=w)[1])
        if w[idx[0]] != 1 or len(idx) > 1:
            assert not np.array_equal(plain, weighted)                         # a kernel that ignores the column must fail
        if len(idx) == 8:                                                      # no block of the weighted gradient is empty
            assert all(np.count_nonzero(g) > 0 for Wb in fit_reference(layers, rows, labels, idx, weights=w)[1] for g in Wb)
    return layers, rows, labels, w


@pytest.fixture(scope="module")
def batch_of():
    """n_side -> ONE ClothBatch of one cloth for the cases that only need a handle to train on (each sets its own network and data)."""
    made = {}

    def get(n_side):
        if n_side not in made:
            made[n_side] = _new_batch(n_side)
        made[n_side].fit_clear()
        return made[n_side]
    yield get
    for b in made.values():
        b.close()


@pytest.mark.parametrize("n_side,widths,dens,seed", EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_exact_data_equals_the_weighted_reference(n_side, widths, dens, seed, batch_of):
    """test_gpu_policy_fit's exact case with integer weights from {-2 .. 3}: the device's loss and every gradient element EQUAL
    fit_reference(..., weights=). B = 8, B = 1 and a repeated row."""
    from gym_cloth_amd.policies import fit_reference
    layers, rows, labels, w = _exact_asserts(widths, dens, seed)
    b = batch_of(n_side)
    b.set_policy_mlp(layers)
    assert b.fit_append(rows, labels, weights=w) == len(rows)
    assert np.array_equal(b.fit_get_weights(), w)
    for idx in (IDX8, IDX1, IDXR):
        ref_loss, ref = fit_reference(layers, rows, labels, idx, weights=w)
        loss, grad = b.fit_grad(idx)
        print("%r B %d: loss %r (reference %r), weights %r" % (widths, len(idx), loss, ref_loss, w[idx].tolist()))
        assert loss == ref_loss and b.fit_loss(idx) == ref_loss
        want = _flat(ref)
        assert np.array_equal(want, want.astype(np.float32))                 # the reference's values are float32 values
        bad = np.nonzero(grad.astype(np.float64) != want)[0]
        assert bad.size == 0, (widths, len(idx), bad[:8], grad[bad[:8]], want[bad[:8]])
        plain = _flat(fit_reference(layers, rows, labels, idx)[1])
        if len(idx) > 1:
            assert not np.array_equal(grad.astype(np.float64), plain)
    # the same through set_weights on rows appended without weights
    b.fit_clear()
    b.fit_append(rows, labels)
    assert np.array_equal(b.fit_get_weights(), np.ones(len(rows), dtype=np.float32))
    unweighted = b.fit_grad(IDX8)
    b.fit_set_weights(w[3:9], first=3)
    b.fit_set_weights(w[:3])
    b.fit_set_weights(w[9:], first=9)
    assert np.array_equal(b.fit_get_weights(), w) and np.array_equal(b.fit_get_weights(4, 3), w[4:7])
    ref_loss, ref = fit_reference(layers, rows, labels, IDX8, weights=w)
    loss, grad = b.fit_grad(IDX8)
    assert loss == ref_loss and np.array_equal(grad.astype(np.float64), _flat(ref)) and not np.array_equal(grad, unweighted[1])
    assert np.array_equal(_blob(b), np.concatenate([np.concatenate([W.reshape(-1), bb]) for W, bb in layers]))      # nothing was updated


# ---- 2. all-ones weights give the unweighted bits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [9, 300], ids=["B9", "B300-two-ranges"])
def test_weights_of_one_change_no_bit(B):
    """Two handles, one network, the same rows. One appends through clothhip_fit_data_append_weighted(weights = NULL) and then writes
    ones with set_weights; the other never calls a new entry. Gradient, loss, fit_loss and the blob after five Adam steps are equal."""
    from gym_cloth_amd import _lib
    widths = [300, 37, 64, 4]
    layers, rows, labels, _ = _random_case(widths, 7, seed=5)
    r = np.random.RandomState(B)
    idx, table = r.randint(0, len(rows), size=B), r.randint(0, len(rows), size=(5, B))
    new, old = _new_batch(10), _new_batch(10)
    for b in (new, old):
        b.set_policy_mlp(layers)
    obs, lab = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(labels, dtype=np.float64)
    assert new._L.clothhip_fit_data_append_weighted(new._h, _lib.fp(obs), _lib.dp(lab), None, len(rows)) == _lib.OK
    new.fit_set_weights(np.ones(len(rows), dtype=np.float32))
    old.fit_append(rows, labels)
    assert new.fit_size() == old.fit_size() == len(rows)
    (la, ga), (lb, gb) = new.fit_grad(idx), old.fit_grad(idx)
    assert la == lb and np.array_equal(_i32(ga), _i32(gb)) and np.abs(ga).max() > 0
    assert new.fit_loss(idx) == old.fit_loss(idx) == la
    assert np.array_equal(new.fit(table, **ADAM), old.fit(table, **ADAM))
    assert np.array_equal(_i32(_blob(new)), _i32(_blob(old))) and not np.array_equal(_blob(new), _flat(layers))
    new.close(); old.close()


# ---- 3. / 4. exact scalings on Gaussian data ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, -2])
def test_a_power_of_two_scales_every_bit(k, batch_of):
    """Every weight 2^k: gradient and loss are 2^k times the unweighted ones, bit for bit (a power of two commutes with every rounding
    away from the subnormals)."""
    widths = [300, 37, 64, 4]
    layers, rows, labels, idx = _random_case(widths, 33, seed=4)
    b = batch_of(10)
    b.set_policy_mlp(layers)
    b.fit_append(rows, labels)
    loss1, grad1 = b.fit_grad(idx)
    assert np.abs(grad1[grad1 != 0]).min() > 2.0 ** -100                      # nowhere near the subnormals
    b.fit_set_weights(np.full(len(rows), 2.0 ** k, dtype=np.float32))
    loss, grad = b.fit_grad(idx)
    scale = np.float32(2.0 ** k)
    assert loss == 2.0 ** k * loss1 and b.fit_loss(idx) == loss
    assert np.array_equal(_i32(grad), _i32(scale * grad1)) and np.abs(grad1).max() > 1e-4


def test_zero_weight_rows_contribute_nothing(batch_of):
    """B = 16: eight rows interleaved with eight rows of weight 0. The gradient equals exactly 0.5 x the gradient of the eight rows alone
    at B = 8 (2 B doubles; a product with a zero dZ leaves every accumulator alone)."""
    widths = [300, 37, 64, 4]
    layers, rows, labels, _ = _random_case(widths, 7, seed=6)
    b = batch_of(10)
    b.set_policy_mlp(layers)
    b.fit_append(rows, labels)
    r = np.random.RandomState(3)
    perm = r.permutation(len(rows))
    live, dead = perm[:8], perm[8:16]
    w = np.ones(len(rows), dtype=np.float32)
    w[dead] = 0.0
    b.fit_set_weights(w)
    idx16 = np.stack([live, dead], axis=1).reshape(-1)
    loss8, grad8 = b.fit_grad(live)
    loss16, grad16 = b.fit_grad(idx16)
    assert np.array_equal(grad16, np.float32(0.5) * grad8) and np.abs(grad8).max() > 1e-4
    # (the loss's tree pairs other elements, so it is not bit for bit: two sums of at most 64 non-negative doubles, each within
    # 64 * 2^-53 of exact relative to its own value)
    assert abs(loss16 - 0.5 * loss8) <= 128 * 2.0 ** -53 * loss8
    b.fit_set_weights(np.ones(len(rows), dtype=np.float32))
    assert not np.array_equal(b.fit_grad(idx16)[1], grad16)                   # the dead rows do have a gradient of their own


# ---- 5. mixed Gaussian weights within an a-priori bound -----------------------------------------------------------------------------------
def _grad_bound_w(layers, rows, labels, w, idx):
    """test_gpu_policy_fit._grad_bound with the row weight carried into dZ's magnitude. The reference is g = w d / 2B; the device forms
    fl(fl(w fl(y - a)) / fl(2B)): three roundings of a value within |w| dy / 2B of g, so
        dg_L = |w| dy / 2B + gamma_3 (|g| + |w| dy / 2B),
    and the loss sum w (y - a)^2 / 4B moves by at most sum |w| (2 |d| dy + dy^2) / 4B plus the double roundings of the sum (1e-14 of
    sum |w| d^2 / 4B). Everything behind dZ_L is that function's, unchanged. Returns (loss, its bound, gradients, their bounds, margin)."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)[idx]
    a = np.asarray(labels, dtype=np.float64).astype(np.float32).astype(np.float64)[idx]
    wr = np.asarray(w, dtype=np.float32).astype(np.float64)[idx][:, None]
    B, L = len(idx), len(layers)
    Ws = [W.astype(np.float64) for W, _ in layers]
    hs, dhs, margin = [x], [np.zeros_like(x)], np.inf
    for l in range(L):
        aW, bb = np.abs(Ws[l]), layers[l][1].astype(np.float64)
        n = Ws[l].shape[1]
        dz = dhs[-1] @ aW.T + _gamma(n + 1) * ((np.abs(hs[-1]) + dhs[-1]) @ aW.T + np.abs(bb))
        z = hs[-1] @ Ws[l].T + bb
        if l + 1 < L:
            margin = min(margin, float((np.abs(z) - dz).min()))
        hs.append(np.maximum(z, 0.0) if l + 1 < L else z)
        dhs.append(np.where(z > 0.0, dz, 0.0) if l + 1 < L else dz)
    d = hs[-1] - a
    aw = np.abs(wr)
    loss = float((wr * d * d).sum() / (4.0 * B))
    dloss = float((aw * (2.0 * np.abs(d) * dhs[-1] + dhs[-1] ** 2)).sum() / (4.0 * B)) + 1e-14 * float((aw * d * d).sum() / (4.0 * B))
    g = wr * d / (2.0 * B)
    dg = aw * dhs[-1] / (2.0 * B)
    dg = dg + _gamma(3) * (np.abs(g) + dg)
    grads, bounds = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        h, dh, ag = hs[l], dhs[l], np.abs(g)
        dW = dg.T @ (np.abs(h) + dh) + ag.T @ dh + _gamma(B + 1) * ((ag + dg).T @ (np.abs(h) + dh))
        db = dg.sum(axis=0) + _gamma(B + 1) * (ag + dg).sum(axis=0)
        grads[l], bounds[l] = (g.T @ h, g.sum(axis=0)), (dW, db)
        if l:
            aW, mask = np.abs(Ws[l]), h > 0
            dgn = (dg @ aW + _gamma(Ws[l].shape[0] + 1) * ((ag + dg) @ aW)) * mask
            g, dg = (g @ Ws[l]) * mask, dgn
    return loss, dloss, grads, _flat(bounds), margin


@pytest.mark.parametrize("n_side,widths,B", [(10, [300, 5, 4], 7), (10, [300, 37, 64, 4], 33), (25, [1875, 64, 64, 4], 33)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_mixed_weights_within_the_a_priori_bound(n_side, widths, B, batch_of):
    """Gaussian weights of both signs on test_gpu_policy_fit's Gaussian case: loss and every gradient element within the computed bound
    of the float64 reference, the ReLU mask exact for every unit of the minibatch (asserted)."""
    from gym_cloth_amd.policies import fit_reference
    layers, rows, labels, idx = _random_case(widths, B, seed=len(widths))
    w = (np.random.RandomState(77).normal(size=len(rows)) * 1.5).astype(np.float32)
    assert (w[idx] < 0).any() and (w[idx] > 0).any()
    ref_loss, dloss, ref, bound, margin = _grad_bound_w(layers, rows, labels, w, idx)
    assert margin > 0.0, margin
    chk_loss, chk = fit_reference(layers, rows, labels, idx, weights=w)       # the bound's own reference is fit_reference's
    assert abs(chk_loss - ref_loss) <= 1e-12 * abs(ref_loss) + 1e-15 and np.allclose(_flat(chk), _flat(ref), rtol=0, atol=1e-13)
    b = batch_of(n_side)
    b.set_policy_mlp(layers)
    b.fit_append(rows, labels, weights=w)
    loss, grad = b.fit_grad(idx)
    err = np.abs(grad.astype(np.float64) - _flat(ref))
    print("%r B %d: mask margin %.3e, loss %.6g err %.3e (bound %.3e), max grad err %.3e, max err / bound %.3f, max |grad| %.3e" % (
        widths, B, margin, loss, abs(loss - ref_loss), dloss, err.max(), (err[bound > 0] / bound[bound > 0]).max(), np.abs(grad).max()))
    assert np.isfinite(grad).all() and np.abs(_flat(ref)).max() > 1e-4
    assert abs(loss - ref_loss) <= dloss
    assert (err <= bound).all(), (np.nonzero(err > bound)[0][:8], err.max())
    assert b.fit_loss(idx) == loss


# ---- 6. members ---------------------------------------------------------------------------------------------------------------------------
def test_members_on_a_weighted_dataset_equal_their_twins(batch_of):
    """G = 3 rows of a population fitted with fit_members on a weighted dataset, in two calls so that the moments matter: every row and
    every returned loss equal a shared-network handle's after the same calls on the same weighted rows."""
    widths = [300, 5, 4]
    n = sum(widths[l + 1] * widths[l] + widths[l + 1] for l in range(len(widths) - 1))
    nets = [_random_layers(widths, 40 + g) for g in range(3)]
    r = np.random.RandomState(9)
    rows, labels = r.uniform(-1, 1, size=(40, 300)).astype(np.float32), r.uniform(-1, 1, size=(40, 4))
    w = r.normal(size=40).astype(np.float32)
    w[::7] = 0.0
    table = r.randint(0, 40, size=(5, 3, 7)).astype(np.int32)
    pop, twin = _new_batch(10), batch_of(10)
    pop.set_policy_population(nets, np.zeros(1, dtype=np.int32))
    pop.fit_append(rows, labels)
    pop.fit_set_weights(w)
    hyper = dict(ADAM, lr=[3e-3, 1e-2, 1e-3])
    members = [2, 0, 1]
    lg, gg = pop.fit_grad_members(members, table[0])
    loss = np.concatenate([pop.fit_members(members, table[:3], hyper), pop.fit_members(members, table[3:], hyper)])
    for j, g in enumerate(members):
        twin.set_policy_mlp(nets[g])
        twin.fit_clear()
        twin.fit_append(rows, labels, weights=w)
        want_l, want_g = twin.fit_grad(table[0, j])
        assert lg[j] == want_l and np.array_equal(_i32(gg[j]), _i32(want_g))
        kw = dict(ADAM, lr=hyper["lr"][j])
        want = np.concatenate([twin.fit(table[:3, j], **kw), twin.fit(table[3:, j], **kw)])
        assert np.array_equal(loss[:, j], want), (g, loss[:, j], want)
        assert np.array_equal(_i32(pop.get_policy_mlp(g, n)), _i32(twin.get_policy_mlp(0, n)))
    twin.fit_clear()
    twin.fit_append(rows, labels)                                             # ... and the weights did matter
    twin.set_policy_mlp(nets[2])
    assert twin.fit_grad(table[0, 0])[0] != lg[0]
    pop.close()


# ---- 7. predict ---------------------------------------------------------------------------------------------------------------------------
def _loss_in_the_kernels_order(y, lab, w):
    """k_fit_loss's sum restated: element i of the [B][4] table goes to thread i % 256, which adds (double)w * (dd * dd) in ascending
    i; the 256 sums are added by a halving tree. -> the SUM (k_fit_sqsum's result; the loss is it / 4B)."""
    yv, av = y.astype(np.float64).reshape(-1), lab.astype(np.float64).reshape(-1)
    wv = np.repeat(w.astype(np.float64), 4)
    dd = yv - av
    term = wv * (dd * dd)
    red = np.zeros(256)
    for i0 in range(0, len(term), 256):
        part = term[i0:i0 + 256]
        red[:len(part)] = red[:len(part)] + part
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return red[0]


def test_predict_is_the_y_of_the_loss():
    """fit_predict's rows and the stored labels and weights, summed on the host in k_fit_loss's order, reproduce fit_grad's loss bits:
    n = 1, n = B, and n = FIT_MAX_BATCH + 3 by index repetition (fit_loss: the chunk sums added in order). The members form gives the
    shared handle's rows. Nothing changed: the next Adam step is a twin's that never predicted."""
    from gym_cloth_amd import _lib
    widths = [300, 37, 64, 4]
    layers, rows, labels, _ = _random_case(widths, 7, seed=7)
    n_rows = len(rows)
    r = np.random.RandomState(21)
    w = r.normal(size=n_rows).astype(np.float32)
    table = r.randint(0, n_rows, size=(3, 9))
    b, twin = _new_batch(10), _new_batch(10)
    for x in (b, twin):
        x.set_policy_mlp(layers)
        x.fit_append(rows, labels, weights=w)
        x.fit(table[:2], **ADAM)
    lab = b.fit_data()[1]
    one = b.fit_predict(np.arange(n_rows))
    assert one.dtype == np.float32 and one.shape == (n_rows, 4) and len({y.tobytes() for y in one}) == n_rows
    for n in (1, 33, _lib.FIT_MAX_BATCH + 3):
        idx = r.randint(0, n_rows, size=n)
        y = b.fit_predict(idx)
        assert y.shape == (n, 4) and np.array_equal(_i32(y), _i32(one[idx]))   # a row's y does not depend on its batch or its chunk
        if n <= _lib.FIT_MAX_BATCH:
            want = b.fit_grad(idx)[0]
            got = _loss_in_the_kernels_order(y, lab[idx], w[idx]) / float(4 * n)
        else:
            want = b.fit_loss(idx)
            cut = _lib.FIT_MAX_BATCH
            got = (_loss_in_the_kernels_order(y[:cut], lab[idx[:cut]], w[idx[:cut]])
                   + _loss_in_the_kernels_order(y[cut:], lab[idx[cut:]], w[idx[cut:]])) / float(4 * n)
        print("predict n %d: loss %r, restated %r" % (n, want, got))
        assert got == want and np.isfinite(want)
    # the members form: a population of three, the same rows under every member
    nets = [layers, _random_layers(widths, 50), _random_layers(widths, 51)]
    pop = _new_batch(10)
    pop.set_policy_population(nets, np.zeros(1, dtype=np.int32))
    pop.fit_append(rows, labels, weights=w)
    idx = r.randint(0, n_rows, size=37)
    ym = pop.fit_predict(idx, members=[2, 0])
    assert ym.shape == (2, 37, 4) and ym.dtype == np.float32
    big = pop.fit_predict(np.tile(idx, 120), members=[1, 2, 0])              # 4440 rows: two chunks per member
    assert np.array_equal(_i32(big[1, :37]), _i32(ym[0])) and np.array_equal(_i32(big[:, 37 * 119:]), _i32(big[:, :37]))
    for j, g in enumerate([2, 0]):
        s = _new_batch(10)
        s.set_policy_mlp(nets[g])
        s.fit_append(rows, labels)
        assert np.array_equal(_i32(ym[j]), _i32(s.fit_predict(idx)))
        s.close()
    assert not np.array_equal(ym[0], ym[1])
    assert np.array_equal(_i32(pop.get_policy_mlp(1, b._mlp_n_params)), _i32(_flat(nets[1])))
    # nothing changed on b: blob now, and moments and step count through the next step
    assert np.array_equal(_i32(_blob(b)), _i32(_blob(twin)))
    assert np.array_equal(b.fit(table[2:], **ADAM), twin.fit(table[2:], **ADAM)) and np.array_equal(_i32(_blob(b)), _i32(_blob(twin)))
    for x in (b, twin, pop):
        x.close()


# ---- 8. executed-action labels ------------------------------------------------------------------------------------------------------------
def _trainer(v, seed=21, gentle=False):
    """gentle: the last layer scaled to a short pull near the centre, [~0, ~0, ~0.05, ~0.05] -- an action that ends no episode by
    itself, so that slots begin on SLOTS rows too."""
    from gym_cloth_amd.policies import MLPTrainer
    layers = _layers([3 * v.P, 5, 4], seed, bias=[0.0, 0.0, 0.05, 0.05] if gentle else None)
    if gentle:
        layers[-1] = (layers[-1][0] * np.float32(0.02), layers[-1][1])
    return MLPTrainer(v, layers)


def _action_launch(prec, n_side):
    """hold, one policy='mlp' launch with a noise table and resets inside (episodes of two actions) that downloads its tables, NO expert
    -> (trainer, env, out, rows int32[n, 3] of the slots that ran, t, e, the observations the slots began on)."""
    from gym_cloth_amd import _lib
    from gym_cloth_amd.envs import slot_start_obs, slot_start_sources
    v = _env(prec, n_side=n_side, max_actions=2)
    v.reset()
    tr = _trainer(v, gentle=n_side == 25)
    before = np.asarray(v.state, dtype=np.float32).reshape(E, -1)
    v.batch.fit_hold()
    noise = np.random.RandomState(17).normal(size=(T, E, 4)) * (0.01 if n_side == 25 else 0.05)
    out = v.step_many(policy="mlp", n_actions=T, want_obs=True, policy_noise=noise)
    assert "expert_actions" not in out and out["ran"].all()
    t_, e_ = np.nonzero(out["ran"])
    rows = np.concatenate([slot_start_sources(out)[t_, e_], (t_ * E + e_)[:, None].astype(np.int32)], axis=1)
    src = rows[:, 0]
    assert (src == _lib.FIT_SRC_HELD).any() and (src == _lib.FIT_SRC_RESETS).any() and (src == _lib.FIT_SRC_SLOTS).any(), src
    assert ((t_ == 0) & (src == _lib.FIT_SRC_HELD)).sum() == E and (out["reset_before"][out["ran"]] > 0).sum() == (src == _lib.FIT_SRC_RESETS).sum()
    return tr, v, out, rows, t_, e_, slot_start_obs(out, before)[t_, e_]


@pytest.mark.parametrize("prec,n_side", [("f32", 10), ("f64", 10), ("f32", 25)])
def test_the_executed_action_is_the_label(prec, n_side):
    """The stored labels are out['actions'][t, e] rounded to float32 -- the network's output plus the noise, before clipping --, the
    observations slot_start_obs's, the weights the table given; then a row list with repeats in another order, behind the first."""
    tr, v, out, rows, t_, e_, want_obs = _action_launch(prec, n_side)
    want_lab = out["actions"][t_, e_].astype(np.float32)
    assert len({a.tobytes() for a in want_lab}) == len(rows)                  # every slot another action: the network read the state
    w = np.random.RandomState(2).normal(size=len(rows)).astype(np.float32)
    w[3] = 0.0
    assert tr.append_launch(rows, labels="action", weights=w) == len(rows) == tr.size()
    obs, lab = tr.data()
    assert obs.shape == (len(rows), 3 * v.P) and lab.dtype == np.float32
    assert np.array_equal(obs, want_obs) and np.array_equal(_i32(lab), _i32(want_lab)) and np.array_equal(_i32(tr.weights()), _i32(w))
    order = np.random.RandomState(4).randint(0, len(rows), size=40)
    assert len(np.unique(order)) < 40 and (np.diff(order) < 0).any()
    assert tr.append_launch(rows[order], labels="action") == len(rows) + 40
    obs2, lab2 = tr.data(len(rows))
    assert np.array_equal(obs2, want_obs[order]) and np.array_equal(_i32(lab2), _i32(want_lab[order]))
    assert np.array_equal(tr.weights(len(rows)), np.ones(40, dtype=np.float32)) and np.array_equal(_i32(tr.weights(0, len(rows))), _i32(w))
    # the gradient over the device-appended rows is the host route's
    idx = np.random.RandomState(5).randint(0, len(rows), size=16)
    got = v.batch.fit_grad(idx)
    tr.clear()
    assert tr.size() == 0 and tr.append(want_obs, want_lab.astype(np.float64), weights=w) == len(rows)
    host = v.batch.fit_grad(idx)
    assert got[0] == host[0] and np.array_equal(_i32(got[1]), _i32(host[1])) and np.abs(got[1]).max() > 0
    v.close()


def test_a_slot_that_did_not_run_appends_nothing():
    """Episodes that end without a reset leave slots with ran == 0: naming one raises the gather's flag, the call is refused with the
    host entry's message for a NaN label, and size, rows and weights are what they were."""
    from gym_cloth_amd import _lib
    w_ = _env("f32", n_side=10, max_actions=2)
    w_.reset()
    tw = _trainer(w_)
    out = w_.step_many(policy="mlp", n_actions=T, want_obs="device", auto_reset=False)
    assert not out["ran"][2:].any() and out["ran"][0].all()
    good = np.array([[_lib.FIT_SRC_SLOTS, 0 * E + e, 0 * E + e] for e in range(E)], dtype=np.int32)
    wg = np.arange(E, dtype=np.float32) - 2.0
    assert tw.append_launch(good, labels="action", weights=wg) == E
    kept, kept_w = tw.data(), tw.weights()
    assert np.array_equal(_i32(kept[1]), _i32(out["actions"][0].astype(np.float32))) and np.array_equal(kept_w, wg)
    bad_row = np.array([[_lib.FIT_SRC_SLOTS, 0 * E + 3, 2 * E + 3]], dtype=np.int32)  # slot 2 of env 3 did not run
    for rows_ in (bad_row, np.concatenate([good, bad_row, good])):
        with pytest.raises(ValueError) as err:
            tw.append_launch(rows_, labels="action", weights=np.full(len(rows_), 5.0, dtype=np.float32))
        assert "labels[%d][0]" % (len(rows_) // 2) in str(err.value), str(err.value)
        assert tw.size() == E
        again = tw.data()
        assert np.array_equal(again[0], kept[0]) and np.array_equal(again[1], kept[1]) and np.array_equal(tw.weights(), kept_w)
    assert tw.append_launch(good[::-1], labels="action") == 2 * E             # the spare capacity the refused call wrote into is reused
    assert np.array_equal(tw.data(E)[1], kept[1][::-1]) and np.array_equal(tw.weights(E), np.ones(E, dtype=np.float32))
    w_.close()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from gym_cloth_amd import _lib
    tr, v, out, rows, t_, e_, want_obs = _action_launch("f32", 10)
    b, L, h = v.batch, v.batch._L, v.batch._h
    n = len(rows)
    w = np.random.RandomState(1).normal(size=n).astype(np.float32)
    tr.append_launch(rows, labels="action", weights=w)
    snap_obs, snap_lab = tr.data()
    blob0 = _blob(b)
    idx = np.arange(8, dtype=np.int32)
    loss0, grad0 = b.fit_grad(idx)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def unchanged():
        assert tr.size() == n and np.array_equal(_i32(tr.weights()), _i32(w))
        o, l = tr.data()
        assert np.array_equal(o, snap_obs) and np.array_equal(l, snap_lab) and np.array_equal(_i32(_blob(b)), _i32(blob0))
        loss, g = b.fit_grad(idx)
        assert loss == loss0 and np.array_equal(_i32(g), _i32(grad0))

    two = np.array([0.5, -0.5], dtype=np.float32)
    y = np.zeros((8, 4), dtype=np.float32)
    for bad in (np.nan, np.inf, -np.inf):                                      # a non-finite weight, in every entry that takes one
        wb = np.array([1.0, bad], dtype=np.float32)
        assert L.clothhip_fit_data_set_weights(h, 0, 2, fp(wb)) == _lib.EINVAL
        assert L.clothhip_fit_data_append_weighted(h, fp(snap_obs[:2].copy()), _lib.dp(snap_lab[:2].astype(np.float64)), fp(wb), 2) == _lib.EINVAL
        assert L.clothhip_fit_data_append_launch_ex(h, _lib.i32p(rows[:2].copy()), 2, _lib.FIT_LABEL_ACTION, fp(wb)) == _lib.EINVAL
        unchanged()
    for first, k in ((n - 1, 2), (n, 1), (-1, 1), (0, n + 1), (2, -1)):          # a range past the end
        assert L.clothhip_fit_data_set_weights(h, first, k, fp(np.zeros(n + 1, dtype=np.float32))) == _lib.EINVAL
        assert L.clothhip_fit_data_get_weights(h, first, k, fp(np.zeros(n + 1, dtype=np.float32))) == _lib.EINVAL
    assert L.clothhip_fit_data_set_weights(h, 0, 2, None) == _lib.EINVAL and L.clothhip_fit_data_get_weights(h, 0, 2, None) == _lib.EINVAL
    assert L.clothhip_fit_data_set_weights(h, n, 0, None) == _lib.OK           # an empty range at the end is a range of the dataset
    for src in (2, -1):                                                        # an unknown label source
        assert L.clothhip_fit_data_append_launch_ex(h, _lib.i32p(rows[:2].copy()), 2, src, None) == _lib.EINVAL
    with pytest.raises(ValueError):
        b.fit_append_launch(rows[:2], labels="action", weights=np.array([1.0, np.nan]))
    assert L.clothhip_fit_data_append_launch_ex(h, _lib.i32p(rows[:1].copy()), 1, _lib.FIT_LABEL_EXPERT, None) == _lib.ESTATE   # no expert was armed
    bad_label = rows[:1].copy()
    bad_label[0, 2] = T * E
    assert L.clothhip_fit_data_append_launch_ex(h, _lib.i32p(bad_label), 1, _lib.FIT_LABEL_ACTION, None) == _lib.EINVAL
    assert L.clothhip_policy_fit_predict(h, _lib.i32p(np.array([0, n], dtype=np.int32)), 2, fp(y)) == _lib.EINVAL
    assert L.clothhip_policy_fit_predict(h, _lib.i32p(idx), 0, fp(y)) == _lib.EINVAL
    assert L.clothhip_policy_fit_predict(h, None, 8, fp(y)) == _lib.EINVAL and L.clothhip_policy_fit_predict(h, _lib.i32p(idx), 8, None) == _lib.EINVAL
    assert L.clothhip_policy_fit_predict_members(h, _lib.i32p(np.zeros(1, dtype=np.int32)), 1, _lib.i32p(idx), 8, fp(y)) == _lib.ESTATE   # no population
    unchanged()
    # a launch in flight
    nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, E, 4)))
    assert L.clothhip_fit_data_set_weights(h, 0, 2, fp(two)) == _lib.ESTATE and L.clothhip_fit_data_get_weights(h, 0, 2, fp(two.copy())) == _lib.ESTATE
    assert L.clothhip_fit_data_append_weighted(h, fp(snap_obs[:2].copy()), _lib.dp(snap_lab[:2].astype(np.float64)), fp(two), 2) == _lib.ESTATE
    assert L.clothhip_fit_data_append_launch_ex(h, _lib.i32p(rows[:2].copy()), 2, _lib.FIT_LABEL_ACTION, None) == _lib.ESTATE
    assert L.clothhip_policy_fit_predict(h, _lib.i32p(idx), 8, fp(y)) == _lib.ESTATE
    b.run_actions_end()
    unchanged()
    # that launch kept no observation tables: its records are there, the SLOTS rows are not; the held rows still are
    assert L.clothhip_fit_data_append_launch_ex(h, _lib.i32p(rows[-1:].copy()), 1, _lib.FIT_LABEL_ACTION, None) == _lib.ESTATE
    held = np.array([[_lib.FIT_SRC_HELD, 0, 0]], dtype=np.int32)
    assert b.fit_append_launch(held, labels="action", weights=[0.25]) == n + 1
    assert np.array_equal(tr.data(n)[1][0], np.zeros(4, dtype=np.float32)) and tr.weights(n)[0] == 0.25   # the action table given was zeros
    # predict without a network, and on a population through the shared call (these change the handle, so they come last)
    b.set_policy_population([_layers([300, 5, 4], 1), _layers([300, 5, 4], 2)], np.zeros(E, dtype=np.int32))
    assert L.clothhip_policy_fit_predict(h, _lib.i32p(idx), 8, fp(y)) == _lib.ESTATE
    for members, n_m in ((np.array([0, 0], dtype=np.int32), 2), (np.array([2], dtype=np.int32), 1), (np.array([0], dtype=np.int32), 0)):
        assert L.clothhip_policy_fit_predict_members(h, _lib.i32p(members), n_m, _lib.i32p(idx), 8, fp(y)) == _lib.EINVAL
    assert L.clothhip_policy_fit_predict_members(h, _lib.i32p(np.zeros(1, dtype=np.int32)), 1, _lib.i32p(idx), 0, fp(y)) == _lib.EINVAL
    b.set_policy_mlp(None)
    assert L.clothhip_policy_fit_predict(h, _lib.i32p(idx), 8, fp(y)) == _lib.ESTATE
    assert L.clothhip_policy_fit_predict_members(h, _lib.i32p(np.zeros(1, dtype=np.int32)), 1, _lib.i32p(idx), 8, fp(y)) == _lib.ESTATE
    assert tr.size() == n + 1 and np.array_equal(_i32(tr.weights(0, n)), _i32(w))
    v.close()
    # LABEL_ACTION before any launch: the held rows exist, a record table does not
    f = _env("f32", n_side=10)
    f.reset()
    tf = _trainer(f)
    f.batch.fit_hold()
    assert f.batch._L.clothhip_fit_data_append_launch_ex(f.batch._h, _lib.i32p(held), 1, _lib.FIT_LABEL_ACTION, None) == _lib.ESTATE
    assert tf.size() == 0
    f.close()


# ---- 10. growth ---------------------------------------------------------------------------------------------------------------------------
def test_growth_keeps_the_weights(batch_of):
    layers, rows, labels, _ = _random_case([300, 5, 4], 7, seed=8)
    b = batch_of(10)
    b.set_policy_mlp(layers)
    w = np.random.RandomState(3).normal(size=len(rows)).astype(np.float32)
    assert len(rows) < 64 and b.fit_append(rows, labels, weights=w) == len(rows)      # the first allocation: 64 rows
    assert b.fit_append(rows, labels) == 2 * len(rows) > 64                           # ... so this one grows the tables
    b.fit_set_weights(-w[:5], first=len(rows) + 2)
    assert b.fit_append(rows, labels, weights=2 * w) == 3 * len(rows)
    want = np.concatenate([w, np.ones(len(rows), dtype=np.float32), 2 * w])
    want[len(rows) + 2:len(rows) + 7] = -w[:5]
    assert np.array_equal(_i32(b.fit_get_weights()), _i32(want))
    obs, lab = b.fit_data()
    assert np.array_equal(obs, np.tile(rows, (3, 1))) and np.array_equal(lab, np.tile(labels.astype(np.float32), (3, 1)))
    b.fit_clear()
    assert b.fit_size() == 0 and b.fit_get_weights().shape == (0,)
    assert b.fit_append(rows[:3], labels[:3]) == 3 and np.array_equal(b.fit_get_weights(), np.ones(3, dtype=np.float32))


# ---- 11. reward_collect -------------------------------------------------------------------------------------------------------------------
N_COLLECT = 3


def _collect(slots_per_launch, scheme="filter", **kw):
    from gym_cloth_amd.demos import reward_collect
    v = _env("f32", n_side=10, max_actions=2)
    v.reset()
    tr = _trainer(v)
    noise = np.random.RandomState(13).normal(size=(N_COLLECT, E, 4)) * 0.05
    col = reward_collect(v, tr, n_actions=N_COLLECT, gamma=0.5, scheme=scheme, policy_noise=noise, slots_per_launch=slots_per_launch,
                         max_launches=8, **kw)
    obs, lab = tr.data()
    res = (col, obs, lab, tr.weights())
    v.close()
    return res


def _recomputed(col, scheme, **kw):
    """The weights again from the returned records, by the functions' own definitions: the launches last to first, chained by the carry."""
    from gym_cloth_amd.demos import returns_carry, returns_to_go, reward_weights
    carry, parts = None, []
    for rec in reversed(col["records"]):
        ran = rec["ran"] & (rec["slot"] < N_COLLECT)
        G, complete = returns_to_go(rec["rew"], ran, rec["done"], rec["reset_before"], 0.5, carry)
        carry = returns_carry(G, complete, ran, rec["reset_before"], carry)
        parts.append((G[ran], complete[ran]))
    G = np.concatenate([p[0] for p in parts[::-1]])
    complete = np.concatenate([p[1] for p in parts[::-1]])
    w = np.zeros(len(G), dtype=np.float32)
    w[complete] = reward_weights(G[complete], scheme, **kw)
    return G, complete, w


def test_reward_collect_is_deterministic_and_does_not_depend_on_the_launches():
    """Two collections from the same seeds store the same bytes. A collection in launches of 2 slots stores, env by env, the rows,
    labels, returns and weights of the collection in one launch of 4 (three slots per env are collected, so every env's third row opens
    an episode the collection does not see the end of: weight 0). The weights are reward_weights(returns_to_go(...)) of the records."""
    one, again = _collect(4, "advantage"), _collect(4, "advantage")
    for a, b in zip(one[1:], again[1:]):
        assert a.tobytes() == b.tobytes()
    col = one[0]
    assert col["appended"] == N_COLLECT * E == len(one[1]) and col["launches"] == 1 and col["first"] == 0
    G, complete, w = _recomputed(col, "advantage")
    assert np.array_equal(col["returns"], G) and np.array_equal(col["complete"], complete) and np.array_equal(_i32(col["weights"]), _i32(w))
    assert np.array_equal(_i32(one[3]), _i32(w)) and (w[complete] != 0).any() and (w < 0).any() and (w > 0).any()
    assert col["open_rows"] == int((~complete).sum()) > 0 and (one[3][~complete] == 0).all()
    assert len(col["episode_return"]) >= E and np.isfinite(col["episode_return"]).all()
    # the labels are the executed actions: not the network's own output on the stored rows (the noise is in them)
    whole, split = _collect(4), _collect(2)
    assert split[0]["launches"] == 2 and whole[0]["launches"] == 1 and split[0]["appended"] == whole[0]["appended"] == N_COLLECT * E
    for e in range(E):
        ia = np.nonzero(whole[0]["row_env"] == e)[0]
        ib = np.nonzero(split[0]["row_env"] == e)[0]
        assert np.array_equal(whole[0]["row_slot"][ia], np.arange(N_COLLECT)) and np.array_equal(split[0]["row_slot"][ib], np.arange(N_COLLECT))
        for k in (1, 2, 3):
            assert whole[k][ia].tobytes() == split[k][ib].tobytes(), (e, k)
        assert np.array_equal(whole[0]["returns"][ia], split[0]["returns"][ib]) and np.array_equal(whole[0]["complete"][ia], split[0]["complete"][ib])
    G, complete, w = _recomputed(split[0], "filter")
    assert np.array_equal(_i32(split[3]), _i32(w)) and set(np.unique(w)) <= {0.0, 1.0} and w.sum() >= 1
    assert split[0]["open_rows"] == whole[0]["open_rows"] > 0


def test_reward_fit_steps_on_the_collected_rows():
    """reward_collect, then reward_fit: the steps run on the weighted rows and move the network; a second collection appends behind the
    first and writes only its own range of weights."""
    from gym_cloth_amd.demos import reward_collect, reward_fit
    v = _env("f32", n_side=10, max_actions=2)
    v.reset()
    tr = _trainer(v)
    noise = np.random.RandomState(14).normal(size=(4, E, 4)) * 0.05
    col = reward_collect(v, tr, n_actions=4, scheme="exp", policy_noise=noise, slots_per_launch=4, temperature=0.5, w_max=4.0)
    before = tr.layers()[0][0].copy()
    first_w = tr.weights()
    fit = reward_fit(v, tr, col, n_steps=3, batch_size=8, seed=0)
    assert fit["rows"] == fit["appended"] == 4 * E and fit["weighted"] == np.count_nonzero(first_w) > 0
    assert fit["losses"].shape == (3,) and np.isfinite(fit["losses"]).all() and not np.array_equal(tr.layers()[0][0], before)
    col2 = reward_collect(v, tr, n_actions=4, scheme="exp", policy_noise=noise, slots_per_launch=4, temperature=0.5, w_max=4.0)
    assert col2["first"] == 4 * E and tr.size() == 8 * E and np.array_equal(_i32(tr.weights(0, 4 * E)), _i32(first_w))
    assert np.array_equal(_i32(tr.weights(4 * E)), _i32(col2["weights"]))
    with pytest.raises(ValueError):
        reward_fit(object(), tr, col2)
    v.close()
