"""GPU tests of the actor-critic from reward: the value network as one more one-row table of the trainer (output width 1
through k_fit_gemm, k_fit_loss<1>) on exactly representable data, within an a-priori bound on Gaussian data, its optimizers bit for bit;
the independence of the critic and the policy on one handle; clothhip_value_predict; clothhip_fit_data_gae against
policies.gae_reference by bytes; the three dataset columns, the zero label source and every refusal; demos.actor_critic_collect. Every
comparison is array_equal or by bytes unless it says otherwise."""
import ctypes as C

import numpy as np
import pytest

from test_actor_critic_host import _records, chain_case
from test_gpu_dagger import E, _env, _layers
from test_gpu_policy_fit import ADAM, OPTIMIZERS, U, _blob, _exact_case, _flat, _gamma, _new_batch, _random_case, _random_layers, _restated_step

pytestmark = pytest.mark.gpu

IDX8, IDX1, IDXR = np.array([7, 2, 11, 0, 5, 9, 4, 1]), np.array([3]), np.array([6, 2, 6, 10, 8, 2, 6, 0])


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def _vblob(b):
    return b.get_value_mlp()


@pytest.fixture(scope="module")
def batch_of():
    """n_side -> ONE ClothBatch of one cloth for the cases that only need a handle to train on (each sets its own networks and data)."""
    made = {}

    def get(n_side):
        if n_side not in made:
            made[n_side] = _new_batch(n_side)
        made[n_side].fit_clear()
        made[n_side].set_policy_mlp(None)
        made[n_side].set_value_mlp(None)
        return made[n_side]
    yield get
    for b in made.values():
        b.close()


def _zero_labels(n):
    return np.zeros((n, 4))


# ---- 1. exact data ------------------------------------------------------------------------------------------------------------------------
def _value_case(widths, dens, seed):
    """test_gpu_policy_fit's _exact_case with a last width of 1: weights and biases in {-1, 0, 1}, rows in {-2 .. 2}; the value targets
    are the first column of its labels, integers in {-3 .. 3}."""
    layers, rows, labels = _exact_case(widths, dens, seed)
    return layers, rows, labels[:, 0].astype(np.float32)


def _value_facts(layers, rows, ret, idx):
    """(the largest sum |a||b| over every inner product of both passes, the fraction of active hidden units, the non-zero count of every
    gradient block), in float64, where all these quantities are exact: g = (v - ret) / B."""
    x, a = rows.astype(np.float64)[idx], ret.astype(np.float64)[idx][:, None]
    B, L = len(idx), len(layers)
    Ws = [W.astype(np.float64) for W, _ in layers]
    hs, worst, active = [x], 0.0, []
    for l in range(L):
        worst = max(worst, (np.abs(hs[-1]) @ np.abs(Ws[l]).T + np.abs(layers[l][1])).max())
        z = hs[-1] @ Ws[l].T + layers[l][1].astype(np.float64)
        if l + 1 < L:
            active.append(z > 0)
        hs.append(np.maximum(z, 0.0) if l + 1 < L else z)
    g = (hs[-1] - a) / float(B)
    worst = max(worst, float(np.abs(hs[-1]).max() + np.abs(a).max()))
    filled = []
    for l in range(L - 1, -1, -1):
        worst = max(worst, (np.abs(g).T @ np.abs(hs[l])).max(), np.abs(g).sum(axis=0).max())
        filled += [int(np.count_nonzero(g.T @ hs[l])), int(np.count_nonzero(g.sum(axis=0)))]
        if l:
            worst = max(worst, (np.abs(g) @ np.abs(Ws[l])).max())
            g = (g @ Ws[l]) * (hs[l] > 0)
    frac = float(np.concatenate([m.reshape(-1) for m in active]).mean()) if active else None
    return worst, frac, filled


def _value_asserts(widths, dens, seed):
    """The preconditions of the exact test, from the float64 reference alone -> (layers, rows, ret). B = 8 (and 1): every quantity of
    both passes is a multiple of 1/8, and 8 sum |a||b| < 2^24 for every inner product, so every partial sum in ANY order is a float32.
    No block of the reference gradient is empty and between a third and two thirds of the hidden units are active at B = 8, so a
    kernel that drops the single output column, row or k of a width-1 tile cannot pass."""
    from gym_cloth_amd.policies import value_fit_reference
    layers, rows, ret = _value_case(widths, dens, seed)
    for idx in (IDX8, IDX1, IDXR):
        worst, frac, filled = _value_facts(layers, rows, ret, idx)
        assert 8.0 * worst < 2.0 ** 24, worst
        loss, grads = value_fit_reference(layers, rows, ret, idx)
        want = _flat(grads)
        assert np.array_equal(want, want.astype(np.float32))                  # the reference's values are float32 values
        if len(idx) == 8:
            assert frac is None or 1.0 / 3.0 <= frac <= 2.0 / 3.0, frac
            assert min(filled) > 0, filled
            assert all(np.count_nonzero(g) > 0 for Wb in grads for g in Wb)
    return layers, rows, ret


VALUE_EXACT_CASES = [  # (n_side, widths, dens, seed): the first seed from 0 for which _value_asserts holds (found on the CPU)
    (10, [300, 5, 1], 1.0, 0),
    (10, [300, 37, 64, 1], 0.3, 0),
    (25, [1875, 37, 64, 1], 0.3, 0),
]


@pytest.mark.parametrize("n_side,widths,dens,seed", VALUE_EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_exact_data_equals_the_value_reference(n_side, widths, dens, seed, batch_of):
    """Small-integer weights, rows and targets, B = 8, B = 1 and a repeated row: the loss and every gradient element EQUAL
    value_fit_reference's. The dataset's labels and weights are not the critic's business: the weights are set to values that would
    change every bit if the critic's loss read them."""
    from gym_cloth_amd.policies import value_fit_reference
    layers, rows, ret = _value_asserts(widths, dens, seed)
    b = batch_of(n_side)
    b.set_value_mlp(layers)
    assert b.fit_append(rows, _zero_labels(len(rows)), weights=np.arange(len(rows)) - 3.0) == len(rows)
    assert np.array_equal(b.fit_get_returns(), np.zeros(len(rows), dtype=np.float32))
    b.fit_set_returns(ret)
    for idx in (IDX8, IDX1, IDXR):
        ref_loss, ref = value_fit_reference(layers, rows, ret, idx)
        loss, grad = b.value_grad(idx)
        assert loss == ref_loss, (loss, ref_loss)
        want = _flat(ref)
        bad = np.nonzero(grad.astype(np.float64) != want)[0]
        assert bad.size == 0, (widths, len(idx), bad[:8], grad[bad[:8]], want[bad[:8]])
    assert np.array_equal(_vblob(b), _flat(layers))                           # nothing was updated


# ---- 2. Gaussian data within an a-priori bound; the split batch sum -------------------------------------------------------------------------
def _value_grad_bound(layers, rows, ret, idx):
    """test_gpu_policy_fit's _grad_bound (Higham's a-priori bounds for float32 inner products in any order, a length-n
    product within gamma_{n+1} sum |a||b| of exact plus the propagated input error) for the critic's loss: g = (v - ret) / B, so
        dg_L = dv / B + 2 u |g|        (the subtraction and the division, one rounding each)
    and the rest of the backward pass as there. The ReLU mask is exact when every hidden pre-activation exceeds its forward bound:
    `margin`, asserted > 0 by the caller. Returns (reference loss, its bound, reference gradients, their bounds as one flat blob,
    margin). Computed, not measured."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)[idx]
    a = np.asarray(ret, dtype=np.float32).astype(np.float64)[idx][:, None]
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
    loss = float((d * d).sum() / (2.0 * B))
    dloss = float((2.0 * np.abs(d) * dhs[-1] + dhs[-1] ** 2).sum() / (2.0 * B)) + 1e-14 * loss
    g = d / float(B)
    dg = dhs[-1] / float(B) + 2.0 * U * np.abs(g)
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


@pytest.mark.parametrize("B", [33, 300])
def test_gaussian_data_within_the_a_priori_bound(B, batch_of):
    """Gaussian weights, uniform rows and targets: the loss and every gradient element lie within the computed bound of the float64
    reference. B = 300 is past FIT_SPLIT_ROWS: the weight gradients' batch sums go through two slabs and k_fit_reduce, with M = 1."""
    from gym_cloth_amd.policies import value_fit_reference
    widths = [300, 37, 64, 1]
    layers, rows, labels, idx = _random_case(widths, B, seed=4)
    ret = labels[:, 0].astype(np.float32)
    ref_loss, dloss, ref, bound, margin = _value_grad_bound(layers, rows, ret, idx)
    assert margin > 0.0, margin
    chk_loss, chk = value_fit_reference(layers, rows, ret, idx)
    assert abs(chk_loss - ref_loss) <= 1e-12 * ref_loss and np.allclose(_flat(chk), _flat(ref), rtol=0, atol=1e-13)
    b = batch_of(10)
    b.set_value_mlp(layers)
    b.fit_append(rows, _zero_labels(len(rows)))
    b.fit_set_returns(ret)
    loss, grad = b.value_grad(idx)
    err = np.abs(grad.astype(np.float64) - _flat(ref))
    print("value %r B %d: mask margin %.3e, loss err %.3e (bound %.3e), max grad err %.3e, max err / bound %.3f, max |grad| %.3e" % (
        widths, B, margin, abs(loss - ref_loss), dloss, err.max(), (err[bound > 0] / bound[bound > 0]).max(), np.abs(grad).max()))
    assert np.isfinite(grad).all() and np.abs(_flat(ref)).max() > 1e-4
    assert abs(loss - ref_loss) <= dloss
    assert (err <= bound).all(), (np.nonzero(err > bound)[0][:8], err.max())


# ---- 3. the optimizers bit for bit; two handles -----------------------------------------------------------------------------------------
def _critic_data(n_rows=40, seed=3, widths=(300, 37, 64, 1)):
    layers, rows, labels, _ = _random_case(list(widths), 7, seed=seed, n_rows=n_rows)
    return layers, rows, labels, labels[:, 1].astype(np.float32)


@pytest.mark.parametrize("name,hyper", OPTIMIZERS, ids=[o[0] for o in OPTIMIZERS])
def test_value_optimizer_steps_bit_for_bit(name, hyper, batch_of):
    """For five steps: g = value_grad(idx_s), then value_fit takes one step on idx_s -- the downloaded blob equals the numpy float32
    restatement of the header's update applied to g. Five steps in one call equal five calls of one; value_fit_reset restarts t and
    the moments."""
    layers, rows, labels, ret = _critic_data()
    table = np.random.RandomState(11).randint(0, len(rows), size=(5, 9)).astype(np.int32)
    b = batch_of(10)
    b.set_value_mlp(layers)
    b.fit_append(rows, labels)
    b.fit_set_returns(ret)
    theta = _vblob(b)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    losses = []
    for s in range(5):
        loss_g, g = b.value_grad(table[s])
        loss = b.value_fit(table[s:s + 1], **hyper)
        assert loss.shape == (1,) and loss[0] == loss_g
        theta, m, v = _restated_step(hyper, theta, m, v, g, s + 1)
        got = _vblob(b)
        assert np.array_equal(_i32(got), _i32(theta)), (name, s, np.abs(got - theta).max())
        losses.append(loss[0])
    assert np.abs(theta - _flat(layers)).max() > 1e-3
    b.set_value_mlp(layers)                                                   # a newly set value network restarts its optimizer
    again = b.value_fit(table, **hyper)
    assert np.array_equal(again, np.array(losses)) and np.array_equal(_i32(_vblob(b)), _i32(theta))
    b.value_fit_reset()
    _, g = b.value_grad(table[1])
    b.value_fit(table[1:2], **hyper)
    first, _, _ = _restated_step(hyper, theta, np.zeros_like(theta), np.zeros_like(theta), g, 1)
    cont, _, _ = _restated_step(hyper, theta, m, v, g, 6)
    assert np.array_equal(_i32(_vblob(b)), _i32(first))
    if name != "sgd":
        assert not np.array_equal(first, cont)


def test_two_handles_give_the_same_bits():
    layers, rows, labels, ret = _critic_data(seed=5)
    table = np.random.RandomState(2).randint(0, len(rows), size=(5, 16))
    got = []
    for k in range(2):
        b = _new_batch(10)
        b.set_value_mlp(layers)
        b.fit_append(rows[:25], labels[:25])
        b.fit_set_returns(ret[:25])
        assert b.fit_append(rows[25:], labels[25:]) == len(rows)              # the columns grew across a reallocation
        b.fit_set_returns(ret[25:], first=25)
        assert np.array_equal(_i32(b.fit_get_returns()), _i32(ret))
        got.append((b.value_fit(table, **ADAM), _vblob(b), b.value_predict(np.arange(len(rows)))))
        b.close()
    for a, c in zip(*got):
        assert a.tobytes() == c.tobytes()
    assert got[0][0][-1] < got[0][0][0]


# ---- 4. independence of the critic and the policy on one handle ----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [9, 300])
def test_the_critic_and_the_policy_do_not_touch_each_other(B):
    """One handle with both networks, a twin that holds the policy alone and never calls a new entry, a twin that holds the critic
    alone. Policy steps and critic steps interleaved on the first: the policy's gradient, loss and blob after 2 + 3 Adam steps are the
    policy twin's after the same steps (so its moments and step count were not touched either: the later steps continue them), and the
    critic's are the critic twin's. fit_gae without WRITE_WEIGHTS and value_predict in between change nothing of the policy."""
    pw, vw = [300, 37, 64, 4], [300, 37, 64, 1]
    _, rows, labels, ret = _critic_data(seed=6)
    pol, val = _random_layers(pw, 60), _random_layers(vw, 61)
    w = np.random.RandomState(4).normal(size=len(rows)).astype(np.float32)
    table = np.random.RandomState(9).randint(0, len(rows), size=(5, B)).astype(np.int32)
    both, p_only, v_only = _new_batch(10), _new_batch(10), _new_batch(10)
    both.set_value_mlp(val)                                                    # the critic first: a policy set afterwards leaves it alone
    both.set_policy_mlp(pol)
    p_only.set_policy_mlp(pol)
    v_only.set_value_mlp(val)
    for x in (both, p_only, v_only):
        x.fit_append(rows, labels, weights=w)
    for x in (both, v_only):
        x.fit_set_returns(ret)
    assert np.array_equal(_i32(_vblob(both)), _i32(_flat(val)))
    lp = [both.fit(table[:2], **ADAM)]
    pol_blob = _blob(both)
    lv = [both.value_fit(table[:3], **ADAM)]
    assert np.array_equal(_i32(_blob(both)), _i32(pol_blob))                   # critic steps: no bit of the policy's blob
    both.fit_gae(0.9, 0.8, write_weights=False)
    ret_gae = both.fit_get_returns()
    both.value_predict(table[0])
    g_both = both.fit_grad(table[2])
    lp.append(both.fit(table[2:], **ADAM))
    val_blob = _vblob(both)
    assert np.array_equal(_i32(both.fit_get_weights()), _i32(w))
    both.fit_set_returns(ret)                                                  # (fit_gae rewrote the targets: the twin did not run it)
    lv.append(both.value_fit(table[3:], **ADAM))
    assert not np.array_equal(_i32(_vblob(both)), _i32(val_blob))
    # the policy twin: the same five steps, no new entry
    lq = [p_only.fit(table[:2], **ADAM)]
    g_twin = p_only.fit_grad(table[2])
    lq.append(p_only.fit(table[2:], **ADAM))
    assert g_both[0] == g_twin[0] and np.array_equal(_i32(g_both[1]), _i32(g_twin[1]))
    assert np.concatenate(lp).tobytes() == np.concatenate(lq).tobytes() and np.array_equal(_i32(_blob(both)), _i32(_blob(p_only)))
    # the critic twin
    lu = [v_only.value_fit(table[:3], **ADAM), v_only.value_fit(table[3:], **ADAM)]
    assert np.concatenate(lv).tobytes() == np.concatenate(lu).tobytes() and np.array_equal(_i32(_vblob(both)), _i32(_vblob(v_only)))
    assert not np.array_equal(ret_gae, ret)
    # dropping or replacing either network leaves the other; a population is no obstacle to the critic
    g0 = both.value_grad(table[0])
    both.set_policy_population([pol, _random_layers(pw, 62)], np.zeros(1, dtype=np.int32))
    g1 = both.value_grad(table[0])
    both.value_fit(table[:1], **ADAM)
    both.set_policy_mlp(None)
    assert g0[0] == g1[0] and np.array_equal(_i32(g0[1]), _i32(g1[1]))
    v_only.value_fit(table[:1], **ADAM)
    assert np.array_equal(_i32(_vblob(both)), _i32(_vblob(v_only)))            # ... nor did the new population restart the critic's optimizer
    p_only.set_value_mlp(val)
    p_only.set_value_mlp(None)
    g2 = p_only.fit_grad(table[2])
    both.set_policy_mlp(unpacked(pw, _blob(p_only)))
    both.set_value_mlp(None)
    g3 = both.fit_grad(table[2])
    assert g2[0] == g3[0] and np.array_equal(_i32(g2[1]), _i32(g3[1]))
    with pytest.raises(Exception):
        both.get_value_mlp()
    for x in (both, p_only, v_only):
        x.close()


def unpacked(widths, blob):
    from gym_cloth_amd.policies import unpack_mlp
    return unpack_mlp(np.asarray(widths), blob)


# ---- 5. value_predict ---------------------------------------------------------------------------------------------------------------------
def _loss_in_the_kernels_order(v, ret):
    """sum (double)(v - ret)^2 as k_fit_loss<1> sums it: thread t of 256 takes elements t, t + 256, ..., then the halving tree."""
    from gym_cloth_amd.policies import _house_sum
    dd = v.astype(np.float64) - ret.astype(np.float64)
    return _house_sum(dd * dd)


@pytest.mark.parametrize("n", [1, 33, 4099])
def test_value_predict_is_the_v_of_the_loss(n, batch_of):
    """value_predict's rows, put through the loss's own arithmetic on the host, give value_grad's loss EXACTLY (n = 4099: per chunk of
    the cap), and a row's v depends on neither its batch nor its chunk."""
    from gym_cloth_amd import _lib
    layers, rows, labels, ret = _critic_data(seed=7)
    b = batch_of(10)
    b.set_value_mlp(layers)
    b.fit_append(rows, labels)
    b.fit_set_returns(ret)
    one = np.concatenate([b.value_predict(np.array([i])) for i in range(len(rows))])
    assert len(set(one.tolist())) == len(rows)
    idx = np.random.RandomState(n).randint(0, len(rows), size=n)
    v = b.value_predict(idx)
    assert v.shape == (n,) and v.dtype == np.float32 and np.array_equal(_i32(v), _i32(one[idx]))
    for lo in range(0, n, _lib.FIT_MAX_BATCH):
        part = slice(lo, min(n, lo + _lib.FIT_MAX_BATCH))
        want = b.value_grad(idx[part])[0]
        got = _loss_in_the_kernels_order(v[part], ret[idx[part]]) / float(2 * len(idx[part]))
        assert got == want and np.isfinite(want) and want > 0, (n, lo, got, want)


# ---- 6. fit_gae -----------------------------------------------------------------------------------------------------------------------------
def _gae_dataset(b, n, seed, rew, nxt, first=0):
    """A critic and `first` + n rows on b; the last n carry (rew, nxt), nxt as indices into the range -> v of the range."""
    r = np.random.RandomState(seed)
    layers = _random_layers([300, 37, 64, 1], seed)
    rows = r.uniform(-1, 1, size=(first + n, 300)).astype(np.float32)
    b.set_value_mlp(layers)
    w0 = r.normal(size=first + n).astype(np.float32)
    assert b.fit_append(rows, _zero_labels(first + n), weights=w0) == first + n
    b.fit_set_transitions(rew, np.where(np.asarray(nxt) >= 0, np.asarray(nxt) + first, nxt), first=first)
    return b.value_predict(np.arange(first, first + n)), w0


def _check_gae(b, v, w0, rew, nxt, first, gamma, lam):
    """adv, ret and the weight column against gae_reference by bytes: without WRITE_WEIGHTS, then plain and normalised at two scales."""
    from gym_cloth_amd.policies import NEXT_NONE, gae_reference
    n = len(v)
    leaf = np.asarray(nxt) == NEXT_NONE
    ret0 = b.fit_get_returns()
    adv_r, ret_r, _ = gae_reference(v, rew, nxt, gamma, lam)
    adv, ret = b.fit_gae(gamma, lam, first=first, n=n, write_weights=False)
    assert adv.tobytes() == adv_r.tobytes() and ret.tobytes() == ret_r.tobytes()
    assert b.fit_get_weights().tobytes() == w0.tobytes()                      # without WRITE_WEIGHTS the column keeps its bytes
    stored = b.fit_get_returns()
    assert stored[first:].tobytes() == ret_r.tobytes() and stored[:first].tobytes() == ret0[:first].tobytes()
    assert np.array_equal(_i32(ret[leaf]), _i32(v[leaf])) and not adv[leaf].any()
    for normalize in (False, True):
        for scale in (0.5, 8.0):
            _, _, w_r = gae_reference(v, rew, nxt, gamma, lam, w_scale=scale, normalize=normalize)
            again = b.fit_gae(gamma, lam, first=first, n=n, write_weights=True, normalize=normalize, w_scale=scale)
            assert again[0].tobytes() == adv_r.tobytes() and again[1].tobytes() == ret_r.tobytes()      # two runs: the same bits
            w = b.fit_get_weights()
            assert w[first:].tobytes() == w_r.tobytes(), (normalize, scale, np.abs(w[first:] - w_r).max())
            assert w[:first].tobytes() == w0[:first].tobytes() and not w[first:][leaf].any()
            assert np.isfinite(w_r).all() and (n == 1 or np.count_nonzero(w_r) > 0)
    assert b.fit_gae(gamma, lam, first=first, n=n, want=False) is None
    return adv_r


def test_gae_on_the_hand_made_chains(batch_of):
    """The twelve rows of the host test (a chain of one, of five, two interleaved, a terminal row, a chain ending in a leaf) behind
    five rows that are not part of the range, and n = 1."""
    rew, nxt, _ = chain_case()
    for first in (0, 5):
        b = batch_of(10)
        v, w0 = _gae_dataset(b, 12, 30 + first, rew, nxt, first=first)
        adv = _check_gae(b, v, w0, rew, nxt, first, 0.99, 0.95)
        assert np.count_nonzero(adv) == 11
        _check_gae(b, v, b.fit_get_weights(), rew, nxt, first, 0.9, 0.0)
    for k, (r1, n1) in enumerate([(np.float32(1.5), -1), (np.float32(0.0), -2)]):                    # n = 1: a terminal row, a lone leaf
        b = batch_of(10)
        v, w0 = _gae_dataset(b, 1, 40 + k, np.array([r1]), np.array([n1]))
        _check_gae(b, v, w0, np.array([r1]), np.array([n1]), 0, 1.0, 1.0)


def test_gae_across_the_chunk_boundary(batch_of):
    """4099 rows of seven interleaved envs with episodes of random length: chains (successor = 7 rows on) cross row 4096, where the
    critic's forward starts its second chunk; the last row of every env is terminal or a leaf."""
    from gym_cloth_amd.demos import episode_links
    from gym_cloth_amd.policies import NEXT_NONE, NEXT_TERMINAL
    n = 4099
    r = np.random.RandomState(77)
    nxt = episode_links(np.arange(n) % 7, np.arange(n) // 7, r.random_sample(n) < 0.12, 7, first=0)
    rew = r.normal(size=n).astype(np.float32)
    assert (nxt[4089:4096] >= 4096).any() and (nxt == NEXT_NONE).any() and (nxt == NEXT_TERMINAL).any()
    b = batch_of(10)
    v, w0 = _gae_dataset(b, n, 50, rew, nxt)
    _check_gae(b, v, w0, rew, nxt, 0, 0.99, 0.95)


def test_gae_with_a_zero_critic_is_returns_to_go(batch_of):
    """An all-zero critic, gamma = lam = 1, small-integer rewards: adv EQUALS demos.returns_to_go of the same records."""
    from gym_cloth_amd.demos import episode_links, returns_to_go
    rew, ran, done, rb = _records(1)
    T, En = rew.shape
    G, _ = returns_to_go(rew, ran, done, rb, gamma=1.0)
    t_, e_ = np.nonzero(ran)
    last_open = np.array([e for e in range(En) if not done[np.nonzero(ran[:, e])[0][-1], e]], dtype=np.int64)
    nxt = episode_links(np.concatenate([e_, last_open]), np.concatenate([t_, np.full(len(last_open), T)]),
                        np.concatenate([done[t_, e_], np.zeros(len(last_open), dtype=bool)]), En, first=0)
    r32 = np.concatenate([rew[t_, e_], np.zeros(len(last_open))]).astype(np.float32)
    n = len(r32)
    b = batch_of(10)
    b.set_value_mlp([(np.zeros((5, 300), dtype=np.float32), np.zeros(5, dtype=np.float32)), (np.zeros((1, 5), dtype=np.float32), np.zeros(1, dtype=np.float32))])
    b.fit_append(np.random.RandomState(3).uniform(-1, 1, size=(n, 300)), _zero_labels(n))
    b.fit_set_transitions(r32, nxt)
    assert not b.value_predict(np.arange(n)).any()
    adv, ret = b.fit_gae(1.0, 1.0, write_weights=True)
    assert len(last_open) > 0 and np.array_equal(adv[:len(t_)].astype(np.float64), G[t_, e_]) and np.abs(G[t_, e_]).max() > 1
    assert np.array_equal(ret, adv) and np.array_equal(b.fit_get_weights(), adv) and not adv[len(t_):].any()


# ---- 7. storage, the zero label source, refusals ------------------------------------------------------------------------------------------
def test_columns_defaults_growth_and_clear(batch_of):
    from gym_cloth_amd import _lib
    layers, rows, labels, ret = _critic_data(seed=8)
    b = batch_of(10)
    n = len(rows)
    assert n < 64 and b.fit_append(rows, labels) == n
    rew, nxt = b.fit_get_transitions()
    assert rew.dtype == np.float32 and nxt.dtype == np.int32 and not rew.any() and (nxt == _lib.FIT_NEXT_NONE).all() and not b.fit_get_returns().any()
    r = np.random.RandomState(2)
    rew1 = r.normal(size=n).astype(np.float32)
    nxt1 = np.where(r.random_sample(n) < 0.3, _lib.FIT_NEXT_TERMINAL, np.minimum(np.arange(n) + 1 + r.randint(0, 3, size=n), n - 1)).astype(np.int32)
    nxt1[-1] = _lib.FIT_NEXT_NONE
    b.fit_set_transitions(rew1, nxt1)
    b.fit_set_returns(ret)
    assert b.fit_append(rows, labels) == 2 * n > 64                            # grows the tables: the columns are kept, the new rows default
    b.fit_set_transitions(-rew1[:5], np.array([2 * n - 1, -1, -2, n + 9, n + 10]), first=n + 2)
    b.fit_set_returns(2 * ret[:3], first=2 * n - 3)
    rew, nxt = b.fit_get_transitions()
    want_rew, want_nxt, want_ret = np.concatenate([rew1, np.zeros(n, dtype=np.float32)]), np.concatenate([nxt1, np.full(n, -2, dtype=np.int32)]), np.concatenate([ret, np.zeros(n, dtype=np.float32)])
    want_rew[n + 2:n + 7], want_nxt[n + 2:n + 7], want_ret[2 * n - 3:] = -rew1[:5], [2 * n - 1, -1, -2, n + 9, n + 10], 2 * ret[:3]
    assert np.array_equal(_i32(rew), _i32(want_rew)) and np.array_equal(nxt, want_nxt) and np.array_equal(_i32(b.fit_get_returns()), _i32(want_ret))
    part = b.fit_get_transitions(n + 1, 4)
    assert np.array_equal(part[1], want_nxt[n + 1:n + 5]) and np.array_equal(_i32(b.fit_get_returns(3, 2)), _i32(want_ret[3:5]))
    b.fit_clear()
    assert b.fit_size() == 0 and b.fit_get_returns().shape == (0,) and b.fit_get_transitions()[1].shape == (0,)
    assert b.fit_append(rows[:3], labels[:3]) == 3
    rew, nxt = b.fit_get_transitions()
    assert not rew.any() and (nxt == -2).all() and not b.fit_get_returns().any()  # nothing of the cleared rows shows


def test_zero_label_rows_against_the_downloaded_table():
    """labels="zero": the observation is the named row of the launch's table, the label (0, 0, 0, 0) whatever label_row says -- no
    expert was armed, and a label row far outside the table is ignored; the transition columns get their defaults."""
    from gym_cloth_amd import _lib
    from gym_cloth_amd.policies import MLPTrainer
    v = _env("f32", n_side=10, max_actions=2)
    v.reset()
    tr = MLPTrainer(v, _layers([3 * v.P, 5, 4], 21))
    v.batch.fit_hold()
    out = v.step_many(policy="mlp", n_actions=3, want_obs=True)
    t_, e_ = np.nonzero(out["ran"])
    rows = np.stack([np.full(len(t_), _lib.FIT_SRC_SLOTS), t_ * E + e_, np.full(len(t_), 10 ** 6)], axis=1)
    w = np.random.RandomState(1).normal(size=len(rows)).astype(np.float32)
    assert tr.append_launch(rows, labels="zero", weights=w) == len(rows)
    obs, lab = tr.data()
    assert np.array_equal(obs, out["obs_t"][t_, e_]) and lab.shape == (len(rows), 4) and not lab.any() and len({o.tobytes() for o in obs}) == len(rows)
    assert np.array_equal(_i32(tr.weights()), _i32(w)) and (v.batch.fit_get_transitions()[1] == _lib.FIT_NEXT_NONE).all()
    held = np.array([[_lib.FIT_SRC_HELD, 2, -7]])
    assert tr.append_launch(held, labels="zero") == len(rows) + 1 and not tr.data(len(rows))[1].any()
    v.close()


def test_refusals_change_nothing():
    from gym_cloth_amd import _lib
    v = _env("f32", n_side=10, max_actions=2)
    v.reset()
    b, L, h = v.batch, v.batch._L, v.batch._h
    pol, val = _layers([300, 5, 4], 1), _layers([300, 5, 1], 2)
    b.set_policy_mlp(pol)
    b.set_value_mlp(val)
    r = np.random.RandomState(0)
    n = 10
    rows, labels = r.uniform(-1, 1, size=(n, 300)).astype(np.float32), r.uniform(-1, 1, size=(n, 4))
    w, ret, rew = (r.normal(size=n).astype(np.float32) for _ in range(3))
    nxt = np.array([2, 3, 4, 5, -1, -1, 8, 9, -2, -2], dtype=np.int32)
    b.fit_append(rows, labels, weights=w)
    b.fit_set_transitions(rew, nxt)
    b.fit_set_returns(ret)
    idx = np.arange(8, dtype=np.int32)
    snap = (b.fit_grad(idx), b.value_grad(idx), _blob(b), _vblob(b))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = _lib.i32p

    def unchanged():
        assert b.fit_size() == n and np.array_equal(_i32(b.fit_get_weights()), _i32(w)) and np.array_equal(_i32(b.fit_get_returns()), _i32(ret))
        r_, n_ = b.fit_get_transitions()
        assert np.array_equal(_i32(r_), _i32(rew)) and np.array_equal(n_, nxt)
        o, l = b.fit_data()
        assert np.array_equal(o, rows) and np.array_equal(l, labels.astype(np.float32))
        now = (b.fit_grad(idx), b.value_grad(idx), _blob(b), _vblob(b))
        assert now[0][0] == snap[0][0] and now[1][0] == snap[1][0]
        for a, c in ((now[0][1], snap[0][1]), (now[1][1], snap[1][1]), (now[2], snap[2]), (now[3], snap[3])):
            assert np.array_equal(_i32(a), _i32(c))

    two, two_i, out2 = np.array([0.5, -0.5], dtype=np.float32), np.array([-1, -2], dtype=np.int32), np.zeros(n + 1, dtype=np.float32)
    # the transitions and the returns: a range outside the dataset, a value that is not finite, a NULL table
    for first, k in ((n - 1, 2), (n, 1), (-1, 1), (0, n + 1), (2, -1)):
        assert L.clothhip_fit_data_set_transitions(h, first, k, fp(out2), ip(np.full(n + 1, -1, dtype=np.int32))) == _lib.EINVAL
        assert L.clothhip_fit_data_get_transitions(h, first, k, fp(out2.copy()), ip(np.zeros(n + 1, dtype=np.int32))) == _lib.EINVAL
        assert L.clothhip_fit_data_set_returns(h, first, k, fp(out2)) == _lib.EINVAL and L.clothhip_fit_data_get_returns(h, first, k, fp(out2.copy())) == _lib.EINVAL
        assert L.clothhip_fit_data_gae(h, first, k, C.byref(_lib.ClothGaeParams(0.9, 0.9, 1.0, 0)), None, None) == _lib.EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        vb = np.array([1.0, bad], dtype=np.float32)
        assert L.clothhip_fit_data_set_transitions(h, 0, 2, fp(vb), ip(two_i)) == _lib.EINVAL
        assert L.clothhip_fit_data_set_returns(h, 0, 2, fp(vb)) == _lib.EINVAL
    assert L.clothhip_fit_data_set_transitions(h, 0, 2, None, ip(two_i)) == _lib.EINVAL and L.clothhip_fit_data_set_transitions(h, 0, 2, fp(two), None) == _lib.EINVAL
    assert L.clothhip_fit_data_get_transitions(h, 0, 2, None, ip(two_i.copy())) == _lib.EINVAL and L.clothhip_fit_data_get_transitions(h, 0, 2, fp(two.copy()), None) == _lib.EINVAL
    assert L.clothhip_fit_data_set_returns(h, 0, 2, None) == _lib.EINVAL and L.clothhip_fit_data_get_returns(h, 0, 2, None) == _lib.EINVAL
    assert L.clothhip_fit_data_set_returns(h, n, 0, None) == _lib.OK and L.clothhip_fit_data_set_transitions(h, n, 0, None, None) == _lib.OK
    # a self link, a backward link, a link past the end, an unknown mark: nothing is written, not even the valid first entry
    for link in (3, 2, 0, n, n + 5, -3):
        assert L.clothhip_fit_data_set_transitions(h, 2, 2, fp(two), ip(np.array([-1, link], dtype=np.int32))) == _lib.EINVAL, link
    with pytest.raises(ValueError):
        b.fit_set_transitions(two, np.array([0, -1]), first=0)
    unchanged()
    # the critic's entries
    g, loss, y = np.zeros(b._val_n_params, dtype=np.float32), np.zeros(1), np.zeros(8, dtype=np.float32)
    adam = _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert L.clothhip_value_fit_grad(h, ip(idx), 0, fp(g), _lib.dp(loss)) == _lib.EINVAL and L.clothhip_value_fit_grad(h, ip(idx), _lib.FIT_MAX_BATCH + 1, fp(g), _lib.dp(loss)) == _lib.EINVAL
    assert L.clothhip_value_fit_grad(h, None, 8, fp(g), _lib.dp(loss)) == _lib.EINVAL
    assert L.clothhip_value_fit_grad(h, ip(np.array([0, n], dtype=np.int32)), 2, fp(g), _lib.dp(loss)) == _lib.EINVAL
    assert L.clothhip_value_fit(h, None, ip(idx), 1, 8, None) == _lib.EINVAL and L.clothhip_value_fit(h, C.byref(adam), ip(idx), -1, 8, None) == _lib.EINVAL
    assert L.clothhip_value_fit(h, C.byref(adam), ip(np.array([0, -1], dtype=np.int32)), 1, 2, None) == _lib.EINVAL
    for field, bad in (("optimizer", 2.0), ("lr", -1.0), ("lr", np.nan), ("beta1", 1.0), ("beta2", 1.5), ("eps", np.inf), ("momentum", -0.1)):
        p = _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
        setattr(p, field, bad)
        assert L.clothhip_value_fit(h, C.byref(p), ip(idx), 1, 8, None) == _lib.EINVAL, field
    assert L.clothhip_value_fit(h, C.byref(adam), ip(idx), 0, 8, None) == _lib.OK             # no steps: nothing changes
    assert L.clothhip_value_predict(h, ip(idx), 0, fp(y)) == _lib.EINVAL and L.clothhip_value_predict(h, None, 8, fp(y)) == _lib.EINVAL
    assert L.clothhip_value_predict(h, ip(idx), 8, None) == _lib.EINVAL and L.clothhip_value_predict(h, ip(np.array([0, n], dtype=np.int32)), 2, fp(y)) == _lib.EINVAL
    # the value network's shape rules: a refused call keeps the earlier one
    wd, blob = np.array([300, 5, 1], dtype=np.int32), _flat(val)
    for widths, n_par in ((np.array([300, 5, 4], dtype=np.int32), blob.size), (np.array([299, 5, 1], dtype=np.int32), blob.size), (np.array([300, 257, 1], dtype=np.int32), blob.size),
                          (wd, blob.size - 1)):
        assert L.clothhip_set_value_mlp(h, 2, ip(widths), fp(blob), n_par) == _lib.EINVAL
    assert L.clothhip_set_value_mlp(h, 5, ip(np.array([300, 5, 5, 5, 5, 1], dtype=np.int32)), fp(blob), blob.size) == _lib.EINVAL
    assert L.clothhip_set_value_mlp(h, 2, ip(wd), None, blob.size) == _lib.EINVAL and L.clothhip_set_value_mlp(h, 2, None, fp(blob), blob.size) == _lib.EINVAL
    assert L.clothhip_get_value_mlp(h, fp(g), g.size + 1) == _lib.EINVAL and L.clothhip_get_value_mlp(h, None, g.size) == _lib.EINVAL
    unchanged()
    # fit_gae: the parameters, unknown flags, a successor outside the range
    G = _lib.ClothGaeParams
    for p in (G(np.nan, 0.9, 1.0, 1), G(0.9, np.inf, 1.0, 1), G(0.9, 0.9, np.nan, 1), G(1.5, 0.9, 1.0, 1), G(-0.1, 0.9, 1.0, 1), G(0.9, 1.01, 1.0, 1), G(0.9, -1e-9, 1.0, 1),
              G(0.9, 0.9, 1.0, 4), G(0.9, 0.9, 1.0, -1)):
        assert L.clothhip_fit_data_gae(h, 0, n, C.byref(p), None, None) == _lib.EINVAL
    assert L.clothhip_fit_data_gae(h, 0, n, None, None, None) == _lib.EINVAL
    ok = G(0.9, 0.9, 1.0, 3)
    assert L.clothhip_fit_data_gae(h, 0, 8, C.byref(ok), None, None) == _lib.EINVAL            # rows 6, 7 point at 8, 9
    assert L.clothhip_fit_data_gae(h, 0, 5, C.byref(ok), None, None) == _lib.EINVAL            # row 3 points at 5
    assert L.clothhip_fit_data_gae(h, 4, 0, C.byref(ok), None, None) == _lib.OK                # an empty range
    unchanged()
    # a launch in flight
    nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, E, 4)))
    assert L.clothhip_fit_data_set_transitions(h, 0, 2, fp(two), ip(two_i)) == _lib.ESTATE and L.clothhip_fit_data_get_transitions(h, 0, 2, fp(two.copy()), ip(two_i.copy())) == _lib.ESTATE
    assert L.clothhip_fit_data_set_returns(h, 0, 2, fp(two)) == _lib.ESTATE and L.clothhip_fit_data_get_returns(h, 0, 2, fp(two.copy())) == _lib.ESTATE
    assert L.clothhip_value_fit_grad(h, ip(idx), 8, fp(g), _lib.dp(loss)) == _lib.ESTATE and L.clothhip_value_fit(h, C.byref(adam), ip(idx), 1, 8, None) == _lib.ESTATE
    assert L.clothhip_value_predict(h, ip(idx), 8, fp(y)) == _lib.ESTATE and L.clothhip_value_fit_reset(h) == _lib.ESTATE
    assert L.clothhip_fit_data_gae(h, 0, n, C.byref(ok), None, None) == _lib.ESTATE
    assert L.clothhip_set_value_mlp(h, 2, ip(wd), fp(blob), blob.size) == _lib.ESTATE and L.clothhip_set_value_mlp(h, 0, None, None, 0) == _lib.ESTATE
    assert L.clothhip_get_value_mlp(h, fp(g), g.size) == _lib.ESTATE
    assert L.clothhip_fit_data_append_launch_ex(h, ip(np.array([[_lib.FIT_SRC_HELD, 0, 0]], dtype=np.int32)), 1, _lib.FIT_LABEL_ZERO, None) == _lib.ESTATE
    b.run_actions_end()
    unchanged()
    # the zero label source still needs its observation: no held rows, no kept table
    assert L.clothhip_fit_data_append_launch_ex(h, ip(np.array([[_lib.FIT_SRC_HELD, 0, 0]], dtype=np.int32)), 1, _lib.FIT_LABEL_ZERO, None) == _lib.ESTATE
    assert L.clothhip_fit_data_append_launch_ex(h, ip(np.array([[_lib.FIT_SRC_SLOTS, 0, 0]], dtype=np.int32)), 1, _lib.FIT_LABEL_ZERO, None) == _lib.ESTATE
    assert L.clothhip_fit_data_append_launch_ex(h, ip(np.array([[7, 0, 0]], dtype=np.int32)), 1, _lib.FIT_LABEL_ZERO, None) == _lib.EINVAL
    assert L.clothhip_fit_data_append_launch_ex(h, ip(np.array([[_lib.FIT_SRC_HELD, 0, 0]], dtype=np.int32)), 1, _lib.FIT_LABEL_ZERO, fp(np.array([np.nan], dtype=np.float32))) == _lib.EINVAL
    unchanged()
    # no critic (these change the handle, so they come last): the policy and the dataset stay
    b.set_value_mlp(None)
    assert L.clothhip_value_fit_grad(h, ip(idx), 8, fp(g), _lib.dp(loss)) == _lib.ESTATE and L.clothhip_value_fit(h, C.byref(adam), ip(idx), 1, 8, None) == _lib.ESTATE
    assert L.clothhip_value_predict(h, ip(idx), 8, fp(y)) == _lib.ESTATE and L.clothhip_get_value_mlp(h, fp(g), g.size) == _lib.ESTATE
    assert L.clothhip_fit_data_gae(h, 0, n, C.byref(ok), None, None) == _lib.ESTATE and L.clothhip_value_fit_reset(h) == _lib.OK
    now = b.fit_grad(idx)
    assert now[0] == snap[0][0] and np.array_equal(_i32(now[1]), _i32(snap[0][1])) and np.array_equal(_i32(b.fit_get_returns()), _i32(ret))
    # an empty dataset
    b.set_value_mlp(val)
    b.fit_clear()
    assert L.clothhip_value_fit_grad(h, ip(idx), 8, fp(g), _lib.dp(loss)) == _lib.ESTATE and L.clothhip_value_predict(h, ip(idx), 8, fp(y)) == _lib.ESTATE
    v.close()


# ---- 8. actor_critic_collect --------------------------------------------------------------------------------------------------------------
N_COLLECT = 3


def _collect(slots_per_launch):
    from gym_cloth_amd.demos import actor_critic_collect
    from gym_cloth_amd.policies import MLPTrainer
    v = _env("f32", n_side=10, max_actions=2)
    v.reset()
    tr = MLPTrainer(v, _layers([3 * v.P, 5, 4], 21))
    noise = np.random.RandomState(13).normal(size=(N_COLLECT, E, 4)) * 0.05
    col = actor_critic_collect(v, tr, n_actions=N_COLLECT, policy_noise=noise, slots_per_launch=slots_per_launch, max_launches=8)
    obs, lab = tr.data()
    rew, nxt = v.batch.fit_get_transitions()
    res = (col, obs, lab, tr.weights(), rew, nxt, v.batch.fit_get_returns())
    v.close()
    return res


def test_actor_critic_collect_is_deterministic_and_does_not_depend_on_the_launches():
    """Two collections from the same seeds store the same bytes in every column. Episodes last two actions at the most and three slots
    per env are collected, so some envs' third row belongs to an episode the collection does not see the end of: its successor is the
    env's LEAF, the state after that slot, appended in the same launch. Every stored link is TERMINAL, or a later row of the same env, or its leaf. A
    collection in launches of 2 slots stores, env by env, the rows of the collection in one launch of 4."""
    from gym_cloth_amd import _lib
    one, again = _collect(4), _collect(4)
    for a, c in zip(one[1:], again[1:]):
        assert a.tobytes() == c.tobytes()
    col, obs, lab, w, rew, nxt, ret = one
    n = len(obs)
    last = (col["ds_slot"] == N_COLLECT - 1) & ~col["leaf"]
    open_envs = col["ds_env"][last & ~col["done"]]                             # the envs whose last collected slot left its episode open
    assert last.sum() == E and 0 < len(open_envs) < E                          # both kinds of last row are met
    assert col["appended"] == N_COLLECT * E and col["open_rows"] == int(col["leaf"].sum()) == len(open_envs) and n == col["appended"] + col["open_rows"] == col["rows"]
    assert np.array_equal(np.sort(col["ds_env"][col["leaf"]]), np.sort(open_envs))
    assert col["launches"] == 1 and col["first"] == 0 and np.array_equal(nxt, col["next"]) and np.array_equal(_i32(rew), _i32(col["rew"]))
    assert not w.any() and not ret.any() and not lab[col["leaf"]].any() and lab[~col["leaf"]].any(axis=1).all() and not rew[col["leaf"]].any()
    assert np.array_equal(col["nonleaf"], np.nonzero(~col["leaf"])[0]) and len(col["episode_return"]) == int(col["done"].sum()) >= E
    for i in range(n):
        e = col["ds_env"][i]
        if col["leaf"][i]:
            assert nxt[i] == _lib.FIT_NEXT_NONE and col["ds_slot"][i] == N_COLLECT
        elif col["done"][i]:
            assert nxt[i] == _lib.FIT_NEXT_TERMINAL
        else:
            k = nxt[i]
            assert i < k < n and col["ds_env"][k] == e and col["ds_slot"][k] == col["ds_slot"][i] + 1
            assert col["leaf"][k] == (col["ds_slot"][i] == N_COLLECT - 1)
    assert col["done"].any() and (nxt >= 0).sum() >= E
    for e in range(E):                                                         # every env's chain ends in TERMINAL or in its leaf
        assert nxt[np.nonzero(col["ds_env"] == e)[0][-1]] == (_lib.FIT_NEXT_NONE if e in open_envs else _lib.FIT_NEXT_TERMINAL)
    whole, split = one, _collect(2)
    assert split[0]["launches"] == 2 and split[0]["appended"] == whole[0]["appended"] and split[0]["open_rows"] == whole[0]["open_rows"]
    for e in range(E):
        ia, ib = np.nonzero(whole[0]["ds_env"] == e)[0], np.nonzero(split[0]["ds_env"] == e)[0]
        assert np.array_equal(whole[0]["ds_slot"][ia], np.arange(N_COLLECT + (e in open_envs))) and np.array_equal(split[0]["ds_slot"][ib], whole[0]["ds_slot"][ia])
        for k in (1, 2, 3, 4, 6):
            assert whole[k][ia].tobytes() == split[k][ib].tobytes(), (e, k)
        # the links, row numbers aside: the same shape of chain
        la, lb = whole[5][ia], split[5][ib]
        assert np.array_equal(la < 0, lb < 0) and np.array_equal(la[la < 0], lb[lb < 0])
        assert np.array_equal(np.searchsorted(ia, la[la >= 0]), np.searchsorted(ib, lb[lb >= 0]))
    assert len({o.tobytes() for o in obs}) == n                               # every row another state: the leaves are not copies


def test_actor_critic_fit_steps_both_networks():
    """actor_critic_collect, then actor_critic_fit: one fit_gae call writes targets and weights that equal gae_reference's of the
    critic's own predictions, the critic steps run on the non-leaf rows only, the policy steps under the written weights; a second
    collection appends behind the first and leaves its columns alone."""
    from gym_cloth_amd.demos import actor_critic_collect, actor_critic_fit
    from gym_cloth_amd.policies import MLPTrainer, ValueTrainer, gae_reference
    v = _env("f32", n_side=10, max_actions=2)
    v.reset()
    tr = MLPTrainer(v, _layers([3 * v.P, 5, 4], 21))
    critic = ValueTrainer(v, _layers([3 * v.P, 6, 1], 22), lr=1e-2)
    noise = np.random.RandomState(14).normal(size=(4, E, 4)) * 0.05
    col = actor_critic_collect(v, tr, n_actions=4, policy_noise=noise, slots_per_launch=4)
    n = col["appended"] + col["open_rows"]
    v0 = critic.predict(np.arange(n))
    pol0, val0 = tr.layers()[0][0].copy(), critic.layers()[0][0].copy()
    fit = actor_critic_fit(v, tr, critic, col, gamma=0.9, lam=0.8, n_value_steps=3, n_policy_steps=3, batch_size=8, seed=0, normalize=True, w_scale=0.5)
    adv_r, ret_r, w_r = gae_reference(v0, col["rew"], col["next"], 0.9, 0.8, w_scale=0.5, normalize=True)
    assert fit["adv"].tobytes() == adv_r.tobytes() and fit["ret"].tobytes() == ret_r.tobytes() and tr.weights().tobytes() == w_r.tobytes()
    assert v.batch.fit_get_returns().tobytes() == ret_r.tobytes() and np.count_nonzero(w_r) == col["appended"] and col["open_rows"] > 0
    assert fit["value_losses"].shape == (3,) and fit["policy_losses"].shape == (3,) and np.isfinite(fit["value_losses"]).all() and np.isfinite(fit["policy_losses"]).all()
    assert not np.array_equal(tr.layers()[0][0], pol0) and not np.array_equal(critic.layers()[0][0], val0)
    table = col["nonleaf"].astype(np.int32)[MLPTrainer.index_table(len(col["nonleaf"]), 3, 8, 0)]
    assert not col["leaf"][table].any()
    loss, grads = critic.grad(col["nonleaf"][:8])
    assert np.isfinite(loss) and len(grads) == 2 and grads[1][0].shape == (1, 6)
    col2 = actor_critic_collect(v, tr, n_actions=4, policy_noise=noise, slots_per_launch=4)
    assert col2["first"] == n and tr.size() == n + col2["appended"] + col2["open_rows"]
    assert tr.weights(0, n).tobytes() == w_r.tobytes() and v.batch.fit_get_returns(0, n).tobytes() == ret_r.tobytes()
    assert np.array_equal(v.batch.fit_get_transitions(0, n)[1], col["next"]) and (col2["next"][col2["next"] >= 0] >= n).all()
    critic.reset()
    with pytest.raises(ValueError):
        actor_critic_fit(object(), tr, critic, col2)
    v.close()
