"""GPU tests of the trainer of the shared policy network (csrc/cloth_policy_fit.hpp, clothhip_fit_data_* / clothhip_policy_fit*):
loss and gradient on exactly representable data, element for element equal to the float64 numpy reference; on random data within an
a-priori rounding bound; the optimizers bit for bit against their float32 numpy restatements; determinism and the hand-over of the
fitted blob to the evaluation and to the episode launch; a fit that learns; every refusal of the header."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_env import base_cfg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                           # unit roundoff of float32


def _gamma(k):
    return k * U / (1.0 - k * U)


def _random_layers(widths, seed):
    """Weights from a seeded RandomState with scale 1 / sqrt(fan-in), rounded to float32 (as test_gpu_mlp_policy.py draws them)."""
    r = np.random.RandomState(seed)
    return [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32),
             (r.normal(size=widths[l + 1]) / np.sqrt(widths[l])).astype(np.float32)) for l in range(len(widths) - 1)]


def _cfg(n_side):
    cfg = base_cfg("tier1", 1337)
    cfg["cloth"]["num_width_points"] = cfg["cloth"]["num_height_points"] = n_side
    cfg["env"]["force_grab"] = True
    return cfg


_batches = {}


@pytest.fixture(scope="module")
def batch_of():
    """n_side -> ONE ClothBatch of one cloth, shared by the cases that only need a handle to train on (each sets its own network and
    clears the dataset first)."""
    def get(n_side):
        if n_side not in _batches:
            from gym_cloth_amd.batch import ClothBatch
            _batches[n_side] = ClothBatch(_cfg(n_side), n_envs=1, precision="f32")
        b = _batches[n_side]
        b.fit_clear()
        return b
    yield get
    for b in _batches.values():
        b.close()
    _batches.clear()


def _new_batch(n_side=10, precision="f32", E=1):
    from gym_cloth_amd.batch import ClothBatch
    return ClothBatch(_cfg(n_side), n_envs=E, precision=precision)


def _blob(b):
    return b.get_policy_mlp(0, b._mlp_n_params)


def _flat(grads):
    return np.concatenate([np.concatenate([np.asarray(W).reshape(-1), np.asarray(bb).reshape(-1)]) for W, bb in grads])


# ---- 1. exact data ------------------------------------------------------------------------------------------------------------------------
def _exact_case(widths, dens, seed, n_rows=12):
    """Weights in {-1, 0, 1} with a fraction dens non-zero, biases in {-1, 0, 1}, rows in {-2 .. 2}, labels in {-3 .. 3}: independent
    draws, so asymmetric in every index."""
    r = np.random.RandomState(seed)
    layers = []
    for l in range(len(widths) - 1):
        shape = (widths[l + 1], widths[l])
        W = (r.randint(0, 2, size=shape) * 2 - 1) * (r.random_sample(shape) < dens)
        layers.append((W.astype(np.float32), r.randint(-1, 2, size=widths[l + 1]).astype(np.float32)))
    rows = r.randint(-2, 3, size=(n_rows, widths[0])).astype(np.float32)
    labels = r.randint(-3, 4, size=(n_rows, 4)).astype(np.float64)
    return layers, rows, labels


def _exact_facts(layers, rows, labels, idx):
    """(the largest sum |a||b| over every inner product of the forward and the backward pass, the fraction of active hidden units,
    per gradient block the fraction of non-zero entries), in float64, where all these quantities are exact."""
    x = rows.astype(np.float64)[idx]
    a = labels[idx]
    B, L = len(idx), len(layers)
    Ws = [W.astype(np.float64) for W, _ in layers]
    hs, worst, active = [x], 0.0, []
    for l in range(L):
        worst = max(worst, (np.abs(hs[-1]) @ np.abs(Ws[l]).T + np.abs(layers[l][1])).max())
        z = hs[-1] @ Ws[l].T + layers[l][1].astype(np.float64)
        if l + 1 < L:
            active.append(z > 0)
        hs.append(np.maximum(z, 0.0) if l + 1 < L else z)
    g = (hs[-1] - a) / (2.0 * B)
    fill = []
    for l in range(L - 1, -1, -1):
        worst = max(worst, (np.abs(g).T @ np.abs(hs[l])).max(), np.abs(g).sum(axis=0).max())
        fill += [np.count_nonzero(g.T @ hs[l]) / float(g.shape[1] * hs[l].shape[1]), np.count_nonzero(g.sum(axis=0)) / float(g.shape[1])]
        if l:
            worst = max(worst, (np.abs(g) @ np.abs(Ws[l])).max())
            g = (g @ Ws[l]) * (hs[l] > 0)
    frac = float(np.concatenate([m.reshape(-1) for m in active]).mean()) if active else None
    return worst, frac, fill


EXACT_CASES = [  # (n_side, widths, dens, seed): the seed is the first from 0 for which the asserts of the test hold (checked on the CPU)
    (10, [300, 4], 1.0, 0),
    (10, [300, 5, 4], 1.0, 0),
    (10, [300, 37, 64, 4], 0.3, 0),
    (10, [300, 256, 256, 256, 4], 0.06, 1),
    (25, [1875, 37, 64, 4], 0.3, 0),
]


@pytest.mark.parametrize("n_side,widths,dens,seed", EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_exact_data_equals_the_reference(n_side, widths, dens, seed, batch_of):
    """Small-integer weights, rows and labels, B = 8: with 2 B = 16 every quantity of both passes is a multiple of 1/16, and since
    16 sum |a||b| < 2^24 for every inner product (asserted) every partial sum in ANY order is a float32 -- so the device's loss and
    every gradient element must EQUAL fit_reference's. About half of the hidden units are active and no gradient block is empty, so
    a swapped operand, a mis-mapped fragment, a wrong mask or a lost tile tail cannot pass. Again with B = 1 and with a repeated row."""
    from gym_cloth_amd.policies import fit_reference
    layers, rows, labels = _exact_case(widths, dens, seed)
    b = batch_of(n_side)
    b.set_policy_mlp(layers)
    assert b.fit_append(rows, labels) == len(rows)
    for idx in (np.array([7, 2, 11, 0, 5, 9, 4, 1]), np.array([3]), np.array([6, 2, 6, 10, 8, 2, 6, 0])):
        worst, frac, fill = _exact_facts(layers, rows, labels, idx)
        print("%r B %d: max sum|a||b| %.3g, active %s, sparsest block %.3f" % (widths, len(idx), worst, frac, min(fill)))
        assert 16.0 * worst < 2.0 ** 24
        if len(idx) == 8:
            assert frac is None or 0.45 <= frac <= 0.57, frac
            assert min(fill) >= 0.11, fill
        ref_loss, ref = fit_reference(layers, rows, labels, idx)
        loss, grad = b.fit_grad(idx)
        assert loss == ref_loss, (loss, ref_loss)
        want = _flat(ref)
        assert np.array_equal(want, want.astype(np.float32))                 # the reference's values are float32 values
        bad = np.nonzero(grad.astype(np.float64) != want)[0]
        assert bad.size == 0, (widths, len(idx), bad[:8], grad[bad[:8]], want[bad[:8]])
    assert np.array_equal(_blob(b), np.concatenate([np.concatenate([W.reshape(-1), bb]) for W, bb in layers]))      # nothing was updated


# ---- 2. random data within an a-priori bound --------------------------------------------------------------------------------------------
def _grad_bound(layers, rows, labels, idx):
    """Higham's a-priori bounds for float32 inner products in ANY order, with or without FMA (a length-n product is within
    gamma_{n+1} sum |a||b| of exact, plus the propagated input error), through the forward pass (test_gpu_mlp_policy.py's _bound) and on
    through the backward pass:
        dg_L   = dy / 2B + 2 u |g|
        d(dW)  = sum_r [dg (|h| + dh) + |g| dh] + gamma_{B+1} sum_r (|g| + dg)(|h| + dh)        (db: h = 1, dh = 0)
        d(dH)  = dg |W| + gamma_{n_out+1} (|g| + dg) |W|
    The ReLU mask is exact when every hidden pre-activation exceeds its forward bound in magnitude: `margin` is the smallest
    |z| - dz, which the caller asserts to be > 0. Under that very precondition (layer by layer: layer l's dz needs only the layers
    before it) a unit with z < 0 is computed as < 0 too, both activations are exactly 0, so dh = 0 there and dh = dz at the active units
    -- tighter than 1-Lipschitz ReLU alone, and what keeps the precondition satisfiable three hidden layers deep. Returns (reference loss, bound on the loss, reference gradients, their bounds as one
    flat blob, margin). Computed, not measured."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)[idx]
    a = np.asarray(labels, dtype=np.float64).astype(np.float32).astype(np.float64)[idx]
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
    loss = float((d * d).sum() / (4.0 * B))
    dloss = float((2.0 * np.abs(d) * dhs[-1] + dhs[-1] ** 2).sum() / (4.0 * B)) + 1e-14 * loss
    g = d / (2.0 * B)
    dg = dhs[-1] / (2.0 * B) + 2.0 * U * np.abs(g)
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


RANDOM_CASES = [(n_side, widths, B) for n_side, widths in [(10, [300, 5, 4]), (10, [300, 37, 64, 4]), (10, [300, 256, 256, 256, 4]),
                                                           (25, [1875, 64, 64, 4])] for B in (7, 33)]


def _forward_margin(layers, rows):
    """Per row: the smallest |z| - dz over its hidden pre-activations, dz the forward bound (as _grad_bound computes it; a row's bound
    depends on that row alone). Rows with a margin <= 0 have meaningless later layers, which does not matter: they are not used."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)
    dx, margin = np.zeros_like(x), np.full(len(x), np.inf)
    for l, (W, bb) in enumerate(layers[:-1]):
        W64, aW = W.astype(np.float64), np.abs(W.astype(np.float64))
        dz = dx @ aW.T + _gamma(W.shape[1] + 1) * ((np.abs(x) + dx) @ aW.T + np.abs(bb.astype(np.float64)))
        z = x @ W64.T + bb.astype(np.float64)
        margin = np.minimum(margin, (np.abs(z) - dz).min(axis=1))
        x, dx = np.maximum(z, 0.0), np.where(z > 0.0, dz, 0.0)
    return margin


def _random_case(widths, B, seed, n_rows=40):
    """_random_layers(widths, seed), a dataset of n_rows rows uniform in [-1, 1) with uniform labels, and a minibatch of B of them (with
    repeats). THE MASK PRECONDITION BY CONSTRUCTION: the worst-case forward bound grows by about sum |w| / 2 ~ 0.4 sqrt(fan-in) per
    layer -- to 5e-3 at the third hidden layer of [300, 256, 256, 256, 4] (pre-activations of standard deviation 0.3: 1.5 % of its units
    lie inside), 6e-3 at the second of [1875, 64, 64, 4] (1.1 %) --, so among the thousands of hidden units of 7 or 33 rows some
    pre-activation lies inside its bound for EVERY seed. The rows are therefore drawn one candidate after the other from the one seeded
    stream and a candidate is kept when all ITS hidden pre-activations clear their bounds (a row's bound depends on that row alone;
    about 1 candidate in 70 for the widest shape, 1 in 2 for 25x25, almost all for the narrow ones): a choice made from the float64 reference and the computed bound alone, never from what the device gives.
    No unit of a row that is used is excluded, and the test asserts the precondition again on its minibatch."""
    layers = _random_layers(widths, seed)
    r = np.random.RandomState(1000 + seed)
    kept, drawn = [], 0
    while sum(len(k) for k in kept) < n_rows:
        cand = r.uniform(-1, 1, size=(256, widths[0])).astype(np.float32)
        drawn += len(cand)
        kept.append(cand[_forward_margin(layers, cand) > 0.0])
        assert drawn <= 64 * 256, "no rows clear the forward bound"
    rows = np.concatenate(kept)[:n_rows]
    labels = r.uniform(-1, 1, size=(n_rows, 4))
    idx = r.randint(0, n_rows, size=B)
    return layers, rows, labels, idx


@pytest.mark.parametrize("n_side,widths,B", RANDOM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_random_data_within_the_a_priori_bound(n_side, widths, B, batch_of):
    """Gaussian weights, uniform rows and labels: every gradient element and the loss lie within the computed bound of the float64
    reference. The bound needs the ReLU mask to be exact, which holds when every hidden pre-activation exceeds its forward bound in
    magnitude -- asserted for every unit of the minibatch, none excluded (_random_case says how its rows are drawn for it)."""
    from gym_cloth_amd.policies import fit_reference
    layers, rows, labels, idx = _random_case(widths, B, seed=len(widths))
    ref_loss, dloss, ref, bound, margin = _grad_bound(layers, rows, labels, idx)
    assert margin > 0.0, margin
    chk_loss, chk = fit_reference(layers, rows, labels, idx)                  # the bound's own reference is fit_reference's
    assert abs(chk_loss - ref_loss) <= 1e-12 * ref_loss and np.allclose(_flat(chk), _flat(ref), rtol=0, atol=1e-13)
    b = batch_of(n_side)
    b.set_policy_mlp(layers)
    b.fit_append(rows, labels)
    loss, grad = b.fit_grad(idx)
    err = np.abs(grad.astype(np.float64) - _flat(ref))
    print("%r B %d: mask margin %.3e, loss err %.3e (bound %.3e), max grad err %.3e, max err / bound %.3f, max |grad| %.3e" % (
        widths, B, margin, abs(loss - ref_loss), dloss, err.max(), (err[bound > 0] / bound[bound > 0]).max(), np.abs(grad).max()))
    assert np.isfinite(grad).all() and np.abs(_flat(ref)).max() > 1e-4
    assert abs(loss - ref_loss) <= dloss
    assert (err <= bound).all(), (np.nonzero(err > bound)[0][:8], err.max())


# ---- 3. the optimizer bit for bit -------------------------------------------------------------------------------------------------------
ADAM = dict(optimizer="adam", lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
OPTIMIZERS = [("adam", ADAM), ("sgd", dict(optimizer="sgd", lr=3e-2, momentum=0.0)), ("sgd_momentum", dict(optimizer="sgd", lr=3e-2, momentum=0.9))]


def _restated_step(hyper, theta, m, v, g, t):
    from gym_cloth_amd.policies import adam_reference, sgd_reference
    if hyper["optimizer"] == "adam":
        return adam_reference(theta, m, v, g, t, lr=hyper["lr"], beta1=hyper["beta1"], beta2=hyper["beta2"], eps=hyper["eps"])
    theta, m = sgd_reference(theta, m, g, lr=hyper["lr"], momentum=hyper["momentum"])
    return theta, m, v


@pytest.mark.parametrize("name,hyper", OPTIMIZERS, ids=[o[0] for o in OPTIMIZERS])
def test_optimizer_steps_bit_for_bit(name, hyper, batch_of):
    """For three steps: g = fit_grad(idx_s), then fit takes one step on idx_s -- the downloaded blob equals the numpy float32
    restatement of the header's update applied to g (so the gradient inside a step is fit_grad's, and the update is the header's,
    operation by operation). Three steps in one call equal three calls of one step; fit_reset restarts t and the moments."""
    widths = [300, 37, 64, 4]
    layers, rows, labels, _ = _random_case(widths, 7, seed=3)
    table = np.random.RandomState(11).randint(0, len(rows), size=(3, 9)).astype(np.int32)
    b = batch_of(10)
    b.set_policy_mlp(layers)
    b.fit_append(rows, labels)
    theta = _blob(b)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    losses = []
    for s in range(3):
        loss_g, g = b.fit_grad(table[s])
        loss = b.fit(table[s:s + 1], **hyper)
        assert loss.shape == (1,) and loss[0] == loss_g                      # the loss before the update
        theta, m, v = _restated_step(hyper, theta, m, v, g, s + 1)
        got = _blob(b)
        assert np.array_equal(got.view(np.int32), theta.view(np.int32)), (name, s, np.abs(got - theta).max())
        losses.append(loss[0])
    assert np.abs(theta - _flat(layers)).max() > 1e-3                         # it moved
    # the same three steps in one call (a newly set network restarts the optimizer)
    b.set_policy_mlp(layers)
    again = b.fit(table, **hyper)
    assert np.array_equal(again, np.array(losses)) and np.array_equal(_blob(b).view(np.int32), theta.view(np.int32))
    # fit_reset: the next step is a first step from the present weights
    b.fit_reset()
    _, g = b.fit_grad(table[1])
    b.fit(table[1:2], **hyper)
    first, _, _ = _restated_step(hyper, theta, np.zeros_like(theta), np.zeros_like(theta), g, 1)
    cont, _, _ = _restated_step(hyper, theta, m, v, g, 4)
    assert np.array_equal(_blob(b).view(np.int32), first.view(np.int32))
    if name != "sgd":                                                          # (plain SGD has no state to restart)
        assert not np.array_equal(first, cont)


# ---- 4. determinism and the hand-over ---------------------------------------------------------------------------------------------------
def test_two_handles_agree_and_the_blob_hands_over():
    """Two handles, the same data, five Adam steps: identical losses and blobs. The fitted blob uploaded to a fresh handle evaluates to
    the bits the fitted handle's policy_eval gives: what the trainer leaves in place is an ordinary network."""
    from gym_cloth_amd.policies import unpack_mlp
    widths = [300, 37, 64, 4]
    layers, rows, labels, _ = _random_case(widths, 7, seed=5)
    table = np.random.RandomState(2).randint(0, len(rows), size=(5, 16))
    blobs, losses, handles = [], [], []
    for k in range(2):
        b = _new_batch(10)
        b.set_policy_mlp(layers)
        b.fit_append(rows[:25], labels[:25])
        assert b.fit_append(rows[25:], labels[25:]) == len(rows)             # the dataset grew across two calls (and a reallocation)
        losses.append(b.fit(table, **ADAM))
        blobs.append(_blob(b))
        handles.append(b)
    assert np.array_equal(losses[0], losses[1]) and np.array_equal(blobs[0].view(np.int32), blobs[1].view(np.int32))
    assert losses[0][-1] < losses[0][0]
    fresh = _new_batch(10)
    fresh.set_policy_mlp(unpack_mlp(np.array(widths), blobs[0]))
    want = handles[0].policy_eval(rows)
    assert np.array_equal(fresh.policy_eval(rows).view(np.int64), want.view(np.int64))
    assert not np.array_equal(want, _eval_with(fresh, layers, rows))           # ... and not the unfitted network's
    for b in handles + [fresh]:
        b.close()


def _eval_with(b, layers, rows):
    b.set_policy_mlp(layers)
    return b.policy_eval(rows)


def test_the_next_launch_runs_the_fitted_weights():
    """25x25, three cloths: a step_many(policy='mlp', n_actions=1) right after MLPTrainer.step, with no set_policy in between, records
    the actions policy_eval (the fitted blob's) gives on the pre-launch observation -- and not the unfitted network's."""
    from gym_cloth_amd.envs import ClothVecEnv
    from gym_cloth_amd.policies import MLPPolicy, MLPTrainer
    v = ClothVecEnv(_cfg(25), n_envs=3, precision="f32", consume_domrand_draws=False)
    v.seed([1337 + e for e in range(3)])
    pre = v.reset().astype(np.float32).reshape(3, -1)
    layers = _random_layers([1875, 37, 64, 4], seed=21)
    pol = MLPPolicy(v, layers)
    before = v.batch.policy_eval(pre)
    tr = MLPTrainer(v, pol, **ADAM)
    r = np.random.RandomState(4)
    rows = (pre[r.randint(0, 3, size=20)] + r.normal(size=(20, 1875)) * 0.01).astype(np.float32)
    assert tr.append(rows, r.uniform(-1, 1, size=(20, 4))) == 20
    losses = tr.step(4, 8, seed=0)
    assert losses.shape == (4,) and np.isfinite(losses).all()
    out = v.step_many(policy="mlp", n_actions=1, want_obs=True)
    assert out["ran"].all()
    want = v.batch.policy_eval(pre)
    assert np.array_equal(out["actions"][0], want)
    assert (np.abs(want - before).max(axis=1) > 1e-4).all()
    got = tr.layers()
    assert [W.shape for W, _ in got] == [(37, 1875), (64, 37), (4, 64)] and not np.array_equal(got[0][0], layers[0][0])
    v.close()


def test_dagger_fit_appends_the_rows_that_ran_and_refits():
    """demos.dagger_fit after demos.dagger_rollout (25x25, three cloths, two slots, the oracle's labels): the dataset grows by the
    rows that ran -- with their float32 labels, which the gradient on exactly those rows shows --, the steps run on it, and a second
    iteration rolls out under the fitted network and appends to the same dataset."""
    from gym_cloth_amd.demos import dagger_fit, dagger_rollout
    from gym_cloth_amd.envs import ClothVecEnv
    from gym_cloth_amd.policies import MLPPolicy, MLPTrainer, fit_reference
    v = ClothVecEnv(_cfg(25), n_envs=3, precision="f32", consume_domrand_draws=False)
    v.seed([1337 + e for e in range(3)])
    v.reset()
    layers = _random_layers([1875, 5, 4], seed=31)
    tr = MLPTrainer(v, MLPPolicy(v, layers), optimizer="sgd", lr=1e-2, momentum=0.5)
    roll = dagger_rollout(v, expert="oracle_corner", n_actions=2, beta=0.5, seed=0)
    ran = roll["ran"]
    assert ran.sum() >= 3 and np.isfinite(roll["labels"][ran]).all()
    n = int(ran.sum())
    loss0, _ = fit_reference(layers, roll["obs"][ran], roll["labels"][ran], np.arange(n))
    fit = dagger_fit(v, tr, roll, n_steps=0, batch_size=4, seed=0)
    assert fit["rows"] == fit["appended"] == n == tr.size() and fit["losses"].shape == (0,)
    got0, _ = tr.grad(np.arange(n))
    assert abs(got0 - loss0) <= 1e-4 * loss0                                   # the rows and the labels that were appended are the rollout's
    fit = dagger_fit(v, tr, {"ran": np.zeros_like(ran), "obs": roll["obs"], "labels": roll["labels"]}, n_steps=5, batch_size=4, seed=1)
    assert fit["rows"] == n and fit["appended"] == 0 and fit["losses"].shape == (5,) and np.isfinite(fit["losses"]).all()
    assert not np.array_equal(tr.layers()[0][0], layers[0][0])
    roll2 = dagger_rollout(v, expert="oracle_corner", n_actions=2, beta=0.0, seed=1)
    fit2 = dagger_fit(v, tr, roll2, n_steps=2, batch_size=4, seed=2)
    assert fit2["rows"] == n + int(roll2["ran"].sum()) == tr.size()
    with pytest.raises(ValueError):
        dagger_fit(object(), tr, roll2)
    v.close()


# ---- 5. it learns -----------------------------------------------------------------------------------------------------------------------
# The largest relative deviation of the device's loss curve from the float64 curve over the 60 steps, measured on an MI355X for each of
# the three seeds (profiles/policy_fit.txt; seed 0's maximum, at step 33, is two orders above the other two's -- no cause is claimed); the test allows
# ten times it, the margin for another card's reduction order.
LEARN_MEASURED_DEVIATION = {0: 3.983e-04, 1: 1.769e-06, 2: 4.389e-07}


def _adam64(layers, rows, labels, table, lr, beta1, beta2, eps):
    """The header's Adam in float64 on fit_reference's gradients: the yardstick curve."""
    from gym_cloth_amd.policies import fit_reference
    ls = [(W.astype(np.float64), bb.astype(np.float64)) for W, bb in layers]
    f = np.float32
    b1, b2, lr, eps = float(f(beta1)), float(f(beta2)), float(f(lr)), float(f(eps))
    ms = [(np.zeros_like(W), np.zeros_like(bb)) for W, bb in ls]
    vs = [(np.zeros_like(W), np.zeros_like(bb)) for W, bb in ls]
    losses = []
    for t, idx in enumerate(table, start=1):
        loss, grads = _reference64(ls, rows, labels, idx)
        losses.append(loss)
        a_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        new = []
        for l in range(len(ls)):
            upd = []
            for k in range(2):
                g = grads[l][k]
                ms[l][k][...] = b1 * ms[l][k] + (1.0 - b1) * g
                vs[l][k][...] = b2 * vs[l][k] + (1.0 - b2) * g * g
                upd.append(ls[l][k] - a_t * ms[l][k] / (np.sqrt(vs[l][k]) + eps))
            new.append(tuple(upd))
        ls = new
    return np.array(losses)


def _reference64(ls, rows, labels, idx):
    """fit_reference's arithmetic on float64 weights (fit_reference rounds its weights to float32: right for the device's blob, not for
    a float64 trajectory)."""
    x = rows.astype(np.float64)[idx]
    a = labels.astype(np.float32).astype(np.float64)[idx]
    B, L = len(idx), len(ls)
    hs = [x]
    for l in range(L):
        z = hs[-1] @ ls[l][0].T + ls[l][1]
        hs.append(np.maximum(z, 0.0) if l + 1 < L else z)
    d = hs[-1] - a
    g = d / (2.0 * B)
    grads = [None] * L
    for l in range(L - 1, -1, -1):
        grads[l] = (g.T @ hs[l], g.sum(axis=0))
        if l:
            g = (g @ ls[l][0]) * (hs[l] > 0.0)
    return float((d * d).sum() / (4.0 * B)), grads


@pytest.mark.parametrize("s", [0, 1, 2])
def test_it_learns(s, batch_of):
    """A [300, 16, 4] teacher labels 256 uniform rows; a student from another seed takes 60 Adam steps of 32 rows (lr 1e-2,
    beta (0.9, 0.999), eps 1e-8). The float64 numpy restatement on the same index table and the device both end at <= 0.25 x their first
    loss, and the device's loss curve stays within ten times the measured relative deviation of the float64 curve -- the float64
    curve is the yardstick, never the device's own."""
    from gym_cloth_amd.policies import MLPPolicy, MLPTrainer
    widths = [300, 16, 4]
    teacher, student = _random_layers(widths, s), _random_layers(widths, s + 50)
    rows = np.random.RandomState(700 + s).uniform(-1, 1, size=(256, 300)).astype(np.float32)

    class Env(object):                                    # what MLPPolicy / MLPTrainer read of an env, around the shared batch
        P, E = 100, 1
        batch = batch_of(10)
        _policy_mlp = None

        def set_policy(self, mlp):
            self.batch.set_policy_mlp(getattr(mlp, "layers", mlp))
            self._policy_mlp = mlp

    env = Env()
    labels = MLPPolicy(env, teacher).reference(rows)
    tr = MLPTrainer(env, student, **ADAM)
    assert tr.append(rows, labels) == 256
    table = MLPTrainer.index_table(256, 60, 32, seed=s)
    ref = _adam64(student, rows, labels, table, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"])
    got = tr.step(60, 32, seed=s)
    dev = np.abs(got - ref) / ref
    print("it learns, seed %d: float64 %.4f -> %.4f, device %.4f -> %.4f, max relative deviation of the loss curve %.3e (step %d)" % (
        s, ref[0], ref[-1], got[0], got[-1], dev.max(), int(dev.argmax())))
    assert ref[-1] <= 0.25 * ref[0] and got[-1] <= 0.25 * got[0]
    assert dev.max() <= 10.0 * LEARN_MEASURED_DEVIATION[s], dev.max()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    """Every CLOTHHIP_ESTATE / CLOTHHIP_EINVAL case of clothhip_policy_fit* and clothhip_fit_data_append, through the library itself.
    After each one the blob, the dataset's size and the gradient on a fixed minibatch are what they were; at the end one more Adam
    step gives the blob and the loss of a twin handle that took the same steps and saw no refusal (so neither the moments nor the step
    count moved)."""
    from gym_cloth_amd import _lib
    from gym_cloth_amd.envs import ClothVecEnv
    widths = [300, 5, 4]
    layers, rows, labels, _ = _random_case(widths, 7, seed=8)
    table = np.random.RandomState(6).randint(0, len(rows), size=(3, 8)).astype(np.int32)
    twin = _new_batch(10)
    v = ClothVecEnv(_cfg(10), n_envs=1, precision="f32", consume_domrand_draws=False)
    v.seed([1337])
    v.reset()
    b = v.batch
    for x in (twin, b):
        x.set_policy_mlp(layers)
        x.fit_append(rows, labels)
        x.fit(table[:2], **ADAM)
    L, h = b._L, b._h
    blob0, (loss0, grad0) = _blob(b), b.fit_grad(table[2])
    assert np.array_equal(blob0, _blob(twin))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def params(**kw):
        d = dict(optimizer=0.0, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0)
        d.update(kw)
        return _lib.ClothFitParams(d["optimizer"], d["lr"], d["beta1"], d["beta2"], d["eps"], d["momentum"])

    def fit(p=None, idx=table[2:3], n_steps=1, B=8):
        p = params() if p is None else p
        loss = np.zeros(max(n_steps, 1))
        return L.clothhip_policy_fit(h, C.byref(p), _lib.i32p(np.ascontiguousarray(idx, dtype=np.int32)), n_steps, B, _lib.dp(loss))

    def grad(idx, B):
        g, loss = np.zeros(grad0.size, dtype=np.float32), np.zeros(1)
        return L.clothhip_policy_fit_grad(h, _lib.i32p(np.ascontiguousarray(idx, dtype=np.int32)), B, fp(g), _lib.dp(loss))

    def unchanged():
        assert np.array_equal(_blob(b).view(np.int32), blob0.view(np.int32)) and b.fit_size() == len(rows)
        loss, g = b.fit_grad(table[2])
        assert loss == loss0 and np.array_equal(g.view(np.int32), grad0.view(np.int32))

    n = len(rows)
    big = np.zeros(_lib.FIT_MAX_BATCH + 1, dtype=np.int32)
    for rc, want in [
            (lambda: fit(B=0), _lib.EINVAL), (lambda: fit(idx=big[None], B=big.size), _lib.EINVAL),            # B < 1, B above the cap
            (lambda: grad(table[2], 0), _lib.EINVAL), (lambda: grad(big, big.size), _lib.EINVAL),
            (lambda: fit(n_steps=-1), _lib.EINVAL),
            (lambda: fit(idx=np.array([[0, 1, 2, n, 3, 4, 5, 6]])), _lib.EINVAL),                               # an index outside [0, n)
            (lambda: fit(idx=np.array([[0, 1, 2, -1, 3, 4, 5, 6]])), _lib.EINVAL),
            (lambda: fit(idx=np.concatenate([table[:1], [[0, 1, 2, n, 3, 4, 5, 6]]]), n_steps=2), _lib.EINVAL), # ... in a later step
            (lambda: grad(np.array([0, n]), 2), _lib.EINVAL), (lambda: grad(np.array([-1, 0]), 2), _lib.EINVAL),
            (lambda: fit(params(optimizer=2.0)), _lib.EINVAL), (lambda: fit(params(optimizer=0.5)), _lib.EINVAL),
            (lambda: fit(params(lr=-1e-3)), _lib.EINVAL), (lambda: fit(params(lr=float("nan"))), _lib.EINVAL),
            (lambda: fit(params(eps=float("inf"))), _lib.EINVAL), (lambda: fit(params(beta1=-0.1)), _lib.EINVAL),
            (lambda: fit(params(beta2=1.0)), _lib.EINVAL), (lambda: fit(params(optimizer=1.0, momentum=-0.9)), _lib.EINVAL),
            (lambda: L.clothhip_policy_fit(h, None, _lib.i32p(table), 1, 8, None), _lib.EINVAL),
            (lambda: L.clothhip_policy_fit(h, C.byref(params()), None, 1, 8, None), _lib.EINVAL),
            (lambda: L.clothhip_policy_fit_grad(h, None, 8, None, None), _lib.EINVAL)]:
        assert rc() == want
        unchanged()
    # the dataset's own refusals: a non-finite observation or label (also one that is finite as a double only), n < 0 -- nothing is appended
    bad_obs, bad_lab, big_lab = rows[:3].copy(), labels[:3].copy(), labels[:3].copy()
    bad_obs[2, 299], bad_lab[1, 3], big_lab[0, 0] = np.nan, np.inf, 1e300
    for o, a, k in [(bad_obs, labels[:3], 3), (rows[:3], bad_lab, 3), (rows[:3], big_lab, 3), (rows[:3], labels[:3], -1), (None, labels[:3], 3)]:
        o = None if o is None else np.ascontiguousarray(o, dtype=np.float32)
        assert L.clothhip_fit_data_append(h, None if o is None else fp(o), _lib.dp(np.ascontiguousarray(a)), k) == _lib.EINVAL
        unchanged()
    # a launch in flight
    nsteps, done = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, 1, 4)))
    assert fit() == _lib.ESTATE and grad(table[2], 8) == _lib.ESTATE
    assert L.clothhip_policy_fit_reset(h) == _lib.ESTATE and L.clothhip_fit_data_clear(h) == _lib.ESTATE
    assert L.clothhip_fit_data_append(h, fp(rows), _lib.dp(labels), 1) == _lib.ESTATE
    b.run_actions_end()
    unchanged()
    # the next step: the twin's
    assert fit() == _lib.OK
    want_loss = twin.fit(table[2:3], **ADAM)
    assert want_loss[0] == loss0 and np.array_equal(_blob(b).view(np.int32), _blob(twin).view(np.int32))
    # an empty dataset, no shared network, a population: CLOTHHIP_ESTATE (these change the handle on purpose, so they come last)
    b.fit_clear()
    assert b.fit_size() == 0 and fit() == _lib.ESTATE and grad(table[2], 8) == _lib.ESTATE
    assert np.array_equal(_blob(b).view(np.int32), _blob(twin).view(np.int32))
    b.fit_append(rows, labels)
    b.set_policy_population([layers, layers], np.zeros(1, dtype=np.int32))
    assert fit() == _lib.ESTATE and grad(table[2], 8) == _lib.ESTATE
    b.set_policy_mlp(None)
    assert fit() == _lib.ESTATE and grad(table[2], 8) == _lib.ESTATE and b.fit_size() == len(rows)
    with pytest.raises(_lib.ClothHipError):
        b.fit_grad(table[2])
    # a new network restarts the optimizer: one step from `layers` is a FIRST step, the twin's after its own reset
    b.set_policy_mlp(layers)
    twin.set_policy_mlp(layers)
    assert np.array_equal(b.fit(table[:1], **ADAM), twin.fit(table[:1], **ADAM))
    assert np.array_equal(_blob(b).view(np.int32), _blob(twin).view(np.int32))
    twin.close()
    v.close()


def test_fp64_handle_fits_in_float32():
    """The fit is float32 on an fp64 handle too: the same data give the fp32 handle's bits."""
    layers, rows, labels, _ = _random_case([300, 5, 4], 7, seed=9)
    table = np.random.RandomState(1).randint(0, len(rows), size=(2, 8))
    res = []
    for prec in ("f32", "f64"):
        b = _new_batch(10, precision=prec)
        b.set_policy_mlp(layers)
        b.fit_append(rows, labels)
        res.append((b.fit_grad(table[0]), b.fit(table, **ADAM), _blob(b)))
        b.close()
    assert res[0][0][0] == res[1][0][0] and np.array_equal(res[0][0][1], res[1][0][1])
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2].view(np.int32), res[1][2].view(np.int32))
