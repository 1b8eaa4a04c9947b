"""GPU tests of PPO on the device: the clipped surrogate (k_fit_loss_ppo, here as the call with a one-row table of constants) on exactly representable data, by bytes against
the numpy restatement of its arithmetic, and within an a-priori bound of the float64 reference on Gaussian data; the old-mean column and
its snapshot on the device; the step, its determinism and what it leaves alone; a fit that freezes where the weighted regression runs
away; every refusal; demos.ppo_fit. Every comparison is array_equal or by bytes unless it says otherwise. Shapes and helpers are those
of tests/test_gpu_fit_weighted.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_dagger import _layers
from test_gpu_env import base_cfg
from test_gpu_fit_weighted import IDX1, IDX8, IDXR, _i32
from test_gpu_policy_fit import ADAM, _blob, _exact_case, _exact_facts, _flat, _gamma, _new_batch, _random_case
from test_ppo_host import EXP_BOUND

pytestmark = pytest.mark.gpu


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


def _forward(layers, obs):
    h = np.asarray(obs, dtype=np.float32).astype(np.float64)
    for l, (W, b) in enumerate(layers):
        h = h @ W.astype(np.float64).T + b.astype(np.float64)
        if l + 1 < len(layers):
            h = np.maximum(h, 0.0)
    return h


def _unclipped(layers, rows, labels, adv, idx, sigma):
    from gym_cloth_amd.policies import fit_reference
    return _flat(fit_reference(layers, rows, labels, idx, weights=2.0 * np.asarray(adv, dtype=np.float64) / sigma ** 2)[1])


# ---- 1. exact data ------------------------------------------------------------------------------------------------------------------------
EXACT_CASES = [  # (n_side, widths, dens, seed): test_gpu_fit_weighted's cases; the asserts below hold for them (checked on the CPU)
    (10, [300, 5, 4], 1.0, 0),
    (10, [300, 37, 64, 4], 0.3, 0),
    (25, [1875, 37, 64, 4], 0.3, 0),
]
EXACT_CLIPPED = (0, 2, 4)
EXACT_CLIP = 0.25          # 1 - eps and 1 + eps are quarters: a clipped row's surrogate (1 +- eps) A is exact, as everything else here


def _four_squares(n):
    """Integers (e0, e1, e2, e3) with e0^2 + e1^2 + e2^2 + e3^2 = n >= 0 (Lagrange: they exist): the largest e0 whose remainder is
    a sum of three squares, that remainder's first decomposition in ascending order."""
    for e0 in range(int(np.sqrt(n)) + 1, -1, -1):
        rest0 = n - e0 * e0
        if rest0 < 0:
            continue
        m = int(np.sqrt(rest0)) + 1
        for e1 in range(m + 1):
            for e2 in range(e1, m + 1):
                rest = rest0 - e1 * e1 - e2 * e2
                if rest < 0:
                    break
                e3 = int(round(np.sqrt(rest)))
                if e3 * e3 == rest:
                    return (e0, e1, e2, e3)
    raise AssertionError(n)


def _exact_ppo(widths, dens, seed):
    """test_gpu_policy_fit's exact case with integer advantages from {-2 .. 3} (test_gpu_fit_weighted's stream) and sigma = 1. A row's
    old mean is the present mean y (an integer vector: rho = exp_fixed(0) = 1, active) unless the row can be CLIPPED exactly: with
    d = a - y, an old mean a - e with |e|^2 = |d|^2 + 6 gives q = 6, x = +3 (rho above the interval: clipped for A > 0), and
    |e|^2 = |d|^2 - 6 >= 0 gives x = -3 (clipped for A < 0). The rows EXACT_CLIPPED get such an old mean: of IDX8's rows two above and
    one below the interval; IDXR meets two of them beside active rows. Preconditions asserted from the reference alone.
    -> (layers, rows, labels, adv, old, y)."""
    from gym_cloth_amd.policies import ppo_reference
    layers, rows, labels = _exact_case(widths, dens, seed)
    adv = np.random.RandomState(5000 + seed).randint(-2, 4, size=len(rows)).astype(np.float32)
    y = _forward(layers, rows)
    assert np.array_equal(y, np.rint(y)) and np.abs(y).max() < 2 ** 20
    old = y.copy()
    for r in EXACT_CLIPPED:
        d2 = int(((labels[r] - y[r]) ** 2).sum())
        assert adv[r] != 0 and (adv[r] > 0 or d2 >= 6)
        e = np.array(_four_squares(d2 + 6 if adv[r] > 0 else d2 - 6), dtype=np.float64) * np.where(np.arange(4) % 2, -1.0, 1.0)
        old[r] = labels[r] - e
    for idx in (IDX8, IDX1, IDXR):
        stats, grads, rho, active = ppo_reference(layers, rows, labels, old, adv, idx, 1.0, EXACT_CLIP)
        worst, frac, _ = _exact_facts(layers, rows, labels, idx)
        # the gradient is 2 A times the unweighted one at rho = 1: multiples of 1 / B, |g| grows by at most 2 max |A|, so every inner
        # product of both passes stays below 2^24 / 16 in magnitude: every partial sum in ANY order is a float32
        assert 16.0 * float(np.abs(adv).max()) * worst < 2.0 ** 24, (worst, adv)
        assert np.all((rho == 1.0) | ~active)                                  # an active row has rho = 1 exactly: no exp enters a gradient
        if len(idx) == 8:
            assert (~active).sum() >= 2 and (active & (rho == 1.0) & (adv[idx] != 0)).sum() >= 2, (active, rho)
            assert (rho[~active] > 1.0).any() and (rho[~active] < 1.0).any()       # clipped on both sides
            assert all(np.count_nonzero(g) > 0 for Wb in grads for g in Wb)     # no gradient block is empty
            assert not np.array_equal(_flat(grads), _unclipped(layers, rows, labels, adv, idx, 1.0))
            assert stats[1] == (~active).sum() / 8.0 and stats[2] > 0.0
        want = _flat(grads)
        assert np.array_equal(want, want.astype(np.float32))
    return layers, rows, labels, adv, old.astype(np.float32), y


@pytest.mark.parametrize("n_side,widths,dens,seed", EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_exact_data_equals_the_ppo_reference(n_side, widths, dens, seed, batch_of):
    """Integer data, sigma = 1, eps = 1/4: loss, clip_fraction, kl and every gradient element EQUAL ppo_reference. B = 8, B = 1 and a
    repeated row."""
    from gym_cloth_amd.policies import ppo_reference
    layers, rows, labels, adv, old, y = _exact_ppo(widths, dens, seed)
    b = batch_of(n_side)
    b.set_policy_mlp(layers)
    assert b.fit_append(rows, labels, weights=adv) == len(rows)
    pred = b.fit_predict(np.arange(len(rows)))
    assert np.array_equal(pred.astype(np.float64), y)                         # the present y, bytes that are uploaded where a row stays active
    b.fit_set_old_means(np.where((old == y.astype(np.float32)).all(axis=1)[:, None], pred, old))
    assert np.array_equal(b.fit_get_old_means(), old)
    for idx in (IDX8, IDX1, IDXR):
        ref_stats, ref, rho, active = ppo_reference(layers, rows, labels, old, adv, idx, 1.0, EXACT_CLIP)
        stats, grad, ratio = b.fit_ppo_grad(idx, 1.0, EXACT_CLIP)
        print("%r B %d: stats %r (reference %r), active %r" % (widths, len(idx), stats.tolist(), ref_stats, active.tolist()))
        assert stats.tolist() == list(ref_stats)
        bad = np.nonzero(grad.astype(np.float64) != _flat(ref))[0]
        assert bad.size == 0, (widths, len(idx), bad[:8], grad[bad[:8]], _flat(ref)[bad[:8]])
        assert np.array_equal(ratio[active], np.ones(int(active.sum()), dtype=np.float32))
        assert np.array_equal(ratio > 1.0 + EXACT_CLIP, rho > 1.0 + EXACT_CLIP) and np.array_equal(ratio < 1.0 - EXACT_CLIP, rho < 1.0 - EXACT_CLIP)
        if len(idx) == 8:
            assert not np.array_equal(grad.astype(np.float64), _unclipped(layers, rows, labels, adv, idx, 1.0))
    assert np.array_equal(_blob(b), _flat(layers))                            # nothing was updated


# ---- 2. the kernel's arithmetic by bytes ------------------------------------------------------------------------------------------------
SIGMA, CLIP = 0.5, 0.2


def _gauss_case(widths, n_rows, seed):
    """_random_case's network and rows (every hidden pre-activation of a row clears its forward bound); actions around the present
    mean at the policy's sigma, old means around it at 0.3 sigma -- so the ratios spread over both sides of both bounds --, Gaussian
    advantages with every fifth one 0. -> (layers, rows, actions float32, old float32, adv float32)."""
    layers, rows, _, _ = _random_case(widths, 1, seed, n_rows=n_rows)
    r = np.random.RandomState(7000 + seed)
    mu = _forward(layers, rows)
    act = (mu + SIGMA * r.normal(size=mu.shape)).astype(np.float32)
    old = (mu + 0.3 * SIGMA * r.normal(size=mu.shape)).astype(np.float32)
    adv = r.normal(size=n_rows).astype(np.float32)
    adv[::5] = 0.0
    return layers, rows, act, old, adv


def _load(b, layers, rows, act, old, adv):
    b.set_policy_mlp(layers)
    b.fit_append(rows, act.astype(np.float64), weights=adv)
    b.fit_set_old_means(old)


def _colsum32(dz):
    """k_fit_colsum restated: float32 sums over the rows in ascending order."""
    s = np.zeros(dz.shape[1], dtype=np.float32)
    for row in dz:
        s = (s + row).astype(np.float32)
    return s


@pytest.mark.parametrize("B", [1, 33, 256, 257, 300, 4096])
def test_the_kernels_arithmetic_by_bytes(B, batch_of):
    """ratio_out, the three statistics and dz -- seen through db of the last layer, its float32 column sum in row order -- against
    ppo_loss_reference(fit_predict(idx), ...). B = 257: a thread's second row; 300 and 4096: several ranges of the split batch sum."""
    from gym_cloth_amd.policies import ppo_loss_reference
    widths = [300, 37, 64, 4]
    layers, rows, act, old, adv = _gauss_case(widths, 64, seed=4)
    b = batch_of(10)
    _load(b, layers, rows, act, old, adv)
    r = np.random.RandomState(B)
    idx = np.array([3]) if B == 1 else np.concatenate([np.arange(min(B, 64)), r.randint(0, 64, size=max(B - 64, 0))])
    y = b.fit_predict(idx)
    want_stats, want_dz, want_ratio, active = ppo_loss_reference(y, act[idx], old[idx], adv[idx], SIGMA, CLIP, B)
    if B >= 33:                                                                # the cases the comparison must meet, from the restatement's inputs alone
        a = adv[idx]
        assert (a == 0).any() and (a > 0).any() and (a < 0).any()
        for side in (want_ratio > 1.0 + CLIP, want_ratio < 1.0 - CLIP):
            assert (side & active & (a != 0)).any() and (side & ~active).any()
        assert ((want_ratio > 1.0 - CLIP) & (want_ratio < 1.0 + CLIP)).any()
    stats, grad, ratio = b.fit_ppo_grad(idx, SIGMA, CLIP)
    print("B %d: stats %r, %d of %d rows not active" % (B, stats.tolist(), int((~active).sum()), B))
    assert ratio.tobytes() == want_ratio.tobytes()
    assert stats.tobytes() == want_stats.tobytes()
    assert grad[-4:].tobytes() == _colsum32(want_dz).tobytes() and np.abs(grad[-4:]).max() > 0


# ---- 3. Gaussian data within an a-priori bound of the float64 reference -------------------------------------------------------------------
def _ppo_bound(layers, rows, act, old, adv, idx, sigma, clip):
    """test_gpu_fit_weighted._grad_bound_w with PPO's dZ. With dy the forward bound on y and d = mu - a:
        q = sum_k (a - mo)^2 - (a - mu)^2 moves by at most dq = sum_k (2 |d| dy + dy^2); its nine double operations add 16 * 2^-53 of
        the sum of the magnitudes; x = q / 2 sigma^2 moves by dx = dq / 2 sigma^2 + that;
        rho_dev = exp_fixed(x_dev) lies within rel = (e^dx - 1) + EXP_BOUND e^dx of rho, relative (EXP_BOUND: the host test's bound of
        exp_fixed against exp);
        g = A rho d / (sigma^2 B): the device forms it from rho_dev and d_dev = d +- dy in four double operations and one float32
        rounding, so dg = |A| rho / (sigma^2 B) (rel (|d| + dy) + dy) + gamma_2 (|g| + that)      -- |A| rho / sigma^2 in the place of |w|;
        an active row stays active and a clipped one clipped when rho keeps rho rel from both bounds: `safe`, per row, which the caller
        asserts (a row with A = 0 is active whatever rho is). A clipped row has g = 0 exactly on both sides.
    The statistics: loss moves by sum_active |A| rho rel / B, kl by sum (2 |mu - mo| dy + dy^2) / (2 sigma^2 B), each plus 1e-14 of
    its magnitude sum for the double roundings; clip_fraction is exact under `safe`. Everything behind dZ is _grad_bound's.
    Returns (stats, their bounds, gradients, their bounds flat, the ReLU margin, safe bool[B])."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)[idx]
    a, mo, A = (np.asarray(v, dtype=np.float32).astype(np.float64)[idx] for v in (act, old, adv))
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
    mu, dy = hs[-1], dhs[-1]
    inv_s2 = 1.0 / (sigma * sigma)
    d = mu - a
    q = ((a - mo) ** 2 - d ** 2).sum(axis=1)
    dq = (2.0 * np.abs(d) * dy + dy ** 2).sum(axis=1) + 16.0 * 2.0 ** -53 * ((a - mo) ** 2 + (np.abs(d) + dy) ** 2).sum(axis=1)
    xx = q * 0.5 * inv_s2
    assert np.abs(xx).max() < 39.0                                            # nowhere near the clamp
    dx = dq * 0.5 * inv_s2 + 2.0 ** -52 * np.abs(xx)
    rho = np.exp(xx)
    rel = np.expm1(dx) + EXP_BOUND * np.exp(dx)
    lo, hi = 1.0 - clip, 1.0 + clip
    safe = (A == 0.0) | (np.minimum(np.abs(rho - lo), np.abs(rho - hi)) > rho * rel)
    s1, s2 = rho * A, np.clip(rho, lo, hi) * A
    active = s1 <= s2
    aA = np.abs(A)
    stats = np.array([-np.where(active, s1, s2).sum() / B, (~active).sum() / float(B), ((mu - mo) ** 2).sum(axis=1).sum() * 0.5 * inv_s2 / B])
    dstats = np.array([(np.where(active, aA * rho * rel, 0.0).sum() + 1e-14 * np.abs(np.where(active, s1, s2)).sum()) / B, 0.0,
                       ((2.0 * np.abs(mu - mo) * dy + dy ** 2).sum() * 0.5 * inv_s2 + 1e-14 * ((mu - mo) ** 2).sum() * 0.5 * inv_s2) / B])
    c = (aA * rho * inv_s2 / B)[:, None]
    g = np.where(active[:, None], (s1[:, None] * d) * inv_s2 / B, 0.0)
    dg = c * (rel[:, None] * (np.abs(d) + dy) + dy)
    dg = np.where(active[:, None], dg + _gamma(2) * (np.abs(g) + dg), 0.0)
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
    return stats, dstats, grads, _flat(bounds), margin, safe


@pytest.mark.parametrize("n_side,widths,B", [(10, [300, 5, 4], 33), (10, [300, 37, 64, 4], 33), (10, [300, 37, 64, 4], 300), (25, [1875, 37, 64, 4], 33)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_gaussian_data_within_the_a_priori_bound(n_side, widths, B, batch_of):
    """Every gradient element and the statistics within the computed bound of ppo_reference; the ReLU mask and the active mask exact
    for every row of the minibatch (asserted): the minibatch is drawn among the rows whose ratio keeps its own error bound from both
    clip bounds -- a choice from the reference and the bound alone."""
    from gym_cloth_amd.policies import ppo_reference
    layers, rows, act, old, adv = _gauss_case(widths, 64, seed=len(widths))
    safe_all = _ppo_bound(layers, rows, act, old, adv, np.arange(64), SIGMA, CLIP)[5]
    assert safe_all.sum() >= 48, int(safe_all.sum())                          # the margin excludes few rows
    idx = np.random.RandomState(B).choice(np.nonzero(safe_all)[0], size=B)
    ref_stats, dstats, ref, bound, margin, safe = _ppo_bound(layers, rows, act, old, adv, idx, SIGMA, CLIP)
    assert margin > 0.0 and safe.all()
    chk_stats, chk, rho, active = ppo_reference(layers, rows, act, old, adv, idx, SIGMA, CLIP)   # the bound's own reference is ppo_reference's
    assert np.allclose(chk_stats, ref_stats, rtol=1e-12, atol=1e-15) and np.allclose(_flat(chk), _flat(ref), rtol=0, atol=1e-13)
    assert active.any() and (~active).any() and (rho > 1.0 + CLIP).any() and (rho < 1.0 - CLIP).any()
    b = batch_of(n_side)
    _load(b, layers, rows, act, old, adv)
    stats, grad, ratio = b.fit_ppo_grad(idx, SIGMA, CLIP)
    err = np.abs(grad.astype(np.float64) - _flat(ref))
    share = (err[bound > 0] / bound[bound > 0]).max()
    print("%r B %d: mask margin %.3e, stats %r err %r (bounds %r), max grad err %.3e, max err / bound %.3f, max |grad| %.3e" % (
        widths, B, margin, stats.tolist(), np.abs(stats - ref_stats).tolist(), dstats.tolist(), err.max(), share, np.abs(grad).max()))
    assert np.isfinite(grad).all() and np.abs(_flat(ref)).max() > 1e-4
    assert (np.abs(stats - ref_stats) <= dstats).all() and stats[1] == ref_stats[1]
    assert (err <= bound).all(), (np.nonzero(err > bound)[0][:8], err.max())


# ---- 4. the snapshot ----------------------------------------------------------------------------------------------------------------------
def test_snapshot_is_predict_and_the_column_follows_the_dataset():
    from gym_cloth_amd import _lib
    widths = [300, 37, 64, 4]
    layers = _layers(widths, 31)
    r = np.random.RandomState(17)
    n = _lib.FIT_MAX_BATCH + 3
    rows, labels = r.uniform(-1, 1, size=(n, 300)).astype(np.float32), r.uniform(-1, 1, size=(n, 4))
    b = _new_batch(10)
    b.set_policy_mlp(layers)
    b.fit_append(rows[:64], labels[:64])                                      # 64 rows: the first capacity
    assert not b.fit_get_old_means().any()
    pred = b.fit_predict(np.arange(64))
    # a sub-range: the rows outside it stay unset (zeros) and refused
    b.fit_snapshot_policy(10, 1)
    b.fit_snapshot_policy(20, 33)
    got = b.fit_get_old_means()
    inside = np.zeros(64, dtype=bool)
    inside[10] = inside[20:53] = True
    assert got[inside].tobytes() == pred[inside].tobytes() and not got[~inside].any() and np.abs(got[inside]).min() > 0
    assert b.fit_ppo_grad(np.array([10, 20, 52]), 1.0)[0].shape == (3,)
    for row in (9, 11, 19, 53, 0, 63):
        with pytest.raises(_lib.ClothHipError, match="row %d has no old mean.*clothhip_fit_data_snapshot_policy.*clothhip_fit_data_set_old_means" % row):
            b.fit_ppo_grad(np.array([10, row]), 1.0)
    # growth keeps the column; the new rows are unset
    b.fit_append(rows[64:], labels[64:])
    assert b.fit_size() == n
    got = b.fit_get_old_means()
    assert got[:64][inside].tobytes() == pred[inside].tobytes() and not got[:64][~inside].any() and not got[64:].any()
    with pytest.raises(_lib.ClothHipError, match="row 64 has no old mean"):
        b.fit_ppo_grad(np.array([10, 64]), 1.0)
    # the whole dataset: two chunks
    b.fit_snapshot_policy()
    assert b.last_kernel_ms > 0.0
    full = b.fit_predict(np.arange(n))
    assert b.fit_get_old_means().tobytes() == full.tobytes() and full[:64].tobytes() == pred.tobytes()
    assert b.fit_get_old_means(n - 2, 2).tobytes() == full[n - 2:].tobytes()
    # five policy steps: the stored means are the EARLIER predict, not the new one
    b.fit(r.randint(0, n, size=(5, 33)), **ADAM)
    moved = b.fit_predict(np.arange(n))
    assert b.fit_get_old_means().tobytes() == full.tobytes() and not np.array_equal(moved, full)
    stats = b.fit_ppo_grad(np.arange(33), 0.5)[0]
    assert stats[2] > 0.0                                                     # the policy has moved away from its snapshot
    # the host route writes the same column
    b.fit_set_old_means(moved[5:9], first=5)
    assert b.fit_get_old_means(4, 6).tobytes() == np.concatenate([full[4:5], moved[5:9], full[9:10]]).tobytes()
    # clear empties it: rows appended afterwards are unset again
    b.fit_clear()
    b.fit_append(rows[:8], labels[:8])
    assert not b.fit_get_old_means().any()
    with pytest.raises(_lib.ClothHipError, match="row 0 has no old mean"):
        b.fit_ppo_grad(np.array([0]), 1.0)
    b.close()


# ---- 5. the step --------------------------------------------------------------------------------------------------------------------------
def test_two_handles_give_the_same_bits_and_the_first_step_is_the_gradients():
    widths = [300, 37, 64, 4]
    layers, rows, act, old, adv = _gauss_case(widths, 64, seed=4)
    table = np.random.RandomState(2).randint(0, 64, size=(5, 33))
    one, two = _new_batch(10), _new_batch(10)
    out = []
    for b in (one, two):
        _load(b, layers, rows, act, old, adv)
        first = b.fit_ppo_grad(table[0], SIGMA, CLIP)
        stats = b.fit_ppo(table, SIGMA, CLIP, **ADAM)
        assert stats.shape == (5, 3) and stats[0].tobytes() == first[0].tobytes()
        out.append((stats, _blob(b)))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert not np.array_equal(out[0][1], _flat(layers)) and (out[0][0][:, 1] > 0).any() and (out[0][0][1:, 2] > 0).all()
    # the optimizer is the policy's: fit_reset restarts it for PPO too -- a handle that takes 2 + 3 steps equals the one that took 5,
    # and a reset in between changes the bits
    three = _new_batch(10)
    _load(three, layers, rows, act, old, adv)
    three.fit_ppo(table[:2], SIGMA, CLIP, **ADAM)
    three.fit_ppo(table[2:], SIGMA, CLIP, **ADAM)
    assert _blob(three).tobytes() == out[0][1].tobytes()
    _load_again = _new_batch(10)
    _load(_load_again, layers, rows, act, old, adv)
    _load_again.fit_ppo(table[:2], SIGMA, CLIP, **ADAM)
    _load_again.fit_reset()
    _load_again.fit_ppo(table[2:], SIGMA, CLIP, **ADAM)
    assert _blob(_load_again).tobytes() != out[0][1].tobytes()
    for b in (one, two, three, _load_again):
        b.close()


@pytest.mark.parametrize("B", [9, 300], ids=["B9", "B300-two-ranges"])
def test_the_existing_entries_keep_their_bits(B):
    """Two handles, one network, one critic, the same rows. One interleaves snapshots, old means from the host and PPO gradients with
    the existing calls; the other never calls a new entry. fit_grad, fit_loss, fit, value_fit and fit_gae return the same bytes on
    both. Then the first takes PPO steps, which move the POLICY alone: the critic's entries still agree."""
    widths = [300, 37, 64, 4]
    layers, rows, act, old, adv = _gauss_case(widths, 40, seed=5)
    critic = _layers([300, 6, 1], 22)
    r = np.random.RandomState(B)
    idx, table = r.randint(0, 40, size=B), r.randint(0, 40, size=(3, B))
    rew = r.normal(size=40).astype(np.float32)
    nxt = np.where(np.arange(40) % 4 == 3, -1, np.arange(40) + 1).astype(np.int32)
    new, twin = _new_batch(10), _new_batch(10)
    for b in (new, twin):
        b.set_policy_mlp(layers)
        b.set_value_mlp(critic)
        b.fit_append(rows, act.astype(np.float64), weights=adv)
        b.fit_set_transitions(rew, nxt)
    new.fit_snapshot_policy()
    g0 = (new.fit_grad(idx), twin.fit_grad(idx))
    assert g0[0][0] == g0[1][0] and g0[0][1].tobytes() == g0[1][1].tobytes()
    new.fit_ppo_grad(idx, SIGMA, CLIP)
    assert new.fit_loss(idx) == twin.fit_loss(idx)
    new.fit_set_old_means(old)
    new.fit_ppo_grad(idx, SIGMA, CLIP)
    assert new.fit(table, **ADAM).tobytes() == twin.fit(table, **ADAM).tobytes() and _blob(new).tobytes() == _blob(twin).tobytes()
    new.fit_snapshot_policy(3, 20)
    assert new.value_fit(table, **ADAM).tobytes() == twin.value_fit(table, **ADAM).tobytes()
    new.fit_ppo_grad(idx, SIGMA, CLIP)
    ga, gb = new.fit_gae(0.9, 0.8, normalize=True), twin.fit_gae(0.9, 0.8, normalize=True)
    assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes() and new.fit_get_weights().tobytes() == twin.fit_get_weights().tobytes()
    g1 = (new.fit_grad(idx), twin.fit_grad(idx))
    assert g1[0][0] == g1[1][0] and g1[0][1].tobytes() == g1[1][1].tobytes() and g1[0][1].tobytes() != g0[0][1].tobytes()
    assert new.fit_predict(idx).tobytes() == twin.fit_predict(idx).tobytes()
    new.fit_ppo(table, SIGMA, CLIP, **ADAM)                                    # the policy moves; the critic and its optimizer do not
    assert _blob(new).tobytes() != _blob(twin).tobytes()
    assert new.value_fit(table, **ADAM).tobytes() == twin.value_fit(table, **ADAM).tobytes()
    assert new.get_value_mlp().tobytes() == twin.get_value_mlp().tobytes()
    ga, gb = new.fit_gae(0.9, 0.8), twin.fit_gae(0.9, 0.8)
    assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes()
    new.close(); twin.close()


# ---- 6. the reason for the feature --------------------------------------------------------------------------------------------------------
FREEZE_SEED, FREEZE_LR = 0, 0.003          # chosen on the CPU: ppo_reference with sgd_reference reaches clip_fraction == 1 within 100 steps


def _freeze_case():
    widths = [300, 16, 4]
    layers = _layers(widths, 60 + FREEZE_SEED)
    r = np.random.RandomState(600 + FREEZE_SEED)
    rows = r.uniform(-1, 1, size=(12, 300)).astype(np.float32)
    act = (_forward(layers, rows) + r.normal(size=(12, 4))).astype(np.float32)
    return widths, layers, rows, act, np.full(12, -1.0, dtype=np.float32)


def _reference_steps_to_freeze(limit=100):
    """Plain SGD on ppo_reference's gradient from the old means = the first means: the step at which clip_fraction == 1, or None."""
    from gym_cloth_amd.policies import ppo_reference, sgd_reference, unpack_mlp
    widths, layers, rows, act, adv = _freeze_case()
    old = _forward(layers, rows).astype(np.float32)
    theta, u = _flat(layers).astype(np.float32), np.zeros(_flat(layers).size, dtype=np.float32)
    for s in range(limit):
        stats, grads, _, _ = ppo_reference(unpack_mlp(np.array(widths, dtype=np.int32), theta), rows, act, old, adv, np.arange(12), 1.0, 0.2)
        if stats[1] == 1.0:
            return s
        theta, u = sgd_reference(theta, u, _flat(grads).astype(np.float32), lr=FREEZE_LR, momentum=0.0)
    return None


def test_negative_advantages_freeze_where_the_weighted_regression_runs_away():
    """12 rows, every advantage -1, sigma = 1, eps = 0.2, plain SGD on the same full batch. The surrogate pushes every row's mean away
    from its action until its ratio has fallen below 1 - eps; then the row is clipped. Once every row is (clip_fraction == 1) the
    gradient is ALL zeros and the network stays where it is, byte for byte. clothhip_policy_fit under w = 2 A / sigma^2 = -2 on the
    same data has no such stop: after the same number of steps its mean |y - a|^2 is larger and still growing."""
    widths, layers, rows, act, adv = _freeze_case()
    at = _reference_steps_to_freeze()
    assert at is not None and 2 <= at < 100, at
    sgd = dict(optimizer="sgd", lr=FREEZE_LR, momentum=0.0)
    idx = np.arange(12)
    sq = lambda b: float(((b.fit_predict(idx).astype(np.float64) - act.astype(np.float64)) ** 2).sum(axis=1).mean())
    b = _new_batch(10)
    b.set_policy_mlp(layers)
    b.fit_append(rows, act.astype(np.float64), weights=adv)
    b.fit_snapshot_policy()
    start, steps, fractions = sq(b), 0, []
    while steps < 100:
        stats = b.fit_ppo_grad(idx, 1.0, 0.2)[0]
        fractions.append(stats[1])
        if stats[1] == 1.0:
            break
        b.fit_ppo(idx[None], 1.0, 0.2, **sgd)
        steps += 1
    print("the reference freezes at step %d, the device at step %d; clip fractions %r" % (at, steps, fractions))
    assert fractions[-1] == 1.0 and fractions[0] == 0.0 and 2 <= steps < 100
    stats, grad, ratio = b.fit_ppo_grad(idx, 1.0, 0.2)
    assert not grad.any() and (ratio <= np.float32(0.8)).all() and abs(stats[0] - 0.8) <= 1e-15 and stats[1] == 1.0      # -sum(0.8 * -1) / 12
    frozen, frozen_sq = _blob(b).tobytes(), sq(b)
    later = b.fit_ppo(np.tile(idx, (10, 1)), 1.0, 0.2, **sgd)
    assert _blob(b).tobytes() == frozen and (later[:, 1] == 1.0).all() and frozen != _flat(layers).tobytes()
    mse = _new_batch(10)
    mse.set_policy_mlp(layers)
    mse.fit_append(rows, act.astype(np.float64), weights=np.full(12, -2.0, dtype=np.float32))
    mse.fit(np.tile(idx, (steps + 9, 1)), **sgd)
    before = sq(mse)
    mse.fit(idx[None], **sgd)
    after = sq(mse)
    print("mean |y - a|^2: start %.4f, PPO frozen at %.4f, weighted regression %.4f -> %.4f after %d steps" % (start, frozen_sq, before, after, steps + 10))
    assert np.isfinite(after) and frozen_sq > start and after > frozen_sq and after > before
    b.close(); mse.close()


# ---- 7. every refusal ---------------------------------------------------------------------------------------------------------------------
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
    pol = _layers([300, 5, 4], 1)
    b.set_policy_mlp(pol)
    r = np.random.RandomState(0)
    n = 10
    rows, labels = r.uniform(-1, 1, size=(n, 300)).astype(np.float32), r.uniform(-1, 1, size=(n, 4))
    w, old = r.normal(size=n).astype(np.float32), r.uniform(-1, 1, size=(n, 4)).astype(np.float32)
    b.fit_append(rows, labels, weights=w)
    b.fit_set_old_means(old[:8])                                               # rows 8 and 9 have no old mean
    old[8:] = 0.0
    idx = np.arange(8, dtype=np.int32)
    adam = _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    b.fit_ppo(idx[None], 0.5, **ADAM)                                          # one step, so that the moments and the step count exist
    snap = (b.fit_grad(idx), b.fit_ppo_grad(idx, 0.5), _blob(b))
    after_one = (b.fit_ppo(idx[None], 0.5, **ADAM), _blob(b))                  # what the NEXT step gives from this state ...
    b.set_policy_mlp(pol)                                                      # ... which is rebuilt: the same network, one step
    b.fit_ppo(idx[None], 0.5, **ADAM)
    assert _blob(b).tobytes() == snap[2].tobytes()
    fp, ip, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), _lib.i32p, _lib.dp
    Q = _lib.ClothPpoParams
    g, st, ra, mu = np.zeros(b._mlp_n_params, dtype=np.float32), np.zeros(3), np.zeros(8, dtype=np.float32), np.zeros((n + 1, 4), dtype=np.float32)

    def unchanged():
        assert b.fit_size() == n and b.fit_get_weights().tobytes() == w.tobytes() and b.fit_get_old_means().tobytes() == old.tobytes()
        o, l = b.fit_data()
        assert np.array_equal(o, rows) and np.array_equal(l, labels.astype(np.float32))
        now = (b.fit_grad(idx), b.fit_ppo_grad(idx, 0.5), _blob(b))
        assert now[0][0] == snap[0][0] and now[0][1].tobytes() == snap[0][1].tobytes() and now[2].tobytes() == snap[2].tobytes()
        assert all(a.tobytes() == c.tobytes() for a, c in zip(now[1], snap[1]))
        with pytest.raises(_lib.ClothHipError, match="row 8 has no old mean"):
            b.fit_ppo_grad(np.array([0, 8]), 0.5)

    ok = Q(0.5, 0.2)
    # no old mean: rows 8, 9
    assert L.clothhip_policy_fit_ppo_grad(h, C.byref(ok), ip(np.array([0, 9], dtype=np.int32)), 2, fp(g), dp(st), fp(ra)) == _lib.ESTATE
    msg = L.clothhip_last_error().decode()
    assert "row 9" in msg and "clothhip_fit_data_snapshot_policy" in msg and "clothhip_fit_data_set_old_means" in msg
    assert L.clothhip_policy_fit_ppo(h, C.byref(adam), C.byref(ok), ip(np.array([[0, 1], [8, 2]], dtype=np.int32)), 2, 2, None) == _lib.ESTATE
    # sigma and eps
    for q in (Q(0.0, 0.2), Q(-1.0, 0.2), Q(np.nan, 0.2), Q(np.inf, 0.2), Q(1e-200, 0.2), Q(0.5, -0.01), Q(0.5, 1.0), Q(0.5, np.nan), Q(0.5, np.inf)):
        assert L.clothhip_policy_fit_ppo_grad(h, C.byref(q), ip(idx), 8, fp(g), dp(st), fp(ra)) == _lib.EINVAL
        assert L.clothhip_policy_fit_ppo(h, C.byref(adam), C.byref(q), ip(idx), 1, 8, dp(st)) == _lib.EINVAL
    # what clothhip_policy_fit refuses, and NULL pointers
    assert L.clothhip_policy_fit_ppo_grad(h, None, ip(idx), 8, fp(g), dp(st), fp(ra)) == _lib.EINVAL
    assert L.clothhip_policy_fit_ppo_grad(h, C.byref(ok), None, 8, fp(g), dp(st), fp(ra)) == _lib.EINVAL
    assert L.clothhip_policy_fit_ppo_grad(h, C.byref(ok), ip(idx), 0, fp(g), dp(st), fp(ra)) == _lib.EINVAL
    assert L.clothhip_policy_fit_ppo_grad(h, C.byref(ok), ip(idx), _lib.FIT_MAX_BATCH + 1, fp(g), dp(st), fp(ra)) == _lib.EINVAL
    assert L.clothhip_policy_fit_ppo_grad(h, C.byref(ok), ip(np.array([0, n], dtype=np.int32)), 2, fp(g), dp(st), fp(ra)) == _lib.EINVAL
    assert L.clothhip_policy_fit_ppo_grad(h, C.byref(ok), ip(np.array([0, -1], dtype=np.int32)), 2, fp(g), dp(st), fp(ra)) == _lib.EINVAL
    assert L.clothhip_policy_fit_ppo(h, None, C.byref(ok), ip(idx), 1, 8, None) == _lib.EINVAL and L.clothhip_policy_fit_ppo(h, C.byref(adam), None, ip(idx), 1, 8, None) == _lib.EINVAL
    assert L.clothhip_policy_fit_ppo(h, C.byref(adam), C.byref(ok), None, 1, 8, None) == _lib.EINVAL and L.clothhip_policy_fit_ppo(h, C.byref(adam), C.byref(ok), ip(idx), -1, 8, None) == _lib.EINVAL
    for field, bad in (("optimizer", 2.0), ("lr", -1.0), ("lr", np.nan), ("beta1", 1.0), ("beta2", 1.5), ("eps", np.inf), ("momentum", -0.1)):
        p = _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
        setattr(p, field, bad)
        assert L.clothhip_policy_fit_ppo(h, C.byref(p), C.byref(ok), ip(idx), 1, 8, None) == _lib.EINVAL, field
    assert L.clothhip_policy_fit_ppo(h, C.byref(adam), C.byref(ok), ip(idx), 0, 8, None) == _lib.OK                # no steps: nothing changes
    assert L.clothhip_policy_fit_ppo_grad(h, C.byref(ok), ip(idx), 8, None, None, None) == _lib.OK                 # every output is optional
    # the column's entries: a range outside the dataset, a value that is not finite, a NULL table
    for first, k in ((n - 1, 2), (n, 1), (-1, 1), (0, n + 1), (2, -1)):
        assert L.clothhip_fit_data_set_old_means(h, first, k, fp(mu)) == _lib.EINVAL and L.clothhip_fit_data_get_old_means(h, first, k, fp(mu.copy())) == _lib.EINVAL
        assert L.clothhip_fit_data_snapshot_policy(h, first, k) == _lib.EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        vb = np.zeros((2, 4), dtype=np.float32)
        vb[1, 2] = bad
        assert L.clothhip_fit_data_set_old_means(h, 0, 2, fp(vb)) == _lib.EINVAL
    assert L.clothhip_fit_data_set_old_means(h, 0, 2, None) == _lib.EINVAL and L.clothhip_fit_data_get_old_means(h, 0, 2, None) == _lib.EINVAL
    assert L.clothhip_fit_data_set_old_means(h, n, 0, None) == _lib.OK and L.clothhip_fit_data_snapshot_policy(h, 4, 0) == _lib.OK
    unchanged()
    # a launch in flight
    nsteps, done = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, 2, 4)))
    assert L.clothhip_policy_fit_ppo_grad(h, C.byref(ok), ip(idx), 8, fp(g), dp(st), fp(ra)) == _lib.ESTATE
    assert L.clothhip_policy_fit_ppo(h, C.byref(adam), C.byref(ok), ip(idx), 1, 8, None) == _lib.ESTATE
    assert L.clothhip_fit_data_snapshot_policy(h, 0, n) == _lib.ESTATE
    assert L.clothhip_fit_data_set_old_means(h, 0, 2, fp(mu)) == _lib.ESTATE and L.clothhip_fit_data_get_old_means(h, 0, 2, fp(mu.copy())) == _lib.ESTATE
    b.run_actions_end()
    unchanged()
    # the moments and the step count are untouched too: the next step is the one that followed the snapshot
    nxt = b.fit_ppo(idx[None], 0.5, **ADAM)
    assert nxt.tobytes() == after_one[0].tobytes() and _blob(b).tobytes() == after_one[1].tobytes()
    # a population: the shared network only
    twin = _new_batch(10)
    twin.set_policy_population([pol, _layers([300, 5, 4], 2)], np.zeros(1, dtype=np.int32))
    twin.fit_append(rows, labels, weights=w)
    th = twin._h
    assert L.clothhip_fit_data_set_old_means(th, 0, n, fp(np.ascontiguousarray(r.uniform(-1, 1, size=(n, 4)).astype(np.float32)))) == _lib.OK   # the column is the dataset's
    assert L.clothhip_fit_data_snapshot_policy(th, 0, n) == _lib.ESTATE and "population" in L.clothhip_last_error().decode()
    assert L.clothhip_policy_fit_ppo_grad(th, C.byref(ok), ip(idx), 8, fp(g), dp(st), fp(ra)) == _lib.ESTATE and "population" in L.clothhip_last_error().decode()
    assert L.clothhip_policy_fit_ppo(th, C.byref(adam), C.byref(ok), ip(idx), 1, 8, None) == _lib.ESTATE
    twin.close()
    # no network, an empty dataset (these change the handle, so they come last)
    b.fit_clear()
    assert L.clothhip_policy_fit_ppo_grad(h, C.byref(ok), ip(idx), 8, fp(g), dp(st), fp(ra)) == _lib.ESTATE and "empty" in L.clothhip_last_error().decode()
    assert L.clothhip_policy_fit_ppo(h, C.byref(adam), C.byref(ok), ip(idx), 1, 8, None) == _lib.ESTATE and L.clothhip_fit_data_snapshot_policy(h, 0, 0) == _lib.ESTATE
    v.close()
    bare = _new_batch(10)
    assert L.clothhip_policy_fit_ppo_grad(bare._h, C.byref(ok), ip(idx), 8, fp(g), dp(st), fp(ra)) == _lib.ESTATE
    assert L.clothhip_fit_data_snapshot_policy(bare._h, 0, 0) == _lib.ESTATE
    bare.close()


# ---- 8. demos.ppo_fit -----------------------------------------------------------------------------------------------------------------------
def _ppo_run(target_kl):
    from gym_cloth_amd.demos import actor_critic_collect, ppo_fit
    from gym_cloth_amd.envs import ClothVecEnv
    from gym_cloth_amd.policies import MLPTrainer, ValueTrainer
    cfg = base_cfg("tier1", 1337)
    cfg["cloth"]["num_width_points"] = cfg["cloth"]["num_height_points"] = 10
    cfg["env"]["force_grab"] = True
    cfg["env"]["max_actions"] = 2
    v = ClothVecEnv(cfg, n_envs=4, precision="f32", consume_domrand_draws=False)
    v.seed([1337 + e for e in range(4)])
    v.reset()
    tr = MLPTrainer(v, _layers([3 * v.P, 5, 4], 21), lr=1e-2)
    critic = ValueTrainer(v, _layers([3 * v.P, 6, 1], 22), lr=1e-2)
    noise = np.random.RandomState(14).normal(size=(4, 4, 4)) * 0.05
    col = actor_critic_collect(v, tr, n_actions=4, policy_noise=noise, slots_per_launch=4)
    n = col["appended"] + col["open_rows"]
    before = tr.predict(np.arange(n))
    fit = ppo_fit(v, tr, critic, col, sigma=0.05, gamma=0.9, lam=0.8, clip=0.2, n_value_steps=3, n_epochs=3, batch_size=8, seed=0, target_kl=target_kl)
    res = (fit, col, before, v.batch.fit_get_old_means(), tr.weights(), _blob(v.batch), v.batch.get_value_mlp())
    with pytest.raises(ValueError):
        ppo_fit(object(), tr, critic, col, sigma=0.05)
    v.close()
    return res


def test_ppo_fit_is_deterministic_and_stops_on_target_kl():
    from gym_cloth_amd.policies import MLPTrainer
    one, again = _ppo_run(None), _ppo_run(None)
    fit, col, before, old, w, blob, vblob = one
    assert blob.tobytes() == again[5].tobytes() and vblob.tobytes() == again[6].tobytes() and fit["ppo_stats"].tobytes() == again[0]["ppo_stats"].tobytes()
    n_mb = len(col["nonleaf"]) // 8
    assert col["appended"] == 16 and n_mb == 2 and fit["epochs"] == 3 and fit["ppo_stats"].shape == (3 * n_mb, 3) and np.isfinite(fit["ppo_stats"]).all()
    assert old.tobytes() == before.tobytes()                                  # ONE snapshot, before any policy step
    assert fit["ppo_stats"][0, 1] == 0.0 and fit["ppo_stats"][0, 2] == 0.0 and (fit["ppo_stats"][1:, 2] > 0.0).all()
    assert w.tobytes() == np.where(col["leaf"], np.float32(0), w).tobytes() and np.count_nonzero(w) == col["appended"]   # the advantages, w_scale 1
    assert fit["value_losses"].shape == (3,) and blob.tobytes() != _flat(_layers([300, 5, 4], 21)).tobytes()
    tables = MLPTrainer.ppo_epoch_tables(col["nonleaf"], 3, 8, 0)
    assert not col["leaf"][np.concatenate(tables)].any()
    stopped = _ppo_run(0.0)
    assert stopped[0]["epochs"] == 1 and stopped[0]["ppo_stats"].shape == (n_mb, 3)
    assert stopped[0]["ppo_stats"].tobytes() == fit["ppo_stats"][:n_mb].tobytes()
