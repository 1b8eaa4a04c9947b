"""GPU tests of PPO with a learned sigma: k_fit_loss_ppo_sigma at a zero head against the fixed-sigma kernel (k_fit_loss_ppo under a one-row table) by bytes on
exactly representable data, by bytes against the numpy restatement of its arithmetic, and within an a-priori bound of the float64
reference on Gaussian data; the old-log-sigma column and its snapshot on the device; the head's optimizer beside the blob's; a fit that
the growing head freezes; what the new entries leave alone, every refusal, demos.ppo_fit(sigma=None). Every comparison is array_equal or
by bytes unless it says otherwise. Shapes and helpers are those of tests/test_gpu_ppo.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_dagger import _layers
from test_gpu_env import base_cfg
from test_gpu_fit_weighted import IDX1, IDX8, IDXR
from test_gpu_policy_fit import ADAM, _blob, _flat, _gamma, _new_batch, _random_case
from test_gpu_ppo import EXACT_CASES, EXACT_CLIP, _colsum32, _exact_ppo, _forward
from test_ppo_host import EXP_BOUND

pytestmark = pytest.mark.gpu

ENT = 1.0 / 64.0
CLIP = 0.2
ZERO4 = np.zeros(4, dtype=np.float32)


@pytest.fixture(scope="module")
def batch_of():
    """n_side -> ONE ClothBatch of one cloth for the cases that only need a handle to train on (each sets its own network, head and data)."""
    made = {}

    def get(n_side):
        if n_side not in made:
            made[n_side] = _new_batch(n_side)
        made[n_side].fit_clear()
        made[n_side].set_policy_log_sigma(None)
        return made[n_side]
    yield get
    for b in made.values():
        b.close()


# ---- 1. exact data: a zero head is the fixed-sigma kernel at sigma = 1 ----------------------------------------------------------------------
@pytest.mark.parametrize("n_side,widths,dens,seed", EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_exact_data_a_zero_head_is_the_fixed_sigma_entry(n_side, widths, dens, seed, batch_of):
    """Integer data, head and old head 0, eps = 1/4: statistics, ratios and the blob's gradient are the BYTES of fit_ppo_grad(sigma = 1),
    the fourth statistic is the entropy's constant, and the head's gradient EQUALS ppo_sigma_reference's: an active row has rho = 1, so
    its term A ((a - mu)^2 - 1) is an integer and the sum over B = 8 or 1 rows divided by B is exact. B = 8, B = 1 and a repeated row."""
    from gym_cloth_amd.policies import ppo_sigma_reference
    from gym_cloth_amd.references import ENTROPY_C
    layers, rows, labels, adv, old, y = _exact_ppo(widths, dens, seed)
    b = batch_of(n_side)
    b.set_policy_mlp(layers)
    b.set_policy_log_sigma(ZERO4)
    assert b.fit_append(rows, labels, weights=adv) == len(rows)
    pred = b.fit_predict(np.arange(len(rows)))
    b.fit_set_old_means(np.where((old == y.astype(np.float32)).all(axis=1)[:, None], pred, old))
    old_ls = np.zeros((len(rows), 4), dtype=np.float32)
    b.fit_set_old_log_sigma(old_ls)
    for idx in (IDX8, IDX1, IDXR):
        fixed_stats, fixed_grad, fixed_ratio = b.fit_ppo_grad(idx, 1.0, EXACT_CLIP)
        stats, grad, grad_ls, ratio = b.fit_ppo_sigma_grad(idx, EXACT_CLIP, 0.0)
        ref_stats, ref, ref_gls, rho, active = ppo_sigma_reference(layers, rows, labels, old, old_ls, adv, idx, ZERO4, EXACT_CLIP, 0.0)
        print("%r B %d: stats %r, grad_ls %r (reference %r), active %r" % (widths, len(idx), stats.tolist(), grad_ls.tolist(), ref_gls.tolist(), active.tolist()))
        assert stats[:3].tobytes() == fixed_stats.tobytes() and stats[3] == ENTROPY_C
        assert ratio.tobytes() == fixed_ratio.tobytes() and grad.tobytes() == fixed_grad.tobytes()
        assert np.array_equal(ref_gls, ref_gls.astype(np.float32)) and np.all((rho == 1.0) | ~active)      # exact, from the reference alone
        assert np.array_equal(grad_ls.astype(np.float64), ref_gls)
        if len(idx) == 8:
            assert np.count_nonzero(ref_gls) >= 2 and (~active).any()
    assert np.array_equal(_blob(b), _flat(layers)) and np.array_equal(b.get_policy_log_sigma(), ZERO4)       # nothing was updated


# ---- 2. the kernel's arithmetic by bytes ------------------------------------------------------------------------------------------------
def _sigma_case(widths, n_rows, seed):
    """test_gpu_ppo._gauss_case with a head: _random_case's network and rows; a head drawn in [-2, 0.5]; actions around the present
    mean at the head's sigma; old means around it at 0.3 sigma and old heads around the head at 0.1, different in every row -- so the
    ratios spread over both sides of both bounds --, Gaussian advantages with every fifth one 0.
    -> (layers, rows, actions, old, old_ls, adv, ls), float32."""
    layers, rows, _, _ = _random_case(widths, 1, seed, n_rows=n_rows)
    r = np.random.RandomState(9000 + seed)
    ls = r.uniform(-2.0, 0.5, size=4).astype(np.float32)
    sig = np.exp(ls.astype(np.float64))
    mu = _forward(layers, rows)
    act = (mu + sig * r.normal(size=mu.shape)).astype(np.float32)
    old = (mu + 0.3 * sig * r.normal(size=mu.shape)).astype(np.float32)
    old_ls = (ls + 0.1 * r.normal(size=mu.shape)).astype(np.float32)
    adv = r.normal(size=n_rows).astype(np.float32)
    adv[::5] = 0.0
    return layers, rows, act, old, old_ls, adv, ls


def _load(b, layers, rows, act, old, old_ls, adv, ls):
    b.set_policy_mlp(layers)
    b.set_policy_log_sigma(ls)
    b.fit_append(rows, act.astype(np.float64), weights=adv)
    b.fit_set_old_means(old)
    b.fit_set_old_log_sigma(old_ls)


@pytest.mark.parametrize("B", [1, 33, 256, 257, 300, 4096])
def test_the_kernels_arithmetic_by_bytes(B, batch_of):
    """The four statistics, ratio_out, the head's gradient and dz -- seen through db of the last layer, its float32 column sum in row
    order -- against ppo_sigma_loss_reference(fit_predict(idx), ...), with ent_coef 0 and 1/64. B = 257: a thread's second row; 300 and
    4096: several ranges of the split batch sum."""
    from gym_cloth_amd.policies import ppo_sigma_loss_reference
    widths = [300, 37, 64, 4]
    layers, rows, act, old, old_ls, adv, ls = _sigma_case(widths, 64, seed=4)
    assert (ls >= -2.0).all() and (ls <= 0.5).all() and len(np.unique(old_ls, axis=0)) == 64
    b = batch_of(10)
    _load(b, layers, rows, act, old, old_ls, adv, ls)
    r = np.random.RandomState(B)
    idx = np.array([6]) if B == 1 else np.concatenate([np.arange(min(B, 64)), r.randint(0, 64, size=max(B - 64, 0))])   # (row 6: active, A > 0)
    y = b.fit_predict(idx)
    for ent in (0.0, ENT):
        want_stats, want_dz, want_gls, want_ratio, active = ppo_sigma_loss_reference(y, act[idx], old[idx], old_ls[idx], adv[idx], ls, CLIP, ent, B)
        assert B > 1 or (active.all() and adv[idx[0]] != 0)
        if B >= 33:                                                            # the cases the comparison must meet, from the restatement's inputs alone
            a = adv[idx]
            assert (a == 0).any() and (a > 0).any() and (a < 0).any()
            for side in (want_ratio > 1.0 + CLIP, want_ratio < 1.0 - CLIP):
                assert (side & active & (a != 0)).any() and (side & ~active).any()
            assert ((want_ratio > 1.0 - CLIP) & (want_ratio < 1.0 + CLIP)).any()
        stats, grad, grad_ls, ratio = b.fit_ppo_sigma_grad(idx, CLIP, ent)
        print("B %d ent %g: stats %r, grad_ls %r, %d of %d rows not active" % (B, ent, stats.tolist(), grad_ls.tolist(), int((~active).sum()), B))
        assert ratio.tobytes() == want_ratio.tobytes()
        assert stats.tobytes() == want_stats.tobytes()
        assert grad_ls.tobytes() == want_gls.tobytes() and np.abs(grad_ls).max() > 0
        assert grad[-4:].tobytes() == _colsum32(want_dz).tobytes() and np.abs(grad[-4:]).max() > 0


# ---- 3. Gaussian data within an a-priori bound of the float64 reference -------------------------------------------------------------------
def _ppo_sigma_bound(layers, rows, act, old, old_ls, adv, idx, ls, clip, ent):
    """test_gpu_ppo._ppo_bound with inv_k = exp(-2 ls_k) in the place of 1 / sigma^2 and the error of the three extra exponentials. E =
    EXP_BOUND is the relative error of one exp_fixed against exp (its arguments -2 ls, -2 lo, 2 lo are exact doubles). With dy the
    forward bound on y, d = mu - a, t_old = (a - mo)^2 invo, t_new = d^2 inv:
        q = sum_k [(t_old - t_new) / 2 + (lo - ls)] moves by at most
        dq = sum_k [ t_old E + ((|d| + dy)^2 inv) E + (2 |d| dy + dy^2) inv ] / 2      (invo's and inv's error, then mu's)
             + 24 * 2^-53 sum_k [ (t_old + (|d| + dy)^2 inv) / 2 + |lo - ls| ]            (nine double operations per component on these magnitudes)
        rho_dev lies within rel = (e^dq - 1) + E e^dq of rho, relative;
        g = A rho d inv / B: from rho_dev, d +- dy and inv (1 + E) in four double operations and one float32 rounding:
            rel2 = (1 + rel) (1 + E) - 1;  dg = |A| rho inv / B (rel2 (|d| + dy) + dy) + gamma_2 (|g| + that);
        h_k = A rho (t_new_k - 1): t_new moves by dt = ((2 |d| dy + dy^2) + (|d| + dy)^2 E) inv + 2^-52 t_new, so
            dh = |A| rho (rel (|t_new - 1| + dt) + dt) + 4 * 2^-53 |h|; grad_ls_k moves by sum_active dh / B + 1e-14 sum |h| / B and the
            float32 rounding 2^-24 (|grad_ls| + that);
        kl_row = sum_k [(ls - lo) + ((so2 inv - 1) + e^2 inv) / 2], e = mu - mo: so2 inv carries (1 + E)^2 - 1, e^2 inv moves by
            (2 |e| dy + dy^2) inv (1 + E) + e^2 inv E; plus 16 * 2^-53 of the magnitudes (so2 inv + 1 + e^2 inv) / 2 + |ls - lo|;
        an active row stays active and a clipped one clipped when rho keeps rho rel from both bounds: `safe`.
    The loss moves by sum_active |A| rho rel / B plus 1e-14 of its magnitude sums (the entropy term among them); H by 4 * 2^-53 of
    sum |ls| + C. Everything behind dZ is test_gpu_policy_fit._grad_bound's.
    Returns (stats, their bounds, gradients, their bounds flat, grad_ls, its bound, the ReLU margin, safe bool[B])."""
    from gym_cloth_amd.references import ENTROPY_C
    E = EXP_BOUND
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)[idx]
    a, mo, lo, A = (np.asarray(v, dtype=np.float32).astype(np.float64)[idx] for v in (act, old, old_ls, adv))
    lsd = np.asarray(ls, dtype=np.float32).astype(np.float64)
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
    inv, invo, so2 = np.exp(-2.0 * lsd), np.exp(-2.0 * lo), np.exp(2.0 * lo)
    d = mu - a
    ad = np.abs(d)
    t_old, t_new, t_hi = (a - mo) ** 2 * invo, d ** 2 * inv, (ad + dy) ** 2 * inv
    q = ((t_old - t_new) / 2.0 + (lo - lsd)).sum(axis=1)
    assert np.abs(q).max() < 39.0 and np.abs(2.0 * lo).max() < 39.0          # nowhere near the clamp
    dq = ((t_old * E + t_hi * E + (2.0 * ad * dy + dy ** 2) * inv) / 2.0).sum(axis=1) + 24.0 * 2.0 ** -53 * ((t_old + t_hi) / 2.0 + np.abs(lo - lsd)).sum(axis=1)
    rho = np.exp(q)
    rel = np.expm1(dq) + E * np.exp(dq)
    lo_c, hi_c = 1.0 - clip, 1.0 + clip
    safe = (A == 0.0) | (np.minimum(np.abs(rho - lo_c), np.abs(rho - hi_c)) > rho * rel)
    s1, s2 = rho * A, np.clip(rho, lo_c, hi_c) * A
    active = s1 <= s2
    aA = np.abs(A)
    H = lsd.sum() + ENTROPY_C
    e = mu - mo
    kl_row = ((lsd - lo) + ((so2 * inv - 1.0) + e ** 2 * inv) / 2.0).sum(axis=1)
    dkl = ((so2 * inv * ((1.0 + E) ** 2 - 1.0) + (2.0 * np.abs(e) * dy + dy ** 2) * inv * (1.0 + E) + e ** 2 * inv * E) / 2.0).sum(axis=1) \
        + 16.0 * 2.0 ** -53 * ((so2 * inv + 1.0 + e ** 2 * inv) / 2.0 + np.abs(lsd - lo)).sum(axis=1)
    sur = np.where(active, s1, s2)
    stats = np.array([-sur.sum() / B - ent * H, (~active).sum() / float(B), kl_row.sum() / B, H])
    dstats = np.array([(np.where(active, aA * rho * rel, 0.0).sum() + 1e-14 * np.abs(sur).sum()) / B + 1e-14 * abs(ent * H), 0.0,
                       (dkl.sum() + 1e-14 * np.abs(kl_row).sum() + 1e-14 * (np.abs(lsd - lo).sum() + ((so2 * inv + 1.0 + e ** 2 * inv) / 2.0).sum())) / B,
                       4.0 * 2.0 ** -53 * (np.abs(lsd).sum() + ENTROPY_C)])
    # the head's gradient
    hrow = np.where(active[:, None], s1[:, None] * (t_new - 1.0), 0.0)
    dt = ((2.0 * ad * dy + dy ** 2) + (ad + dy) ** 2 * E) * inv + 2.0 ** -52 * t_new
    dh = np.where(active[:, None], (aA * rho)[:, None] * (rel[:, None] * (np.abs(t_new - 1.0) + dt) + dt) + 4.0 * 2.0 ** -53 * np.abs(hrow), 0.0)
    gls = -hrow.sum(axis=0) / B - ent
    dgls = (dh.sum(axis=0) + 1e-14 * np.abs(hrow).sum(axis=0)) / B
    dgls = dgls + 2.0 ** -24 * (np.abs(gls) + dgls)
    # dZ and the backward pass
    rel2 = (1.0 + rel) * (1.0 + E) - 1.0
    c = (aA * rho / B)[:, None] * inv[None, :]
    g = np.where(active[:, None], (s1[:, None] * d) * inv / B, 0.0)
    dg = c * (rel2[:, None] * (ad + dy) + dy)
    dg = np.where(active[:, None], dg + _gamma(2) * (np.abs(g) + dg), 0.0)
    grads, bounds = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        h, dh_, ag = hs[l], dhs[l], np.abs(g)
        dW = dg.T @ (np.abs(h) + dh_) + ag.T @ dh_ + _gamma(B + 1) * ((ag + dg).T @ (np.abs(h) + dh_))
        db = dg.sum(axis=0) + _gamma(B + 1) * (ag + dg).sum(axis=0)
        grads[l], bounds[l] = (g.T @ h, g.sum(axis=0)), (dW, db)
        if l:
            aW, mask = np.abs(Ws[l]), h > 0
            dgn = (dg @ aW + _gamma(Ws[l].shape[0] + 1) * ((ag + dg) @ aW)) * mask
            g, dg = (g @ Ws[l]) * mask, dgn
    return stats, dstats, grads, _flat(bounds), gls, dgls, margin, safe


BOUND_CASES = [(10, [300, 5, 4], 33), (10, [300, 37, 64, 4], 33), (10, [300, 37, 64, 4], 300), (25, [1875, 37, 64, 4], 33)]


@pytest.mark.parametrize("n_side,widths,B", BOUND_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_gaussian_data_within_the_a_priori_bound(n_side, widths, B, batch_of):
    """Every gradient element of the blob, the head's gradient and the statistics within the computed bound of ppo_sigma_reference; the
    ReLU mask and the active mask exact for every row of the minibatch (asserted): the minibatch is drawn among the rows whose ratio
    keeps its own error bound from both clip bounds -- a choice from the reference and the bound alone."""
    from gym_cloth_amd.policies import ppo_sigma_reference
    layers, rows, act, old, old_ls, adv, ls = _sigma_case(widths, 64, seed=len(widths))
    safe_all = _ppo_sigma_bound(layers, rows, act, old, old_ls, adv, np.arange(64), ls, CLIP, ENT)[7]
    assert safe_all.sum() >= 40, int(safe_all.sum())                          # the margin leaves most rows (at 1875 inputs and sigma = 0.16: 45 of 64)
    idx = np.random.RandomState(B).choice(np.nonzero(safe_all)[0], size=B)
    ref_stats, dstats, ref, bound, ref_gls, dgls, margin, safe = _ppo_sigma_bound(layers, rows, act, old, old_ls, adv, idx, ls, CLIP, ENT)
    assert margin > 0.0 and safe.all()
    chk_stats, chk, chk_gls, rho, active = ppo_sigma_reference(layers, rows, act, old, old_ls, adv, idx, ls, CLIP, ENT)   # the bound's own reference is ppo_sigma_reference's
    assert np.allclose(chk_stats, ref_stats, rtol=1e-12, atol=1e-15) and np.allclose(_flat(chk), _flat(ref), rtol=0, atol=1e-13)
    assert np.allclose(chk_gls, ref_gls, rtol=1e-12, atol=1e-15)
    assert active.any() and (~active).any() and (rho > 1.0 + CLIP).any() and (rho < 1.0 - CLIP).any()
    b = batch_of(n_side)
    _load(b, layers, rows, act, old, old_ls, adv, ls)
    stats, grad, grad_ls, ratio = b.fit_ppo_sigma_grad(idx, CLIP, ENT)
    err = np.abs(grad.astype(np.float64) - _flat(ref))
    share = (err[bound > 0] / bound[bound > 0]).max()
    err_ls, err_st = np.abs(grad_ls.astype(np.float64) - ref_gls), np.abs(stats - ref_stats)
    print("%r B %d: mask margin %.3e, stats %r err %r (bounds %r), max grad err %.3e, max err / bound: blob %.3e head %.3e stats %.3e, max |grad| %.3e, grad_ls %r" % (
        widths, B, margin, stats.tolist(), err_st.tolist(), dstats.tolist(), err.max(), share, (err_ls / dgls).max(),
        (err_st[dstats > 0] / dstats[dstats > 0]).max(), np.abs(grad).max(), grad_ls.tolist()))
    assert np.isfinite(grad).all() and np.abs(_flat(ref)).max() > 1e-4 and np.abs(ref_gls).max() > 1e-3
    assert (err_st <= dstats).all() and stats[1] == ref_stats[1]
    assert (err_ls <= dgls).all(), (err_ls, dgls)
    assert (err <= bound).all(), (np.nonzero(err > bound)[0][:8], err.max())


# ---- 4. the snapshot ----------------------------------------------------------------------------------------------------------------------
def test_snapshot_stores_the_head_and_the_column_follows_the_dataset():
    from gym_cloth_amd import _lib
    widths = [300, 37, 64, 4]
    layers = _layers(widths, 31)
    r = np.random.RandomState(17)
    n = _lib.FIT_MAX_BATCH + 3                                                 # 4099: two chunks of the predict, 65 blocks of the fill
    rows, labels = r.uniform(-1, 1, size=(n, 300)).astype(np.float32), r.uniform(-1, 1, size=(n, 4))
    ls = np.array([-1.25, 0.5, -0.03125, -2.0], dtype=np.float32)
    b = _new_batch(10)
    b.set_policy_mlp(layers)
    b.fit_append(rows[:64], labels[:64])                                      # 64 rows: the first capacity
    # without a head: what the snapshot did before -- the new column stays unset, and the sigma entries refuse the rows
    b.fit_snapshot_policy(0, 5)
    assert not b.fit_get_old_log_sigma().any() and b.fit_get_old_means(0, 5).tobytes() == b.fit_predict(np.arange(5)).tobytes()
    with pytest.raises(_lib.ClothHipError, match="no log-sigma head"):
        b.fit_ppo_sigma_grad(np.array([0]))
    b.set_policy_log_sigma(ls)
    with pytest.raises(_lib.ClothHipError, match="row 0 has no old log sigma.*clothhip_fit_data_snapshot_policy.*clothhip_fit_data_set_old_log_sigma"):
        b.fit_ppo_sigma_grad(np.array([0]))
    assert b.fit_ppo_grad(np.array([0, 4]), 1.0)[0].shape == (3,)             # the fixed-sigma entry needs the old mean alone
    pred = b.fit_predict(np.arange(64))
    # a sub-range with a head: n = 1 and n = 33; the rows outside stay unset (zeros) and refused
    b.fit_snapshot_policy(10, 1)
    b.fit_snapshot_policy(20, 33)
    inside = np.zeros(64, dtype=bool)
    inside[10] = inside[20:53] = True
    got, means = b.fit_get_old_log_sigma(), b.fit_get_old_means()
    assert got[inside].tobytes() == np.tile(ls, (34, 1)).tobytes() and not got[~inside].any()
    assert means[inside].tobytes() == pred[inside].tobytes() and means[:5].tobytes() == pred[:5].tobytes() and not means[5:10].any()
    assert b.fit_ppo_sigma_grad(np.array([10, 20, 52]))[0].shape == (4,)
    for row in (9, 11, 19, 53, 0, 63):
        with pytest.raises(_lib.ClothHipError, match="row %d has no old" % row):
            b.fit_ppo_sigma_grad(np.array([10, row]))
    # growth keeps the column; the new rows are unset
    b.fit_append(rows[64:], labels[64:])
    assert b.fit_size() == n
    got = b.fit_get_old_log_sigma()
    assert got[:64][inside].tobytes() == np.tile(ls, (34, 1)).tobytes() and not got[:64][~inside].any() and not got[64:].any()
    with pytest.raises(_lib.ClothHipError, match="row 64 has no old mean"):
        b.fit_ppo_sigma_grad(np.array([10, 64]))
    # the whole dataset under ANOTHER head: every row holds the new head's bytes, the old means are predict's
    ls2 = np.array([0.25, -0.75, 1.0, -1.5], dtype=np.float32)
    b.set_policy_log_sigma(ls2)
    b.fit_snapshot_policy()
    assert b.last_kernel_ms > 0.0
    full = b.fit_predict(np.arange(n))
    assert b.fit_get_old_log_sigma().tobytes() == np.tile(ls2, (n, 1)).tobytes() and b.fit_get_old_means().tobytes() == full.tobytes()
    assert b.fit_get_old_log_sigma(n - 2, 2).tobytes() == np.tile(ls2, (2, 1)).tobytes()
    # the stored head is the EARLIER one once the head moves; the host route writes the same column
    b.fit_ppo_sigma(r.randint(0, n, size=(3, 33)), CLIP, ENT, **ADAM)
    assert not np.array_equal(b.get_policy_log_sigma(), ls2) and b.fit_get_old_log_sigma().tobytes() == np.tile(ls2, (n, 1)).tobytes()
    assert b.fit_ppo_sigma_grad(np.arange(33))[0][2] > 0.0                    # the policy has moved away from its snapshot
    b.fit_set_old_log_sigma(np.tile(ls, (4, 1)), first=5)
    assert b.fit_get_old_log_sigma(4, 6).tobytes() == np.concatenate([ls2[None], np.tile(ls, (4, 1)), ls2[None]]).tobytes()
    # clear empties it: rows appended afterwards are unset again
    b.fit_clear()
    b.fit_append(rows[:8], labels[:8])
    assert not b.fit_get_old_log_sigma().any() and not b.fit_get_old_means().any()
    b.fit_set_old_means(full[:8])
    with pytest.raises(_lib.ClothHipError, match="row 0 has no old log sigma"):
        b.fit_ppo_sigma_grad(np.array([0]))
    b.close()


# ---- 5. the head's optimizer ------------------------------------------------------------------------------------------------------------------
SGD = dict(optimizer="sgd", lr=3e-2, momentum=0.0)


def test_the_head_follows_the_restated_optimizers_and_the_blob_stands_still():
    """Every advantage 0 and ent_coef = 1/64: the surrogate and dz vanish, the head's gradient is -1/64 on every component. Under SGD
    the blob's bytes stand still and the head follows sgd_reference for ten steps; under Adam, after three squared-error steps of the
    blob (its t = 3), the head follows adam_reference from ITS OWN t = 1."""
    from gym_cloth_amd.policies import adam_reference, sgd_reference
    layers, rows, act, old, old_ls, adv, ls = _sigma_case([300, 37, 64, 4], 64, seed=4)
    g = np.full(4, -ENT, dtype=np.float32)
    table = np.random.RandomState(1).randint(0, 64, size=(10, 33))
    b = _new_batch(10)
    _load(b, layers, rows, act, old, old_ls, np.zeros(64, dtype=np.float32), ls)
    stats, heads = b.fit_ppo_sigma(table, CLIP, ENT, **SGD)
    assert _blob(b).tobytes() == _flat(layers).tobytes() and (stats[:, 1] == 0.0).all()
    want, u = ls.copy(), np.zeros(4, dtype=np.float32)
    for s in range(10):
        assert heads[s].tobytes() == want.tobytes(), s
        want, u = sgd_reference(want, u, g, lr=SGD["lr"], momentum=0.0)
    assert b.get_policy_log_sigma().tobytes() == want.tobytes() and not np.array_equal(want, ls)
    assert np.array_equal(stats[:, 3], [ppo_H(h) for h in heads])
    # Adam, both optimizers fresh: the blob takes three squared-error steps first (under weights of 1, which then go back to 0), so
    # its step count is 3 when the head's first step comes
    b.fit_reset()
    b.set_policy_log_sigma(ls)
    b.fit_set_weights(np.ones(64, dtype=np.float32))
    b.fit(table[:3], **ADAM)
    assert _blob(b).tobytes() != _flat(layers).tobytes()
    b.fit_set_weights(np.zeros(64, dtype=np.float32))
    stats, heads = b.fit_ppo_sigma(table[:5], CLIP, ENT, **ADAM)
    want, m, v = ls.copy(), np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float32)
    for s in range(5):
        assert heads[s].tobytes() == want.tobytes(), s
        want, m, v = adam_reference(want, m, v, g, s + 1, lr=ADAM["lr"], beta1=ADAM["beta1"], beta2=ADAM["beta2"], eps=ADAM["eps"])
    assert b.get_policy_log_sigma().tobytes() == want.tobytes()
    # the blob under a zero gradient: Adam's moments of the three steps decay but its step m / (sqrt(v) + eps) is not 0 -- it moves on
    # as five more steps of fit under zero weights move it: the same bytes on a twin that never heard of a head (steps 4 .. 8 of both)
    twin = _new_batch(10)
    twin.set_policy_mlp(layers)
    twin.fit_append(rows, act.astype(np.float64), weights=np.ones(64, dtype=np.float32))
    twin.fit(table[:3], **ADAM)
    twin.fit_set_weights(np.zeros(64, dtype=np.float32))
    twin.fit(table[:5], **ADAM)
    assert _blob(b).tobytes() == _blob(twin).tobytes()
    b.close(); twin.close()


def ppo_H(head):
    from gym_cloth_amd.references import ENTROPY_C
    h = 0.0
    for k in range(4):
        h = h + float(head[k])
    return h + ENTROPY_C


def test_steps_add_up_two_handles_agree_and_the_resets():
    """2 + 3 steps equal 5 steps and two handles agree, in the blob, the head and the statistics. set_policy_log_sigma restarts the
    head's moments ONLY: the blob's next step is the twin's, the head's next step is adam_reference's first. fit_reset restarts both."""
    from gym_cloth_amd.policies import adam_reference
    layers, rows, act, old, old_ls, adv, ls = _sigma_case([300, 37, 64, 4], 64, seed=4)
    table = np.random.RandomState(2).randint(0, 64, size=(6, 33))
    one, two, split = _new_batch(10), _new_batch(10), _new_batch(10)
    out = []
    for b in (one, two):
        _load(b, layers, rows, act, old, old_ls, adv, ls)
        first = b.fit_ppo_sigma_grad(table[0], CLIP, ENT)
        stats, heads = b.fit_ppo_sigma(table[:5], CLIP, ENT, **ADAM)
        assert stats.shape == (5, 4) and stats[0].tobytes() == first[0].tobytes() and heads[0].tobytes() == ls.tobytes()
        out.append((stats, heads, _blob(b), b.get_policy_log_sigma()))
    assert all(a.tobytes() == c.tobytes() for a, c in zip(out[0], out[1]))
    assert not np.array_equal(out[0][2], _flat(layers)) and not np.array_equal(out[0][3], ls) and (out[0][0][:, 1] > 0).any()
    _load(split, layers, rows, act, old, old_ls, adv, ls)
    sa, ha = split.fit_ppo_sigma(table[:2], CLIP, ENT, **ADAM)
    sb, hb = split.fit_ppo_sigma(table[2:5], CLIP, ENT, **ADAM)
    assert np.concatenate([sa, sb]).tobytes() == out[0][0].tobytes() and np.concatenate([ha, hb]).tobytes() == out[0][1].tobytes()
    assert _blob(split).tobytes() == out[0][2].tobytes() and split.get_policy_log_sigma().tobytes() == out[0][3].tobytes()
    # the head's moments alone: `one` gets its own head's values back, `two` is left as it is
    head5 = out[0][3]
    one.set_policy_log_sigma(head5)
    gls = one.fit_ppo_sigma_grad(table[5], CLIP, ENT)[2]
    assert gls.tobytes() == two.fit_ppo_sigma_grad(table[5], CLIP, ENT)[2].tobytes()
    one.fit_ppo_sigma(table[5:], CLIP, ENT, **ADAM)
    two.fit_ppo_sigma(table[5:], CLIP, ENT, **ADAM)
    assert _blob(one).tobytes() == _blob(two).tobytes()                         # the blob's optimizer went on: t = 6 on both
    fresh = adam_reference(head5, np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float32), gls, 1, lr=ADAM["lr"], beta1=ADAM["beta1"],
                           beta2=ADAM["beta2"], eps=ADAM["eps"])[0]
    assert one.get_policy_log_sigma().tobytes() == fresh.tobytes() and two.get_policy_log_sigma().tobytes() != fresh.tobytes()
    # fit_reset restarts both: from the same blob and head, the step is the first step of a fresh optimizer for the blob AND the head
    split.fit_reset()
    head, blob = split.get_policy_log_sigma(), _blob(split)
    _, grad, gls, _ = split.fit_ppo_sigma_grad(table[5], CLIP, ENT)
    split.fit_ppo_sigma(table[5:], CLIP, ENT, **ADAM)
    z4, zn = np.zeros(4, dtype=np.float32), np.zeros(blob.size, dtype=np.float32)
    kw = dict(lr=ADAM["lr"], beta1=ADAM["beta1"], beta2=ADAM["beta2"], eps=ADAM["eps"])
    assert split.get_policy_log_sigma().tobytes() == adam_reference(head, z4, z4, gls, 1, **kw)[0].tobytes()
    assert _blob(split).tobytes() == adam_reference(blob, zn, zn, grad, 1, **kw)[0].tobytes()
    for b in (one, two, split):
        b.close()


# ---- 6. the growing head freezes the fit ----------------------------------------------------------------------------------------------------
FREEZE_SEED, FREEZE_LR, FREEZE_LS, FREEZE_K = 1, 1e-4, 2.0, 3.0      # chosen on the CPU: the reference freezes at step 14, margins 1e-3


def _freeze_case():
    """Twelve rows, every advantage +1, every label component three sigma (+- 20 %) from the first mean, sigma = e^2: the mean's pull
    on a ratio goes with 1 / sigma^2, the head's does not -- it is the HEAD that grows until every ratio has passed 1 + eps."""
    widths = [300, 16, 4]
    layers = _layers(widths, 60 + FREEZE_SEED)
    r = np.random.RandomState(600 + FREEZE_SEED)
    rows = r.uniform(-1, 1, size=(12, 300)).astype(np.float32)
    sig = np.exp(FREEZE_LS)
    act = (_forward(layers, rows) + FREEZE_K * sig * np.where(r.uniform(size=(12, 4)) < 0.5, -1, 1) * r.uniform(0.8, 1.2, size=(12, 4))).astype(np.float32)
    return widths, layers, rows, act, np.ones(12, dtype=np.float32), np.full(4, FREEZE_LS, dtype=np.float32)


def _reference_steps_to_freeze(limit=100):
    """Plain SGD of blob and head on ppo_sigma_reference's gradients from the old means = the first means and the old head = the first
    head: (the step at which clip_fraction == 1 or None, the smallest relative distance of a ratio from a clip bound at that step, the
    same one step before, the head at that step)."""
    from gym_cloth_amd.policies import ppo_sigma_reference, sgd_reference, unpack_mlp
    widths, layers, rows, act, adv, ls = _freeze_case()
    old, old_ls = _forward(layers, rows).astype(np.float32), np.tile(ls, (12, 1))
    theta, u, ul = _flat(layers).astype(np.float32), np.zeros(_flat(layers).size, dtype=np.float32), np.zeros(4, dtype=np.float32)
    before = None
    for s in range(limit):
        stats, grads, gls, rho, _ = ppo_sigma_reference(unpack_mlp(np.array(widths, dtype=np.int32), theta), rows, act, old, old_ls, adv, np.arange(12), ls, CLIP, 0.0)
        m = float(np.minimum(np.abs(rho / (1.0 - CLIP) - 1.0), np.abs(rho / (1.0 + CLIP) - 1.0)).min())
        if stats[1] == 1.0:
            return s, m, before, ls
        before = m
        theta, u = sgd_reference(theta, u, _flat(grads).astype(np.float32), lr=FREEZE_LR, momentum=0.0)
        ls, ul = sgd_reference(ls, ul, gls.astype(np.float32), lr=FREEZE_LR, momentum=0.0)
    return None, m, before, ls


def test_the_growing_head_freezes_the_fit():
    widths, layers, rows, act, adv, ls = _freeze_case()
    at, margin_at, margin_before, ref_head = _reference_steps_to_freeze()
    assert at is not None and 2 <= at < 100 and margin_at >= 1e-6 and margin_before >= 1e-6, (at, margin_at, margin_before)
    assert (ref_head > ls).all()                                              # the reference's head has grown
    sgd = dict(optimizer="sgd", lr=FREEZE_LR, momentum=0.0)
    idx = np.arange(12)
    b = _new_batch(10)
    b.set_policy_mlp(layers)
    b.set_policy_log_sigma(ls)
    b.fit_append(rows, act.astype(np.float64), weights=adv)
    b.fit_snapshot_policy()
    steps, fractions = 0, []
    while steps < 100:
        stats = b.fit_ppo_sigma_grad(idx, CLIP, 0.0)[0]
        fractions.append(stats[1])
        if stats[1] == 1.0:
            break
        b.fit_ppo_sigma(idx[None], CLIP, 0.0, **sgd)
        steps += 1
    head = b.get_policy_log_sigma()
    print("the reference freezes at step %d (margins %.3e, %.3e before), the device at step %d; head %r -> %r (reference %r); clip fractions %r" % (
        at, margin_at, margin_before, steps, ls.tolist(), head.tolist(), ref_head.tolist(), fractions))
    assert fractions[-1] == 1.0 and fractions[0] == 0.0 and steps == at
    # both heads take float32 SGD steps from the same start: a step's rounding differs by at most one ulp of a value near 2 (2.4e-7),
    # the gradients by parts in 10^6 of a step of 4e-4 -- at most 14 (2.4e-7 + 1e-9) < 1e-5 apart after 14 steps
    assert (head > ls).all() and np.abs(head.astype(np.float64) - ref_head).max() <= 1e-5
    stats, grad, grad_ls, ratio = b.fit_ppo_sigma_grad(idx, CLIP, 0.0)
    assert not grad.any() and not grad_ls.any() and (ratio >= np.float32(1.2)).all() and abs(stats[0] + 1.2) <= 1e-15 and stats[1] == 1.0
    frozen = (_blob(b).tobytes(), head.tobytes())
    later, heads = b.fit_ppo_sigma(np.tile(idx, (10, 1)), CLIP, 0.0, **sgd)
    assert (_blob(b).tobytes(), b.get_policy_log_sigma().tobytes()) == frozen and (later[:, 1] == 1.0).all() and frozen[0] != _flat(layers).tobytes()
    assert heads.tobytes() == np.tile(head, (10, 1)).tobytes()
    b.close()


# ---- 7. untouched ground --------------------------------------------------------------------------------------------------------------------
SIGMA = 0.5


@pytest.mark.parametrize("B", [9, 300], ids=["B9", "B300-two-ranges"])
def test_the_existing_entries_keep_their_bits(B):
    """Two handles, one network, the same rows and old means. One holds a head and interleaves the new entries with the existing calls;
    the other never calls a new entry. fit_grad, fit_ppo_grad, fit and fit_ppo return the same bytes on both, and leave the same blob.
    Then the first takes steps with the head (which move ITS blob), both get the network again, and the existing steps agree again."""
    layers, rows, act, old, old_ls, adv, ls = _sigma_case([300, 37, 64, 4], 40, seed=5)
    r = np.random.RandomState(B)
    idx, table = r.randint(0, 40, size=B), r.randint(0, 40, size=(3, B))
    new, twin = _new_batch(10), _new_batch(10)
    for b in (new, twin):
        b.set_policy_mlp(layers)
        b.fit_append(rows, act.astype(np.float64), weights=adv)
        b.fit_set_old_means(old)
    new.set_policy_log_sigma(ls)
    new.fit_set_old_log_sigma(old_ls)

    def same(f):
        a, c = f(new), f(twin)
        a, c = (a, c) if isinstance(a, tuple) else ((a,), (c,))
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, c))
        return a
    g0 = same(lambda b: b.fit_grad(idx))
    new.fit_ppo_sigma_grad(idx, CLIP, ENT)
    same(lambda b: b.fit_ppo_grad(idx, SIGMA, CLIP))
    new.fit_snapshot_policy(3, 20)                                            # with a head: both old columns; the twin's: the old means
    twin.fit_snapshot_policy(3, 20)
    same(lambda b: b.fit_get_old_means())
    new.fit_ppo_sigma_grad(idx, CLIP, 0.0)
    same(lambda b: b.fit(table, **ADAM))
    same(_blob)
    new.fit_ppo_sigma_grad(idx, CLIP, ENT)
    same(lambda b: b.fit_ppo(table, SIGMA, CLIP, **ADAM))
    same(_blob)
    g1 = same(lambda b: b.fit_grad(idx))
    assert g1[1].tobytes() != g0[1].tobytes()
    same(lambda b: b.fit_predict(idx))
    assert new.get_policy_log_sigma().tobytes() == ls.tobytes()                # no existing entry moved the head
    # steps with the head move the first handle's blob and its policy optimizer; a new network restarts both handles alike
    new.fit_snapshot_policy()
    new.fit_ppo_sigma(table, CLIP, ENT, **ADAM)
    assert _blob(new).tobytes() != _blob(twin).tobytes() and new.get_policy_log_sigma().tobytes() != ls.tobytes()
    moved_head = new.get_policy_log_sigma()
    for b in (new, twin):
        b.set_policy_mlp(layers)
        b.fit_set_old_means(old)
    assert new.get_policy_log_sigma().tobytes() == moved_head.tobytes()        # setting a network leaves the head's values alone
    same(lambda b: b.fit_ppo(table, SIGMA, CLIP, **ADAM))
    same(lambda b: b.fit(table, **ADAM))
    same(_blob)
    new.close(); twin.close()


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
    old_ls = r.uniform(-1, 0, size=(n, 4)).astype(np.float32)
    ls = np.array([-0.5, -0.25, -0.75, -1.0], dtype=np.float32)
    b.set_policy_log_sigma(ls)
    b.fit_append(rows, labels, weights=w)
    b.fit_set_old_means(old[:9])                                               # row 9 has no old mean, rows 8 and 9 no old log sigma
    b.fit_set_old_log_sigma(old_ls[:8])
    old[9:], old_ls[8:] = 0.0, 0.0
    idx = np.arange(8, dtype=np.int32)
    adam = _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    b.fit_ppo_sigma(idx[None], CLIP, ENT, **ADAM)                              # one step, so that all moments and both step counts exist
    snap = (b.fit_grad(idx), b.fit_ppo_sigma_grad(idx, CLIP, ENT), _blob(b), b.get_policy_log_sigma())
    after_one = (b.fit_ppo_sigma(idx[None], CLIP, ENT, **ADAM), _blob(b), b.get_policy_log_sigma())      # what the NEXT step gives from this state ...
    b.set_policy_mlp(pol)                                                      # ... which is rebuilt: the same network and head, one step
    b.set_policy_log_sigma(ls)
    b.fit_ppo_sigma(idx[None], CLIP, ENT, **ADAM)
    assert _blob(b).tobytes() == snap[2].tobytes() and b.get_policy_log_sigma().tobytes() == snap[3].tobytes()
    fp, ip, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), _lib.i32p, _lib.dp
    Q = _lib.ClothPpoSigmaParams
    g, gl, st, ra = np.zeros(b._mlp_n_params, dtype=np.float32), np.zeros(4, dtype=np.float32), np.zeros(4), np.zeros(8, dtype=np.float32)
    mu = np.zeros((n + 1, 4), dtype=np.float32)

    def unchanged():
        assert b.fit_size() == n and b.fit_get_weights().tobytes() == w.tobytes()
        assert b.fit_get_old_means().tobytes() == old.tobytes() and b.fit_get_old_log_sigma().tobytes() == old_ls.tobytes()
        o, l = b.fit_data()
        assert np.array_equal(o, rows) and np.array_equal(l, labels.astype(np.float32))
        now = (b.fit_grad(idx), b.fit_ppo_sigma_grad(idx, CLIP, ENT), _blob(b), b.get_policy_log_sigma())
        assert now[0][0] == snap[0][0] and now[0][1].tobytes() == snap[0][1].tobytes() and now[2].tobytes() == snap[2].tobytes() and now[3].tobytes() == snap[3].tobytes()
        assert all(a.tobytes() == c.tobytes() for a, c in zip(now[1], snap[1]))
        with pytest.raises(_lib.ClothHipError, match="row 8 has no old log sigma"):
            b.fit_ppo_sigma_grad(np.array([0, 8]))

    ok = Q(CLIP, ENT)
    grad_call = lambda q, ix, B: L.clothhip_policy_fit_ppo_sigma_grad(h, q, ix, B, fp(g), fp(gl), dp(st), fp(ra))
    # a row without an old mean (9: named first) or without an old log sigma (8)
    assert grad_call(C.byref(ok), ip(np.array([0, 9], dtype=np.int32)), 2) == _lib.ESTATE
    msg = L.clothhip_last_error().decode()
    assert "row 9" in msg and "no old mean" in msg and "clothhip_fit_data_snapshot_policy" in msg
    assert grad_call(C.byref(ok), ip(np.array([0, 8], dtype=np.int32)), 2) == _lib.ESTATE
    msg = L.clothhip_last_error().decode()
    assert "row 8" in msg and "no old log sigma" in msg and "clothhip_fit_data_set_old_log_sigma" in msg
    assert L.clothhip_policy_fit_ppo_sigma(h, C.byref(adam), C.byref(ok), ip(np.array([[0, 1], [8, 2]], dtype=np.int32)), 2, 2, None, None) == _lib.ESTATE
    # eps and the entropy coefficient
    for q in (Q(-0.01, ENT), Q(1.0, ENT), Q(np.nan, ENT), Q(np.inf, ENT), Q(CLIP, -1e-9), Q(CLIP, np.nan), Q(CLIP, np.inf)):
        assert grad_call(C.byref(q), ip(idx), 8) == _lib.EINVAL
        assert L.clothhip_policy_fit_ppo_sigma(h, C.byref(adam), C.byref(q), ip(idx), 1, 8, dp(st), fp(gl)) == _lib.EINVAL
    # what clothhip_policy_fit_ppo refuses, and NULL pointers
    assert grad_call(None, ip(idx), 8) == _lib.EINVAL and grad_call(C.byref(ok), None, 8) == _lib.EINVAL
    assert grad_call(C.byref(ok), ip(idx), 0) == _lib.EINVAL and grad_call(C.byref(ok), ip(idx), _lib.FIT_MAX_BATCH + 1) == _lib.EINVAL
    assert grad_call(C.byref(ok), ip(np.array([0, n], dtype=np.int32)), 2) == _lib.EINVAL and grad_call(C.byref(ok), ip(np.array([0, -1], dtype=np.int32)), 2) == _lib.EINVAL
    fit_call = lambda p, q, ix, s: L.clothhip_policy_fit_ppo_sigma(h, p, q, ix, s, 8, None, None)
    assert fit_call(None, C.byref(ok), ip(idx), 1) == _lib.EINVAL and fit_call(C.byref(adam), None, ip(idx), 1) == _lib.EINVAL
    assert fit_call(C.byref(adam), C.byref(ok), None, 1) == _lib.EINVAL and fit_call(C.byref(adam), C.byref(ok), ip(idx), -1) == _lib.EINVAL
    for field, bad in (("optimizer", 2.0), ("lr", -1.0), ("lr", np.nan), ("beta1", 1.0), ("beta2", 1.5), ("eps", np.inf), ("momentum", -0.1)):
        p = _lib.ClothFitParams(0.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
        setattr(p, field, bad)
        assert fit_call(C.byref(p), C.byref(ok), ip(idx), 1) == _lib.EINVAL, field
    assert fit_call(C.byref(adam), C.byref(ok), ip(idx), 0) == _lib.OK                                              # no steps: nothing changes
    assert L.clothhip_policy_fit_ppo_sigma_grad(h, C.byref(ok), ip(idx), 8, None, None, None, None) == _lib.OK       # every output is optional
    # the head's setter and the column's entries
    for bad in ([0.0, np.nan, 0.0, 0.0], [0.0, 0.0, np.inf, 0.0], [10.5, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, -10.5]):
        assert L.clothhip_set_policy_log_sigma(h, fp(np.array(bad, dtype=np.float32))) == _lib.EINVAL
    assert L.clothhip_get_policy_log_sigma(h, None) == _lib.EINVAL
    for first, k in ((n - 1, 2), (n, 1), (-1, 1), (0, n + 1), (2, -1)):
        assert L.clothhip_fit_data_set_old_log_sigma(h, first, k, fp(mu)) == _lib.EINVAL and L.clothhip_fit_data_get_old_log_sigma(h, first, k, fp(mu.copy())) == _lib.EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        vb = np.zeros((2, 4), dtype=np.float32)
        vb[1, 2] = bad
        assert L.clothhip_fit_data_set_old_log_sigma(h, 0, 2, fp(vb)) == _lib.EINVAL
    assert L.clothhip_fit_data_set_old_log_sigma(h, 0, 2, None) == _lib.EINVAL and L.clothhip_fit_data_get_old_log_sigma(h, 0, 2, None) == _lib.EINVAL
    assert L.clothhip_fit_data_set_old_log_sigma(h, n, 0, None) == _lib.OK
    unchanged()
    # a launch in flight
    nsteps, done = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, 2, 4)))
    assert grad_call(C.byref(ok), ip(idx), 8) == _lib.ESTATE and fit_call(C.byref(adam), C.byref(ok), ip(idx), 1) == _lib.ESTATE
    assert L.clothhip_set_policy_log_sigma(h, fp(ls)) == _lib.ESTATE and L.clothhip_set_policy_log_sigma(h, None) == _lib.ESTATE
    assert L.clothhip_get_policy_log_sigma(h, fp(gl)) == _lib.ESTATE
    assert L.clothhip_fit_data_set_old_log_sigma(h, 0, 2, fp(mu)) == _lib.ESTATE and L.clothhip_fit_data_get_old_log_sigma(h, 0, 2, fp(mu.copy())) == _lib.ESTATE
    b.run_actions_end()
    unchanged()
    # the moments and both step counts are untouched too: the next step is the one that followed the snapshot
    nxt = b.fit_ppo_sigma(idx[None], CLIP, ENT, **ADAM)
    assert nxt[0].tobytes() == after_one[0][0].tobytes() and nxt[1].tobytes() == after_one[0][1].tobytes()
    assert _blob(b).tobytes() == after_one[1].tobytes() and b.get_policy_log_sigma().tobytes() == after_one[2].tobytes()
    # a population: the shared network only (the head and the column may exist beside it)
    twin = _new_batch(10)
    twin.set_policy_population([pol, _layers([300, 5, 4], 2)], np.zeros(1, dtype=np.int32))
    twin.set_policy_log_sigma(ls)
    twin.fit_append(rows, labels, weights=w)
    th = twin._h
    assert L.clothhip_fit_data_set_old_log_sigma(th, 0, n, fp(np.ascontiguousarray(old_ls))) == _lib.OK
    assert L.clothhip_policy_fit_ppo_sigma_grad(th, C.byref(ok), ip(idx), 8, fp(g), fp(gl), dp(st), fp(ra)) == _lib.ESTATE and "population" in L.clothhip_last_error().decode()
    assert L.clothhip_policy_fit_ppo_sigma(th, C.byref(adam), C.byref(ok), ip(idx), 1, 8, None, None) == _lib.ESTATE and "population" in L.clothhip_last_error().decode()
    assert twin.get_policy_log_sigma().tobytes() == ls.tobytes()
    twin.close()
    # no head, an empty dataset, no network (these change the handle, so they come last)
    b.set_policy_log_sigma(None)
    assert grad_call(C.byref(ok), ip(idx), 8) == _lib.ESTATE and "no log-sigma head" in L.clothhip_last_error().decode()
    assert fit_call(C.byref(adam), C.byref(ok), ip(idx), 1) == _lib.ESTATE and L.clothhip_get_policy_log_sigma(h, fp(gl)) == _lib.ESTATE
    b.set_policy_log_sigma(ls)
    b.fit_clear()
    assert grad_call(C.byref(ok), ip(idx), 8) == _lib.ESTATE and "empty" in L.clothhip_last_error().decode()
    v.close()
    bare = _new_batch(10)
    bare.set_policy_log_sigma(ls)
    assert L.clothhip_policy_fit_ppo_sigma_grad(bare._h, C.byref(ok), ip(idx), 8, fp(g), fp(gl), dp(st), fp(ra)) == _lib.ESTATE
    bare.close()


# ---- 8. demos.ppo_fit(sigma=None) -------------------------------------------------------------------------------------------------------------
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
    tr.set_log_sigma(np.log(0.05))
    head = tr.log_sigma()
    noise = np.random.RandomState(14).normal(size=(4, 4, 4)) * tr.sigma()       # unit noise scaled by the head on the host
    col = actor_critic_collect(v, tr, n_actions=4, policy_noise=noise, slots_per_launch=4)
    n = col["appended"] + col["open_rows"]
    before = tr.predict(np.arange(n))
    fit = ppo_fit(v, tr, critic, col, gamma=0.9, lam=0.8, clip=0.2, n_value_steps=3, n_epochs=3, batch_size=8, seed=0, target_kl=target_kl, ent_coef=ENT)
    res = (fit, col, before, v.batch.fit_get_old_means(), v.batch.fit_get_old_log_sigma(), head, _blob(v.batch), v.batch.get_value_mlp())
    v.close()
    return res


def test_ppo_fit_with_the_learned_head_is_deterministic_and_stops_on_target_kl():
    one, again = _ppo_run(None), _ppo_run(None)
    fit, col, before, old, old_ls, head, blob, vblob = one
    assert blob.tobytes() == again[6].tobytes() and vblob.tobytes() == again[7].tobytes()
    assert fit["ppo_stats"].tobytes() == again[0]["ppo_stats"].tobytes() and fit["log_sigma"].tobytes() == again[0]["log_sigma"].tobytes()
    assert fit["log_sigma_after"].tobytes() == again[0]["log_sigma_after"].tobytes()
    n_mb = len(col["nonleaf"]) // 8
    assert col["appended"] == 16 and n_mb == 2 and fit["epochs"] == 3 and fit["ppo_stats"].shape == (3 * n_mb, 4) and np.isfinite(fit["ppo_stats"]).all()
    assert fit["log_sigma"].shape == (3 * n_mb, 4) and fit["log_sigma"][0].tobytes() == head.tobytes()
    assert old.tobytes() == before.tobytes() and old_ls.tobytes() == np.tile(head, (len(old), 1)).tobytes()     # ONE snapshot of both columns, before any policy step
    # at the snapshot kl's only term is sum_k (exp_fixed(2 l) exp_fixed(-2 l) - 1) / 2: two exponentials within EXP_BOUND each, a product
    # and a difference of one rounding each, four components, halved
    assert fit["ppo_stats"][0, 1] == 0.0 and abs(fit["ppo_stats"][0, 2]) <= 2.0 * (2.0 * EXP_BOUND + 2.0 ** -52) and (fit["ppo_stats"][1:, 2] > 1e-9).all()
    assert fit["log_sigma_after"].tobytes() != head.tobytes() and blob.tobytes() != _flat(_layers([300, 5, 4], 21)).tobytes()
    stopped = _ppo_run(0.0)
    assert stopped[0]["epochs"] == 1 and stopped[0]["ppo_stats"].shape == (n_mb, 4)
    assert stopped[0]["ppo_stats"].tobytes() == fit["ppo_stats"][:n_mb].tobytes()
