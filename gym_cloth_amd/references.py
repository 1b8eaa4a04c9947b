"""The numpy restatements the GPU tests pin the device to, and that a user can check a fit against: the trainer's three objectives in
float64 over the one pass of mlp.py (fit_reference, value_fit_reference, ppo_reference, ppo_sigma_reference, q_fit_reference, dpg_reference), and what the device computes
restated operation by operation, bit for bit (gae_reference, DDPG's concat_reference, td_loss_reference, dpg_dz_reference and polyak_reference, exp_fixed_reference, ppo_loss_reference, ppo_sigma_loss_reference, adam_reference, sgd_reference, Philox, the
cross-entropy planner's sampling, scoring and refit, and the exploration noise made on the device: log_fixed_reference,
normal_fixed_reference, policy_noise_reference). numpy and math only; nothing here touches the library."""
import math

import numpy as np

from .mlp import mlp_backward, mlp_float64, mlp_forward


def fit_reference(layers, obs, labels, idx, weights=None):
    """Pure-numpy float64 loss and gradient of the trainer's objective, for tests and for users who want to check a fit:
    L = 1 / (4 B) sum_r w_r sum_k (y_rk - a_rk)^2 over the rows idx [B] of (obs [n, in], labels [n, 4], weights [n] or None: all 1 --
    then torch.nn.MSELoss()) with ReLU after every layer but the last and ReLU' = 1 where the pre-activation is > 0, else 0. The
    normaliser is B, whatever the weights sum to. obs, labels, the per-row weights and the network's weights are rounded to float32
    first (what the device stores), the arithmetic is float64. Returns (loss, [(dW, db), ...]) in `layers`' shapes."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    Ws, bs = mlp_float64(layers)
    x = np.asarray(obs, dtype=np.float32).astype(np.float64)[ix]
    a = np.asarray(labels, dtype=np.float64).astype(np.float32).astype(np.float64)[ix]
    B = len(ix)
    hs = mlp_forward(Ws, bs, x)
    d = hs[-1] - a
    if weights is None:
        loss = float((d * d).sum() / (4.0 * B))
        g = d / (2.0 * B)
    else:
        w = np.asarray(weights, dtype=np.float64).astype(np.float32).astype(np.float64).reshape(-1)[ix][:, None]
        loss = float((w * (d * d)).sum() / (4.0 * B))
        g = w * d / (2.0 * B)
    return loss, mlp_backward(Ws, hs, g)


def value_fit_reference(layers, obs, ret, idx):
    """Pure-numpy float64 loss and gradient of the critic's objective (clothhip_value_fit_grad): L_V = 1 / (2 B) sum_r (v_r - ret_r)^2
    over the rows idx [B] of (obs [n, in], ret [n]), UNWEIGHTED, the network as fit_reference takes it with a last width of 1. obs, ret
    and the network's weights are rounded to float32 first (what the device stores), the arithmetic is float64. Returns
    (loss, [(dW, db), ...]) in `layers`' shapes."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    Ws, bs = mlp_float64(layers)
    if Ws[-1].shape[0] != 1:
        raise ValueError("a value network ends in ONE output (got %d)" % Ws[-1].shape[0])
    x = np.asarray(obs, dtype=np.float32).astype(np.float64)[ix]
    a = np.asarray(ret, dtype=np.float64).astype(np.float32).astype(np.float64).reshape(-1)[ix][:, None]
    B = len(ix)
    hs = mlp_forward(Ws, bs, x)
    d = hs[-1] - a
    loss = float((d * d).sum() / (2.0 * B))
    g = d / float(B)
    return loss, mlp_backward(Ws, hs, g)


NEXT_TERMINAL, NEXT_NONE = -1, -2          # _lib.FIT_NEXT_*: a row's successor column besides a row number


def _house_sum(x):
    """The device's reduction order over x [n] float64: thread t of 256 adds elements t, t + 256, ... in ascending order from +0.0, then a
    halving tree adds the 256 sums. (Elements that do not take part are passed as +0.0: s + 0.0 keeps the bits of a sum that began at +0.0.)"""
    x = np.asarray(x, dtype=np.float64)
    k = (len(x) + 255) // 256
    tab = np.zeros((max(k, 1), 256))
    tab.reshape(-1)[:len(x)] = x
    red = np.zeros(256)
    for row in tab:
        red = red + row
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return red[0]


def gae_reference(v, rew, next, gamma, lam, w_scale=1.0, normalize=False):
    """clothhip_fit_data_gae restated in float64 numpy, operation by operation (include/clothhip.h: ADVANTAGES AND VALUE TARGETS ON THE
    DEVICE): v [n] float32 the critic on the rows of a range, rew [n] float32, next [n] int with successors as indices INTO THE RANGE
    (the dataset's column minus `first` where it is >= 0), NEXT_TERMINAL or NEXT_NONE (a leaf). For a non-leaf row the chain r, next[r],
    ... stops after a row whose next is TERMINAL or whose successor is a leaf; delta = (rew + gamma nv) - v, A = sum (gamma lam)^k
    delta_k accumulated for k ascending with coef = coef c. Returns (adv float32[n], ret float32[n], w float32[n]): adv = (float)A,
    ret = (float)(A + v), w = (float)((float32)w_scale A^) with A^ = A, or normalised (A - mean) / (std + 1e-8) over the non-leaf rows in
    the device's reduction order; a leaf has adv 0, ret v, w 0. Bit for bit what the device writes."""
    v64 = np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1)
    r64 = np.asarray(rew, dtype=np.float32).astype(np.float64).reshape(-1)
    nx = np.asarray(next).astype(np.int64).reshape(-1)
    n = len(v64)
    if not (len(r64) == len(nx) == n):
        raise ValueError("v, rew and next must have one length")
    if ((nx >= 0) & ((nx <= np.arange(n)) | (nx >= n))).any() or (nx < NEXT_NONE).any():
        raise ValueError("a successor lies behind its row and inside the range (or is NEXT_TERMINAL / NEXT_NONE)")
    gamma, c = float(gamma), float(gamma) * float(lam)
    leaf = nx == NEXT_NONE
    A = np.zeros(n)
    for r in np.nonzero(~leaf)[0]:
        acc, coef, cur = 0.0, 1.0, int(r)
        while True:
            k = int(nx[cur])
            nv = 0.0 if k < 0 else v64[k]
            delta = (r64[cur] + gamma * nv) - v64[cur]
            acc = acc + coef * delta
            coef = coef * c
            if k < 0 or leaf[k]:
                break
            cur = k
        A[r] = acc
    with np.errstate(over='ignore'):
        adv = A.astype(np.float32)
        ret = np.where(leaf, v64, A + v64).astype(np.float32)
    hat = A
    cnt = int((~leaf).sum())
    if normalize and cnt:
        mean = _house_sum(np.where(leaf, 0.0, A)) / float(cnt)
        d = A - mean
        std = np.sqrt(_house_sum(np.where(leaf, 0.0, d * d)) / float(cnt))
        hat = d / (std + 1e-8)
    with np.errstate(over='ignore', invalid='ignore'):
        w = np.where(leaf, 0.0, float(np.float32(w_scale)) * hat).astype(np.float32)
    return adv, ret, w


def _clamp(a, bound):
    """min(max(a, -bound), +bound), exact in any float format; bound = inf: a itself."""
    b = float(np.float32(bound))
    return np.minimum(np.maximum(a, -b), b)


def ddpg_successors(next, idx):
    """The successor table of a DDPG minibatch as the library makes it on the host: succ[r] = next[idx[r]], for a terminal row the row
    itself (its value is ignored). ValueError for a leaf in idx (next == NEXT_NONE): it has no transition. `next` is the dataset's column."""
    ix = np.asarray(idx, dtype=np.int64)
    nx = np.asarray(next).astype(np.int64)[ix]
    if (nx == NEXT_NONE).any():
        raise ValueError("idx names a leaf row (no transition): position %d" % int(np.nonzero((nx == NEXT_NONE).reshape(-1))[0][0]))
    return np.where(nx >= 0, nx, ix)


def q_fit_reference(q_layers, target_q_layers, target_policy_layers, obs, labels, rew, next, idx, gamma, act_bound=np.inf):
    """Pure-numpy float64 loss and gradient of DDPG's critic step (clothhip_q_fit_grad): over the rows idx [B] of the dataset (obs [n, 3P],
    labels [n, 4] the executed actions, rew [n], next [n] its successor column)
        y_r = rew_r + gamma Q'(s'_r, clamp(mu'(s'_r)))   (0 in the place of Q' behind a terminal row),   L = 1 / (2 B) sum_r (Q(s_r, clamp(a_r)) - y_r)^2
    with Q the Q network over rows [s, a] of 3P + 4 values, Q' and mu' the target copies; y is a constant of the gradient. Every
    stored value is rounded to float32 first, the arithmetic is float64 (y is NOT rounded to float32, as the device does: on exactly
    representable data that is no difference). Returns (loss, [(dW, db), ...] of the Q network, y [B], q [B])."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    succ = ddpg_successors(next, ix)
    terminal = np.asarray(next).astype(np.int64)[ix] == NEXT_TERMINAL
    x = np.asarray(obs, dtype=np.float32).astype(np.float64)
    a = np.asarray(labels, dtype=np.float64).astype(np.float32).astype(np.float64)[ix]
    r = np.asarray(rew, dtype=np.float64).astype(np.float32).astype(np.float64).reshape(-1)[ix]
    B = len(ix)
    mu_n = mlp_forward(*mlp_float64(target_policy_layers), x[succ])[-1]
    qn = mlp_forward(*mlp_float64(target_q_layers), np.concatenate([x[succ], _clamp(mu_n, act_bound)], axis=1))[-1][:, 0]
    y = r + float(gamma) * np.where(terminal, 0.0, qn)
    Ws, bs = mlp_float64(q_layers)
    hs = mlp_forward(Ws, bs, np.concatenate([x[ix], _clamp(a, act_bound)], axis=1))
    d = hs[-1][:, 0] - y
    loss = float((d * d).sum() / (2.0 * B))
    return loss, mlp_backward(Ws, hs, (d / float(B))[:, None]), y, hs[-1][:, 0]


def dpg_reference(policy_layers, q_layers, obs, idx, act_bound=np.inf):
    """Pure-numpy float64 loss and gradient of DDPG's actor step (clothhip_policy_fit_dpg_grad): L = -1 / B sum_r Q(s_r, clamp(mu(s_r))) over
    the policy's weights, the critic fixed. dA = dL/da is the critic's input gradient at its four action columns; the clamp's gate sets
    dz_rk = 0 where (mu_rk >= bound and dA_rk < 0) or (mu_rk <= -bound and dA_rk > 0) and passes dA_rk otherwise. Returns
    (stats = [loss, gated fraction, mean |dA|], [(dW, db), ...] of the policy, dA [B, 4])."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    x = np.asarray(obs, dtype=np.float32).astype(np.float64)[ix]
    B, b = len(ix), float(np.float32(act_bound))
    Wp, bp = mlp_float64(policy_layers)
    hp = mlp_forward(Wp, bp, x)
    mu = hp[-1]
    Wq, bq = mlp_float64(q_layers)
    hq = mlp_forward(Wq, bq, np.concatenate([x, _clamp(mu, act_bound)], axis=1))
    g = np.full((B, 1), -1.0 / B)
    for l in range(len(Wq) - 1, 0, -1):
        g = (g @ Wq[l]) * (hq[l] > 0.0)
    dA = (g @ Wq[0])[:, -4:]
    gated = ((mu >= b) & (dA < 0.0)) | ((mu <= -b) & (dA > 0.0))
    stats = np.array([-hq[-1][:, 0].sum() / B, gated.sum() / (4.0 * B), np.abs(dA).sum() / (4.0 * B)])
    return stats, mlp_backward(Wp, hp, np.where(gated, 0.0, dA)), dA


def concat_reference(obs, act, idx, act_bound=np.inf, expert=False):
    """k_fit_concat restated, bit for bit: float32 [B, 3P + 4] = [obs[idx], min(max(act, -bound), +bound)]; act float32 [B, 4] is one
    action per minibatch row -- the label column at idx (the critic's step), or a network's output on the minibatch. expert: act is
    the EXPERT column at idx, and a row without an expert action (component 0 a NaN by its bits) gets four +0.0 by a select, whatever
    its other components hold."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    x, a = np.asarray(obs, dtype=np.float32), np.asarray(act, dtype=np.float32)
    if a.shape != (len(ix), 4):
        raise ValueError("act must hold one action per minibatch row: shape (%d, 4)" % len(ix))
    with np.errstate(invalid='ignore'):
        c = _clamp(a, act_bound).astype(np.float32)
    if expert:
        c = np.where(expert_mask(a)[:, None], c, np.float32(0.0)).astype(np.float32)
    return np.concatenate([x[ix], c], axis=1)


def expert_mask(a):
    """bool [B]: which rows of an expert column float32 [B, 4] carry an expert action -- the device's test on the bits of component 0:
    (bits & 0x7fffffff) > 0x7f800000 means none."""
    bits = np.ascontiguousarray(np.asarray(a, dtype=np.float32)[:, 0]).view(np.uint32)
    return (bits & np.uint32(0x7fffffff)) <= np.uint32(0x7f800000)


def dpg_bc_dz_reference(dA, y, q, qe, expert, act_bound=np.inf, q_coef=1.0, bc_coef=0.0):
    """k_fit_dpg_bc restated in numpy float32 / float64, bit for bit, reduction order included: dA float32 [B, 4], y float32 [B, 4] the
    policy's output, q float32 [B] the critic on the policy's action, qe float32 [B] the critic on the expert's (None: no Q-filter),
    expert float32 [B, 4] the expert column at the minibatch rows. Returns (dz float32[B, 4], stats float64[6] = -mean q, gated
    fraction, mean |dA|, bc_loss, labelled share, filter-pass share)."""
    g, mu = np.asarray(dA, dtype=np.float32), np.asarray(y, dtype=np.float32)
    q32, ae = np.asarray(q, dtype=np.float32).reshape(-1), np.asarray(expert, dtype=np.float32)
    b, qc, bc = np.float32(act_bound), np.float32(q_coef), np.float32(bc_coef)
    B = len(g)
    m = expert_mask(ae)
    f = m.copy() if qe is None else (m & (np.asarray(qe, dtype=np.float32).reshape(-1) > q32))
    gated = ((mu >= b) & (g < 0.0)) | ((mu <= -b) & (g > 0.0))
    with np.errstate(invalid='ignore', over='ignore'):
        a = (qc * np.where(gated, np.float32(0.0), g).astype(np.float32)).astype(np.float32)
        e = np.where(f[:, None], np.minimum(np.maximum(ae, -b), b), np.float32(0.0)).astype(np.float32)
        d = (mu - e).astype(np.float32)
        bt = ((bc * d).astype(np.float32) / np.float32(2 * B)).astype(np.float32)
        clone = f[:, None] & (bc != 0.0)
        dz = np.where(clone, (a + bt).astype(np.float32), a).astype(np.float32)      # (elsewhere NO addition: the sign of a zero survives)
        dd = mu.astype(np.float64) - e.astype(np.float64)
    sq = np.where(f[:, None], dd * dd, 0.0)
    stats = np.array([-_house_sum(q32.astype(np.float64)) / float(B), _house_sum_rows(gated.astype(np.float64)) / float(4 * B),
                      _house_sum_rows(np.abs(g).astype(np.float64)) / float(4 * B), _house_sum_rows(sq) / float(4 * B),
                      _house_sum(m.astype(np.float64)) / float(B), _house_sum(f.astype(np.float64)) / float(B)])
    return dz, stats


def dpg_bc_reference(policy_layers, q_layers, obs, expert, idx, act_bound=np.inf, q_coef=1.0, bc_coef=0.0, q_filter=True, mask=None):
    """Pure-numpy float64 loss and gradient of the actor's step of DDPG from demonstrations (clothhip_policy_fit_dpg_bc_grad):
        L = q_coef (-1 / B sum_r Q(s_r, clamp(mu(s_r)))) + bc_coef / (4 B) sum_{r: f_r} sum_k (mu_rk - clamp(a_E_rk))^2
    over the policy's weights, the critic fixed; f_r = the row carries an expert action (expert [n, 4], the dataset's column) and,
    q_filter, Q(s_r, clamp(a_E_r)) > Q(s_r, clamp(mu(s_r))), decided from the float64 values (mask [B] bool: f given, held fixed --
    for finite differences). No gradient flows through f or the expert's action; the policy-gradient term's dz is dpg_reference's
    gate. Returns dict(loss, stats [6] = -mean Q, gated fraction, mean |dA|, bc_loss, labelled share, filter-pass share; grads
    [(dW, db), ...] of the policy; dA, dz [B, 4]; q, qe [B] (qe None without the filter); m, f bool [B])."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    x = np.asarray(obs, dtype=np.float32).astype(np.float64)[ix]
    ae32 = np.asarray(expert, dtype=np.float32)[ix]
    B, b = len(ix), float(np.float32(act_bound))
    qc, bc = float(np.float32(q_coef)), float(np.float32(bc_coef))
    m = expert_mask(ae32)
    e = np.where(m[:, None], _clamp(np.where(m[:, None], ae32, np.float32(0.0)).astype(np.float64), act_bound), 0.0)
    Wp, bp = mlp_float64(policy_layers)
    hp = mlp_forward(Wp, bp, x)
    mu = hp[-1]
    Wq, bq = mlp_float64(q_layers)
    hq = mlp_forward(Wq, bq, np.concatenate([x, _clamp(mu, act_bound)], axis=1))
    q = hq[-1][:, 0]
    qe = mlp_forward(Wq, bq, np.concatenate([x, e], axis=1))[-1][:, 0] if q_filter else None
    if mask is not None:
        f = np.asarray(mask, dtype=bool).reshape(-1) & m
    else:
        f = m & (qe > q) if q_filter else m.copy()
    g = np.full((B, 1), -1.0 / B)
    for l in range(len(Wq) - 1, 0, -1):
        g = (g @ Wq[l]) * (hq[l] > 0.0)
    dA = (g @ Wq[0])[:, -4:]
    gated = ((mu >= b) & (dA < 0.0)) | ((mu <= -b) & (dA > 0.0))
    diff = np.where(f[:, None], mu - e, 0.0)
    bc_loss = (diff * diff).sum() / (4.0 * B)
    dz = qc * np.where(gated, 0.0, dA) + bc * diff / (2.0 * B)
    stats = np.array([-q.sum() / B, gated.sum() / (4.0 * B), np.abs(dA).sum() / (4.0 * B), bc_loss, m.sum() / float(B), f.sum() / float(B)])
    return dict(loss=qc * stats[0] + bc * bc_loss, stats=stats, grads=mlp_backward(Wp, hp, dz), dA=dA, dz=dz, q=q, qe=qe, m=m, f=f)


def td_loss_reference(q, qn, rew, next, gamma):
    """k_fit_loss_td restated in numpy from the float32 q [B] (the critic) and qn [B] (the target critic on the successors), bit for
    bit, reduction order included: rew [B] and next [B] are the minibatch rows' reward and successor column. Returns (y float32[B], dz
    float32[B], stats float64[3] = loss, mean q, mean y)."""
    q32, qn32 = np.asarray(q, dtype=np.float32).reshape(-1), np.asarray(qn, dtype=np.float32).reshape(-1)
    r64 = np.asarray(rew, dtype=np.float32).astype(np.float64).reshape(-1)
    B = len(q32)
    nv = np.where(np.asarray(next).reshape(-1) == NEXT_TERMINAL, 0.0, qn32.astype(np.float64))
    with np.errstate(over='ignore'):
        y = (r64 + float(gamma) * nv).astype(np.float32)
        dz = (q32 - y) / np.float32(B)
    dd = q32.astype(np.float64) - y.astype(np.float64)
    stats = np.array([_house_sum(dd * dd) / float(2 * B), _house_sum(q32.astype(np.float64)) / float(B), _house_sum(y.astype(np.float64)) / float(B)])
    return y, dz.astype(np.float32), stats


def _house_sum_rows(x):
    """The device's reduction order over x [B, 4] float64 where a thread owns whole ROWS: thread t of 256 adds its rows t, t + 256, ...
    ascending, a row's four components in ascending order, from +0.0; then the halving tree."""
    x = np.asarray(x, dtype=np.float64)
    k = max((len(x) + 255) // 256, 1)
    tab = np.zeros((k * 256, 4))
    tab[:len(x)] = x
    tab = tab.reshape(k, 256, 4)
    red = np.zeros(256)
    for kk in range(k):
        for c in range(4):
            red = red + tab[kk, :, c]
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return red[0]


def dpg_dz_reference(dA, y, q, act_bound=np.inf):
    """k_fit_dpg_dz restated in numpy, bit for bit, reduction order included: dA float32 [B, 4] the critic's input gradient at the
    action columns, y float32 [B, 4] the policy's output, q float32 [B] the critic's. Returns (dz float32[B, 4], stats float64[3] =
    -mean q, gated fraction, mean |dA|)."""
    g, mu = np.asarray(dA, dtype=np.float32), np.asarray(y, dtype=np.float32)
    b = np.float32(act_bound)
    B = len(g)
    gated = ((mu >= b) & (g < 0.0)) | ((mu <= -b) & (g > 0.0))
    dz = np.where(gated, np.float32(0.0), g).astype(np.float32)
    stats = np.array([-_house_sum(np.asarray(q, dtype=np.float32).astype(np.float64)) / float(B), _house_sum_rows(gated.astype(np.float64)) / float(4 * B),
                      _house_sum_rows(np.abs(g).astype(np.float64)) / float(4 * B)])
    return dz, stats


def polyak_reference(target, theta, tau):
    """k_fit_polyak restated, bit for bit: float32 fl(fl(omt target) + fl(t theta)) with t = (float32)tau, omt = (float32)(1 - tau)."""
    t, omt = np.float32(float(tau)), np.float32(1.0 - float(tau))
    tg, th = np.asarray(target, dtype=np.float32), np.asarray(theta, dtype=np.float32)
    return ((omt * tg).astype(np.float32) + (t * th).astype(np.float32)).astype(np.float32)


_LOG2E, _LN2_HI, _LN2_LO = float.fromhex('0x1.71547652b82fep+0'), float.fromhex('0x1.62e42feep-1'), float.fromhex('0x1.a39ef35793c76p-33')
_EXP_COEF = [1.0 / math.factorial(i) for i in range(14)]      # correctly rounded quotients of exact integers, as the compiler folds them


def exp_fixed_reference(x):
    """The device's exponential restated in float64 numpy, operation by operation (include/clothhip.h: PPO ON THE DEVICE; csrc/
    cloth_exp_fixed.hpp exp_fixed): x clamped to [-40, 40], k = rint(x log2e), r = (x - k ln2_hi) - k ln2_lo with fdlibm's constants,
    Horner over 1 / i! for i = 13 .. 0 with a rounded product and a rounded sum per step, the result scaled by 2^k exactly. Bit for bit
    what the kernel and clothhip_selftest_exp_fixed compute; within 2.2e-16 relative of math.exp, and exactly 1.0 at 0."""
    x = np.minimum(np.maximum(np.asarray(x, dtype=np.float64), -40.0), 40.0)
    k = np.rint(x * _LOG2E)
    r = (x - k * _LN2_HI) - k * _LN2_LO
    p = np.full_like(x, _EXP_COEF[13])
    for i in range(12, -1, -1):
        p = p * r + _EXP_COEF[i]
    return np.ldexp(p, k.astype(np.int64))


def ppo_loss_reference(y, actions, old, adv, sigma, clip, B):
    """k_fit_loss_ppo restated in float64 numpy from a given float32 y, bit for bit, reduction order included (include/clothhip.h: PPO
    ON THE DEVICE): y, actions, old [B, 4] and adv [B] are the minibatch's rows in order (the network's output, the stored labels, old
    means and weights, all float32). Returns (stats float64[3] = loss, clip_fraction, kl; dz float32[B, 4]; ratio float32[B]; active
    bool[B])."""
    f64 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
    mu, a, mo, A = f64(y).reshape(-1, 4), f64(actions).reshape(-1, 4), f64(old).reshape(-1, 4), f64(adv).reshape(-1)
    if not (len(mu) == len(a) == len(mo) == len(A) == int(B)):
        raise ValueError("y, actions, old [B, 4] and adv [B] must hold the B rows of the minibatch")
    inv_s2 = 1.0 / (float(sigma) * float(sigma))
    half, lo, hi, Bd = 0.5 * inv_s2, 1.0 - float(clip), 1.0 + float(clip), float(int(B))
    q, kl = np.zeros(len(A)), np.zeros(len(A))
    for k in range(4):
        d_old, d_new, e = a[:, k] - mo[:, k], a[:, k] - mu[:, k], mu[:, k] - mo[:, k]
        q = q + (d_old * d_old - d_new * d_new)
        kl = kl + e * e
    rho = exp_fixed_reference(q * half)
    s1, s2 = rho * A, np.minimum(np.maximum(rho, lo), hi) * A
    active = s1 <= s2
    with np.errstate(over='ignore'):
        dz = np.where(active[:, None], (((s1[:, None] * (mu - a)) * inv_s2) / Bd).astype(np.float32), np.float32(0.0)).astype(np.float32)
    stats = np.array([-_house_sum(np.where(active, s1, s2)) / Bd, _house_sum(np.where(active, 0.0, 1.0)) / Bd, _house_sum(kl * half) / Bd])
    return stats, dz, rho.astype(np.float32), active


def ppo_reference(layers, obs, actions, old, adv, idx, sigma, clip):
    """Pure-numpy float64 loss and gradient of PPO's clipped surrogate for a Gaussian policy of fixed standard deviation sigma whose
    mean is the network's output, beside fit_reference and with its conventions (obs [n, in], actions [n, 4], old [n, 4] the old
    means, adv [n] the advantages, all rounded to float32 first; idx [B] the minibatch; math.exp):
        rho_r = exp((|a - mu_old|^2 - |a - mu|^2) / (2 sigma^2))   (the exponent clamped to [-40, 40], as the device does),
        L = -1 / B sum_r min(rho_r A_r, clip(rho_r, 1 - eps, 1 + eps) A_r),
    a row is ACTIVE when rho A <= clip(rho) A (the first term is the minimum: its gradient counts; inside the interval both are equal),
    dL/dmu_rk = A rho (mu_rk - a_rk) / (sigma^2 B) on active rows, else 0. Returns (stats, [(dW, db), ...], rho float64[B], active
    bool[B]) with stats = (loss, clip_fraction = share of rows not active, kl = 1 / B sum_r |mu - mu_old|^2 / (2 sigma^2))."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    Ws, bs = mlp_float64(layers)
    f64 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    x, a, mo, A = f64(obs)[ix], f64(actions)[ix], f64(old)[ix], f64(adv).reshape(-1)[ix]
    B = len(ix)
    hs = mlp_forward(Ws, bs, x)
    mu = hs[-1]
    inv_s2 = 1.0 / (float(sigma) * float(sigma))
    q = ((a - mo) ** 2 - (a - mu) ** 2).sum(axis=1)
    rho = np.array([math.exp(min(max(v, -40.0), 40.0)) for v in q * (0.5 * inv_s2)])
    s1, s2 = rho * A, np.clip(rho, 1.0 - float(clip), 1.0 + float(clip)) * A
    active = s1 <= s2
    stats = (float(-np.where(active, s1, s2).sum() / B), float((~active).sum() / float(B)), float((((mu - mo) ** 2).sum(axis=1) * (0.5 * inv_s2)).sum() / B))
    g = np.where(active[:, None], (s1[:, None] * (mu - a)) * inv_s2 / B, 0.0)
    return stats, mlp_backward(Ws, hs, g), rho, active


ENTROPY_C = 5.675754132818691          # 2 (1 + ln 2 pi): the entropy of four unit Gaussians (csrc/cloth_policy_fit.hpp FIT_ENTROPY_C)


def ppo_sigma_loss_reference(y, actions, old, old_ls, adv, ls, clip, ent_coef, B):
    """k_fit_loss_ppo_sigma restated in float64 numpy from a given float32 y, bit for bit, reduction order included (include/clothhip.h:
    PPO WITH A LEARNED SIGMA): y, actions, old, old_ls [B, 4] and adv [B] are the minibatch's rows in order (the network's output, the
    stored labels, old means, old log sigmas and weights), ls [4] the head, all float32. Returns (stats float64[4] = loss,
    clip_fraction, kl, entropy; dz float32[B, 4]; grad_ls float32[4]; ratio float32[B]; active bool[B])."""
    f64 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
    mu, a, mo, lo, A = f64(y).reshape(-1, 4), f64(actions).reshape(-1, 4), f64(old).reshape(-1, 4), f64(old_ls).reshape(-1, 4), f64(adv).reshape(-1)
    lsd = f64(ls).reshape(4)
    if not (len(mu) == len(a) == len(mo) == len(lo) == len(A) == int(B)):
        raise ValueError("y, actions, old, old_ls [B, 4] and adv [B] must hold the B rows of the minibatch")
    lo_c, hi_c, Bd, ent = 1.0 - float(clip), 1.0 + float(clip), float(int(B)), float(ent_coef)
    inv = exp_fixed_reference(-2.0 * lsd)
    q, klq, kld = np.zeros(len(A)), np.zeros(len(A)), np.zeros(len(A))
    t_new = np.zeros_like(mu)
    for k in range(4):
        invo, so2 = exp_fixed_reference(-2.0 * lo[:, k]), exp_fixed_reference(2.0 * lo[:, k])
        d_old, d_new, e = a[:, k] - mo[:, k], a[:, k] - mu[:, k], mu[:, k] - mo[:, k]
        t_old = (d_old * d_old) * invo
        t_new[:, k] = (d_new * d_new) * inv[k]
        q = q + (((t_old - t_new[:, k]) * 0.5) + (lo[:, k] - lsd[k]))
        klq = klq + (((so2 * inv[k]) - 1.0) + ((e * e) * inv[k]))
        kld = kld + (lsd[k] - lo[:, k])
    kl = kld + klq * 0.5
    rho = exp_fixed_reference(q)
    s1, s2 = rho * A, np.minimum(np.maximum(rho, lo_c), hi_c) * A
    active = s1 <= s2
    with np.errstate(over='ignore'):
        dz = np.where(active[:, None], (((s1[:, None] * (mu - a)) * inv[None, :]) / Bd).astype(np.float32), np.float32(0.0)).astype(np.float32)
    hk = np.where(active[:, None], s1[:, None] * (t_new - 1.0), 0.0)
    hs = 0.0
    for k in range(4):
        hs = hs + lsd[k]
    H = hs + ENTROPY_C
    stats = np.array([(-_house_sum(np.where(active, s1, s2)) / Bd) - (ent * H), _house_sum(np.where(active, 0.0, 1.0)) / Bd, _house_sum(kl) / Bd, H])
    with np.errstate(over='ignore'):
        grad_ls = np.array([(-_house_sum(hk[:, k]) / Bd) - ent for k in range(4)]).astype(np.float32)
    return stats, dz, grad_ls, rho.astype(np.float32), active


def ppo_sigma_reference(layers, obs, actions, old, old_ls, adv, idx, ls, clip, ent_coef=0.0):
    """Pure-numpy float64 loss and gradients of PPO's clipped surrogate for a Gaussian policy whose mean is the network's output and
    whose standard deviation is exp(ls), ls [4] a state-independent head, minus ent_coef times the policy's entropy; beside
    ppo_reference and with its conventions (obs [n, in], actions, old, old_ls [n, 4] the old means and old log sigmas, adv [n], all
    rounded to float32 first, as is ls; idx [B] the minibatch; math.exp):
        log rho_r = sum_k [ ((a - mo)^2 exp(-2 lo) - (a - mu)^2 exp(-2 ls)) / 2 + (lo - ls) ]      (clamped to [-40, 40])
        L = -1 / B sum_r min(rho_r A_r, clip(rho_r, 1 - eps, 1 + eps) A_r) - ent_coef H,   H = sum_k ls_k + 2 (1 + ln 2 pi),
    a row ACTIVE when rho A <= clip(rho) A; on active rows dL/dmu_rk = A rho (mu_rk - a_rk) exp(-2 ls_k) / B and the row adds
    -A rho ((a - mu)^2 exp(-2 ls_k) - 1) / B to dL/dls_k, which also gets -ent_coef. kl = 1 / B sum_r KL(old || new) of the two diagonal
    Gaussians. Returns (stats = (loss, clip_fraction, kl, H), [(dW, db), ...], grad_ls float64[4], rho float64[B], active bool[B])."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    Ws, bs = mlp_float64(layers)
    f64 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    x, a, mo, lo, A = f64(obs)[ix], f64(actions)[ix], f64(old)[ix], f64(old_ls)[ix], f64(adv).reshape(-1)[ix]
    lsd = f64(ls).reshape(4)
    B = len(ix)
    hs = mlp_forward(Ws, bs, x)
    mu = hs[-1]
    exp = np.vectorize(math.exp, otypes=[np.float64])      # ONE exponential for the head and the old heads: equal inputs, equal values
    inv, invo = exp(-2.0 * lsd), exp(-2.0 * lo)
    t_new = (a - mu) ** 2 * inv
    q = ((((a - mo) ** 2) * invo - t_new) / 2.0 + (lo - lsd)).sum(axis=1)
    rho = np.array([math.exp(min(max(v, -40.0), 40.0)) for v in q])
    s1, s2 = rho * A, np.clip(rho, 1.0 - float(clip), 1.0 + float(clip)) * A
    active = s1 <= s2
    H = float(lsd.sum() + 2.0 * (1.0 + math.log(2.0 * math.pi)))
    kl = ((lsd - lo) + ((exp(2.0 * lo) + (mu - mo) ** 2) * inv - 1.0) / 2.0).sum(axis=1)
    stats = (float(-np.where(active, s1, s2).sum() / B - float(ent_coef) * H), float((~active).sum() / float(B)), float(kl.sum() / B), H)
    g = np.where(active[:, None], (s1[:, None] * (mu - a)) * inv / B, 0.0)
    grad_ls = -np.where(active[:, None], s1[:, None] * (t_new - 1.0), 0.0).sum(axis=0) / B - float(ent_coef)
    return stats, mlp_backward(Ws, hs, g), grad_ls, rho, active


def adam_reference(theta, m, v, g, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """The device's Adam step restated in numpy float32, operation by operation (include/clothhip.h, clothhip_policy_fit): t is the
    1-based step count. Returns the new (theta, m, v), float32."""
    f = np.float32
    b1, b2, g = f(beta1), f(beta2), np.asarray(g, dtype=f)
    a_t = f(float(f(lr)) * np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t))
    omb1, omb2 = f(1.0 - float(b1)), f(1.0 - float(b2))
    m = (b1 * np.asarray(m, dtype=f)).astype(f) + (omb1 * g).astype(f)
    v = (b2 * np.asarray(v, dtype=f)).astype(f) + (omb2 * (g * g).astype(f)).astype(f)
    q = m / (np.sqrt(v).astype(f) + f(eps)).astype(f)
    return (np.asarray(theta, dtype=f) - (a_t * q.astype(f)).astype(f)).astype(f), m.astype(f), v.astype(f)


def sgd_reference(theta, u, g, lr=1e-3, momentum=0.0):
    """The device's SGD step in numpy float32: u = fl(fl(mu u) + g), theta = fl(theta - fl(lr u)). Returns the new (theta, u)."""
    f = np.float32
    u = ((f(momentum) * np.asarray(u, dtype=f)).astype(f) + np.asarray(g, dtype=f)).astype(f)
    return (np.asarray(theta, dtype=f) - (f(lr) * u).astype(f)).astype(f), u


# ---- the cross-entropy planner (clothhip.h: PLAN ACTIONS ON THE DEVICE; csrc/cloth_plan.hpp) ----------------------------------------------
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)
_EPS_SCALE = np.array([0x33DDB3D7], dtype=np.uint32).view(np.float32)[0]      # (float)(sqrt(3) / 2^24)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (standard constants). ctr: four arrays of uint32 values of one shape, key: two ints. Returns the four output words
    as uint64 arrays below 2^32."""
    c = list(np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _U32 for x in ctr]))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
        p0, p1 = _PHILOX_M0 * c[0], _PHILOX_M1 * c[2]                  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _U32]
    return c


def philox_eps(seed, k, i):
    """population_eps(seed, k, i) of csrc/cloth_philox.hpp as float32, i an integer array: Philox4x32-10 keyed by the two halves of seed
    on the counter (i lo, i hi, k, 0); the four words' top 24 bits summed and centred, times (float)(sqrt(3) / 2^24). Zero mean, unit
    variance, |eps| <= 3.47 -- the variate of the MLP population and of the planner's candidates."""
    i = np.asarray(i, dtype=np.uint64)
    seed = int(seed)
    r = philox4x32_10((i & _U32, i >> np.uint64(32), np.uint64(int(k) & 0xFFFFFFFF), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))
    S = sum(x >> np.uint64(8) for x in r)
    D = S.astype(np.int64) - (2 ** 25 - 2)
    return D.astype(np.int32).astype(np.float32) * _EPS_SCALE


# ---- the exploration noise (clothhip.h: EXPLORATION NOISE ON THE DEVICE; csrc/cloth_philox.hpp normal_fixed) ------------------------------
_NORMAL_TAG = 0x4E000000
_HALF_PI, _SQRT2 = 1.5707963267948966, 1.4142135623730951
_COS_COEF = [(-1.0) ** i / math.factorial(2 * i) for i in range(11)]          # correctly rounded quotients of exact integers (20!, 21!
_SIN_COEF = [(-1.0) ** i / math.factorial(2 * i + 1) for i in range(11)]      # are doubles), as the compiler folds them
_LOG_COEF = [1.0 / (2 * i + 1) for i in range(14)]


def log_fixed_reference(u):
    """log_fixed of csrc/cloth_philox.hpp in float64 numpy, operation by operation, for positive normal u: m 2^k from the bits with m
    brought into [1/sqrt2, sqrt2), s = (m - 1) / (m + 1), 2 s P(s^2) with P Horner over 1 / (2 i + 1) for i = 13 .. 0, plus k ln2_lo,
    then plus k ln2_hi. Within 6.2 * 2^-53 relative of log."""
    u = np.ascontiguousarray(u, dtype=np.float64)            # (a scalar becomes [1])
    bits = u.view(np.uint64)
    k = (bits >> np.uint64(52)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m >= _SQRT2
    m = np.where(big, m * 0.5, m)
    k = np.where(big, k + 1, k)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full_like(z, _LOG_COEF[13])
    for i in range(12, -1, -1):
        p = p * z + _LOG_COEF[i]
    kd = k.astype(np.float64)
    return ((2.0 * s) * p + kd * _LN2_LO) + kd * _LN2_HI


def normal_uniforms(seed, env, slot):
    """The integers of normal_fixed for (seed, env, slot), arrays of one shape: (n1, n2) uint64 [..., 2], pair j = 0, 1 in the last axis --
    the top 52 bits of the first and of the last two words of Philox4x32-10 at counter (slot lo, slot hi, env, 0x4E000000 + j)."""
    seed = int(seed)
    env, slot = np.broadcast_arrays(np.asarray(env, dtype=np.uint64), np.asarray(slot, dtype=np.uint64))
    n1, n2 = [], []
    for j in range(2):
        r = philox4x32_10((slot & _U32, slot >> np.uint64(32), env & _U32, np.uint64(_NORMAL_TAG + j)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        n1.append((r[0] << np.uint64(20)) | (r[1] >> np.uint64(12)))
        n2.append((r[2] << np.uint64(20)) | (r[3] >> np.uint64(12)))
    return np.stack(n1, axis=-1), np.stack(n2, axis=-1)


def normal_fixed_reference(seed, env, slot):
    """normal_fixed of csrc/cloth_philox.hpp in float64 numpy, bit for bit: float64 [..., 4], four independent standard normals of (seed,
    env, slot) by Box-Muller over Philox, every operation one IEEE double rounding (include/clothhip.h: EXPLORATION NOISE ON THE DEVICE
    has it operation by operation). seed in [0, 2^64), env in [0, 2^32), slot in [0, 2^64), env and slot arrays of one shape."""
    n1, n2 = normal_uniforms(seed, env, slot)
    u1 = (n1.astype(np.float64) + 0.5) * 2.0 ** -52
    q = (n2 >> np.uint64(50)).astype(np.int64)
    t = ((n2 & np.uint64(2 ** 50 - 1)).astype(np.float64) + 0.5) * 2.0 ** -50 - 0.5
    x = t * _HALF_PI
    x2 = x * x
    c, s = np.full_like(x, _COS_COEF[10]), np.full_like(x, _SIN_COEF[10])
    for i in range(9, -1, -1):
        c = c * x2 + _COS_COEF[i]
        s = s * x2 + _SIN_COEF[i]
    s = x * s
    qc = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    qs = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    rad = np.sqrt(-2.0 * log_fixed_reference(u1))
    return np.stack([rad * qc, rad * qs], axis=-1).reshape(n1.shape[:-1] + (4,))


def policy_noise_reference(seed, T, E, sigma, slot_base=None):
    """The table clothhip_policy_noise_fill makes, bit for bit: float64 [T, E, 4] with [t, e, k] = sigma[e, k] * z_k(seed, e,
    slot_base[e] + t). sigma is a scalar, [4] or [E, 4] of float64 (for a log-sigma head pass exp_fixed_reference of the float32 head);
    slot_base int[E], None: zeros."""
    T, E = int(T), int(E)
    sg = np.asarray(sigma, dtype=np.float64)
    sg = np.broadcast_to(sg if sg.ndim else sg.reshape(1), (E, 4))
    base = np.zeros(E, dtype=np.uint64) if slot_base is None else np.asarray(slot_base).astype(np.uint64).reshape(E)
    slot = base[None, :] + np.arange(T, dtype=np.uint64)[:, None]
    env = np.broadcast_to(np.arange(E, dtype=np.uint64)[None, :], (T, E))
    return np.ascontiguousarray(sg[None] * normal_fixed_reference(seed, env, slot))


def _plan_clip(v, lo, hi):
    """clip(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v), lo / hi per action component (the last axis)."""
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def plan_sample_reference(mean, std, act_low, act_high, n_candidates, seed=0, iteration=0):
    """k_plan_sample in numpy, bit for bit: mean, std float64 [E, H, 4] -> the action table [H, E K, 4];
    x[h][e K + k][a] = clip(mean + std * (double)eps(seed, iteration, ((e K + k) H + h) 4 + a)), candidate k = 0 = clip(mean).
    iteration is iter0 + it."""
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    E, H, _ = mean.shape
    K = int(n_candidates)
    lo = np.broadcast_to(np.asarray(act_low, dtype=np.float64), (4,))
    hi = np.broadcast_to(np.asarray(act_high, dtype=np.float64), (4,))
    slot = np.arange(E * K, dtype=np.int64)[None, :, None]
    h = np.arange(H, dtype=np.int64)[:, None, None]
    a = np.arange(4, dtype=np.int64)[None, None, :]
    eps = philox_eps(seed, iteration, (slot * H + h) * 4 + a).astype(np.float64)            # [H, E K, 4]
    m = np.repeat(mean.transpose(1, 0, 2), K, axis=1)                                      # [H, E K, 4]: row e K + k is env e's
    sd = np.repeat(std.transpose(1, 0, 2), K, axis=1)
    step = sd * eps
    v = np.where((slot % K) == 0, m, m + step)
    return np.ascontiguousarray(_plan_clip(v, lo, hi))


def plan_score_reference(records, penalty=1.0):
    """The planner's score of every branch from a launch's records [H, n]: the coverage of the last executed slot (ran != 0), minus
    `penalty` when any executed slot has oob or tear; -inf for a column without an executed slot. float64 [n]."""
    ran = records['ran'] != 0
    H, n = ran.shape
    last = np.where(ran.any(axis=0), H - 1 - np.argmax(ran[::-1], axis=0), -1)
    bad = (ran & ((records['oob'] != 0) | (records['tear'] != 0))).any(axis=0)
    cov = records['coverage'][np.maximum(last, 0), np.arange(n)]
    return np.where(last < 0, -np.inf, np.where(bad, cov - float(penalty), cov))


def plan_refit_reference(x, scores, mean, std, n_elite, alpha=1.0, min_std=0.0, done=None):
    """k_plan_refit in numpy, bit for bit: the action table x [H, E K, 4] and scores [E, K] -> (mean, std after the refit, elite
    bool[E, K], top int32[E]). Candidates are ranked by (score descending, k ascending); per (h, a) the elites are summed in
    ascending k: mu = sum / M, var = sum (x - mu)^2 / M, sd = sqrt(var); mean <- alpha mu + beta mean, std <- max(min_std, alpha sd +
    beta std), beta = 1 - alpha. An env with done set keeps its rows, has no elites and top -1."""
    x = np.asarray(x, dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float64)
    E, K = scores.shape
    H, M = x.shape[0], int(n_elite)
    mean = np.array(np.broadcast_to(np.asarray(mean, dtype=np.float64), (E, H, 4)))
    std = np.array(np.broadcast_to(np.asarray(std, dtype=np.float64), (E, H, 4)))
    ms = np.broadcast_to(np.asarray(min_std, dtype=np.float64), (4,))
    alpha = np.float64(alpha)
    beta = np.float64(1.0) - alpha
    Md = np.float64(M)
    elite = np.zeros((E, K), dtype=bool)
    top = np.full(E, -1, dtype=np.int32)
    for e in range(E):
        if done is not None and done[e]:
            continue
        order = np.lexsort((np.arange(K), -scores[e]))                # score descending, then k ascending
        top[e] = order[0]
        elite[e, order[:M]] = True
        ks = np.nonzero(elite[e])[0]                                  # ascending k
        xe = x[:, e * K + ks, :]                                      # [H, M, 4]
        tot = np.zeros((H, 4))
        for j in range(M):
            tot = tot + xe[:, j, :]
        mu = tot / Md
        sq = np.zeros((H, 4))
        for j in range(M):
            d = xe[:, j, :] - mu
            sq = sq + d * d
        sd = np.sqrt(sq / Md)
        mean[e] = alpha * mu + beta * mean[e]
        ns = alpha * sd + beta * std[e]
        std[e] = np.where(ns < ms, ms, ns)
    return mean, std, elite, top


def cem_reference(env, scratch_batch, horizon, n_candidates, n_elite, n_iters, mean, std, min_std=0.0, alpha=1.0, penalty=1.0, seed=0,
                  iter0=0):
    """clothhip_plan_cem's loop on the host, from its parts: plan_sample_reference, scratch_batch.fork_from(env.batch), the host-table
    run_actions launch on scratch_batch (E K cloths), plan_score_reference, plan_refit_reference, and the best-so-far rule. Returns the
    dict ClothBatch.plan_cem returns with want_scores and want_candidates. On one scratch batch both routes run the same kernels on
    the same states, so every table agrees bit for bit."""
    E, K, H, n = env.E, int(n_candidates), int(horizon), int(n_iters)
    mean = np.array(np.broadcast_to(np.asarray(mean, dtype=np.float64), (E, H, 4)))
    std = np.array(np.broadcast_to(np.asarray(std, dtype=np.float64), (E, H, 4)))
    done = np.asarray(env._ep_done, dtype=bool)
    rep = np.repeat(np.arange(E), K)
    ep = env._episode_params()
    lo, hi = env.action_space.low, env.action_space.high
    best_a, best_s = np.full((E, H, 4), np.nan), np.full(E, np.nan)
    scores, cands = np.zeros((n, E, K)), np.zeros((n, H, E * K, 4))
    for it in range(n):
        x = plan_sample_reference(mean, std, lo, hi, K, seed=seed, iteration=iter0 + it)
        scratch_batch.fork_from(env.batch, rep)
        ns = np.ascontiguousarray(env.num_steps[rep], dtype=np.int32)
        dn = np.ascontiguousarray(done[rep], dtype=np.uint8)
        rec = scratch_batch.run_actions(ep, H, ns, dn, actions=x)[0]
        sc = plan_score_reference(rec, penalty).reshape(E, K)
        mean, std, _, top = plan_refit_reference(x, sc, mean, std, n_elite, alpha=alpha, min_std=min_std, done=done)
        for e in np.nonzero(~done)[0]:
            if it == 0 or sc[e, top[e]] > best_s[e]:
                best_s[e] = sc[e, top[e]]
                best_a[e] = x[:, e * K + top[e], :]
        scores[it], cands[it] = sc, x
    return dict(mean=mean, std=std, actions=best_a, score=best_s, scores=scores, candidates=cands)
