"""The cases of the DDPG tests, shared by tests/test_ddpg_host.py, which checks their preconditions on the CPU, and
tests/test_gpu_ddpg.py, which runs them: the exactly representable case with the facts its asserts rest on, and the Gaussian case with
its a-priori rounding bound. Everything here is numpy over the float64 references; nothing touches the library."""
import numpy as np

from test_actor_critic_host import chain_case
from test_gpu_policy_fit import U, _exact_case, _flat, _gamma, _random_layers

NONE, TERMINAL = -2, -1
# B = 8 with two terminal rows (11, 0), six that bootstrap, among them row 8 whose successor is the LEAF, row 10; B = 1; a repeated row
IDX8, IDX1, IDXR = np.array([7, 2, 11, 0, 5, 8, 4, 1]), np.array([3]), np.array([6, 2, 6, 9, 8, 2, 6, 0])
GAMMA, TAU, BOUND = 0.5, 0.5, 1.0
G_GAMMA, G_BOUND = 0.9, 0.25          # the Gaussian cases' discount and action bound

EXACT_CASES = [  # (n_side, policy widths, Q widths, dens, seed): the first seed from 0 for which exact_asserts holds (found on the CPU)
    (10, [300, 5, 4], [304, 5, 1], 1.0, 0),
    (10, [300, 37, 64, 4], [304, 37, 64, 1], 0.3, 0),
    (25, [1875, 37, 64, 4], [1879, 37, 64, 1], 0.3, 1),
]


def clamp(a, bound):
    return np.minimum(np.maximum(a, -bound), bound)


# ---- exactly representable data -------------------------------------------------------------------------------------------------------------
def exact_case(pw, qw, dens, seed):
    """Four networks with weights and biases in {-1, 0, 1} (test_gpu_policy_fit's _exact_case: the policy, its target, the Q network,
    its target -- four different draws), twelve rows in {-2 .. 2} with labels in {-3 .. 3} (the clamp at 1 changes more than half of
    them), rewards in {-2 .. 2}, and the successor column of test_actor_critic_host's chain_case: chains, three terminal rows, one leaf."""
    pol, rows, labels = _exact_case(pw, dens, seed)
    rew = np.random.RandomState(4000 + seed).randint(-2, 3, size=12).astype(np.float32)
    rew[10] = 0.0
    return dict(pol=pol, tpol=_exact_case(pw, dens, 1000 + seed)[0], q=_exact_case(qw, dens, 2000 + seed)[0], tq=_exact_case(qw, dens, 3000 + seed)[0],
                rows=rows, labels=labels, rew=rew, next=chain_case()[1])


def _forward_facts(layers, x):
    """(activations, the largest sum |a||b| over the forward's inner products, the hidden units' activity) in float64."""
    Ws = [W.astype(np.float64) for W, _ in layers]
    hs, worst, active = [x], 0.0, []
    for l in range(len(Ws)):
        b = layers[l][1].astype(np.float64)
        worst = max(worst, float((np.abs(hs[-1]) @ np.abs(Ws[l]).T + np.abs(b)).max()))
        z = hs[-1] @ Ws[l].T + b
        if l + 1 < len(Ws):
            active.append(z > 0)
        hs.append(np.maximum(z, 0.0) if l + 1 < len(Ws) else z)
    return hs, worst, active


def _backward_facts(layers, hs, g, weights=True, to_input=False):
    """(the largest sum |a||b| over the backward's inner products, the non-zero count of every gradient block, the input gradient)."""
    Ws = [W.astype(np.float64) for W, _ in layers]
    worst, filled = 0.0, []
    for l in range(len(Ws) - 1, -1, -1):
        if weights:
            worst = max(worst, float((np.abs(g).T @ np.abs(hs[l])).max()), float(np.abs(g).sum(axis=0).max()))
            filled += [int(np.count_nonzero(g.T @ hs[l])), int(np.count_nonzero(g.sum(axis=0)))]
        if l or to_input:
            worst = max(worst, float((np.abs(g) @ np.abs(Ws[l])).max()))
            g = (g @ Ws[l]) * (hs[l] > 0 if l else 1.0)
    return worst, filled, g


def exact_facts(c, idx, gamma=GAMMA, bound=BOUND):
    """What the exact test's preconditions are asserted from, of the minibatch idx, in float64 where every quantity is exact."""
    ix = np.asarray(idx)
    x, a = c['rows'].astype(np.float64), c['labels'][ix]
    nx = np.asarray(c['next'])[ix]
    succ = np.where(nx >= 0, nx, ix)
    B = len(ix)
    worst, active = 0.0, {}
    hs, w, _ = _forward_facts(c['tpol'], x[succ]); worst = max(worst, w)
    hn, w, _ = _forward_facts(c['tq'], np.concatenate([x[succ], clamp(hs[-1], bound)], axis=1)); worst = max(worst, w)
    y = c['rew'].astype(np.float64)[ix] + gamma * np.where(nx == TERMINAL, 0.0, hn[-1][:, 0])
    hq, w, active['critic'] = _forward_facts(c['q'], np.concatenate([x[ix], clamp(a, bound)], axis=1)); worst = max(worst, w)
    worst = max(worst, float((np.abs(hq[-1][:, 0]) + np.abs(y)).max()))
    w, filled_q, _ = _backward_facts(c['q'], hq, ((hq[-1][:, 0] - y) / B)[:, None]); worst = max(worst, w)
    hp, w, active['policy'] = _forward_facts(c['pol'], x[ix]); worst = max(worst, w)
    ha, w, active['critic_on_mu'] = _forward_facts(c['q'], np.concatenate([x[ix], clamp(hp[-1], bound)], axis=1)); worst = max(worst, w)
    w, _, dX = _backward_facts(c['q'], ha, np.full((B, 1), -1.0 / B), weights=False, to_input=True); worst = max(worst, w)
    dA, mu = dX[:, -4:], hp[-1]
    gated = ((mu >= bound) & (dA < 0)) | ((mu <= -bound) & (dA > 0))
    w, filled_p, _ = _backward_facts(c['pol'], hp, np.where(gated, 0.0, dA)); worst = max(worst, w)
    frac = {k: (float(np.concatenate([m.reshape(-1) for m in v]).mean()) if v else None) for k, v in active.items()}
    return dict(worst=worst, active=frac, filled=filled_q + filled_p, gated=int(gated.sum()), clamped=int((clamp(a, bound) != a).sum()),
                terminal=int((nx == TERMINAL).sum()), boot=int((nx >= 0).sum()), leaf_succ=int(((nx >= 0) & (np.asarray(c['next'])[succ] == NONE)).sum()))


def exact_asserts(pw, qw, dens, seed):
    """The preconditions of the exact test, from the float64 references alone -> the case. With B = 8, gamma = 1/2 and integer data
    every quantity of every pass is a multiple of 1/16; 16 sum |a||b| < 2^24 for every inner product, so every partial sum in ANY order
    is a float32 and the device's values must EQUAL the references'. At B = 8: between a third and two thirds of the hidden units of
    every pass a gradient runs through are active; no gradient block is empty; the minibatch holds at least two terminal and two
    bootstrapping rows and a row whose successor is the leaf; the gate fires on 8 to 24 of its 32 components; the clamp changes at
    least a quarter of the label components; the critic's gradient at gamma = 0 is another one."""
    from gym_cloth_amd.policies import dpg_reference, q_fit_reference
    c = exact_case(pw, qw, dens, seed)
    assert not (np.asarray(c['next'])[np.concatenate([IDX8, IDX1, IDXR])] == NONE).any()
    for idx in (IDX8, IDX1, IDXR):
        f = exact_facts(c, idx)
        assert 16.0 * f['worst'] < 2.0 ** 24, f['worst']
        loss, gq, y, q = q_fit_reference(c['q'], c['tq'], c['tpol'], c['rows'], c['labels'], c['rew'], c['next'], idx, GAMMA, BOUND)
        stats, gp, dA = dpg_reference(c['pol'], c['q'], c['rows'], idx, BOUND)
        for want in (_flat(gq), _flat(gp), dA, y, q):
            assert np.array_equal(want, want.astype(np.float32))              # the references' values are float32 values
        if len(idx) == 8:
            assert all(v is None or 1.0 / 3.0 <= v <= 2.0 / 3.0 for v in f['active'].values()), f['active']
            assert min(f['filled']) > 0, f['filled']
            assert all(np.count_nonzero(g) > 0 for Wb in gq + gp for g in Wb)
            assert f['terminal'] >= 2 and f['boot'] >= 2 and f['leaf_succ'] >= 1, f
            assert 8 <= f['gated'] <= 24 and stats[1] == f['gated'] / 32.0, f['gated']
            assert f['clamped'] >= 8, f['clamped']
            g0 = q_fit_reference(c['q'], c['tq'], c['tpol'], c['rows'], c['labels'], c['rew'], c['next'], idx, 0.0, BOUND)[1]
            assert not np.array_equal(_flat(g0), _flat(gq))
    return c


# ---- Gaussian data and the a-priori bound -----------------------------------------------------------------------------------------------------
def forward_bound(layers, x, dx):
    """test_gpu_policy_fit's forward bound (Higham: a float32 inner product of length n in any order lies within gamma_{n+1} sum |a||b| of
    exact, plus the propagated input error) over rows x whose elements carry the absolute error dx. Returns (hs, dhs, margin per row):
    margin is the smallest |z| - dz over the row's hidden pre-activations (inf without a hidden layer) -- where it is > 0 the ReLU mask
    is exact, an inactive unit's error is 0 and an active one's is dz."""
    hs, dhs, margin = [x], [dx], np.full(len(x), np.inf)
    L = len(layers)
    for l, (W, bb) in enumerate(layers):
        W64, aW, b64 = W.astype(np.float64), np.abs(W.astype(np.float64)), bb.astype(np.float64)
        dz = dhs[-1] @ aW.T + _gamma(W.shape[1] + 1) * ((np.abs(hs[-1]) + dhs[-1]) @ aW.T + np.abs(b64))
        z = hs[-1] @ W64.T + b64
        if l + 1 < L:
            margin = np.minimum(margin, (np.abs(z) - dz).min(axis=1))
        hs.append(np.maximum(z, 0.0) if l + 1 < L else z)
        dhs.append(np.where(z > 0.0, dz, 0.0) if l + 1 < L else dz)
    return hs, dhs, margin


def backward_bound(layers, hs, dhs, g, dg, weights=True, to_input=False):
    """test_gpu_policy_fit's backward bound from the last layer's g = dL/dz with error dg:
        d(dW) = sum_r [dg (|h| + dh) + |g| dh] + gamma_{B+1} sum_r (|g| + dg)(|h| + dh)        (db: h = 1, dh = 0)
        d(dH) = dg |W| + gamma_{n_out+1} (|g| + dg) |W|
    Returns (gradients, their bounds, (the input gradient, its bound) with to_input). The masks are exact (forward_bound's margin)."""
    B, L = len(g), len(layers)
    Ws = [W.astype(np.float64) for W, _ in layers]
    grads, bounds = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        h, dh, ag = hs[l], dhs[l], np.abs(g)
        if weights:
            dW = dg.T @ (np.abs(h) + dh) + ag.T @ dh + _gamma(B + 1) * ((ag + dg).T @ (np.abs(h) + dh))
            db = dg.sum(axis=0) + _gamma(B + 1) * (ag + dg).sum(axis=0)
            grads[l], bounds[l] = (g.T @ h, g.sum(axis=0)), (dW, db)
        if l or to_input:
            aW, mask = np.abs(Ws[l]), (h > 0 if l else np.ones_like(h, dtype=bool))
            dgn = (dg @ aW + _gamma(Ws[l].shape[0] + 1) * ((ag + dg) @ aW)) * mask
            g, dg = (g @ Ws[l]) * mask, dgn
    return grads, bounds, (g, dg)


def critic_bound(c, idx, gamma, bound):
    """The critic's step in float64 with its a-priori error bounds. Beyond the trainer's: the target policy's output error enters the
    target critic's action columns (the clamp is 1-Lipschitz), and the TD target adds its own roundings,
        dy = gamma dqn + u |y| + 4 2^-53 (|rew| + gamma |qn|)        (the target critic's error, the rounding to float32, the double operations)
        dg = ((dq + dy) / B) (1 + 2 u) + 2 u |g|                      (the float32 subtraction and division)
    Returns dict(loss, dloss, grads, bound (flat), y, dy, q, dq, margin): margin the smallest ReLU margin of the three passes."""
    ix = np.asarray(idx)
    x = np.asarray(c['rows'], dtype=np.float32).astype(np.float64)
    a = np.asarray(c['labels'], dtype=np.float64).astype(np.float32).astype(np.float64)[ix]
    r = np.asarray(c['rew'], dtype=np.float32).astype(np.float64)[ix]
    nx = np.asarray(c['next'])[ix]
    succ = np.where(nx >= 0, nx, ix)
    B, zeros = len(ix), np.zeros((len(ix), x.shape[1]))
    ht, dht, m1 = forward_bound(c['tpol'], x[succ], zeros)
    hn, dhn, m2 = forward_bound(c['tq'], np.concatenate([x[succ], clamp(ht[-1], bound)], axis=1), np.concatenate([zeros, dht[-1]], axis=1))
    boot = nx != TERMINAL
    qn, dqn = np.where(boot, hn[-1][:, 0], 0.0), np.where(boot, dhn[-1][:, 0], 0.0)
    y = r + gamma * qn
    dy = gamma * dqn + U * np.abs(y) + 4.0 * 2.0 ** -53 * (np.abs(r) + gamma * np.abs(qn))
    hq, dhq, m3 = forward_bound(c['q'], np.concatenate([x[ix], clamp(a, bound)], axis=1), np.zeros((B, x.shape[1] + 4)))
    q, dq = hq[-1][:, 0], dhq[-1][:, 0]
    d, e = q - y, dq + dy
    loss = float((d * d).sum() / (2.0 * B))
    dloss = float((2.0 * np.abs(d) * e + e * e).sum() / (2.0 * B)) + 1e-14 * loss
    g = (d / float(B))[:, None]
    dg = (e / float(B))[:, None] * (1.0 + 2.0 * U) + 2.0 * U * np.abs(g)
    grads, bounds, _ = backward_bound(c['q'], hq, dhq, g, dg)
    # the margins of the target passes count only where the row bootstraps: a terminal row's target value is not read
    margin = min(float(m3.min()), float(np.where(boot, np.minimum(m1, m2), np.inf).min()))
    return dict(loss=loss, dloss=dloss, grads=grads, bound=_flat(bounds), y=y, dy=dy, q=q, dq=dq, margin=margin)


def actor_bound(c, idx, bound):
    """The actor's step in float64 with its a-priori error bounds: the policy's output error enters the critic's action columns, the
    constant fl(-1 / fl(B)) is within u / B of -1 / B, the input-gradient chain is the trainer's d(dH) down to layer 0, and the gate
    is the reference's wherever it is decided: gate_margin is the smallest of ||mu| - bound| - dmu over all components and of
    |dA| - d(dA) over the components outside the box, which the caller asserts > 0. Returns dict(stats, dstats, grads, bound (flat),
    dA, ddA, margin, gate_margin)."""
    ix = np.asarray(idx)
    x = np.asarray(c['rows'], dtype=np.float32).astype(np.float64)[ix]
    B, zeros = len(ix), np.zeros((len(ix), x.shape[1]))
    hp, dhp, m1 = forward_bound(c['pol'], x, zeros)
    mu, dmu = hp[-1], dhp[-1]
    hq, dhq, m2 = forward_bound(c['q'], np.concatenate([x, clamp(mu, bound)], axis=1), np.concatenate([zeros, dmu], axis=1))
    _, _, (dX, ddX) = backward_bound(c['q'], hq, dhq, np.full((B, 1), -1.0 / B), np.full((B, 1), U / B), weights=False, to_input=True)
    dA, ddA = dX[:, -4:], ddX[:, -4:]
    outside = np.abs(mu) >= bound
    gated = ((mu >= bound) & (dA < 0)) | ((mu <= -bound) & (dA > 0))
    gate_margin = min(float((np.abs(np.abs(mu) - bound) - dmu).min()), float(np.where(outside, np.abs(dA) - ddA, np.inf).min()))
    grads, bounds, _ = backward_bound(c['pol'], hp, dhp, np.where(gated, 0.0, dA), np.where(gated, 0.0, ddA))
    stats = np.array([-hq[-1][:, 0].sum() / B, gated.sum() / (4.0 * B), np.abs(dA).sum() / (4.0 * B)])
    dstats = np.array([dhq[-1][:, 0].sum() / B, 0.0, ddA.sum() / (4.0 * B)]) + 1e-14 * np.abs(stats)
    return dict(stats=stats, dstats=dstats, grads=grads, bound=_flat(bounds), dA=dA, ddA=ddA, margin=min(float(m1.min()), float(m2.min())),
                gate_margin=gate_margin, gated=int(gated.sum()))


def gaussian_case(pw, qw, B, seed, n_rows=48, bound=G_BOUND, zero_action_columns=False):
    """Four Gaussian networks (_random_layers), n_rows rows uniform in [-1, 1) with labels uniform in [-2 bound, 2 bound) (the clamp at
    bound = 1/4 changes half of them, and the policies' outputs, of standard deviation 0.3 or so, lie on both sides of it), Gaussian rewards, and a successor column of chains: row i is followed by row i + 1 with probability
    3/4, else terminal; the last row is a leaf. THE MASK AND GATE PRECONDITIONS BY CONSTRUCTION, as test_gpu_policy_fit's _random_case
    has them: candidates are drawn one after the other from the one seeded stream and a candidate is kept when every pass it can take
    part in -- as a minibatch row or as a successor -- clears its forward bound and its gate is decided (all are properties of that
    row alone: B only scales dA and its bound together). A choice made from the float64 reference and the computed bounds alone; the
    tests assert the preconditions again on their minibatch. zero_action_columns: the Q network's layer-0 action columns are zeros
    (before the rows are chosen; its dA is 0, so the gate's margin is not asked for: such a case is the critic's alone). Returns the case (exact_case's keys) and idx [B] over its non-leaf rows."""
    c = dict(pol=_random_layers(pw, seed), tpol=_random_layers(pw, seed + 1), q=_random_layers(qw, seed + 2), tq=_random_layers(qw, seed + 3))
    if zero_action_columns:                                                   # a Q network that does not read the action: a value network in disguise
        c['q'][0][0][:, -4:] = 0.0
    r = np.random.RandomState(1000 + seed)
    kept_x, kept_a, have, drawn = [], [], 0, 0
    while have < n_rows:
        cand = dict(c, rows=r.uniform(-1, 1, size=(128, pw[0])).astype(np.float32), labels=r.uniform(-2.0 * bound, 2.0 * bound, size=(128, 4)),
                    rew=np.zeros(128, dtype=np.float32), next=np.full(128, TERMINAL))
        drawn += 128
        ok = _row_margins(cand, bound, gate=not zero_action_columns) > 0.0
        kept_x.append(cand['rows'][ok]); kept_a.append(cand['labels'][ok])
        have += int(ok.sum())
        assert drawn <= 64 * 128, "no rows clear the bounds"
    c['rows'], c['labels'] = np.concatenate(kept_x)[:n_rows], np.concatenate(kept_a)[:n_rows]
    c['rew'] = r.normal(size=n_rows).astype(np.float32)
    nxt = np.where(r.random_sample(n_rows) < 0.75, np.arange(n_rows) + 1, TERMINAL)
    nxt[-2], nxt[-1] = n_rows - 1, NONE                                       # the last row is a leaf that the row before it bootstraps from
    c['next'] = nxt
    idx = r.randint(0, n_rows - 1, size=B)
    idx[0] = n_rows - 2
    return c, idx


def _row_margins(c, bound, gate=True):
    """Per row of c: the smallest margin of every pass the row can take part in, as a minibatch row (the critic on its label, the
    policy, the critic on the policy's action, the gate) or as a successor (the target policy, the target critic on its action)."""
    x = np.asarray(c['rows'], dtype=np.float32).astype(np.float64)
    a = np.asarray(c['labels'], dtype=np.float64).astype(np.float32).astype(np.float64)
    n, zeros = len(x), np.zeros_like(x)
    m = np.full(n, np.inf)
    ht, dht, mt = forward_bound(c['tpol'], x, zeros)
    m = np.minimum(m, mt)
    m = np.minimum(m, forward_bound(c['tq'], np.concatenate([x, clamp(ht[-1], bound)], axis=1), np.concatenate([zeros, dht[-1]], axis=1))[2])
    m = np.minimum(m, forward_bound(c['q'], np.concatenate([x, clamp(a, bound)], axis=1), np.zeros((n, x.shape[1] + 4)))[2])
    hp, dhp, mp = forward_bound(c['pol'], x, zeros)
    mu, dmu = hp[-1], dhp[-1]
    hq, dhq, mq = forward_bound(c['q'], np.concatenate([x, clamp(mu, bound)], axis=1), np.concatenate([zeros, dmu], axis=1))
    m = np.minimum(m, np.minimum(mp, mq))
    if not gate:                                                              # (a critic that ignores the action has dA = 0: no gate to decide, and no actor's test)
        return m
    _, _, (dX, ddX) = backward_bound(c['q'], hq, dhq, np.full((n, 1), -1.0), np.full((n, 1), U), weights=False, to_input=True)
    dA, ddA = dX[:, -4:], ddX[:, -4:]
    m = np.minimum(m, (np.abs(np.abs(mu) - bound) - dmu).min(axis=1))
    return np.minimum(m, np.where(np.abs(mu) >= bound, np.abs(dA) - ddA, np.inf).min(axis=1))
