"""The cases of the tests of DDPG from demonstrations, shared by tests/test_ddpg_bc_host.py, which checks their
preconditions on the CPU, and tests/test_gpu_ddpg_bc.py, which runs them: ddpg_cases' cases with an EXPERT column beside them, the exact
case with the facts its asserts rest on, and the Gaussian case with the a-priori bound of the behaviour-cloning term. Everything here is
numpy over the float64 references; nothing touches the library."""
import numpy as np

import ddpg_cases as D
from ddpg_cases import U, _flat, clamp

NO_EXPERT = np.array([0x7fc00000] * 4, dtype=np.uint32).view(np.float32)      # the expert column's fill: four quiet NaNs
BC, QCS = 0.5, (1.0, 2.0)                   # the exact test's bc_coef and its two q_coef
G_QC, G_BC = 0.75, 1.5                      # the Gaussian test's coefficients: neither product is exact


def expert_mask(a):
    bits = np.ascontiguousarray(np.asarray(a, dtype=np.float32)[:, 0]).view(np.uint32)
    return (bits & np.uint32(0x7fffffff)) <= np.uint32(0x7f800000)


# ---- exactly representable data -------------------------------------------------------------------------------------------------------------
# (n_side, policy widths, Q widths, dens, seed) of ddpg_cases.EXACT_CASES with eseed: the first expert seed from 0 for which
# exact_bc_asserts holds (found on the CPU; test_ddpg_bc_host.py asserts it is the first)
EXACT_BC_CASES = [
    (10, [300, 5, 4], [304, 5, 1], 1.0, 0, 2),
    (10, [300, 37, 64, 4], [304, 37, 64, 1], 0.3, 0, 1),
    (25, [1875, 37, 64, 4], [1879, 37, 64, 1], 0.3, 1, 1),
]
TIE_ROW = 7                                 # IDX8[0] and IDX8's only 7: the row whose expert action is made an exact tie


def exact_bc_case(pw, qw, dens, seed, eseed):
    """ddpg_cases.exact_case with an expert column: expert actions in {-3 .. 3} (the clamp at 1 changes more than half of them) from
    RandomState(6000 + eseed); rows 1 and 9 carry none; row TIE_ROW's expert action is set to clamp(mu(s)) of that very row, the
    policy's own clamped action in float64 (integers here): the critic then rates both EXACTLY alike, a tie BY CONSTRUCTION, while the
    policy's unclamped output differs from it wherever it lies outside the box."""
    c = D.exact_case(pw, qw, dens, seed)
    r = np.random.RandomState(6000 + eseed)
    ex = r.randint(-3, 4, size=(12, 4)).astype(np.float32)
    mu = D._forward_facts(c['pol'], c['rows'].astype(np.float64))[0][-1]
    ex[TIE_ROW] = clamp(mu[TIE_ROW], D.BOUND).astype(np.float32)
    ex[1] = NO_EXPERT
    ex[9] = NO_EXPERT
    c['expert'] = ex
    return c


def exact_bc_facts(c, idx, qc, bc=BC, bound=D.BOUND):
    """The largest sum |a||b| over the inner products that the BC step adds to ddpg_cases.exact_facts' (the critic's forward on the
    expert's action; the policy's backward from the new dz), the non-zero count of every gradient block, and the reference's result."""
    from gym_cloth_amd.references import dpg_bc_reference
    ref = dpg_bc_reference(c['pol'], c['q'], c['rows'], c['expert'], idx, bound, qc, bc, True)
    ix = np.asarray(idx)
    x = c['rows'].astype(np.float64)[ix]
    m = expert_mask(c['expert'][ix])
    e = np.where(m[:, None], clamp(np.where(m[:, None], c['expert'][ix], 0.0).astype(np.float64), bound), 0.0)
    _, w1, _ = D._forward_facts(c['q'], np.concatenate([x, e], axis=1))
    hp, w2, _ = D._forward_facts(c['pol'], x)
    w3, filled, _ = D._backward_facts(c['pol'], hp, ref['dz'])
    return dict(worst=max(w1, w2, w3, float(np.abs(ref['dz']).max())), filled=filled, ref=ref)


def exact_bc_asserts(pw, qw, dens, seed, eseed):
    """The preconditions of the exact test, from the float64 reference alone -> the case. With B = 8, bc_coef = 1/2 and integer data dz
    is a multiple of 1/32 (q_coef g of 1/8, bc d / (2 B) of 1/32), at B = 1 of 1/4; 32 sum |a||b| < 2^24 for every inner product, so
    every partial sum in ANY order is a float32 and the device's values must EQUAL the reference's. At IDX8, under the filter: at least
    two labelled rows pass it, at least two fail it with qe < q, row TIE_ROW is labelled and ties (qe == q) -- and its cloning term
    would not be zero --, one row is unlabelled; the gradient with the filter differs from the one without, and from plain DPG's."""
    from gym_cloth_amd.references import dpg_bc_reference, dpg_reference
    c = exact_bc_case(pw, qw, dens, seed, eseed)
    D.exact_asserts(pw, qw, dens, seed)                                       # (ddpg_cases' own preconditions, of the same networks and rows)
    assert D.IDX8[0] == TIE_ROW and list(D.IDX8).count(TIE_ROW) == 1 and 1 in D.IDX8 and 9 in D.IDXR
    for idx in (D.IDX8, D.IDX1, D.IDXR):
        for qc in QCS:
            f = exact_bc_facts(c, idx, qc)
            ref = f['ref']
            assert 32.0 * f['worst'] < 2.0 ** 24, f['worst']
            for want in (_flat(ref['grads']), ref['dz'], ref['dA'], ref['q'], ref['qe'], ref['stats']):
                assert np.array_equal(want, want.astype(np.float32))              # the reference's values are float32 values
            if len(idx) == 8 and idx is D.IDX8:
                m, fl, q, qe = ref['m'], ref['f'], ref['q'], ref['qe']
                assert m.sum() == 7 and not m[list(D.IDX8).index(1)]
                assert fl.sum() >= 2 and (m & (qe < q)).sum() >= 2, (fl.sum(), (m & (qe < q)).sum())
                assert m[0] and qe[0] == q[0] and not fl[0]                           # the tie does not pass
                mu = D._forward_facts(c['pol'], c['rows'].astype(np.float64)[idx])[0][-1]
                assert (mu[0] != clamp(mu[0], D.BOUND)).any()                         # ... though cloning it would move the policy
                assert min(f['filled']) > 0, f['filled']
                off = dpg_bc_reference(c['pol'], c['q'], c['rows'], c['expert'], idx, D.BOUND, qc, BC, False)
                assert off['f'].sum() == 7 and not np.array_equal(_flat(off['grads']), _flat(ref['grads']))
                plain = dpg_reference(c['pol'], c['q'], c['rows'], idx, D.BOUND)
                assert not np.array_equal(qc * _flat(plain[1]), _flat(ref['grads'])) and np.array_equal(plain[0], ref['stats'][:3])
    return c


# ---- Gaussian data and the a-priori bound -----------------------------------------------------------------------------------------------------
# B -> seed: the first seed from 0 for which gaussian_bc_ok holds (found on the CPU from the float64 reference and the computed bounds
# alone; test_ddpg_bc_host.py asserts it is the first). The weight scale is ddpg_cases' own; with_checked_expert says how the expert
# actions are drawn and why.
GAUSSIAN_BC_SEEDS = {8: 1, 257: 0}
PW, QW = [300, 37, 64, 4], [304, 37, 64, 1]


def with_expert(c, seed, bound=D.G_BOUND, unlabelled=0.25):
    """c with an expert column: actions uniform in [-2 bound, 2 bound) (the clamp changes half of the components) from
    RandomState(5000 + seed), a quarter of the rows without one."""
    r = np.random.RandomState(5000 + seed)
    n = len(c['rows'])
    ex = r.uniform(-2.0 * bound, 2.0 * bound, size=(n, 4)).astype(np.float32)
    ex[r.random_sample(n) < unlabelled] = NO_EXPERT
    return dict(c, expert=ex)


def _expert_row_margins(c, ex, bound):
    """Per row of c with the candidate expert column ex: min(the ReLU margin of the critic's pass on [s, clamp(a_E)] -- (0, 0, 0, 0)
    for a row without one --, |qe - q| - (dqe + dq)), q the critic on the policy's action with actor_bound's bound. A property of the
    row alone: no quantity depends on the minibatch."""
    x = np.asarray(c['rows'], dtype=np.float32).astype(np.float64)
    n, zeros = len(x), np.zeros_like(x)
    hp, dhp, _ = D.forward_bound(c['pol'], x, zeros)
    hq, dhq, _ = D.forward_bound(c['q'], np.concatenate([x, clamp(hp[-1], bound)], axis=1), np.concatenate([zeros, dhp[-1]], axis=1))
    m = expert_mask(ex)
    e = np.where(m[:, None], clamp(np.where(m[:, None], ex, np.float32(0.0)).astype(np.float64), bound), 0.0)
    he, dhe, me = D.forward_bound(c['q'], np.concatenate([x, e], axis=1), np.zeros((n, x.shape[1] + 4)))
    return np.minimum(me, np.abs(he[-1][:, 0] - hq[-1][:, 0]) - (dhe[-1][:, 0] + dhq[-1][:, 0]))


def with_checked_expert(c, seed, bound=D.G_BOUND, unlabelled=0.25):
    """with_expert, THE FILTER'S PRECONDITION BY CONSTRUCTION, as ddpg_cases.gaussian_case has the masks' and the gate's: a free draw
    leaves about one row in five with |qe - q| inside the two forward bounds or a hidden unit of the expert pass inside its own, so no
    seed among the first 64 clears all 257 rows of the larger minibatch -- and shrinking the weight scale would not help, since qe - q,
    the pre-activations and their bounds all scale alike. Instead candidates are drawn one after the other from the one seeded stream,
    RandomState(5000 + seed), a whole column at a time, and a row keeps the FIRST candidate (an action, or none) that clears
    _expert_row_margins -- a choice made from the float64 reference and the computed bounds alone, and a property of that row alone.
    The tests assert the preconditions again on their minibatch, over every row."""
    r = np.random.RandomState(5000 + seed)
    n = len(c['rows'])
    ex, done = np.tile(NO_EXPERT, (n, 1)), np.zeros(n, dtype=bool)
    for _ in range(64):
        cand = r.uniform(-2.0 * bound, 2.0 * bound, size=(n, 4)).astype(np.float32)
        cand[r.random_sample(n) < unlabelled] = NO_EXPERT
        ok = ~done & (_expert_row_margins(c, cand, bound) > 0.0)
        ex[ok], done = cand[ok], done | ok
        if done.all():
            return dict(c, expert=ex)
    raise AssertionError("no expert action clears the bounds for rows %r" % (np.nonzero(~done)[0][:8],))


def gaussian_bc_case(B, seed):
    c, idx = D.gaussian_case(PW, QW, B, seed=seed, n_rows=48 if B <= 48 else 300)
    return with_checked_expert(c, seed), idx


def actor_bc_bound(c, idx, bound, qc, bc, q_filter=True):
    """ddpg_cases.actor_bound extended by the behaviour-cloning term. The extension, with u = 2^-24, g the gated dA with its bound dg
    (0 where gated) and mu the policy's output with its bound dmu; the clamped expert action e is exact (min and max of float32 values):
        a = fl(qc g):                   da  = qc dg (1 + u) + u |qc g|
        d = fl(mu - e):                 dd  = dmu (1 + u) + u |mu - e|
        bd = fl(bc d):                  dbd = bc dd (1 + u) + u bc |mu - e|
        b = fl(bd / fl(2 B)):           db  = dbd / (2 B) (1 + u) + u |b|           (2 B <= 8192 is a float32)
        dz = fl(a + b):                 ddz = (da + db) (1 + u) + u |a + b|          on the rows with f_r, else ddz = da
    The BC loss, a double sum of squares of the float32 mu: |(mu + t - e)^2 - (mu - e)^2| <= 2 |mu - e| dmu + dmu^2 per element, plus
    1e-14 relative for the double arithmetic. The labelled share and the filter-pass share are exact WHEN THE FILTER IS DECIDED: the
    critic's value on the expert's action has the forward bound dqe of exact inputs, its value on the policy's action the bound dq of
    actor_bound, and filter_margin = min over EVERY row of |qe - q| - (dqe + dq) (for a row without an expert action qe is the value
    on the action (0, 0, 0, 0), as the device computes it), which the caller asserts > 0 beside the ReLU margins (the expert pass's
    among them) and the gate's. Returns actor_bound's dict with stats / dstats of six, dz, ddz, f, m, q, dq, qe, dqe, filter_margin."""
    from gym_cloth_amd.references import dpg_bc_reference
    ab = D.actor_bound(c, idx, bound)
    ix = np.asarray(idx)
    x = np.asarray(c['rows'], dtype=np.float32).astype(np.float64)[ix]
    B, zeros = len(ix), np.zeros((len(ix), x.shape[1]))
    hp, dhp, m1 = D.forward_bound(c['pol'], x, zeros)
    mu, dmu = hp[-1], dhp[-1]
    hq, dhq, _ = D.forward_bound(c['q'], np.concatenate([x, clamp(mu, bound)], axis=1), np.concatenate([zeros, dmu], axis=1))
    q, dq = hq[-1][:, 0], dhq[-1][:, 0]
    m = expert_mask(c['expert'][ix])
    e = np.where(m[:, None], clamp(np.where(m[:, None], c['expert'][ix], np.float32(0.0)).astype(np.float64), bound), 0.0)
    he, dhe, m3 = D.forward_bound(c['q'], np.concatenate([x, e], axis=1), np.zeros((B, x.shape[1] + 4)))
    qe, dqe = he[-1][:, 0], dhe[-1][:, 0]
    filter_margin = float((np.abs(qe - q) - (dqe + dq)).min()) if q_filter else np.inf
    f = m & (qe > q) if q_filter else m.copy()
    gated = ((mu >= bound) & (ab['dA'] < 0)) | ((mu <= -bound) & (ab['dA'] > 0))
    g, dg = np.where(gated, 0.0, ab['dA']), np.where(gated, 0.0, ab['ddA'])
    a, da = qc * g, qc * dg * (1.0 + U) + U * np.abs(qc * g)
    d = np.where(f[:, None], mu - e, 0.0)
    dd = dmu * (1.0 + U) + U * np.abs(d)
    dbd = bc * dd * (1.0 + U) + U * bc * np.abs(d)
    b = bc * d / (2.0 * B)
    db = dbd / (2.0 * B) * (1.0 + U) + U * np.abs(b)
    clone = f[:, None] & (bc != 0.0)
    dz = np.where(clone, a + b, a)
    ddz = np.where(clone, (da + db) * (1.0 + U) + U * np.abs(a + b), da)
    grads, bounds, _ = D.backward_bound(c['pol'], hp, dhp, dz, ddz)
    bc_loss = (d * d).sum() / (4.0 * B)
    dbc = np.where(f[:, None], 2.0 * np.abs(d) * dmu + dmu * dmu, 0.0).sum() / (4.0 * B) + 1e-14 * bc_loss
    stats = np.concatenate([ab['stats'], [bc_loss, m.sum() / float(B), f.sum() / float(B)]])
    dstats = np.concatenate([ab['dstats'], [dbc, 0.0, 0.0]])
    ref = dpg_bc_reference(c['pol'], c['q'], c['rows'], c['expert'], idx, bound, qc, bc, q_filter)
    assert np.allclose(_flat(grads), _flat(ref['grads']), rtol=0, atol=1e-13) and np.allclose(stats, ref['stats'], rtol=0, atol=1e-13) and np.array_equal(f, ref['f'])
    return dict(ab, stats=stats, dstats=dstats, grads=grads, bound=_flat(bounds), dz=dz, ddz=ddz, f=f, m=m, q=q, dq=dq, qe=qe, dqe=dqe,
                margin=min(ab['margin'], float(m3.min())), filter_margin=filter_margin)


def gaussian_bc_ok(B, seed):
    """Whether the Gaussian case of this seed may be compared: every ReLU margin, the gate's margin and the filter's margin over EVERY
    row of the minibatch are > 0, and the minibatch has labelled rows that pass the filter, labelled rows that fail it and rows without
    an expert action. From the reference and the bounds alone -> (ok, the case, idx, the bound's dict)."""
    c, idx = gaussian_bc_case(B, seed)
    ab = actor_bc_bound(c, idx, D.G_BOUND, G_QC, G_BC)
    ok = ab['margin'] > 0.0 and ab['gate_margin'] > 0.0 and ab['filter_margin'] > 0.0
    ok = ok and ab['f'].sum() >= 1 and (ab['m'] & ~ab['f']).sum() >= 1 and (~ab['m']).sum() >= 1
    return bool(ok), c, idx, ab
