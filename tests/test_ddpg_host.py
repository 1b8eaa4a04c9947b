"""Host tests of DDPG on the device, no GPU: the float64 references against central finite differences of their own
loss; the bit-for-bit restatements of the four kernels against the float64 references on exactly representable data; the successor
table and the leaf refusal; the preconditions of the GPU file's exact test, found here on the CPU; the header, the exports and the
bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddpg_cases as D
from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.policies import (concat_reference, dpg_dz_reference, dpg_reference, polyak_reference, q_fit_reference, td_loss_reference)
from gym_cloth_amd.references import _house_sum, ddpg_successors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_net(widths, seed):
    r = np.random.RandomState(seed)
    return [(r.normal(size=(widths[l + 1], widths[l])).astype(np.float32) / np.float32(np.sqrt(widths[l])), (0.3 * r.normal(size=widths[l + 1])).astype(np.float32))
            for l in range(len(widths) - 1)]


def _tiny_case(seed=0, P=2):
    """A 3P = 6 wide observation: policy [6, 5, 4], Q [10, 7, 1], their targets, nine rows with chains, terminals and a leaf."""
    r = np.random.RandomState(seed)
    c = dict(pol=_small_net([3 * P, 5, 4], seed), tpol=_small_net([3 * P, 5, 4], seed + 1), q=_small_net([3 * P + 4, 7, 1], seed + 2), tq=_small_net([3 * P + 4, 7, 1], seed + 3))
    c['rows'] = r.uniform(-1, 1, size=(9, 3 * P)).astype(np.float32)
    c['labels'] = r.uniform(-1.5, 1.5, size=(9, 4))
    c['rew'] = r.normal(size=9).astype(np.float32)
    c['next'] = np.array([1, 2, D.TERMINAL, 4, 8, D.TERMINAL, 7, D.TERMINAL, D.NONE])
    return c, np.array([0, 3, 4, 2, 6, 4, 7])


# ---- the float64 references against finite differences of their own loss ------------------------------------------------------------------
H = 2.0 ** -10      # the step, exactly representable: a float32 weight of magnitude < 4 plus or minus H is a float32


def _fd_check(loss_of, layers, grads):
    """Central differences of loss_of(layers) in every 7th weight against grads. THE TOLERANCE, from the step: inside one linear region
    of the ReLUs and the clamp either loss is a polynomial of degree <= 2 L = 4 in one weight with coefficients of order 1 (inputs,
    weights and targets of order 1, B rows averaged), so the central difference errs by h^2 / 6 |L'''| <= h^2 = 9.6e-7 times a
    constant of order 1, and by rounding eps |L| / h = 1e-13; 1e-5 max(1, |g|) covers the constant ten times over. A step that
    crosses a kink of a ReLU or of the clamp errs by O(h) = 1e-3 instead, a hundred times the tolerance: such an element fails,
    so the cases are chosen (seeded, on the CPU) so that none of the probed steps crosses one."""
    probed = 0
    for l in range(len(layers)):
        for part in (0, 1):
            flat = layers[l][part].reshape(-1)
            for i in range(0, flat.size, 7):
                keep = flat[i]
                flat[i] = keep + np.float32(H); up = loss_of(layers)
                flat[i] = keep - np.float32(H); dn = loss_of(layers)
                flat[i] = keep
                g = grads[l][part].reshape(-1)[i]
                assert abs((up - dn) / (2.0 * H) - g) <= 1e-5 * max(1.0, abs(g)), (l, part, i, (up - dn) / (2.0 * H), g)
                probed += 1
    return probed


def test_q_reference_against_finite_differences():
    c, idx = _tiny_case(0)
    args = (c['rows'], c['labels'], c['rew'], c['next'], idx, 0.9, 1.0)
    loss, grads, y, q = q_fit_reference(c['q'], c['tq'], c['tpol'], *args)
    assert loss > 0 and y.shape == q.shape == (7,)
    assert y[3] == np.float64(c['rew'][2]) and y[0] != np.float64(c['rew'][0])           # a terminal row's target is its reward; a bootstrapping row's is not
    q_layers = [(W.copy(), b.copy()) for W, b in c['q']]
    assert _fd_check(lambda layers: q_fit_reference(layers, c['tq'], c['tpol'], *args)[0], q_layers, grads) >= 10
    # the target is a constant of the gradient: moving the target networks moves y, and the loss, but the critic's own derivative is the above
    other = q_fit_reference(c['q'], c['q'], c['pol'], *args)
    assert not np.array_equal(other[2], y)
    # gamma = 0: the targets are the rewards, whatever the target networks are
    zero = q_fit_reference(c['q'], c['tq'], c['tpol'], c['rows'], c['labels'], c['rew'], c['next'], idx, 0.0, 1.0)
    assert np.array_equal(zero[2], c['rew'][idx].astype(np.float64))
    with pytest.raises(ValueError):
        q_fit_reference(c['q'], c['tq'], c['tpol'], c['rows'], c['labels'], c['rew'], c['next'], np.array([0, 8]), 0.9, 1.0)


@pytest.mark.parametrize("bound", [np.inf, 100.0])
def test_dpg_reference_against_finite_differences(bound):
    """Without a clamp in reach the gate never fires and the gradient is the derivative of -mean Q(s, mu(s)) in the policy's weights."""
    c, idx = _tiny_case(0)
    stats, grads, dA = dpg_reference(c['pol'], c['q'], c['rows'], idx, bound)
    assert stats[1] == 0.0 and stats[2] > 0 and dA.shape == (7, 4)
    pol = [(W.copy(), b.copy()) for W, b in c['pol']]
    assert _fd_check(lambda layers: dpg_reference(layers, c['q'], c['rows'], idx, bound)[0][0], pol, grads) >= 10
    # dA is the derivative in the action itself: move the policy's output bias, which shifts every row's action by the same amount
    db = grads[-1][1]
    assert np.allclose(db, dA.sum(axis=0), rtol=0, atol=1e-15)


def test_the_gate_holds_outward_moves_and_passes_inward_ones():
    """A policy whose output is its bias: components at +2, -2, +0.5, -2 under bound 1. Under a critic that is linear in the action
    with coefficients (+1, +1, +1, -1), L = -Q has dA = -(+1, +1, +1, -1) / B: the step would raise a_0 (outside, further out: held),
    raise a_1 (outside below, inward: passes), raise a_2 (inside: passes), lower a_3 (outside below, further out: held)."""
    P = 2
    pol = [(np.zeros((4, 3 * P), dtype=np.float32), np.array([2.0, -2.0, 0.5, -2.0], dtype=np.float32))]
    W = np.zeros((1, 3 * P + 4), dtype=np.float32)
    W[0, -4:] = [1.0, 1.0, 1.0, -1.0]
    rows = np.random.RandomState(0).uniform(-1, 1, size=(5, 3 * P)).astype(np.float32)
    stats, grads, dA = dpg_reference(pol, [(W, np.zeros(1, dtype=np.float32))], rows, np.arange(4), 1.0)
    assert np.array_equal(dA, np.tile([-0.25, -0.25, -0.25, 0.25], (4, 1)))
    assert np.array_equal(grads[0][1], [0.0, -1.0, -1.0, 0.0]) and stats[1] == 0.5 and stats[2] == 0.25
    assert stats[0] == -(1.0 - 1.0 + 0.5 + 1.0)                                      # Q saw the CLAMPED action (1, -1, 0.5, -1)
    dz, st = dpg_dz_reference(dA.astype(np.float32), np.tile(pol[0][1], (4, 1)), np.full(4, 1.5, dtype=np.float32), 1.0)
    assert np.array_equal(dz, np.tile(np.array([0.0, -0.25, -0.25, 0.0], dtype=np.float32), (4, 1))) and np.array_equal(st, [-1.5, 0.5, 0.25])
    assert dpg_dz_reference(dA.astype(np.float32), np.tile(pol[0][1], (4, 1)), np.zeros(4, dtype=np.float32), np.inf)[1][1] == 0.0


# ---- the restatements against the float64 references on exact data; the preconditions of the GPU file's exact test --------------------------
@pytest.mark.parametrize("n_side,pw,qw,dens,seed", D.EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_exact_preconditions_and_restatements(n_side, pw, qw, dens, seed):
    """exact_asserts holds at the listed seed and at no smaller one; on that data, where float32 arithmetic is exact, the bit-for-bit
    restatements fed the float64 references' own values give the float64 references' results."""
    from gym_cloth_amd.mlp import mlp_float64, mlp_forward
    assert pw[0] == 3 * n_side * n_side and qw[0] == pw[0] + 4
    for earlier in range(seed):
        with pytest.raises(AssertionError):
            D.exact_asserts(pw, qw, dens, earlier)
    c = D.exact_asserts(pw, qw, dens, seed)
    for idx in (D.IDX8, D.IDX1, D.IDXR):
        B = len(idx)
        loss, gq, y, q = q_fit_reference(c['q'], c['tq'], c['tpol'], c['rows'], c['labels'], c['rew'], c['next'], idx, D.GAMMA, D.BOUND)
        succ = ddpg_successors(c['next'], idx)
        x = c['rows'].astype(np.float64)
        X = concat_reference(c['rows'], c['labels'][idx], idx, D.BOUND)
        assert X.dtype == np.float32 and X.shape == (B, pw[0] + 4) and np.array_equal(X[:, :-4], c['rows'][idx]) and np.abs(X[:, -4:]).max() == 1.0
        assert np.array_equal(mlp_forward(*mlp_float64(c['q']), X.astype(np.float64))[-1][:, 0], q)
        mu_n = mlp_forward(*mlp_float64(c['tpol']), x[succ])[-1]
        qn = mlp_forward(*mlp_float64(c['tq']), concat_reference(c['rows'], mu_n, succ, D.BOUND).astype(np.float64))[-1][:, 0]
        y32, dz, stats = td_loss_reference(q, qn, c['rew'][idx], np.asarray(c['next'])[idx], D.GAMMA)
        assert np.array_equal(y32.astype(np.float64), y) and np.array_equal(dz.astype(np.float64), (q - y) / B)
        assert stats[0] == loss and stats[1] == q.sum() / B and stats[2] == y.sum() / B
        assert np.array_equal(gq[-1][1], [dz.astype(np.float64).sum()])
        st, gp, dA = dpg_reference(c['pol'], c['q'], c['rows'], idx, D.BOUND)
        mu = mlp_forward(*mlp_float64(c['pol']), x[idx])[-1]
        qa = mlp_forward(*mlp_float64(c['q']), concat_reference(c['rows'], mu, idx, D.BOUND).astype(np.float64))[-1][:, 0]
        dz4, st32 = dpg_dz_reference(dA, mu, qa, D.BOUND)
        assert np.array_equal(st32, st) and np.array_equal(gp[-1][1], dz4.astype(np.float64).sum(axis=0))
    for a, b in ((c['tpol'], c['pol']), (c['tq'], c['q'])):
        tg, th = D._flat(a), D._flat(b)
        assert np.array_equal(polyak_reference(tg, th, D.TAU).astype(np.float64), 0.5 * tg.astype(np.float64) + 0.5 * th.astype(np.float64))


def test_restatements_round_as_the_kernels_do():
    """Where float32 arithmetic is NOT exact the restatements round per operation: y once from double, dz twice in float32, the
    polyak update three times; the reductions are the house order, another sum than numpy's pairwise one."""
    r = np.random.RandomState(5)
    B = 300
    q, qn, rew = (r.normal(size=B).astype(np.float32) for _ in range(3))
    nxt = np.where(r.random_sample(B) < 0.3, D.TERMINAL, 7)
    y, dz, stats = td_loss_reference(q, qn, rew, nxt, 0.99)
    want_y = (rew.astype(np.float64) + 0.99 * np.where(nxt == D.TERMINAL, 0.0, qn.astype(np.float64))).astype(np.float32)
    assert y.dtype == dz.dtype == np.float32 and np.array_equal(y, want_y) and np.array_equal(y[nxt == D.TERMINAL], rew[nxt == D.TERMINAL])
    assert np.array_equal(dz, ((q - y).astype(np.float32) / np.float32(B)).astype(np.float32))
    dd = q.astype(np.float64) - y.astype(np.float64)
    assert stats[0] == _house_sum(dd * dd) / 600.0 and abs(stats[0] - (dd * dd).sum() / 600.0) <= 1e-13
    dA, mu = r.normal(size=(B, 4)).astype(np.float32), r.normal(size=(B, 4)).astype(np.float32)
    dz4, st = dpg_dz_reference(dA, mu, q, 0.5)
    gated = ((mu >= 0.5) & (dA < 0)) | ((mu <= -0.5) & (dA > 0))
    assert 0.2 < st[1] == gated.mean() < 0.4 and np.array_equal(dz4, np.where(gated, np.float32(0), dA)) and abs(st[2] - np.abs(dA.astype(np.float64)).mean()) <= 1e-13
    assert st[0] == -_house_sum(q.astype(np.float64)) / B
    tg, th = r.normal(size=1000).astype(np.float32), r.normal(size=1000).astype(np.float32)
    for tau in (0.005, 0.3):
        got = polyak_reference(tg, th, tau)
        t, omt = np.float32(tau), np.float32(1.0 - tau)
        assert got.dtype == np.float32 and np.array_equal(got, np.float32(omt * tg) + np.float32(t * th))
        assert not np.array_equal(got.astype(np.float64), (1.0 - tau) * tg.astype(np.float64) + tau * th.astype(np.float64))
    assert np.array_equal(polyak_reference(tg, th, 0.0), tg + np.float32(0.0) * th) and np.array_equal(polyak_reference(tg, th, 1.0), np.float32(0.0) * tg + th)
    X = concat_reference(tg.reshape(10, 100), 3.0 * dA[:4], np.array([9, 0, 9, 3]), 1.0)
    assert np.array_equal(X[:, :100], tg.reshape(10, 100)[[9, 0, 9, 3]]) and np.array_equal(X[:, 100:], np.clip(3.0 * dA[:4], -1, 1).astype(np.float32))
    assert np.array_equal(concat_reference(tg.reshape(10, 100), 3.0 * dA[:4], np.array([9, 0, 9, 3]))[:, 100:], (3.0 * dA[:4]).astype(np.float32))
    with pytest.raises(ValueError):
        concat_reference(tg.reshape(10, 100), dA[:3], np.array([9, 0, 9, 3]))


# ---- the successor table and the leaf refusal -------------------------------------------------------------------------------------------------
def test_successor_table_and_leaf_refusal():
    _, nxt, episodes = D.chain_case()
    assert np.array_equal(ddpg_successors(nxt, D.IDX8), [9, 4, 11, 0, 7, 10, 6, 3])       # a terminal row names itself; row 8's successor is the leaf
    assert np.array_equal(ddpg_successors(nxt, np.array([[1, 9], [0, 8]])), [[3, 9], [0, 10]])
    with pytest.raises(ValueError, match="leaf"):
        ddpg_successors(nxt, np.array([3, 10, 4]))
    nonleaf = np.nonzero(nxt != D.NONE)[0]
    assert np.array_equal(nonleaf, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]) and (ddpg_successors(nxt, nonleaf) >= nonleaf).all()


# ---- the Gaussian case: its preconditions hold by construction --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n_rows", [(8, 48), (257, 300)])
def test_gaussian_case_preconditions(B, n_rows):
    c, idx = D.gaussian_case([300, 37, 64, 4], [304, 37, 64, 1], B, seed=4, n_rows=n_rows)
    cb, ab = D.critic_bound(c, idx, D.G_GAMMA, D.G_BOUND), D.actor_bound(c, idx, D.G_BOUND)
    assert cb['margin'] > 0 and ab['margin'] > 0 and ab['gate_margin'] > 0
    nx = np.asarray(c['next'])[idx]
    assert not (nx == D.NONE).any() and (nx == D.TERMINAL).sum() >= 1 and (np.asarray(c['next'])[nx[nx >= 0]] == D.NONE).sum() >= 1
    assert 0.1 <= ab['gated'] / (4.0 * B) <= 0.6 and (np.abs(c['labels'][idx]) > D.G_BOUND).mean() >= 0.25
    loss, grads, y, q = q_fit_reference(c['q'], c['tq'], c['tpol'], c['rows'], c['labels'], c['rew'], c['next'], idx, D.G_GAMMA, D.G_BOUND)
    assert abs(loss - cb['loss']) <= 1e-12 * loss and np.allclose(D._flat(grads), D._flat(cb['grads']), rtol=0, atol=1e-13) and np.allclose(y, cb['y'], rtol=0, atol=1e-13)
    stats, gp, dA = dpg_reference(c['pol'], c['q'], c['rows'], idx, D.G_BOUND)
    assert np.allclose(stats, ab['stats'], rtol=0, atol=1e-13) and np.allclose(D._flat(gp), D._flat(ab['grads']), rtol=0, atol=1e-13) and np.allclose(dA, ab['dA'], rtol=0, atol=1e-15)
    assert np.abs(D._flat(grads)).max() > 1e-4 and np.abs(D._flat(gp)).max() > 1e-5
    assert cb['bound'].max() < 0.05 * np.abs(D._flat(grads)).max() and ab['bound'].max() < 0.05 * np.abs(D._flat(gp)).max()      # the bounds bind


# ---- the header, the exports, the bindings ----------------------------------------------------------------------------------------------------
NEW = ["clothhip_set_q_mlp", "clothhip_get_q_mlp", "clothhip_ddpg_sync_targets", "clothhip_ddpg_get_targets", "clothhip_ddpg_set_targets", "clothhip_q_fit_grad", "clothhip_q_fit",
       "clothhip_q_fit_reset", "clothhip_policy_fit_dpg_grad", "clothhip_policy_fit_dpg", "clothhip_ddpg_polyak", "clothhip_ddpg_last_tables", "clothhip_ddpg_fit"]
_CTYPES = {"clothhip_handle *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int32_t": C.c_int32, "size_t": C.c_size_t, "double": C.c_double,
           "float *": C.POINTER(C.c_float), "const float *": C.POINTER(C.c_float), "double *": C.POINTER(C.c_double),
           "const ClothFitParams *": C.POINTER(_lib.ClothFitParams), "const ClothDdpgParams *": C.POINTER(_lib.ClothDdpgParams)}


def test_symbols_declared_exported_bound_with_the_headers_signatures():
    hdr = open(os.path.join(ROOT, "include", "clothhip.h")).read()
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    L = _lib.load()
    for name in NEW:
        m = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        assert m, name
        types = [re.sub(r"\s*\w+$", "", re.sub(r"/\*.*?\*/", "", p).strip()).strip() for p in m.group(1).split(",")]
        assert name in bound and bound[name][0] is C.c_int, name
        assert bound[name][1] == [_CTYPES[t] for t in types], (name, types)
        assert getattr(L, name) is not None
    assert re.search(r"typedef struct ClothDdpgParams \{ double gamma, tau; float act_bound; int32_t flags", hdr)
    assert [f[0] for f in _lib.ClothDdpgParams._fields_] == ["gamma", "tau", "act_bound", "flags"] and C.sizeof(_lib.ClothDdpgParams) == 24
    for k, v in (("Q", _lib.Q_STATS), ("DPG", _lib.DPG_STATS), ("DDPG", _lib.DDPG_STATS)):
        assert re.search(r"#define CLOTHHIP_%s_STATS %d\b" % (k, v), hdr)
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7 and re.search(r"#define CLOTHHIP_ABI_VERSION 7\b", hdr)      # the change is additive
    for call in [lambda: L.clothhip_set_q_mlp(None, 0, None, None, 0), lambda: L.clothhip_get_q_mlp(None, None, 0), lambda: L.clothhip_ddpg_sync_targets(None),
                 lambda: L.clothhip_ddpg_get_targets(None, None, None), lambda: L.clothhip_ddpg_set_targets(None, None, None), lambda: L.clothhip_q_fit_grad(None, None, None, 1, None, None, None, None),
                 lambda: L.clothhip_q_fit(None, None, None, None, 0, 1, None), lambda: L.clothhip_q_fit_reset(None),
                 lambda: L.clothhip_policy_fit_dpg_grad(None, None, None, 1, None, None, None), lambda: L.clothhip_policy_fit_dpg(None, None, None, None, 0, 1, None),
                 lambda: L.clothhip_ddpg_polyak(None, 0.5), lambda: L.clothhip_ddpg_last_tables(None, 1, None, None, None),
                 lambda: L.clothhip_ddpg_fit(None, None, None, None, None, 0, 1, None)]:
        assert call() == _lib.EINVAL                                              # NULL handle: a status, no device touched


def test_the_kernels_live_in_their_own_header_included_by_the_trainer_alone():
    csrc = os.path.join(ROOT, "gym_cloth_amd", "csrc")
    text = open(os.path.join(csrc, "cloth_fit_ddpg.hpp")).read()
    for k in ("k_fit_concat", "k_fit_loss_td", "k_fit_dpg_dz", "k_fit_polyak"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, text), k
    assert "atomic" not in text.replace("no floating-point atomics", "")
    sources = [f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp")) and f != "cloth_fit_ddpg.hpp"]
    users = [f for f in sources if '"cloth_fit_ddpg.hpp"' in open(os.path.join(csrc, f)).read()]
    assert users == ["api_fit.hip"]


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s) before refusing its arguments" % name)


def test_wrappers_refuse_before_any_library_call():
    b = ClothBatch.__new__(ClothBatch)
    b._L, b._h, b.P, b.E, b._q_n_params, b._mlp_n_params = _NoLibrary(), None, 3, 2, 10, 10
    with pytest.raises(ValueError):
        b.set_q_mlp([(np.zeros((4, 13)), np.zeros(4))])                           # an action's width, not a value's
    for kw in [dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=np.nan), dict(gamma=0.9, act_bound=0.0), dict(gamma=0.9, act_bound=-1.0), dict(gamma=0.9, act_bound=np.nan)]:
        with pytest.raises(ValueError):
            b.q_grad(np.array([0, 1]), **kw)
        with pytest.raises(ValueError):
            b.q_fit(np.zeros((2, 3), dtype=int), **kw)
    for tau in (-0.1, 1.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            b.ddpg_polyak(tau)
        with pytest.raises(ValueError):
            b.ddpg_fit(np.zeros((2, 3), dtype=int), 0.9, tau)
    for idx in [np.zeros((2, 2), dtype=int), np.zeros(0, dtype=int), np.zeros(3), np.array([0, -1])]:
        with pytest.raises(ValueError):
            b.q_grad(idx, 0.9)
        with pytest.raises(ValueError):
            b.dpg_grad(idx)
    with pytest.raises(ValueError):
        b.dpg_fit(np.zeros((2, 3), dtype=int), optimizer="lbfgs")
    with pytest.raises(ValueError):
        b.ddpg_fit(np.zeros((2, 3), dtype=int), 0.9, 0.005, q_hyper=dict(lr=-1.0))
    b._q_n_params = 0
    for call in (lambda: b.q_grad(np.array([0]), 0.9), lambda: b.dpg_grad(np.array([0])), lambda: b.get_q_mlp(), lambda: b.ddpg_targets()):
        with pytest.raises(_lib.ClothHipError):
            call()
