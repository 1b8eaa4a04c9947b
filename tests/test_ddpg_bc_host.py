"""Host tests of DDPG from demonstrations, no GPU: the float64 reference against central finite differences of its own
loss with the filter's mask held fixed; the bit-for-bit restatement of k_fit_dpg_bc against the float64 reference on exactly
representable data; the tie; the NaN-row rules of the expert column on the Python side; the demo_fraction tables; the preconditions of
the GPU file's exact and Gaussian tests, found here on the CPU; the header, the exports and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddpg_bc_cases as K
import ddpg_cases as D
from gym_cloth_amd import _lib
from gym_cloth_amd.batch import ClothBatch
from gym_cloth_amd.batch_fit import bc_params, expert_rows, has_expert
from gym_cloth_amd.demos import demo_table
from gym_cloth_amd.references import concat_reference, dpg_bc_dz_reference, dpg_bc_reference, dpg_dz_reference, dpg_reference, expert_mask
from test_ddpg_host import H, _fd_check, _tiny_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny_bc_case(seed=0):
    """test_ddpg_host's tiny case with an expert column: rows 2 and 6 carry none."""
    c, idx = _tiny_case(seed)
    ex = np.random.RandomState(70 + seed).uniform(-1.5, 1.5, size=(9, 4)).astype(np.float32)
    ex[2] = K.NO_EXPERT
    ex[6] = K.NO_EXPERT
    return dict(c, expert=ex), idx


# ---- the float64 reference against finite differences of its own loss ---------------------------------------------------------------------
@pytest.mark.parametrize("q_filter", [True, False])
def test_dpg_bc_reference_against_finite_differences(q_filter):
    """The step is test_ddpg_host's H = 2^-10 and the tolerance is _fd_check's, derived there from the step: the BC term adds a
    polynomial of degree 2 L = 4 in one weight with coefficients of order 1 to a loss of that kind, so the same bound holds. The
    filter's mask is held fixed at the reference's own (no gradient flows through it); bound = 100: no clamp or gate in reach."""
    assert H == 2.0 ** -10
    c, idx = _tiny_bc_case(0)
    ref = dpg_bc_reference(c['pol'], c['q'], c['rows'], c['expert'], idx, 100.0, 0.75, 1.5, q_filter)
    assert ref['m'].sum() == 5 and (0 < ref['f'].sum() < 5 if q_filter else ref['f'].sum() == 5) and ref['stats'][3] > 0
    assert abs(ref['loss'] - (0.75 * ref['stats'][0] + 1.5 * ref['stats'][3])) < 1e-15
    pol = [(W.copy(), b.copy()) for W, b in c['pol']]
    loss_of = lambda layers: dpg_bc_reference(layers, c['q'], c['rows'], c['expert'], idx, 100.0, 0.75, 1.5, q_filter, mask=ref['f'])['loss']
    assert _fd_check(loss_of, pol, ref['grads']) >= 10
    # the two terms alone: q_coef = 1, bc_coef = 0 is dpg_reference; q_coef = 0 is the squared error to the expert's actions over 4 B
    plain = dpg_reference(c['pol'], c['q'], c['rows'], idx, 100.0)
    only_q = dpg_bc_reference(c['pol'], c['q'], c['rows'], c['expert'], idx, 100.0, 1.0, 0.0, q_filter)
    assert np.array_equal(D._flat(only_q['grads']), D._flat(plain[1])) and np.array_equal(only_q['stats'][:3], plain[0])
    only_bc = dpg_bc_reference(c['pol'], c['q'], c['rows'], c['expert'], idx, 100.0, 0.0, 1.0, False)
    mu = only_bc['dz'] * 0.0 + D._forward_facts(c['pol'], c['rows'].astype(np.float64)[idx])[0][-1]
    m = expert_mask(c['expert'][idx])
    want = np.where(m[:, None], mu - c['expert'][idx].astype(np.float64), 0.0)
    assert np.allclose(only_bc['dz'], want / (2.0 * len(idx)), rtol=0, atol=1e-15) and abs(only_bc['loss'] - (want * want).sum() / (4.0 * len(idx))) < 1e-15


# ---- the restatement against the float64 reference on exact data; the tie --------------------------------------------------------------------
@pytest.mark.parametrize("n_side,pw,qw,dens,seed,eseed", K.EXACT_BC_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_exact_preconditions_and_the_restatement(n_side, pw, qw, dens, seed, eseed):
    """exact_bc_asserts holds at the listed expert seed and at none before it; on that data dpg_bc_dz_reference, fed the reference's own
    dA, y, q and qe as float32, EQUALS the float64 reference: dz and the six statistics; and concat_reference's expert mode gives the
    clamped expert action, four zeros for a row without one."""
    for earlier in range(eseed):
        with pytest.raises(AssertionError):
            K.exact_bc_asserts(pw, qw, dens, seed, earlier)
    c = K.exact_bc_asserts(pw, qw, dens, seed, eseed)
    for idx in (D.IDX8, D.IDX1, D.IDXR):
        mu = D._forward_facts(c['pol'], c['rows'].astype(np.float64)[idx])[0][-1].astype(np.float32)
        for qc in K.QCS:
            for q_filter in (True, False):
                ref = dpg_bc_reference(c['pol'], c['q'], c['rows'], c['expert'], idx, D.BOUND, qc, K.BC, q_filter)
                dz, stats = dpg_bc_dz_reference(ref['dA'], mu, ref['q'], ref['qe'] if q_filter else None, c['expert'][idx], D.BOUND, qc, K.BC)
                assert np.array_equal(dz.astype(np.float64), ref['dz']) and np.array_equal(stats, ref['stats']), (len(idx), qc, q_filter)
        X = concat_reference(c['rows'], c['expert'][idx], idx, D.BOUND, expert=True)
        m = expert_mask(c['expert'][idx])
        assert np.array_equal(X[:, :-4], c['rows'][idx]) and not np.isnan(X).any() and not X[~m, -4:].any() and np.abs(X[:, -4:]).max() <= D.BOUND
        assert np.array_equal(X[m, -4:], D.clamp(c['expert'][idx][m], D.BOUND))


def test_a_tie_does_not_pass_the_filter():
    """qe == q in float32 does not pass; the next float32 above does; a NaN in qe does not; without the filter every labelled row passes.
    Where the row does not pass NO addition is made: a gated -0.0 keeps its sign, and with q_coef = 1 dz is dpg_dz_reference's by bytes."""
    dA = np.array([[0.5, -0.25, -0.0, 1.0]] * 8, dtype=np.float32)
    y = np.array([[0.5, 2.0, -0.5, -2.0]] * 8, dtype=np.float32)
    ex = np.array([[0.25, 0.5, -3.0, 3.0]] * 8, dtype=np.float32)
    ex[4] = K.NO_EXPERT
    q = np.ones(8, dtype=np.float32)                                           # (B = 8: 2 B is a power of two, every value below is exact)
    qe = np.array([1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), np.nextafter(np.float32(1.0), np.float32(0.0)), np.nan, 5.0, 0.0, -1.0, 0.5], dtype=np.float32)
    dz, stats = dpg_bc_dz_reference(dA, y, q, qe, ex, 1.0, 1.0, 0.5)
    plain, pst = dpg_dz_reference(dA, y, q, 1.0)
    assert stats[4] == 7.0 / 8.0 and stats[5] == 1.0 / 8.0 and np.array_equal(stats[:3], pst)
    for r in (0, 2, 3, 4, 5, 6, 7):
        assert dz[r].tobytes() == plain[r].tobytes(), r
    assert np.signbit(dz[0, 2]) and dz[1].tobytes() != plain[1].tobytes()
    e = np.array([0.25, 0.5, -1.0, 1.0])
    assert np.array_equal(dz[1].astype(np.float64), plain[1].astype(np.float64) + 0.5 * (y[1].astype(np.float64) - e) / 16.0)
    assert stats[3] == ((y[1].astype(np.float64) - e) ** 2).sum() / 32.0
    off, ost = dpg_bc_dz_reference(dA, y, q, None, ex, 1.0, 1.0, 0.5)
    assert ost[5] == 7.0 / 8.0 and off[4].tobytes() == plain[4].tobytes() and all(off[r].tobytes() == dz[1].tobytes() for r in (0, 1, 2, 3, 5, 6, 7))
    # bc_coef = 0: the loss is still reported, and no addition is made anywhere
    zero, zst = dpg_bc_dz_reference(dA, y, q, None, ex, 1.0, 1.0, 0.0)
    assert zero.tobytes() == plain.tobytes() and zst[3] == ost[3] == 7.0 * stats[3] > 0
    # (the float64 reference's own tie is exact_bc_asserts': row TIE_ROW of the exact cases)


# ---- the expert column's rows on the Python side -------------------------------------------------------------------------------------------
def test_expert_rows_hold_four_values_or_four_fill_patterns():
    nan2 = np.array([0xffc00001], dtype=np.uint32).view(np.float32)[0]      # another NaN: negative, with a payload
    a = expert_rows([[1, 2, 3, 4], [np.nan] * 4, [nan2] * 4, [-0.0, 0.0, 1e-40, -3.5]])
    assert a.dtype == np.float32 and a.shape == (4, 4)
    bits = a.view(np.uint32)
    assert (bits[1] == _lib.FIT_NO_EXPERT_BITS).all() and (bits[2] == _lib.FIT_NO_EXPERT_BITS).all() and _lib.FIT_NO_EXPERT_BITS == 0x7fc00000
    assert np.array_equal(a[0], [1, 2, 3, 4]) and a[3].tobytes() == np.array([-0.0, 0.0, 1e-40, -3.5], dtype=np.float32).tobytes()
    assert list(has_expert(a)) == [True, False, False, True] and list(expert_mask(a)) == [True, False, False, True]
    assert bits.tobytes() == np.concatenate([a[:1], K.NO_EXPERT[None], K.NO_EXPERT[None], a[3:]]).tobytes()
    for bad in ([[1, 2, np.nan, 4]], [[np.nan, 1, 1, 1]], [[np.inf, 0, 0, 0]], [[0, 0, 0, -np.inf]], [[1e39, 0, 0, 0]], [[np.nan, np.nan, np.nan, np.inf]],
                [1, 2, 3, 4], [[1, 2, 3]], np.zeros((2, 2, 4))):
        with pytest.raises(ValueError):
            expert_rows(bad)
    assert expert_rows(np.zeros((0, 4))).shape == (0, 4)


class _NoLibrary(object):
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s) before refusing its arguments" % name)


def test_wrappers_refuse_before_any_library_call():
    b = ClothBatch.__new__(ClothBatch)
    b._L, b._h, b.P, b.E, b._q_n_params, b._mlp_n_params = _NoLibrary(), None, 3, 2, 10, 10
    with pytest.raises(ValueError):
        b.fit_set_expert([[1, 2, np.nan, 4]])
    for kw in [dict(q_coef=-1.0), dict(bc_coef=-0.5), dict(q_coef=np.nan), dict(bc_coef=np.inf), dict(q_coef=0.0, bc_coef=0.0), dict(q_coef=1e39)]:
        with pytest.raises(ValueError):
            bc_params(**kw)
        with pytest.raises(ValueError):
            b.dpg_bc_grad(np.array([0, 1]), **kw)
        with pytest.raises(ValueError):
            b.dpg_bc_fit(np.zeros((2, 3), dtype=int), **kw)
        with pytest.raises(ValueError):
            b.ddpg_fit(np.zeros((2, 3), dtype=int), 0.9, 0.005, bc=kw)
    p = bc_params(0.0, 2.0, False)
    assert (p.q_coef, p.bc_coef, p.flags, p.reserved) == (0.0, 2.0, 0, 0) and bc_params(1.0, 0.0, True).flags == _lib.BC_QFILTER
    with pytest.raises(ValueError):
        b.fit_append_launch(np.zeros((1, 3), dtype=int), labels="expert+action")
    with pytest.raises(ValueError):
        b.dpg_bc_grad(np.zeros((2, 2), dtype=int))


# ---- demo_fraction ----------------------------------------------------------------------------------------------------------------------------
def test_demo_tables_share_determinism_and_refusal():
    from gym_cloth_amd.trainers import MLPTrainer
    replay, labelled = np.arange(10, 50), np.array([12, 13, 40])
    plain = demo_table(replay, labelled, 5, 9, 3, None)
    assert np.array_equal(plain, replay.astype(np.int32)[MLPTrainer.index_table(40, 5, 9, 3)]) and plain.dtype == np.int32
    for frac, k in ((0.5, 4), (0.0, 0), (1.0, 9), (0.12, 1), (0.1, 0)):
        t = demo_table(replay, labelled, 5, 9, 3, frac)
        assert t.shape == (5, 9) and t.dtype == np.int32 and np.isin(t[:, :k], labelled).all() and np.array_equal(t[:, k:], plain[:, k:]), frac
        assert np.array_equal(t, demo_table(replay, labelled, 5, 9, 3, frac))              # a pure function of its arguments
        assert np.isin(t, replay).all()
    a, b = demo_table(replay, labelled, 5, 9, 3, 0.5), demo_table(replay, labelled, 5, 9, 4, 0.5)
    assert not np.array_equal(a[:, :4], b[:, :4]) and len(np.unique(a[:, :4])) == 3
    with pytest.raises(ValueError):
        demo_table(replay, np.zeros(0, dtype=int), 5, 9, 3, 0.5)
    assert np.array_equal(demo_table(replay, np.zeros(0, dtype=int), 5, 9, 3, None), plain)    # ... which is asked for only with a fraction
    for frac in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError):
            demo_table(replay, labelled, 5, 9, 3, frac)


# ---- the Gaussian case's preconditions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 257])
def test_gaussian_case_preconditions(B):
    """The listed seed is the first whose case may be compared; there EVERY row's |qe - q| exceeds the sum of both forward bounds, every
    margin is > 0, the bound binds, and the extension's pieces are what the helper says they are."""
    seed = K.GAUSSIAN_BC_SEEDS[B]
    for earlier in range(seed):
        assert not K.gaussian_bc_ok(B, earlier)[0]
    ok, c, idx, ab = K.gaussian_bc_ok(B, seed)
    assert ok and ab['margin'] > 0 and ab['gate_margin'] > 0 and ab['filter_margin'] > 0
    assert (np.abs(ab['qe'] - ab['q']) > ab['dqe'] + ab['dq']).all() and len(ab['q']) == B
    assert 0 < ab['f'].sum() < ab['m'].sum() < B and 0 < ab['gated'] < 4 * B
    g = np.abs(D._flat(ab['grads']))
    assert ab['bound'].max() < 0.05 * g.max()
    free = K.with_expert(c, seed)
    assert 0.5 < (K._expert_row_margins(free, free['expert'], D.G_BOUND) > 0).mean() < 0.95      # what with_checked_expert's docstring says of a free draw


# ---- the header, the exports, the bindings ----------------------------------------------------------------------------------------------------
NEW = ["clothhip_fit_data_set_expert", "clothhip_fit_data_get_expert", "clothhip_policy_fit_dpg_bc_grad", "clothhip_policy_fit_dpg_bc", "clothhip_ddpg_fit_bc"]
_CTYPES = {"clothhip_handle *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double,
           "float *": C.POINTER(C.c_float), "const float *": C.POINTER(C.c_float), "double *": C.POINTER(C.c_double),
           "const ClothFitParams *": C.POINTER(_lib.ClothFitParams), "const ClothDdpgParams *": C.POINTER(_lib.ClothDdpgParams),
           "const ClothBcParams *": C.POINTER(_lib.ClothBcParams)}


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
    assert re.search(r"typedef struct ClothBcParams \{ float q_coef, bc_coef; int32_t flags; int32_t reserved; \} ClothBcParams;", hdr)
    assert [f[0] for f in _lib.ClothBcParams._fields_] == ["q_coef", "bc_coef", "flags", "reserved"] and C.sizeof(_lib.ClothBcParams) == 16
    assert re.search(r"#define CLOTHHIP_BC_QFILTER 1\b", hdr) and _lib.BC_QFILTER == 1
    assert re.search(r"CLOTHHIP_FIT_LABEL_ACTION_EXPERT = 4\b", hdr) and _lib.FIT_LABEL_ACTION_EXPERT == 4
    for k, v in (("DPG_BC", _lib.DPG_BC_STATS), ("DDPG_BC", _lib.DDPG_BC_STATS), ("DPG", 3), ("DDPG", 6)):
        assert re.search(r"#define CLOTHHIP_%s_STATS %d\b" % (k, v), hdr)
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7 and re.search(r"#define CLOTHHIP_ABI_VERSION 7\b", hdr)      # the change is additive
    for call in [lambda: L.clothhip_fit_data_set_expert(None, 0, 0, None), lambda: L.clothhip_fit_data_get_expert(None, 0, 0, None),
                 lambda: L.clothhip_policy_fit_dpg_bc_grad(None, None, None, None, 1, None, None, None, None, None, None),
                 lambda: L.clothhip_policy_fit_dpg_bc(None, None, None, None, None, 0, 1, None),
                 lambda: L.clothhip_ddpg_fit_bc(None, None, None, None, None, None, 0, 1, None)]:
        assert call() == _lib.EINVAL                                              # NULL handle: a status, no device touched


def test_the_kernel_and_the_column_are_where_the_design_says():
    csrc = os.path.join(ROOT, "gym_cloth_amd", "csrc")
    text = open(os.path.join(csrc, "cloth_fit_ddpg.hpp")).read()
    assert re.search(r"__global__[^;{]*\bk_fit_dpg_bc\b", text) and re.search(r"template <bool LABEL, bool EXPERT = false> __global__[^;{]*\bk_fit_concat\b", text)
    handle = open(os.path.join(csrc, "api_handle.hpp")).read()
    assert re.search(r"COL_OLD_LS, COL_EXP, FIT_COLS \}", handle) and re.search(r"\{0, 4, true, 0x7fc00000u\},\s*// COL_EXP", handle)
