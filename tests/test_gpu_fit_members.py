"""GPU tests of the grouped calls of the trainer (clothhip_policy_fit*_members; the k_fit_* kernels of csrc/cloth_policy_fit.hpp, which
carry the member index): rows of a population fitted in the launches of one network. Every comparison is array_equal on
the bits, and the twin is always a SECOND handle that carries the member as its shared network and is fitted by clothhip_policy_fit* --
the same kernels through members = {0}, n_m = 1, pinned to float64 numpy and to the restated optimizers by test_gpu_policy_fit.py:
gradient and loss, the optimizers' steps with per-member learning rates, the per-row step count, the resets, one handle taken from a
shared network to a population and back, the hand-over to the evaluation and to the episode launch, an fp64 handle, every refusal, and
a DAgger collection into an MLPEnsemble."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_dagger import _RECORDS, _env
from test_gpu_policy_fit import _new_batch, _random_layers

pytestmark = pytest.mark.gpu

G, N_ROWS = 3, 40
ADAM = dict(optimizer="adam", beta1=0.9, beta2=0.999, eps=1e-8)
OPTIMIZERS = {"adam": ADAM, "sgd": dict(optimizer="sgd", momentum=0.0), "sgd-momentum": dict(optimizer="sgd", momentum=0.9)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else (a.view(np.int64) if a.dtype == np.float64 else a)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _data(n_in, seed=3):
    r = np.random.RandomState(seed)
    return r.uniform(-1, 1, size=(N_ROWS, n_in)).astype(np.float32), r.uniform(-1, 1, size=(N_ROWS, 4))


def _nets(widths, seed=40):
    return [_random_layers(widths, seed + g) for g in range(G)]


def _n_params(widths):
    return sum(widths[l + 1] * widths[l] + widths[l + 1] for l in range(len(widths) - 1))


def _stride(n):
    return (n + 63) // 64 * 64


_handles = {}


@pytest.fixture(scope="module")
def handle():
    """(n_side, precision, which) -> ONE ClothBatch of one cloth with an empty dataset; the cases put their own networks and rows on it."""
    def get(n_side=10, prec="f32", which="pop"):
        key = (n_side, prec, which)
        if key not in _handles:
            _handles[key] = _new_batch(n_side, prec)
        b = _handles[key]
        b.fit_clear()
        return b
    yield get
    for b in _handles.values():
        b.close()
    _handles.clear()


def _population(b, nets, rows, labels):
    b.set_policy_population(nets, np.zeros(b.E, dtype=np.int32))
    b.fit_clear()
    b.fit_append(rows, labels)
    return b


def _twin(t, layers, rows, labels):
    """The twin: `layers` as the shared network of handle t (a fresh optimizer), the same dataset."""
    t.set_policy_mlp(layers)
    t.fit_clear()
    t.fit_append(rows, labels)
    return t


def _row(b, g, n, pad=False):
    return b.get_policy_mlp(g, _stride(n) if pad else n)


# ---- 1. the gradient ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 300], ids=["B5", "B300-two-ranges"])
@pytest.mark.parametrize("n_side,widths", [(10, [300, 4]), (10, [300, 5, 4]), (10, [300, 37, 64, 4]), (25, [1875, 7, 4])],
                         ids=lambda w: "x".join(map(str, w)) if isinstance(w, list) else str(w))
def test_gradient_equals_each_twins(n_side, widths, B, handle):
    """fit_grad_members(members=[2, 0]) with other index rows per member: gradient and loss of each member are its twin's fit_grad.
    B = 300 is two 256-row ranges (slabs and the reduce) and, over 40 stored rows, names rows more than once."""
    rows, labels = _data(widths[0])
    nets = _nets(widths)
    b = _population(handle(n_side), nets, rows, labels)
    t = handle(n_side, which="twin")
    idx = np.random.RandomState(11).randint(0, N_ROWS, size=(2, B)).astype(np.int32)
    assert not np.array_equal(idx[0], idx[1]) and (B <= N_ROWS or len(np.unique(idx[0])) < B)
    members = [2, 0]
    loss, grad = b.fit_grad_members(members, idx)
    assert loss.shape == (2,) and grad.shape == (2, _n_params(widths)) and grad.dtype == np.float32
    for j, g in enumerate(members):
        want_loss, want_grad = _twin(t, nets[g], rows, labels).fit_grad(idx[j])
        print("member %d: loss %.17g (twin %.17g), max |grad| %.3e" % (g, loss[j], want_loss, np.abs(grad[j]).max()))
        assert loss[j] == want_loss and np.isfinite(want_loss)
        assert _same(grad[j], want_grad) and np.abs(want_grad).max() > 0
    assert not _same(grad[0], grad[1])
    for g in range(G):                                                       # nothing was updated
        assert _same(_row(b, g, _n_params(widths)), np.concatenate([np.concatenate([W.reshape(-1), c]) for W, c in nets[g]]))


# ---- 2. / 6. steps ------------------------------------------------------------------------------------------------------------------------
def _steps_case(b, t, opt):
    widths = [300, 5, 4]
    n, B = _n_params(widths), 7
    rows, labels = _data(300)
    nets = _nets(widths)
    _population(b, nets, rows, labels)
    uploaded = [_row(b, g, n, pad=True) for g in range(G)]
    assert _stride(n) > n and all((u[n:] == 0).all() for u in uploaded)
    members, lr = [2, 0], [3e-3, 1e-2]
    table = np.random.RandomState(12).randint(0, N_ROWS, size=(5, 2, B)).astype(np.int32)
    hyper = dict(OPTIMIZERS[opt], lr=lr)
    loss = np.concatenate([b.fit_members(members, table[:3], hyper), b.fit_members(members, table[3:], hyper)])
    assert loss.shape == (5, 2)
    for j, g in enumerate(members):
        _twin(t, nets[g], rows, labels)
        kw = dict(OPTIMIZERS[opt], lr=lr[j])
        want = np.concatenate([t.fit(table[:3, j], **kw), t.fit(table[3:, j], **kw)])
        print("%s member %d: losses %r, twin %r" % (opt, g, loss[:, j].tolist(), want.tolist()))
        assert _same(loss[:, j], want)
        got = _row(b, g, n, pad=True)
        assert _same(got[:n], t.get_policy_mlp(0, n)) and not _same(got, uploaded[g])
        assert (_bits(got[n:]) == 0).all()                                   # the pad stays zeros
    assert _same(_row(b, 1, n, pad=True), uploaded[1])                       # the row not named keeps its bytes


@pytest.mark.parametrize("opt", sorted(OPTIMIZERS))
def test_steps_equal_each_twins(opt, handle):
    """Three steps, then a second call of two, per-member learning rates: the trained rows and the returned losses are the twins' after the
    same five steps; the untrained row's whole stride is what was uploaded; every pad is zeros."""
    _steps_case(handle(), handle(which="twin"), opt)


def test_steps_on_an_fp64_handle(handle):
    """The fit is float32 on a precision='f64' handle too: the same case, twin included, on fp64 handles."""
    _steps_case(handle(prec="f64"), handle(prec="f64", which="twin"), "adam")


# ---- 3. the per-row step count ------------------------------------------------------------------------------------------------------------------
def test_every_row_has_its_own_step_count(handle):
    """Member 0 for two steps, then members [0, 1] for two: row 1 is a fresh twin after two steps (it started at t = 1), row 0 its twin
    after four."""
    widths = [300, 5, 4]
    n = _n_params(widths)
    rows, labels = _data(300)
    nets = _nets(widths)
    b, t = _population(handle(), nets, rows, labels), handle(which="twin")
    r = np.random.RandomState(13)
    first, second = r.randint(0, N_ROWS, size=(2, 1, 6)).astype(np.int32), r.randint(0, N_ROWS, size=(2, 2, 6)).astype(np.int32)
    hyper = dict(ADAM, lr=1e-2)
    l1 = b.fit_members([0], first, hyper)
    l2 = b.fit_members([0, 1], second, hyper)
    _twin(t, nets[0], rows, labels)
    want0 = np.concatenate([t.fit(first[:, 0], **hyper), t.fit(second[:, 0], **hyper)])
    assert _same(np.concatenate([l1[:, 0], l2[:, 0]]), want0) and _same(_row(b, 0, n), t.get_policy_mlp(0, n))
    _twin(t, nets[1], rows, labels)
    want1 = t.fit(second[:, 1], **hyper)
    assert _same(l2[:, 1], want1) and _same(_row(b, 1, n), t.get_policy_mlp(0, n))
    # (the count matters to these bits: Adam's step size at t = 3, 4 is not the one at t = 1, 2, so a row 1 that shared row 0's count
    # would not be its twin's.) Row 2 was never named:
    assert _same(_row(b, 2, n), np.concatenate([np.concatenate([W.reshape(-1), c]) for W, c in nets[2]]))


# ---- 4. resets ----------------------------------------------------------------------------------------------------------------------------
def test_resets(handle):
    """fit_reset_members([0]) restarts row 0 only; set_policy_members (the map alone) restarts none; set_policy_population restarts all."""
    from gym_cloth_amd.policies import unpack_mlp
    widths = [300, 5, 4]
    n = _n_params(widths)
    rows, labels = _data(300)
    nets = _nets(widths)
    b, t = _population(handle(), nets, rows, labels), handle(which="twin")
    r = np.random.RandomState(14)
    ta, tb, tc = (r.randint(0, N_ROWS, size=(2, 2, 6)).astype(np.int32) for _ in range(3))
    hyper = dict(ADAM, lr=1e-2)
    b.fit_members([0, 1], ta, hyper)
    b.fit_reset_members([0])
    b.set_policy_members(np.array([1], dtype=np.int32))
    lb = b.fit_members([0, 1], tb, hyper)
    _twin(t, nets[0], rows, labels)
    t.fit(ta[:, 0], **hyper)
    t.fit_reset()
    want = t.fit(tb[:, 0], **hyper)
    assert _same(lb[:, 0], want) and _same(_row(b, 0, n), t.get_policy_mlp(0, n))
    row0_reset = t.get_policy_mlp(0, n)
    _twin(t, nets[1], rows, labels)
    t.fit(ta[:, 1], **hyper)
    want = t.fit(tb[:, 1], **hyper)                                           # neither the reset of row 0 nor the new map restarted row 1
    assert _same(lb[:, 1], want) and _same(_row(b, 1, n), t.get_policy_mlp(0, n))
    _twin(t, nets[0], rows, labels)                                           # (and a row 0 that had NOT been restarted would be another row)
    t.fit(ta[:, 0], **hyper)
    t.fit(tb[:, 0], **hyper)
    assert not _same(t.get_policy_mlp(0, n), row0_reset)
    # a new population restarts every row: the rows as they are now, uploaded again, take FIRST steps
    now = [unpack_mlp(np.array(widths), _row(b, g, n)) for g in range(G)]
    b.set_policy_population(now, np.zeros(1, dtype=np.int32))
    lc = b.fit_members([0, 1], tc, hyper)
    for j in range(2):
        _twin(t, now[j], rows, labels)
        assert _same(lc[:, j], t.fit(tc[:, j], **hyper)) and _same(_row(b, j, n), t.get_policy_mlp(0, n))
    b.fit_reset_members()                                                     # all rows: the next step of row 1 is a first step again
    now1 = unpack_mlp(np.array(widths), _row(b, 1, n))
    l1 = b.fit_members([1], tc[:1, 1:], hyper)
    _twin(t, now1, rows, labels)
    assert _same(l1[:, 0], t.fit(tc[:1, 1], **hyper)) and _same(_row(b, 1, n), t.get_policy_mlp(0, n))


def test_one_handle_from_a_shared_network_to_a_population_and_back():
    """ONE handle, a dataset of 320 small-integer rows, Adam: a shared network for 3 steps at B = 5; a population of 3 rows, 2 steps on
    members [2, 0] and 1 step on member [1] alone (n_m = 1 on a row other than 0); a new shared network for 3 steps at B = 300 (two
    256-row ranges). Every stage's losses and final weights are, bit for bit, those of a FRESH handle given that stage's calls alone: no
    moment and no step count carries over, and the one moment table survives [n_params] -> [3][stride] -> [n_params]."""
    widths, n_rows = [300, 5, 4], 320
    n = _n_params(widths)
    r = np.random.RandomState(16)
    rows, labels = r.randint(-2, 3, size=(n_rows, 300)).astype(np.float32), r.randint(-3, 4, size=(n_rows, 4)).astype(np.float64)
    nets, first, last = _nets(widths), _random_layers(widths, 50), _random_layers(widths, 51)
    t1, t2, t2b, t3 = (r.randint(0, n_rows, size=s).astype(np.int32) for s in [(3, 5), (2, 2, 5), (1, 1, 5), (3, 300)])
    hyper = dict(ADAM, lr=1e-2)

    def shared(layers, table):
        def stage(x):
            x.set_policy_mlp(layers)
            return [x.fit(table, **hyper)], [x.get_policy_mlp(0, n)]
        return stage

    def population(x):
        x.set_policy_population(nets, np.zeros(x.E, dtype=np.int32))
        losses = [x.fit_members([2, 0], t2, hyper), x.fit_members([1], t2b, hyper)]
        return losses, [_row(x, g, n, pad=True) for g in range(G)]

    b = _new_batch(10)
    b.fit_append(rows, labels)
    for name, stage in [("shared, B = 5", shared(first, t1)), ("population", population), ("shared, B = 300", shared(last, t3))]:
        got_loss, got_w = stage(b)
        fresh = _new_batch(10)
        fresh.fit_append(rows, labels)
        want_loss, want_w = stage(fresh)
        fresh.close()
        print("%s: losses %r, fresh handle %r" % (name, [l.tolist() for l in got_loss], [l.tolist() for l in want_loss]))
        assert len(got_loss) == len(want_loss) and len(got_w) == len(want_w)
        assert all(np.isfinite(l).all() and (l > 0).all() for l in want_loss)
        assert all(_same(g, w) for g, w in zip(got_loss, want_loss)), name
        assert all(_same(g, w) for g, w in zip(got_w, want_w)), name
    assert not _same(got_w[0], np.concatenate([np.concatenate([W.reshape(-1), c]) for W, c in last]))      # (the last stage did train)
    b.close()


# ---- 5. the hand-over ---------------------------------------------------------------------------------------------------------------------
def test_fitted_rows_reach_the_evaluation_and_the_launch(handle):
    """After a group fit through an MLPEnsemble on six 10x10 envs: policy_eval_members on the stored rows is each twin's policy_eval, and
    a 2-action step_many(policy='mlp', auto_reset=False) under the map [0, 1, 2, 0, 1, 2] equals, env by env, the launch of an env that
    carries that env's downloaded row as its shared network -- actions and records."""
    from gym_cloth_amd.policies import MLPEnsemble
    widths = [300, 5, 4]
    rows, labels = _data(300)
    nets = _nets(widths)
    v, w = _env("f32", n_side=10), _env("f32", n_side=10)
    ens = MLPEnsemble(v, nets, lr=[1e-2, 3e-3, 1e-3])
    assert ens.member.tolist() == [0, 1, 2, 0, 1, 2] and ens.size() == 0
    ens.append(rows, labels)
    loss = ens.step(3, 8, seed=5)
    assert loss.shape == (3, G) and np.isfinite(loss).all()
    fitted = [ens.layers(g) for g in range(G)]
    assert all(not _same(fitted[g][0][0], nets[g][0][0]) for g in range(G))
    acts = ens.actions(rows)
    assert acts.shape == (G, N_ROWS, 4) and _same(ens.disagreement(rows), acts.var(axis=0).mean(axis=1))
    t = handle(which="twin")
    for g in range(G):
        t.set_policy_mlp(fitted[g])
        assert _same(acts[g], t.policy_eval(rows))
        assert _same(v.batch.policy_eval_members(rows, np.full(N_ROWS, g, dtype=np.int32)), acts[g])

    def launch(x):
        x.seed([1337 + e for e in range(x.E)])
        x.reset()
        return x.step_many(policy="mlp", n_actions=2, auto_reset=False)
    first = ens.get_action(_first_obs(v))
    out = launch(v)
    assert out["ran"][0].all() and len({out["actions"][0, e].tobytes() for e in range(3)}) == 3
    assert _same(out["actions"][0], first)                                    # get_action: row member[e] on obs[e], the launch's bits
    for g in range(G):
        w.set_policy(fitted[g])
        ref = launch(w)
        for e in np.nonzero(ens.member == g)[0]:
            for k in _RECORDS:
                assert np.array_equal(out[k][:, e], ref[k][:, e], equal_nan=True), (g, e, k)
    v.close(); w.close()


def _first_obs(x):
    x.seed([1337 + e for e in range(x.E)])
    return np.asarray(x.reset(), dtype=np.float32).reshape(x.E, -1)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    """Every refused call of the header on one handle, with its return code; afterwards its rows are what they were, and one further
    group step gives the rows and losses of a handle that never saw a refused call (so no moment and no step count moved)."""
    from gym_cloth_amd import _lib
    from gym_cloth_amd.envs import ClothVecEnv
    from test_gpu_policy_fit import _cfg
    widths = [300, 5, 4]
    n = _n_params(widths)
    rows, labels = _data(300)
    ROWS = 17                                                                 # (G networks and 14 more rows: enough members to pass the n_m * B cap)
    nets = _nets(widths)
    nets = nets + [nets[g % G] for g in range(ROWS - G)]
    table = np.random.RandomState(15).randint(0, N_ROWS, size=(3, 2, 8)).astype(np.int32)
    hyper = dict(ADAM, lr=1e-2)
    v = ClothVecEnv(_cfg(10), n_envs=1, precision="f32", consume_domrand_draws=False)
    v.seed([1337])
    v.reset()
    b, c = v.batch, _new_batch(10)
    for x in (b, c):
        _population(x, nets, rows, labels)
        x.fit_members([2, 0], table[:2], hyper)
    L, h = b._L, b._h
    before = [_row(b, g, n, pad=True) for g in range(ROWS)]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: _lib.i32p(np.ascontiguousarray(a, dtype=np.int32))

    def params(n_m=2, **kw):
        p = (_lib.ClothFitParams * n_m)()
        for j in range(n_m):
            d = dict(optimizer=0.0, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0)
            d.update({k: (x[j] if isinstance(x, (list, tuple)) else x) for k, x in kw.items()})
            for k, x in d.items():
                setattr(p[j], k, x)
        return p

    def fit(p=None, members=(2, 0), n_m=None, idx=table[2:3], n_steps=1, B=8):
        n_m = len(members) if n_m is None else n_m
        p = params(max(n_m, 1)) if p is None else p
        loss = np.zeros(max(n_steps, 1) * max(n_m, 1))
        return L.clothhip_policy_fit_members(h, p, ip(members), n_m, ip(idx), n_steps, B, _lib.dp(loss))

    def grad(members=(2, 0), n_m=None, idx=table[2], B=8):
        n_m = len(members) if n_m is None else n_m
        g, loss = np.zeros((max(n_m, 1), n), dtype=np.float32), np.zeros(max(n_m, 1))
        return L.clothhip_policy_fit_grad_members(h, ip(members), n_m, ip(idx), B, fp(g), _lib.dp(loss))

    def unchanged():
        for g in range(ROWS):
            assert _same(_row(b, g, n, pad=True), before[g]), g
        assert b.fit_size() == N_ROWS

    big_b = np.zeros((2, _lib.FIT_MAX_BATCH + 1), dtype=np.int32)
    assert ROWS * _lib.FIT_MAX_BATCH > _lib.FIT_MAX_MEMBER_ROWS               # all ROWS members at the batch cap: n_m * B over ITS cap
    all_rows, wide = np.arange(ROWS), np.zeros((1, ROWS, _lib.FIT_MAX_BATCH), dtype=np.int32)
    bad_hi, bad_lo = table[2:3].copy(), table[2:3].copy()
    bad_hi[0, 1, 3], bad_lo[0, 0, 0] = N_ROWS, -1
    later = np.concatenate([table[:1], bad_hi])
    einval = [
        lambda: fit(n_m=0), lambda: grad(n_m=0), lambda: fit(n_m=-1),                                       # n_m < 1
        lambda: fit(members=(ROWS, 0)), lambda: fit(members=(0, -1)), lambda: grad(members=(ROWS, 0)),              # a member outside [0, rows)
        lambda: fit(members=(1, 1)), lambda: grad(members=(2, 2)),                                          # a repeated member
        lambda: fit(B=0), lambda: grad(B=0), lambda: fit(idx=big_b[None], B=big_b.shape[1]), lambda: grad(idx=big_b, B=big_b.shape[1]),
        lambda: fit(members=all_rows, idx=wide, B=_lib.FIT_MAX_BATCH), lambda: grad(members=all_rows, idx=wide[0], B=_lib.FIT_MAX_BATCH),
        lambda: fit(n_steps=-1),
        lambda: fit(idx=bad_hi), lambda: fit(idx=bad_lo), lambda: fit(idx=later, n_steps=2), lambda: grad(idx=bad_hi[0]), lambda: grad(idx=bad_lo[0]),
        lambda: fit(params(optimizer=2.0)), lambda: fit(params(lr=[1e-2, -1e-3])), lambda: fit(params(lr=[float("nan"), 1e-2])),
        lambda: fit(params(eps=float("inf"))), lambda: fit(params(beta1=[0.9, -0.1])), lambda: fit(params(beta2=[1.0, 0.999])),
        lambda: fit(params(optimizer=1.0, momentum=[0.0, -0.9])),
        lambda: fit(params(optimizer=[0.0, 1.0])), lambda: fit(params(optimizer=[1.0, 0.0])),               # differing optimizer fields
        lambda: L.clothhip_policy_fit_members(h, None, ip((2, 0)), 2, ip(table[2:3]), 1, 8, None),          # NULL where a table is needed
        lambda: L.clothhip_policy_fit_members(h, params(), None, 2, ip(table[2:3]), 1, 8, None),
        lambda: L.clothhip_policy_fit_members(h, params(), ip((2, 0)), 2, None, 1, 8, None),
        lambda: L.clothhip_policy_fit_grad_members(h, None, 2, ip(table[2]), 8, None, None),
        lambda: L.clothhip_policy_fit_grad_members(h, ip((2, 0)), 2, None, 8, None, None),
        lambda: L.clothhip_policy_fit_reset_members(h, ip((0, 0)), 2), lambda: L.clothhip_policy_fit_reset_members(h, ip((ROWS,)), 1),
        lambda: L.clothhip_policy_fit_reset_members(h, ip((0,)), 0),
    ]
    for i, call in enumerate(einval):
        assert call() == _lib.EINVAL, i
        unchanged()
    assert fit(n_steps=0) == _lib.OK                                          # n_steps == 0 returns 0 and changes nothing
    unchanged()
    # a launch in flight
    nsteps, done = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint8)
    b.run_actions_begin(v._episode_params(), 1, nsteps, done, actions=np.zeros((1, 1, 4)))
    assert fit() == _lib.ESTATE and grad() == _lib.ESTATE and L.clothhip_policy_fit_reset_members(h, None, 0) == _lib.ESTATE
    b.run_actions_end()
    unchanged()
    # an empty dataset (the same rows come back afterwards)
    b.fit_clear()
    assert fit() == _lib.ESTATE and grad() == _lib.ESTATE
    b.fit_append(rows, labels)
    unchanged()
    # one further group step: the rows and losses of the handle that saw none of this
    got, want = b.fit_members([2, 0], table[2:3], hyper), c.fit_members([2, 0], table[2:3], hyper)
    assert _same(got, want)
    for g in range(ROWS):
        assert _same(_row(b, g, n, pad=True), _row(c, g, n, pad=True)), g
    assert not _same(_row(b, 0, n), before[0][:n])
    # a shared network ("use clothhip_policy_fit"), then no network: these change the handle on purpose, so they come last
    b.set_policy_mlp(nets[0])
    assert fit() == _lib.ESTATE and grad() == _lib.ESTATE and L.clothhip_policy_fit_reset_members(h, None, 0) == _lib.ESTATE
    assert b"clothhip_policy_fit" in L.clothhip_last_error()
    b.set_policy_mlp(None)
    assert fit() == _lib.ESTATE and grad() == _lib.ESTATE and L.clothhip_policy_fit_reset_members(h, None, 0) == _lib.ESTATE
    with pytest.raises(_lib.ClothHipError):
        b.fit_grad_members([0], table[2, :1])
    # the shared trainer still refuses a population
    one = (_lib.ClothFitParams * 1)(_lib.ClothFitParams(0.0, 1e-2, 0.9, 0.999, 1e-8, 0.0))
    assert c._L.clothhip_policy_fit(c._h, one, ip(table[2, 0]), 1, 8, None) == _lib.ESTATE
    c.close()
    v.close()


# ---- 8. a DAgger collection into an ensemble ------------------------------------------------------------------------------------------------
def test_dagger_collect_with_an_ensemble():
    """Six envs, 4 actions, the oracle-corner expert, one whole-slot launch through demos.dagger_collect with an MLPEnsemble in the
    trainer's place: the stored rows are the bytes of slot_start_obs[ran] and float32(labels[ran]), as test_gpu_fit_launch.py checks for
    the trainer; a following step returns finite losses [n_steps, G]. (25x25 cloths: the oracle-corner expert is defined for that grid
    alone, and step_many refuses it on any other.)"""
    from gym_cloth_amd.demos import dagger_collect, dagger_mixture
    from gym_cloth_amd.envs import slot_start_obs
    from gym_cloth_amd.policies import MLPEnsemble
    N = 4
    nets = _nets([1875, 5, 4])
    a, b = _env("f32"), _env("f32")
    for x in (a, b):
        x.reset()
    ea, eb = MLPEnsemble(a, nets), MLPEnsemble(b, nets)
    before = np.asarray(a.state, dtype=np.float32).reshape(a.E, -1)
    whole = a.step_many(policy="mlp", n_actions=N, want_obs=True, expert="oracle_corner", expert_mix=dagger_mixture(N, a.E, 0.5, 7))
    ran = whole["ran"]
    assert ran.any()
    res = dagger_collect(b, eb, "oracle_corner", n_actions=N, beta=0.5, seed=7, slots_per_launch=N, max_launches=1)
    assert res["launches"] == 1 and res["appended"] == int(ran.sum()) == eb.size() and ea.size() == 0
    obs, lab = eb.data()
    assert _same(obs, slot_start_obs(whole, before)[ran]) and _same(lab, whole["expert_actions"][ran].astype(np.float32))
    loss = eb.step(2, 8, seed=3)
    assert loss.shape == (2, G) and np.isfinite(loss).all() and (loss > 0).all()
    assert len({loss[0, g] for g in range(G)}) == G                          # three networks on three bootstraps
    a.close(); b.close()
