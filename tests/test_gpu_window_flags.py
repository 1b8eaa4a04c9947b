"""The early order of the eight-wave fp32 LEAN build with per-window flags (Variant::sweep_starts_early): waves 1-7 test whole
windows of the strain table and publish, per window, a bit in the flag mask F and then one in the tested mask D; wave 0 walks from window 0 and,
where its reach is used up, continues at the first window that is untested or flagged -- it jumps over tested quiet windows, at the head of the
table and in holes between flagged ones. The same waves reset the collision hash table behind their last window. A different SCHEDULE, not
different arithmetic: records, observations, particles and the count of sweeps run equal the standard fp32 variant's (CLOTHHIP_DEBUG_LEAN=0:
pre-pass, barrier, sweep) bit for bit, and stats[4] (once: walks that gave up waiting) stays 0. tests/test_window_flag_rule.py pins the rule
itself on the CPU."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, T = 8, 3


def _run(tier, lean, monkeypatch, n_side=25, nospec=False, phases=None):
    import bench
    from gym_cloth_amd.envs import ClothVecEnv
    monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", str(lean))
    for name, val in (("CLOTHHIP_DEBUG_NOSPEC", "1" if nospec else None), ("CLOTHHIP_DEBUG_PHASES", phases)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    env = ClothVecEnv(bench.bench_cfg(n_side, 0.02, tier), n_envs=E, precision="f32", consume_domrand_draws=False)
    for e in range(E):
        env.np_randoms[e] = np.random.RandomState(1000 + e)
    env.reset()
    acts = np.ascontiguousarray(np.stack([np.random.RandomState(2000 + e).uniform(-1, 1, size=(T, 4)) for e in range(E)], axis=1))
    waits = []
    out = env.step_many(acts, auto_reset=True)                       # episode launch: actions, terminal tests, in-kernel resets
    var_fused = env.batch.last_variant()
    st = env.batch.debug_stats()
    waits.append(st[:, 4].copy())
    sweeps = st[:, 0].copy()
    a = np.stack([np.random.RandomState(3000 + e).uniform(-1, 1, size=4) for e in range(E)])
    obs, rew, done, info = env.step(a, auto_reset=False)              # the per-step path
    var_step = env.batch.last_variant()
    st = env.batch.debug_stats()
    waits.append(st[:, 4].copy())
    res = dict(rew=out["rew"].copy(), executed=out["executed"].copy(), done=out["done"].copy(), cov=out["actual_coverage"].copy(),
               obs=out["obs"].copy(), obs2=obs.copy(), rew2=rew.copy(), exec2=env.last_executed.copy(),
               sweeps=sweeps, sweeps2=st[:, 0].copy(),              # sweeps run: counted alike in both orders
               state=[x.copy() for x in env.batch.get_state()])
    env.close()
    return res, (var_fused, var_step), waits


_REF = {}


def _standard(tier, monkeypatch, n_side=25):
    """The standard fp32 variant's result (the barriered order), computed once per (tier, grid) and never changed."""
    key = (tier, n_side)
    if key not in _REF:
        res, (vf, vs), _ = _run(tier, 0, monkeypatch, n_side=n_side)
        assert not vf["lean"] and not vs["lean"] and vf["fused"] >= 1 and vs["fused"] == 0, (vf, vs)
        _REF[key] = res
    return _REF[key]


def _same(a, b):
    for k in a:
        if k == "state":
            for x, y in zip(a[k], b[k]):
                assert np.array_equal(x, y), k
        else:
            assert np.array_equal(a[k], b[k]), k


def _early_ran(variants, waits, spec):
    for v in variants:           # the library says which kernel ran: without this "bit-identical" could mean "never ran"
        assert v["lean"] and v["threads"] == 512 and v["particles_per_thread"] == 2 and v["table_mode"] == 2 and v["precision"] == "f32", v
        assert v["spec_n_side"] == spec, v
    for w in waits:
        assert (w == 0).all(), w


def _n_windows(n_side):
    from gym_cloth_amd import _lib
    from test_sweep_rule import window_table
    return window_table(_lib, n_side)["nW"]


def _gets_the_variant(n, monkeypatch):
    import bench
    from gym_cloth_amd import _lib
    L = _lib.load()
    monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", "8")
    p = _lib.params_from_cfg(bench.bench_cfg(n, 0.02, "tier1"))
    out = np.zeros(24, dtype=np.int32)
    return bool(L.clothhip_selftest_layout(C.byref(p), 1, E, 256, _lib.i32p(out), 24) == 0 and out[10] and tuple(out[12:15]) == (512, 2, 2)
                and out[22] and out[23])


@pytest.mark.parametrize("tier", ["tier1", "tier3"])
def test_window_flags_equal_the_barriered_standard_variant(tier, monkeypatch):
    assert _n_windows(25) == 55                                      # two words per mask in the specialised build
    ref = _standard(tier, monkeypatch)
    got, variants, waits = _run(tier, 8, monkeypatch)
    _early_ran(variants, waits, 25)
    assert ref["executed"].sum() > 10000 and ref["sweeps"].sum() > 100
    assert tier != "tier1" or ref["exec2"].sum() > 1000
    _same(ref, got)


def test_window_flags_generic_build_and_walk_every_window(monkeypatch):
    """The generic build (grid sizes, and so the number of mask words, from the kernel arguments) takes the early order too; PH_NOSKIP
    (CLOTHHIP_DEBUG_PHASES=31: walk every window) is the same build's barriered order, with the hash-table reset in its old place."""
    ref = _standard("tier1", monkeypatch)
    got, variants, waits = _run("tier1", 8, monkeypatch, nospec=True)
    _early_ran(variants, waits, 0)
    _same(ref, got)
    allw, variants, waits = _run("tier1", 8, monkeypatch, phases="31")
    _early_ran(variants, waits, 0)
    for k in ("sweeps", "sweeps2"):                                  # (PH_NOSKIP sweeps in every substep: its count is its own)
        allw.pop(k)
    _same({k: v for k, v in ref.items() if k in allw}, allw)


def test_window_flags_27x27_needs_a_third_mask_word(monkeypatch):
    nW = _n_windows(27)
    assert 64 < nW <= 96, nW
    ref = _standard("tier1", monkeypatch, n_side=27)
    got, variants, waits = _run("tier1", 8, monkeypatch, n_side=27)
    _early_ran(variants, waits, 0)
    _same(ref, got)


def test_window_flags_largest_grid_of_the_variant(monkeypatch):
    """The largest grid the layout plan gives the variant must fit the masks (128 windows): asserted here, not assumed."""
    have = [n for n in range(3, 65) if _gets_the_variant(n, monkeypatch)]
    assert have, have
    largest = have[-1]
    assert largest >= 27 and _n_windows(largest) <= 128, (largest, _n_windows(largest))
    ref = _standard("tier1", monkeypatch, n_side=largest)
    got, variants, waits = _run("tier1", 8, monkeypatch, n_side=largest)
    _early_ran(variants, waits, 25 if largest == 25 else 0)
    _same(ref, got)


def test_window_flags_3x3_is_one_window(monkeypatch):
    have = [n for n in range(3, 26) if _gets_the_variant(n, monkeypatch)]
    assert have and have[0] == 3 and _n_windows(3) == 1, have
    ref = _standard("tier1", monkeypatch, n_side=3)
    got, variants, waits = _run("tier1", 8, monkeypatch, n_side=3)
    _early_ran(variants, waits, 0)
    _same(ref, got)


def test_window_flags_time_sliced_launch_equals_the_unsliced_one(monkeypatch):
    """The same action streams in ONE launch and in two: the second continues the operations the first one's time budget cut. The masks and the
    collision counters are rebuilt with everything else in LDS when a launch begins."""
    import bench
    from gym_cloth_amd.envs import ClothVecEnv
    monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", "8")
    monkeypatch.delenv("CLOTHHIP_DEBUG_NOSPEC", raising=False)
    monkeypatch.delenv("CLOTHHIP_DEBUG_PHASES", raising=False)
    streams = np.stack([np.random.RandomState(2000 + e).uniform(-1, 1, size=(T, 4)) for e in range(E)])   # [E, T, 4]

    def fresh():
        env = ClothVecEnv(bench.bench_cfg(25, 0.02, "tier1"), n_envs=E, precision="f32", consume_domrand_draws=False)
        for e in range(E):
            env.np_randoms[e] = np.random.RandomState(1000 + e)
        env.reset()
        return env

    def records(out, e, n):
        return [(out["rew"][t, e], bool(out["done"][t, e]), int(out["executed"][t, e]), out["actual_coverage"][t, e].tobytes()) for t in range(n)]

    a = fresh()
    ref = a.step_many(np.ascontiguousarray(streams.transpose(1, 0, 2)), max_resets=8)
    ms = float(a.batch.last_kernel_ms)
    _early_ran([a.batch.last_variant()], [a.batch.debug_stats()[:, 4]], 25)
    a.close()
    assert ms > 0.0 and ref["ran"].all()
    b = fresh()
    cnt = np.zeros(E, dtype=np.int64)
    got = [[] for _ in range(E)]
    for launch, budget in enumerate((0.5 * ms, 0.0)):
        idx = np.minimum(cnt[None, :] + np.arange(T)[:, None], T - 1)
        out = b.step_many(streams[np.arange(E)[None, :], idx], max_resets=8, time_budget_ms=budget)
        _early_ran([b.batch.last_variant()], [b.batch.debug_stats()[:, 4]], 25)
        for e in range(E):
            n_e = int(out["ran"][:, e].sum())
            got[e] += records(out, e, min(n_e, T - len(got[e])))
            cnt[e] += n_e
        if launch == 0:
            assert (cnt < T).any(), "the budget must cut the launch"
    b.close()
    for e in range(E):
        assert len(got[e]) == T and got[e] == records(ref, e, T), e


def _plain(lean, monkeypatch, pos=None, n=40):
    """A ClothBatch stepped with bare updates, optionally from an uploaded state: positions, sweeps run, stats[4], variant."""
    import bench
    from gym_cloth_amd import ClothBatch
    monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", str(lean))
    monkeypatch.delenv("CLOTHHIP_DEBUG_NOSPEC", raising=False)
    monkeypatch.delenv("CLOTHHIP_DEBUG_PHASES", raising=False)
    b = ClothBatch(bench.bench_cfg(25, 0.02, "tier1"), n_envs=E, precision="f32")
    if pos is not None:
        b.set_state(pos=pos, prev=pos)
    b.update(n)
    v, st = b.last_variant(), b.debug_stats()
    assert v["lean"] == (lean == 8) and (lean == 0 or (v["threads"], v["particles_per_thread"], v["table_mode"], v["spec_n_side"]) == (512, 2, 2, 25)), v
    res = (b.positions().copy(), st[:, 0].copy(), st[:, 4].copy())
    b.close()
    return res


def test_window_flags_cloth_at_rest_counts_no_sweep(monkeypatch):
    """A flat cloth settling with no action: no window is ever flagged, the walk jumps from its first grant to the table's end, corrects
    nothing, and the debug stats count no sweep in either order."""
    (p0, sw0, _), (p8, sw8, w8) = _plain(0, monkeypatch), _plain(8, monkeypatch)
    assert np.array_equal(p0, p8)
    assert (sw0 == 0).all() and (sw8 == 0).all(), (sw0, sw8)
    assert (w8 == 0).all(), w8


def hole_state(lib_module, base):
    """A flat 25x25 cloth (`base`: its positions at rest) with a few particles lifted near the first rows and a few near the last rows, and
    what the window table says about it: (pos, windows flagged at that state, reach of every window)."""
    from test_sweep_rule import window_table
    W = window_table(lib_module, 25)
    n = 25
    pos = np.array(base, dtype=np.float64).reshape(n * n, 3)
    assert np.ptp(pos[:, 2]) == 0.0                                  # flat
    rest = np.linalg.norm(pos[W["A"]] - pos[W["B"]], axis=1)
    assert abs(rest.min() - 1.0 / (n - 1)) < 1e-6
    for p in (1 * n + 5, 1 * n + 12, 23 * n + 7, 23 * n + 15):
        pos[p, 2] += 0.035                                           # every structural and shear spring of the particle is over-stretched
    ln = np.linalg.norm(pos[W["A"]] - pos[W["B"]], axis=1)
    over = ln > rest * 1.1 * (1 + 1e-3)
    assert over.sum() >= 16 and not (np.abs(ln / (rest * 1.1) - 1.0) < 1e-3).any()     # nothing near the limit: fp32 decides alike
    slot_of = np.empty(W["S"], dtype=np.int64)
    sa = W["spring_at"]
    slot_of[sa[sa >= 0]] = np.nonzero(sa >= 0)[0]
    flagged = np.zeros(W["nW"], dtype=bool)
    flagged[slot_of[over] >> 6] = True
    reach = np.array([(int(W["ent"][w * 64]) >> 28) << W["rshift"] for w in range(W["nW"])])
    return pos, flagged, reach


def hole_of(flagged, reach):
    """The longest run of consecutive unflagged windows that lies behind a flagged window, beyond the reach of every flagged window before
    it, and in front of another flagged window: (first, length)."""
    best = (0, 0)
    fl = np.nonzero(flagged)[0]
    for i in range(len(fl) - 1):
        lo = int(max(fl[:i + 1] + reach[fl[:i + 1]])) + 1
        hi = int(fl[i + 1])
        if hi - lo > best[1]:
            best = (lo, hi - lo)
    return best


def test_window_flags_jump_over_a_hole(monkeypatch):
    """Over-stretched springs near the first and near the last rows of a flat cloth, nothing in between: at the uploaded state at least 8
    consecutive windows between the two groups hold no over-stretched spring and lie beyond the reach of the first group's windows -- the walk
    has a hole to jump over, and flagged windows behind it that it must not miss."""
    import bench
    from gym_cloth_amd import _lib, ClothBatch
    monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", "0")
    b = ClothBatch(bench.bench_cfg(25, 0.02, "tier1"), n_envs=1, precision="f32")
    base = b.positions()[0].copy()                                   # the cloth as created: flat, at rest
    b.close()
    pos, flagged, reach = hole_state(_lib, base)
    first, length = hole_of(flagged, reach)
    assert length >= 8, (first, length, np.nonzero(flagged)[0])
    assert flagged[:first].any() and flagged[first + length:].any() and not flagged[first:first + length].any()
    (p0, sw0, _), (p8, sw8, w8) = _plain(0, monkeypatch, pos=pos, n=5), _plain(8, monkeypatch, pos=pos, n=5)
    assert np.array_equal(p0, p8)
    assert (sw0 >= 1).all() and np.array_equal(sw0, sw8), (sw0, sw8)
    assert (w8 == 0).all(), w8
