"""The early walk of the eight-wave fp32 LEAN build (Variant::sweep_starts_early): wave 0 walks the window table from window 0
while waves 1-7 run the strain pre-pass over all particles, and takes the pre-pass's bounds only where its own reach is used up. That is a
different SCHEDULE of the strain phase, not different arithmetic: records, observations and particles equal the standard fp32 variant's
(CLOTHHIP_DEBUG_LEAN=0: pre-pass, barrier, sweep) bit for bit, and the walk never gives up waiting for the pre-pass (stats[4] == 0).
tests/test_early_walk_rule.py pins the rule itself on the CPU."""
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
    waits.append(env.batch.debug_stats()[:, 4].copy())
    a = np.stack([np.random.RandomState(3000 + e).uniform(-1, 1, size=4) for e in range(E)])
    obs, rew, done, info = env.step(a, auto_reset=False)              # the per-step path
    var_step = env.batch.last_variant()
    waits.append(env.batch.debug_stats()[:, 4].copy())
    res = dict(rew=out["rew"].copy(), executed=out["executed"].copy(), done=out["done"].copy(), cov=out["actual_coverage"].copy(),
               obs=out["obs"].copy(), obs2=obs.copy(), rew2=rew.copy(), exec2=env.last_executed.copy(),
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
        assert (w == 0).all(), w                                     # no walk gave up waiting for the pre-pass


@pytest.mark.parametrize("tier", ["tier1", "tier3"])
def test_early_walk_equals_the_barriered_standard_variant(tier, monkeypatch):
    ref = _standard(tier, monkeypatch)
    got, variants, waits = _run(tier, 8, monkeypatch)
    _early_ran(variants, waits, 25)
    assert ref["executed"].sum() > 10000
    assert tier != "tier1" or ref["exec2"].sum() > 1000              # (tier 3 at this size: every episode ends inside the launch, the step idles)
    _same(ref, got)


def test_early_walk_generic_build_and_walk_every_window(monkeypatch):
    """The generic build (grid sizes from the kernel arguments) takes the early walk too; PH_NOSKIP (CLOTHHIP_DEBUG_PHASES=31: walk every
    window, the barriered order) is the same build's exhaustive walk. Both equal the standard variant."""
    ref = _standard("tier1", monkeypatch)
    got, variants, waits = _run("tier1", 8, monkeypatch, nospec=True)
    _early_ran(variants, waits, 0)
    _same(ref, got)
    allw, variants, waits = _run("tier1", 8, monkeypatch, phases="31")
    _early_ran(variants, waits, 0)
    _same(ref, allw)


def test_early_walk_27x27_splits_the_particles_elsewhere(monkeypatch):
    """729 particles: the second particles of the pre-pass threads (t + 448) are 448 .. 728, more than four waves of them."""
    ref = _standard("tier1", monkeypatch, n_side=27)
    got, variants, waits = _run("tier1", 8, monkeypatch, n_side=27)
    _early_ran(variants, waits, 0)
    _same(ref, got)


def test_early_walk_time_sliced_launch_equals_the_unsliced_one(monkeypatch):
    """The same action streams in ONE launch and in two: a first launch whose time budget (half the whole launch's kernel time) cuts every
    env somewhere inside its sequence, and a second one that continues the operations in flight and runs the rest. Per env the
    (reward, done, executed, coverage) records of its first T actions are the same (a sliced launch keeps no per-slot observations)."""
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


def test_early_walk_cloth_at_rest_counts_no_sweep(monkeypatch):
    """A flat cloth settling with no action: no spring is ever flagged, so the walk only waits for the pre-pass's count, corrects nothing,
    and the debug stats count no sweep -- as the barriered order, which skips the sweep."""
    import bench
    from gym_cloth_amd import ClothBatch
    res = []
    for lean in (0, 8):
        monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", str(lean))
        b = ClothBatch(bench.bench_cfg(25, 0.02, "tier1"), n_envs=E, precision="f32")
        b.update(40)
        v, st = b.last_variant(), b.debug_stats()
        assert v["lean"] == (lean == 8) and (lean == 0 or (v["threads"], v["particles_per_thread"], v["table_mode"]) == (512, 2, 2)), v
        res.append((b.positions().copy(), st[:, 0].copy(), st[:, 4].copy()))
        b.close()
    (p0, sw0, _), (p8, sw8, w8) = res
    assert np.array_equal(p0, p8)
    assert (sw0 == 0).all() and (sw8 == 0).all(), (sw0, sw8)
    assert (w8 == 0).all(), w8


def test_early_walk_smallest_grid_waits_at_the_tables_end(monkeypatch):
    """3x3, the smallest grid the layout plan gives the variant: nine particles, so most pre-pass waves own none, and so few windows
    that wave 0 is at the table's end before the pre-pass has counted itself done -- the bounded wait, which must never run out."""
    import ctypes as C
    from gym_cloth_amd import _lib
    import bench
    L = _lib.load()
    smallest = None
    for n in range(3, 26):
        monkeypatch.setenv("CLOTHHIP_DEBUG_LEAN", "8")
        p = _lib.params_from_cfg(bench.bench_cfg(n, 0.02, "tier1"))
        out = np.zeros(24, dtype=np.int32)
        if L.clothhip_selftest_layout(C.byref(p), 1, E, 256, _lib.i32p(out), 24) == 0 and out[10] and tuple(out[12:15]) == (512, 2, 2) and out[22] and out[23]:
            smallest = n
            break
    assert smallest is not None and smallest * smallest < 448, smallest
    ref = _standard("tier1", monkeypatch, n_side=smallest)
    got, variants, waits = _run("tier1", 8, monkeypatch, n_side=smallest)
    _early_ran(variants, waits, 0)
    _same(ref, got)
