"""GPU tests of clothhip_fork (ClothBatch.fork_from): a whole cloth copied from env slot to env slot, within a handle and between
handles, on the device. A fork must carry everything a cloth is -- positions, previous positions, the pin bytes with their grab
multiplicities and the pinned-from-outside bit, the tear flag, the rest lengths, the material -- so that the copy's trajectory is the
source's, bit for bit, in both precisions; the references are the source env itself and, in fp64, the reference's golden captures."""
import numpy as np
import pytest

from helpers import BatchReplay
from test_gpu_parity import cfg_from_golden
from test_gpu_material import FRICTION, material

pytestmark = pytest.mark.gpu


def checkpoint_ends(ops):
    """index behind the k-th checkpoint op, for replay_ops(stop=...)"""
    return [i + 1 for i, op in enumerate(ops) if op[0] == "checkpoint"]


def full_state(b, e):
    pos, prev, pin = b.get_state(e, 1)
    return pos[0], prev[0], pin[0], b.pin_counts(e, 1)[0], bool(b.tear[e]), b.get_rest(e, 1)[0]


def same_cloth(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


# ---- 1. a state in the middle of a pull, with grab multiplicities and an outside pin ---------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_fork_of_a_mid_pull_state_continues_bit_for_bit(prec, oracle_lib, monkeypatch):
    """g_traj_lift_pull_25 replayed to its checkpoint inside the pull (five points held). Env 1 is then grabbed a second time at a held
    point (multiplicity 2 -- Gripper.adjust moves such a point twice) and gets a point pinned from outside; env 0 stays the reference's.
    Both are forked into two flat envs of the same handle and into a handle of another E. State, raw pin bytes, tear flag and rest lengths
    must be equal, and so must every later checkpoint of the remaining ops; in fp64 env 0 and its copies still equal the capture."""
    from gym_cloth_amd import ClothBatch
    monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    g = oracle_lib.load_golden("g_traj_lift_pull_25.npz")
    ends = checkpoint_ends(g["ops"])
    K = 9                                                                   # checkpoint 9: 70 of the pull's 150 adjust+update done
    a = ClothBatch(cfg_from_golden(g), n_envs=4, precision=prec)
    b = ClothBatch(cfg_from_golden(g), n_envs=5, precision=prec)
    oracle_lib.replay_ops(BatchReplay(a), g["ops"], stop=ends[K])
    a.reset_flat([0, 0, 1, 1])
    held = np.nonzero(a.get_state(1, 1)[2][0])[0]
    assert len(held) == 5
    xy = np.zeros((4, 2)); xy[1] = a.positions(1, 1)[0][held[0], :2]
    assert a.grab(xy, radius=1e-9, active=[0, 1, 0, 0])[1] == 1             # Gripper.grab at the point itself: held twice now
    a.pin_points(1, [7])
    cnt = a.pin_counts()
    assert (cnt[1] & 0x7F).max() == 2 and cnt[1, 7] == 0x80 and cnt[0].max() == 1 and not cnt[2:].any()
    assert a.get_state(1, 1)[2][0].max() == 1                               # ... which get_state's 0/1 `pinned` cannot show
    a.fork_from(a, [0, 1], [2, 3])
    b.fork_from(a, [0, 1, 1], [4, 0, 2])
    pairs = [(a, 2, 0), (a, 3, 1), (b, 4, 0), (b, 0, 1), (b, 2, 1)]
    for h, d, s in pairs:
        assert same_cloth(full_state(h, d), full_state(a, s)), (h is a, d, s)
    assert not b.pin_counts(1, 1).any() and not b.pin_counts(3, 1).any()    # the envs not named stay as they were
    got = {id(a): [], id(b): []}
    for h in (a, b):
        oracle_lib.replay_ops(BatchReplay(h), g["ops"], lambda k, h=h: got[id(h)].append([full_state(h, e) for e in range(h.E)]),
                              start=ends[K])
    assert len(got[id(a)]) == len(g["cp_pos"]) - K - 1 == 6
    if prec == "f32":
        assert a.last_variant() == b.last_variant(), (a.last_variant(), b.last_variant())
    for k in range(6):
        for h, d, s in pairs:
            assert same_cloth(got[id(h)][k][d], got[id(a)][k][s]), (k, h is a, d, s)
        assert not same_cloth(got[id(a)][k][0][:2], got[id(a)][k][1][:2])   # the decorated cloth goes elsewhere: both are exercised
        if prec == "f64":
            st = got[id(a)][k][0]
            assert np.array_equal(st[0], g["cp_pos"][K + 1 + k]) and np.array_equal(st[1], g["cp_prev"][K + 1 + k]), k
            assert np.array_equal(st[2].astype(bool), g["cp_pinned"][K + 1 + k].astype(bool)), k
    a.close(); b.close()


# ---- 2. the tear flag is copied --------------------------------------------------------------------------------------------------------------
def test_fork_copies_the_tear_flag_f64(oracle_lib):
    """g_traj_tear_25 up to the checkpoint at which the cloth has torn: the copy is torn too (clothhip_set_state would have cleared the
    flag), the destination's other env is not, and the last op gives the capture's last checkpoint on both."""
    from gym_cloth_amd import ClothBatch
    g = oracle_lib.load_golden("g_traj_tear_25.npz")
    ends = checkpoint_ends(g["ops"])
    assert list(g["cp_tear"]) == [0, 0, 0, 0, 1, 1]
    a = ClothBatch(cfg_from_golden(g), n_envs=2, precision="f64")
    b = ClothBatch(cfg_from_golden(g), n_envs=2, precision="f64")
    oracle_lib.replay_ops(BatchReplay(a), g["ops"], stop=ends[4])
    assert a.tear.tolist() == [True, True] and b.tear.tolist() == [False, False]
    b.fork_from(a, [0], [1])
    assert b.tear.tolist() == [False, True]
    assert same_cloth(full_state(b, 1), full_state(a, 0))
    for h in (a, b):
        oracle_lib.replay_ops(BatchReplay(h), g["ops"], start=ends[4])
    assert same_cloth(full_state(b, 1), full_state(a, 0)) and b.tear.tolist() == [False, True]
    assert np.array_equal(b.positions(1, 1)[0], g["cp_pos"][5]) and np.array_equal(b.get_state(1, 1)[1][0], g["cp_prev"][5])
    a.close(); b.close()


# ---- 3. rest tables --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_flat_to_flat_fork_keeps_the_shared_table_and_its_builds(prec, monkeypatch):
    from gym_cloth_amd import ClothBatch
    import bench
    monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    monkeypatch.delenv("CLOTHHIP_DEBUG_NOSPEC", raising=False)
    cfg = bench.bench_cfg(25, 0.02)
    a = ClothBatch(cfg, n_envs=2, precision=prec)
    b = ClothBatch(cfg, n_envs=3, precision=prec)
    fresh = ClothBatch(cfg, n_envs=3, precision=prec)
    a.grab_top([0.5, 0.5]); a.update(5, delta=[0.0, 0.0, 0.0025])
    b.fork_from(a, [0, 1], [0, 2])
    b.fork_from(b, [0], [1])                                                 # within one handle as well
    b.update(1); fresh.update(1); a.update(1)
    assert b.last_variant() == fresh.last_variant(), (b.last_variant(), fresh.last_variant())
    assert b.last_variant()["lean"] and b.last_variant()["spec_n_side"] == 25, b.last_variant()
    for e in range(3):
        assert same_cloth(full_state(b, e), full_state(a, 0)), e
    a.close(); b.close(); fresh.close()


def _tier2_handle(cfg, seeds, prec="f64"):
    from gym_cloth_amd import ClothBatch
    b = ClothBatch(cfg, n_envs=len(seeds), precision=prec)
    pos = np.empty((len(seeds), b.P, 3)); rest = np.empty((len(seeds), b.S))
    for e, s in enumerate(seeds):                                            # the noisy vertical sheet of tier 2, fixed draws
        pos[e], rest[e] = b.init_grid(2, bool(s % 2), np.random.RandomState(s).rand(b.P))
    b.set_state(pos, pos, np.zeros((len(seeds), b.P), dtype=np.uint8), rest, rest_shared=False)
    return b


def test_tier2_source_into_a_flat_handle_switches_it_to_per_env_rest_f64(monkeypatch):
    """Per-env rest rows forked into a handle that shares the flat table: the destination rows equal the source's, its third env keeps the
    flat lengths (and still steps like a fresh flat handle's), and 200 update()s of the copies are the sources'."""
    from gym_cloth_amd import ClothBatch
    import bench
    monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    cfg = bench.bench_cfg(25, 0.02, "tier2")
    a = _tier2_handle(cfg, [11, 12])
    b = ClothBatch(cfg, n_envs=3, precision="f64")
    fresh = ClothBatch(cfg, n_envs=1, precision="f64")
    flat_rest = b.get_rest(1, 1)[0]
    assert not np.array_equal(a.get_rest(0, 1)[0], a.get_rest(1, 1)[0]) and not np.array_equal(a.get_rest(0, 1)[0], flat_rest)
    b.fork_from(a, [1, 0], [0, 2])
    assert np.array_equal(b.get_rest(), np.stack([a.get_rest(1, 1)[0], flat_rest, a.get_rest(0, 1)[0]]))
    for h in (a, b, fresh):
        h.update(200)
    assert not b.last_variant()["lean"] and b.last_variant() == a.last_variant()
    assert same_cloth(full_state(b, 0), full_state(a, 1)) and same_cloth(full_state(b, 2), full_state(a, 0))
    assert same_cloth(full_state(b, 1), full_state(fresh, 0))
    assert np.abs(b.positions(0, 1) - b.positions(2, 1)).max() > 1e-3
    a.close(); b.close(); fresh.close()


def test_tier2_to_tier2_fork_with_a_permutation_f64():
    import bench
    cfg = bench.bench_cfg(25, 0.02, "tier2")
    a = _tier2_handle(cfg, [21, 22, 23])
    b = _tier2_handle(cfg, [31, 32, 33])
    perm = [2, 0, 1]
    b.fork_from(a, perm, [0, 1, 2])
    assert np.array_equal(b.get_rest(), a.get_rest()[perm])
    a.update(60); b.update(60)
    for d, s in enumerate(perm):
        assert same_cloth(full_state(b, d), full_state(a, s)), (d, s)
    a.close(); b.close()


# ---- 4. materials ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,dst_mixed", [("f64", False), ("f64", True), ("f32", True)])
def test_fork_carries_the_material(prec, dst_mixed, oracle_lib, monkeypatch):
    """Source: env 1 of a default handle holds the friction fixture's material (ks 7000, damping 1.2, plane_friction 0.5), stopped at the
    fixture's third checkpoint (31 of the lift's adjust+update done). A default fork gives the destination env that material -- through
    the destination's table, rebuilt (dst_mixed False) or copied record by record on the device (dst_mixed True: it already holds one)
    --, its launches leave the grid-specialised build, and the rest of the ops give the source's bits; in fp64 the capture's."""
    from gym_cloth_amd import ClothBatch
    monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    monkeypatch.delenv("CLOTHHIP_DEBUG_NOSPEC", raising=False)
    g = oracle_lib.load_golden("g_traj_friction_25.npz")
    base = oracle_lib.load_golden("g_traj_lift_pull_25.npz")["cfg"]
    ends = checkpoint_ends(g["ops"])
    a = ClothBatch(cfg_from_golden({"cfg": base}), n_envs=2, precision=prec)
    b = ClothBatch(cfg_from_golden({"cfg": base}), n_envs=3, precision=prec)
    a.set_material(material(base, **FRICTION), env0=1, n=1)
    if dst_mixed:
        b.set_material(material(base, density=150.0), env0=1, n=1)
    own = b.get_material(1, 1).copy()
    oracle_lib.replay_ops(BatchReplay(a), g["ops"], stop=ends[3])
    b.fork_from(a, [1, 0], [2, 0])
    assert np.array_equal(b.get_material(2, 1), a.get_material(1, 1)) and b.get_material(2, 1)["ks"][0] == 7000.0
    assert np.array_equal(b.get_material(0, 1), a.get_material(0, 1)) and np.array_equal(b.get_material(1, 1), own)
    for h in (a, b):
        oracle_lib.replay_ops(BatchReplay(h), g["ops"], start=ends[3])
    assert b.last_variant()["spec_n_side"] == 0
    assert a.last_variant() == b.last_variant()
    assert same_cloth(full_state(b, 2), full_state(a, 1)) and same_cloth(full_state(b, 0), full_state(a, 0))
    assert np.abs(a.positions(0, 1) - a.positions(1, 1)).max() > 1e-3
    if prec == "f64":
        assert np.array_equal(b.positions(2, 1)[0], g["cp_pos"][8]) and np.array_equal(b.get_state(2, 1)[1][0], g["cp_prev"][8])
    a.close(); b.close()


def test_state_only_fork_keeps_the_destinations_material_f64(oracle_lib, monkeypatch):
    """CLOTHHIP_FORK_STATE_ONLY: the friction env's STATE into a uniform handle, which keeps its material and its specialised build, and
    from there equals a uniform handle that was given the same state by upload."""
    from gym_cloth_amd import ClothBatch
    monkeypatch.delenv("CLOTHHIP_DEBUG_LEAN", raising=False)
    monkeypatch.delenv("CLOTHHIP_DEBUG_NOSPEC", raising=False)
    g = oracle_lib.load_golden("g_traj_friction_25.npz")
    base = oracle_lib.load_golden("g_traj_lift_pull_25.npz")["cfg"]
    ends = checkpoint_ends(g["ops"])
    a = ClothBatch(cfg_from_golden({"cfg": base}), n_envs=2, precision="f64")
    c = ClothBatch(cfg_from_golden({"cfg": base}), n_envs=2, precision="f64")
    d = ClothBatch(cfg_from_golden({"cfg": base}), n_envs=2, precision="f64")
    a.set_material(material(base, **FRICTION), env0=1, n=1)
    oracle_lib.replay_ops(BatchReplay(a), g["ops"], stop=ends[3])
    assert a.pin_counts(1, 1).max() == 1                                     # so that an upload can state the same pins
    before = c.get_material().copy()
    c.fork_from(a, [1], [0], state_only=True)
    assert np.array_equal(c.get_material(), before)
    pos, prev, pin = a.get_state(1, 1)
    d.set_state(pos, prev, pin, env0=0, n=1)
    for h in (a, c, d):
        oracle_lib.replay_ops(BatchReplay(h), g["ops"], start=ends[3])
    assert c.last_variant()["spec_n_side"] == 25 and c.last_variant() == d.last_variant()
    assert same_cloth(full_state(c, 0), full_state(d, 0))
    assert np.abs(c.positions(0, 1) - a.positions(1, 1)).max() > 1e-3        # ... and not the friction env's trajectory
    a.close(); c.close(); d.close()


# ---- 5. index rules --------------------------------------------------------------------------------------------------------------------------
def test_fork_index_rules_and_fan_out(monkeypatch):
    from gym_cloth_amd import ClothBatch
    import bench
    cfg = bench.bench_cfg(25, 0.02)
    a = ClothBatch(cfg, n_envs=3, precision="f64")
    b = ClothBatch(cfg, n_envs=6, precision="f64")
    a.grab_top([0.5, 0.5]); a.update(4, delta=[0.001, 0.0, 0.0025])
    b.grab_top([0.25, 0.25]); b.update(2, delta=[0.0, 0.001, 0.0025])
    f32 = ClothBatch(cfg, n_envs=2, precision="f32")
    small = ClothBatch(bench.bench_cfg(10, 0.02), n_envs=2, precision="f64")

    def everything(h):
        return [full_state(h, e) for e in range(h.E)] + [h.get_material()]

    for dst, src, d, s in ((b, a, [1, 1], [0, 2]),          # a destination twice
                           (a, a, [0, 1], [1, 2]),          # env 1 is source and destination on one handle
                           (b, a, [0, 6], [0, 1]), (b, a, [0, -1], [0, 1]), (b, a, [0, 1], [0, 3]), (b, a, [0, 1], [-1, 0]),
                           (b, f32, [0], [0]), (f32, a, [0], [0]),          # precisions differ
                           (b, small, [0], [0]), (small, a, [0], [0])):     # grids differ
        before = everything(dst)
        with pytest.raises(ValueError):
            dst.fork_from(src, s, d)
        after = everything(dst)
        assert all(same_cloth(x, y) for x, y in zip(before[:-1], after[:-1])) and np.array_equal(before[-1], after[-1]), (d, s)
    before = everything(b)
    b.fork_from(a, [], [])                                   # n = 0: succeeds, does nothing
    assert all(same_cloth(x, y) for x, y in zip(before[:-1], everything(b)[:-1]))
    b.fork_from(a, [2] * 6, np.arange(6))                    # one source, every env of the destination
    for e in range(6):
        assert same_cloth(full_state(b, e), full_state(a, 2)), e
    a.update(3); b.update(3)
    for e in range(6):
        assert same_cloth(full_state(b, e), full_state(a, 2)), e
    for h in (a, b, f32, small):
        h.close()


def test_fork_of_a_50x50_pair_f32():
    from gym_cloth_amd import ClothBatch
    import bench
    cfg = bench.bench_cfg(50, 0.0095)
    a = ClothBatch(cfg, n_envs=2, precision="f32")
    b = ClothBatch(cfg, n_envs=2, precision="f32")
    a.grab_top(np.array([[0.5, 0.5], [0.25, 0.75]])); a.update(3, delta=[0.0, 0.001, 0.0025])
    b.fork_from(a, [0, 1], [1, 0])
    a.update(2); b.update(2)
    assert a.last_variant() == b.last_variant()
    assert same_cloth(full_state(b, 1), full_state(a, 0)) and same_cloth(full_state(b, 0), full_state(a, 1))
    assert not np.array_equal(a.positions(0, 1), a.positions(1, 1))
    a.close(); b.close()


# ---- 6. operations a time slice left in flight -----------------------------------------------------------------------------------------------
def test_fork_drops_the_destinations_parked_operation_only_f64():
    """A time-sliced launch parks every env's first action inside the handle. A fork FROM that handle leaves them parked; a fork INTO its
    env 1 (of the state env 1 started from) drops env 1's only. The next launch then completes the others' actions and starts env 1's
    anew: every record equals an undisturbed twin's, which ran the same actions in one unsliced launch."""
    from test_gpu_fused import _bench_env
    from gym_cloth_amd import ClothBatch
    E = 4
    acts = np.stack([np.random.RandomState(2000 + e).uniform(-0.5, 0.5, size=(3, 4)) for e in range(E)], axis=1)
    a = _bench_env(E, "f64"); a.reset()
    u = _bench_env(E, "f64"); u.reset()
    assert not a.batch.in_flight().any()
    out = a.step_many(acts, time_budget_ms=5.0)
    assert not out["ran"].any(), "the slice must end inside the first action"
    assert a.batch.in_flight().all()
    with pytest.raises(RuntimeError, match="in flight"):
        a.snapshot()
    side = ClothBatch(a.cfg, n_envs=2, precision="f64")
    side.fork_from(a.batch, [0, 3], [0, 1])                  # FROM: nothing changes for the source
    assert a.batch.in_flight().all() and not side.in_flight().any()
    a.batch.fork_from(u.batch, [1], [1])                     # INTO env 1: back to where it started, its parked action dropped
    assert a.batch.in_flight().tolist() == [True, False, True, True]
    oa = a.step_many(acts)
    ou = u.step_many(acts)
    for k in ("rew", "done", "ran", "executed", "n_grabbed", "actual_coverage", "variance_inv"):
        assert np.array_equal(oa[k], ou[k]), (k, oa[k], ou[k])
    assert np.array_equal(oa["obs"], ou["obs"])
    a.close(); u.close(); side.close()
