"""GPU tests of the remaining C-ABI surface: async run + sync, device-resident schedules / observations,
determinism across envs and runs (race check), force_grab, partial reset of a vector env, error paths."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_env import base_cfg

pytestmark = pytest.mark.gpu


def _pull_state(oracle_lib):
    g = oracle_lib.load_golden("g_traj_lift_pull_25.npz")
    return g, (g["cp_pos"][9], g["cp_prev"][9], g["cp_pinned"][9], g["rest"])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_deterministic_across_envs_and_runs(prec, oracle_lib):
    """Same state + same schedule -> bit-identical results in every env and in a second run (no data race, no
    dependence on workgroup placement or LDS-atomic ordering)."""
    from gym_cloth_amd import ClothBatch, make_schedules
    g, st = _pull_state(oracle_lib)
    outs = []
    for rep in range(2):
        b = ClothBatch(base_cfg("tier1", 1), n_envs=96, precision=prec)
        b.set_state(*st)
        s = make_schedules(96, active=1, break_on_tear=1, n_pull_end=120, n_griprest_end=180, n_total=400,
                           dx_pull=0.0012, dy_pull=0.0016)
        ex = b.run(s)
        assert (ex == 400).all()
        pos, prev, pin = b.get_state()
        assert all(np.array_equal(pos[0], pos[e]) and np.array_equal(prev[0], prev[e]) for e in range(96))
        outs.append((pos[0].copy(), prev[0].copy(), pin[0].copy()))
        b.close()
    assert all(np.array_equal(a, c) for a, c in zip(outs[0], outs[1]))


def test_async_run_and_device_schedule_and_obs(oracle_lib):
    """clothhip_run_async + clothhip_sync, clothhip_run_device_sched_async (schedule table already on the device,
    as after an RCCL broadcast) and clothhip_write_obs_f32_device give the same result as the synchronous path."""
    from gym_cloth_amd import ClothBatch, make_schedules
    from gym_cloth_amd._lib import SCHED_DTYPE
    from helpers import DeviceBuffer
    g, st = _pull_state(oracle_lib)
    E = 8
    s = make_schedules(E, active=1, break_on_tear=1, n_pull_end=40, n_griprest_end=60, n_total=100,
                       dx_pull=0.0012, dy_pull=0.0016)
    s["active"][3] = 0
    ref = ClothBatch(base_cfg("tier1", 1), n_envs=E, precision="f32"); ref.set_state(*st)
    ex_ref = ref.run(s); pos_ref = ref.positions()
    a = ClothBatch(base_cfg("tier1", 1), n_envs=E, precision="f32"); a.set_state(*st)
    a.run_async(s); ex_a = a.sync()
    assert np.array_equal(ex_a, ex_ref) and ex_ref[3] == 0 and np.array_equal(a.positions(), pos_ref)
    d = ClothBatch(base_cfg("tier1", 1), n_envs=E, precision="f32"); d.set_state(*st)
    assert s.dtype == SCHED_DTYPE and s.nbytes == 64 * E
    dev_s = DeviceBuffer(s.nbytes)                      # the schedule table as a collective would leave it: on the device
    dev_s.upload(np.frombuffer(s.tobytes(), dtype=np.uint8))
    d.run_device_sched_async(dev_s.ptr); ex_d = d.sync()
    assert np.array_equal(ex_d, ex_ref) and np.array_equal(d.positions(), pos_ref)
    obs = DeviceBuffer(E * 3 * 625 * 4)
    d.write_obs_f32_device(obs.ptr); d.sync(False)
    assert np.array_equal(obs.download(np.float32, (E, 625, 3)), pos_ref.astype(np.float32))
    dev_s.free(); obs.free()
    assert d.last_kernel_ms > 0
    for x in (ref, a, d):
        x.close()


def test_force_grab_and_no_grab_penalty(oracle_lib):
    """force_grab grows the radius by 0.02 until something is grabbed (cloth_env.py:434-444); without it an empty
    grab is a no-op action with the -0.01 penalty (cloth_env.py:490-493, :564-565)."""
    from gym_cloth_amd.envs import ClothVecEnv
    cfg = base_cfg("tier1", 5)
    act = np.array([[0.99, 0.99, -0.2, -0.2]])          # after the reset pulls there is usually no cloth under (0.995, 0.995)
    v = ClothVecEnv(cfg, n_envs=1, precision="f64"); v.seed(5); v.reset()
    pos = v.batch.positions()[0]
    d2 = (pos[:, 0] - 0.995) ** 2 + (pos[:, 1] - 0.995) ** 2
    if d2.min() < cfg["env"]["grip_radius"]:
        pytest.skip("cloth happens to lie under the corner for this seed")
    obs, rew, done, info = v.step(act)
    assert v.last_grabbed[0] == 0 and v.last_executed[0] == 0 and info["num_sim_steps"][0] == 0
    assert abs(rew[0] - (-0.01)) < 1e-12
    cfg["env"]["force_grab"] = True
    f = ClothVecEnv(cfg, n_envs=1, precision="f64"); f.seed(5); f.reset()
    assert np.array_equal(f.batch.positions()[0], pos)
    oc = oracle_lib.OracleCloth(oracle_lib.load_golden("g_traj_lift_pull_25.npz")["cfg"])
    p, q, pin = f.batch.get_state()
    oc.set_state(p[0], q[0], pin[0])
    r, n = cfg["env"]["grip_radius"], 0
    while n == 0:
        r += 0.02
        n = oc.grab_top(0.995, 0.995, r)
    f.step(act)
    assert f.last_grabbed[0] == n and f.last_executed[0] > 1000
    v.close(); f.close()


def test_partial_reset_leaves_other_envs_untouched():
    from gym_cloth_amd.envs import ClothVecEnv
    v = ClothVecEnv(base_cfg("tier1", 11), n_envs=4, precision="f32"); v.seed(11); v.reset()
    before = v.batch.get_state()
    mask = np.array([False, True, False, True])
    v.reset(mask)
    after = v.batch.get_state()
    for e in (0, 2):
        assert all(np.array_equal(before[k][e], after[k][e]) for k in range(3))
    for e in (1, 3):
        assert not np.array_equal(before[0][e], after[0][e]) and v.num_steps[e] == 0
    v.close()


def test_error_paths():
    from gym_cloth_amd import ClothBatch, make_schedules
    b = ClothBatch(base_cfg("tier1", 1), n_envs=2, precision="f32")
    with pytest.raises(ValueError):
        b.run(make_schedules(2, active=1, n_up_end=10, n_uprest_end=5, n_total=20))       # decreasing boundaries
    with pytest.raises(ValueError):
        b.run(make_schedules(3, active=1, n_total=1))                                       # wrong batch size
    with pytest.raises(ValueError):
        b.pin_points(0, [9999])
    with pytest.raises(ValueError):
        b.get_state(env0=1, n=5)
    b.close()
    with pytest.raises(ValueError):
        ClothBatch(base_cfg("tier1", 1), n_envs=0)


SMALL_CALLS = dict(T=2, R=1, px=8, fork=([0, 1], [3, 2]))            # (src envs, dst envs)
LARGE_CALLS = dict(T=6, R=2, px=16, fork=([0, 1, 2, 3], [0, 1, 2, 3]))


def _short_env(E, prec, n_side):
    """A vector env whose actions and resets are short (the buffers' sizes do not depend on how long an action runs)."""
    import bench
    from gym_cloth_amd.envs import ClothVecEnv
    cfg = bench.bench_cfg(n_side, 0.02)
    cfg["env"].update(iters_up_rest=10, iters_pull_max=60, iters_grip_rest=20, iters_rest=40)
    v = ClothVecEnv(cfg, n_envs=E, precision=prec, consume_domrand_draws=False)
    for e in range(E):
        v.np_randoms[e] = np.random.RandomState(1000 + e)
    return v


def _calls(va, vb, c, E):
    """Every call that sizes a buffer by its arguments, on handle va.batch (forks come from vb.batch): what the calls returned."""
    a, T, R = va.batch, c["T"], c["R"]
    a.fork_from(vb.batch, c["fork"][0], c["fork"][1])
    acts = np.stack([np.random.RandomState(2000 + e).uniform(-1, 1, size=(T, 4)) for e in range(E)], axis=1)
    done = np.array([1, 1, 0, 0], dtype=np.uint8)                    # two envs start with an in-kernel reset
    rec, rst, obs, robs = a.run_actions(va._episode_params(), T, np.zeros(E, dtype=np.int32), done, actions=acts,
                                        scripts=va._prepare_scripts(R), want_obs=True)
    assert (rec["reset_before"][0, :2] == 1).all() and robs[:2, 0].any()
    ran = rec["ran"] == 1
    obs = np.where(ran[..., None], obs, np.float32(0))               # (a slot that did not run leaves its observation unwritten)
    kw = dict(width=c["px"], height=c["px"])
    flags = (np.arange(T * E) % 3 != 0) & ran.reshape(-1)
    out = {"rec": rec, "rst": rst, "obs": obs, "robs": robs,
           "img_slots": a.render_obs("slots", valid=ran.reshape(-1), fmt="rgbd", **kw), "img_resets": a.render_obs("resets", fmt="depth", **kw),
           "img_host": a.render_obs("host", obs=obs.reshape(T * E, -1), valid=flags, swap_sides=np.arange(T * E) % 2, fmt="rgb", **kw)}
    assert out["img_slots"].shape == (T * E, c["px"], c["px"], 4) and out["img_slots"].any() and out["img_host"].any()
    out["pos"], out["prev"], out["pin"] = a.get_state()
    out["mat"], out["tear"], out["rest"] = a.get_material(), a.tear, a.get_rest()
    return out


def _round(prec, n_side, small_first):
    E = 4
    va, vb = _short_env(E, prec, n_side), _short_env(E, prec, n_side)
    pos = vb.batch.positions()
    pos[..., 2] += np.random.RandomState(7).uniform(0.0, 0.01, size=pos.shape[:2])   # the source of the forks: four different cloths
    vb.batch.set_state(pos, pos)
    m = vb.batch.get_material(2, 1); m["ks"] *= 0.5; m["damping"] *= 1.5
    vb.batch.set_material(m, env0=2)                                                  # ... one of another fabric
    if small_first:
        _calls(va, vb, SMALL_CALLS, E)
        m = va.batch.get_material(1, 1); m["density"] *= 2.0
        va.batch.set_material(m, env0=1)
    out = _calls(va, vb, LARGE_CALLS, E)
    va.close(); vb.close()
    return out


@pytest.mark.parametrize("prec,n_side", [("f32", 25), ("f64", 9)])
def test_buffers_regrow_and_handles_recycle(prec, n_side):
    """The staging of the episode launches, of render_obs and of the fork is sized by the call: small calls first (T = 2, one reset
    script, 8x8 pixels, a fork of 2 envs, a material on one env), then larger ones on the same handle (T = 6, two scripts, 16x16
    pixels, a fork of all 4 envs from a second handle) make every one of these buffers regrow. The records, observations,
    images and states of the larger calls equal, byte for byte, those of a fresh handle that only ever ran the larger calls;
    and closing both handles and running the whole sequence on new ones, five more times in one process, gives the same again."""
    fresh = _round(prec, n_side, small_first=False)
    first = _round(prec, n_side, small_first=True)
    assert fresh["rec"]["executed"].sum() > 0 and (fresh["mat"]["ks"][2] != fresh["mat"]["ks"][0])
    rounds = [first] + [_round(prec, n_side, small_first=True) for _ in range(5)]
    for r in rounds:
        assert set(r) == set(fresh)
        for k in fresh:
            assert fresh[k].dtype == r[k].dtype and fresh[k].tobytes() == r[k].tobytes(), k
