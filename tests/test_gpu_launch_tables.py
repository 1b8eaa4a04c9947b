"""GPU test of which tables the last episode launch left readable (clothhip.h: clothhip_render_obs, ROWS NAMED BY WHERE THEY LIE ON THE
DEVICE, clothhip_run_actions_labels): one handle walked through the states a launch can leave it in, and in each state the status code of
the five entries that read those tables, against a table written out from the header's words."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_env import base_cfg

pytestmark = pytest.mark.gpu

E, T, R, W = 2, 1, 2, 8       # cloths, action slots, reset scripts per env, image side


def test_readers_of_the_launch_tables_state_by_state():
    """States in order: no launch yet; a launch without want_obs; want_obs = 1 with scripts, downloaded; the same with 2 (kept); a _begin
    in flight (armed, both tables kept); after its _end; a _begin refused by its argument checks (the tables stay); a _begin refused after
    the line from which the tables may be overwritten (they are gone, the labels stay); an armed launch with the slot table alone; an
    unarmed one. Per state the codes of render_obs(SLOTS), render_obs(RESETS), fit_hold of SLOTS rows, fit_data_append_launch of one
    (SLOTS, 0, label 0) entry and run_actions_labels. Where a table is readable its row count is T * E (slots) or E * n_scripts (resets):
    render_obs refuses any other n, the row sources refuse the first row behind it."""
    from gym_cloth_amd import _lib
    from gym_cloth_amd.envs import ClothVecEnv
    OK, EINVAL, ESTATE = _lib.OK, _lib.EINVAL, _lib.ESTATE
    SLOTS, RESETS = _lib.FIT_SRC_SLOTS, _lib.FIT_SRC_RESETS
    v = ClothVecEnv(base_cfg("tier1", 1337), n_envs=E, precision="f32", consume_domrand_draws=False)
    v.seed([1337 + e for e in range(E)])
    v.reset()
    L, h, P = v.batch._L, v.batch._h, v.P
    ep = v._episode_params()
    rp = v.batch.render_params(width=W, height=W)
    img = np.zeros((E * R + 2, W, W, 4), dtype=np.uint8)
    off = np.zeros(E * R + 2, dtype=np.uint8)             # valid[n] == 0: a reset row no script filled is not rasterised
    acts = np.zeros((T, E, 4))
    scripts = np.zeros((E, R), dtype=_lib.RESET_SCRIPT_DTYPE)      # void scripts: a reset source that resets nothing
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def begin(policy=_lib.POLICY_TABLE, with_scripts=False, want_resets=0, want_obs=0, want_reset_obs=0):
        nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
        return L.clothhip_run_actions_begin(h, C.byref(ep), T, policy, vp(acts), 0, None, vp(scripts) if with_scripts else None,
                                            R if with_scripts else 0, _lib.i32p(nsteps), _lib.u8p(done), None, 0, 0, want_resets, want_obs,
                                            want_reset_obs, 0.0)

    def end(obs=False, robs=False):
        nsteps, done = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
        rec = np.zeros((T, E), dtype=_lib.STEP_RECORD_DTYPE)
        o = np.zeros((T, E, 3 * P), dtype=np.float32) if obs else None
        ro = np.zeros((E, R, 3 * P), dtype=np.float32) if robs else None
        assert L.clothhip_run_actions_end(h, _lib.i32p(nsteps), _lib.u8p(done), vp(rec), None, vp(o), vp(ro), None) == OK
        return rec

    def render(source, n):
        return L.clothhip_render_obs(h, C.byref(rp), source, None, n, _lib.u8p(off), None, _lib.IMG_RGBD, _lib.u8p(img), None)

    def hold(source, rows):
        src = np.array([[source, r] for r in rows], dtype=np.int32)
        return L.clothhip_fit_hold(h, _lib.i32p(src))

    def append(source=SLOTS, row=0, label=0):
        return L.clothhip_fit_data_append_launch(h, _lib.i32p(np.array([[source, row, label]], dtype=np.int32)), 1)

    def labels():
        return L.clothhip_run_actions_labels(h, _lib.dp(np.zeros((T, E, 4))), None)

    def state(name, want):
        """want: the codes of (render SLOTS, render RESETS, hold SLOTS rows, append_launch, labels), the counts being those of the tables"""
        got = (render(_lib.OBS_SLOTS, T * E), render(_lib.OBS_RESETS, E * R), hold(SLOTS, range(E)), append(), labels())
        print(name, got)
        assert got == want, (name, got, want)
        if want[0] == OK:
            assert [render(_lib.OBS_SLOTS, n) for n in (T * E - 1, T * E + 1)] == [EINVAL, EINVAL], name
            assert hold(SLOTS, (T * E - 1, T * E)) == EINVAL and hold(SLOTS, (-1, 0)) == EINVAL, name
        if want[1] == OK:
            assert [render(_lib.OBS_RESETS, n) for n in (E * R - 1, E * R + 1, T * E)] == [EINVAL, EINVAL, EINVAL], name
            assert hold(RESETS, (E * R - 2, E * R - 1)) == OK and hold(RESETS, (0, E * R)) == EINVAL, name
        if want[3] == OK:
            assert append(SLOTS, T * E - 1, T * E) == EINVAL and append(SLOTS, T * E, 0) == EINVAL, name

    none = (ESTATE,) * 5
    state("1 no launch yet", none)
    assert begin() == OK
    end()
    state("2 a launch without want_obs", none)
    assert begin(with_scripts=True, want_obs=1, want_reset_obs=1) == OK
    end(obs=True, robs=True)
    state("3 want_obs = 1 with scripts, downloaded", (OK, OK, OK, ESTATE, ESTATE))
    assert begin(with_scripts=True, want_obs=2, want_reset_obs=2) == OK
    end()
    state("4 want_obs = 2 with scripts, kept", (OK, OK, OK, ESTATE, ESTATE))
    assert L.clothhip_run_actions_expert(h, _lib.POLICY_ORACLE_CORNER, T, None, None) == OK
    assert begin(with_scripts=True, want_obs=2, want_reset_obs=2) == OK
    state("5 a _begin in flight", none)
    assert end()["ran"].all()                              # (so every label is a finite action: the append below may succeed)
    state("6 after _end of an armed launch", (OK,) * 5)
    assert begin(policy=7) == EINVAL                       # an unknown policy: refused before anything is touched
    state("7 after a _begin refused by its argument checks", (OK,) * 5)
    assert begin(want_resets=1) == EINVAL                  # reset outputs without a reset source: refused when the tables may be gone
    state("8 after a _begin refused past the tables' invalidation", (ESTATE, ESTATE, ESTATE, ESTATE, OK))
    assert L.clothhip_run_actions_expert(h, _lib.POLICY_ORACLE_CORNER, T, None, None) == OK
    assert begin(want_obs=2) == OK
    assert end()["ran"].all()
    state("9a an armed launch with the slot table alone", (OK, ESTATE, OK, OK, OK))
    assert begin(want_obs=1) == OK
    end(obs=True)
    state("9b an unarmed launch after it", (OK, ESTATE, OK, ESTATE, ESTATE))
    v.close()
