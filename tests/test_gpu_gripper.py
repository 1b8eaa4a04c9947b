"""GPU tests of the gripper kernel (k_grab: Gripper.grab_top / Gripper.grab, gripper.pyx:23-53) against the reference's
index sets on flat, lifted and FOLDED states (two layers under the gripper), in both precisions."""
import numpy as np
import pytest

from oracle import gripper_exact
from test_gpu_parity import cfg_from_golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("top", [True, False])
def test_grab_sets_match_reference(prec, top, oracle_lib):
    from gym_cloth_amd import ClothBatch
    g = oracle_lib.load_golden("g_gripper_25.npz")
    n = len(g["xy"])
    b = ClothBatch(cfg_from_golden(g), n_envs=n, precision=prec)
    b.set_state(g["pos"], g["pos"], np.zeros((n, 625), dtype=np.uint8))
    cnt = (b.grab_top if top else b.grab)(g["xy"])
    pin = b.get_state()[2].astype(bool)
    want = g["grab_top"] if top else g["grab"]
    assert any(len(w) > 5 for w in want), "the fixture must contain a multi-layer grab"
    radius, pos = g["cfg"]["grip_radius"], b.positions()
    lv = gripper_exact.levels(g["cfg"]["height"], g["cfg"]["thickness"])
    for q in range(n):
        got = set(np.nonzero(pin[q])[0].tolist())
        ref = set(want[q])
        if prec == "f64":
            assert got == ref and cnt[q] == len(ref), (q, sorted(got ^ ref))
        # both precisions: the exact reference (oracle/gripper_exact.py: every operation one rounding in the handle's type) on the positions
        # the handle holds -- in fp32 a point near a boundary may differ from the fp64 fixture, and the reference says which way
        exact = (gripper_exact.grab_top(pos[q], g["xy"][q], radius, lv, g["cfg"]["thickness"], prec)[0] if top
                 else gripper_exact.grab(pos[q], g["xy"][q], radius, prec))
        assert got == set(exact.tolist()) and cnt[q] == len(exact), (q, sorted(got ^ set(exact.tolist())))
    # grabbing again appends the same points a second time (multiplicity): release clears both
    cnt2 = (b.grab_top if top else b.grab)(g["xy"])
    assert np.array_equal(cnt2 > 0, cnt > 0)
    b.release()
    assert not b.get_state()[2].any()
    b.close()
