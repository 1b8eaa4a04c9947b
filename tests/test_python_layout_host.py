"""Host tests of where the Python side lives (no GPU): policies.py re-exports, under its old name, everything that moved to mlp.py,
references.py and trainers.py; mlp.py stands on numpy alone; no module of the package imports torch."""
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every name gym_cloth_amd.policies defined before the split, by the module that defines it now
HOMES = {
    "policies": ["_data_delta", "OracleCornerPolicy", "HighestPointPolicy", "RandomPolicy", "LookaheadPolicy", "MLPPolicy", "es_coefficients",
                 "MLPPopulation", "CEMPolicy"],
    "mlp": ["MLP_MAX_LAYERS", "MLP_MAX_WIDTH", "pack_mlp", "unpack_mlp", "pack_population", "population_stride"],
    "references": ["fit_reference", "value_fit_reference", "NEXT_TERMINAL", "NEXT_NONE", "_house_sum", "gae_reference", "exp_fixed_reference",
                   "ppo_loss_reference", "ppo_reference", "adam_reference", "sgd_reference", "philox4x32_10", "philox_eps", "_plan_clip",
                   "plan_sample_reference", "plan_score_reference", "plan_refit_reference", "cem_reference"],
    "trainers": ["MLPTrainer", "ValueTrainer", "ensemble_disagreement", "MLPEnsemble"],
}
MODULES = ["mlp", "references", "trainers", "policies", "batch", "batch_policy", "batch_fit", "batch_plan", "envs", "demos"]


@pytest.mark.parametrize("home", sorted(HOMES))
def test_policies_exports_every_old_name(home):
    policies = importlib.import_module("gym_cloth_amd.policies")
    mod = importlib.import_module("gym_cloth_amd." + home)
    for name in HOMES[home]:
        assert getattr(policies, name) is getattr(mod, name), name
        assert name in vars(mod), "%s is not %s's own" % (name, home)
    if home != "policies":          # defined there, not handed on from yet another module
        own = [n for n in HOMES[home] if callable(getattr(mod, n))]
        assert all(getattr(mod, n).__module__ == "gym_cloth_amd." + home for n in own)


def test_mlp_stands_alone_and_no_module_imports_torch():
    """mlp.py, loaded by its path outside the package (importing it as gym_cloth_amd.mlp would run the package's __init__ first),
    brings in no module of the package; then every module of the package is imported and torch is not among sys.modules -- the idiom
    of test_dist_sockets.test_package_does_not_import_torch, over the modules of the Python side."""
    code = ("import sys, importlib.util as u; sys.path.insert(0, %r); "
            "s = u.spec_from_file_location('standalone_mlp', %r); m = u.module_from_spec(s); s.loader.exec_module(m); "
            "own = [k for k in sys.modules if k.split('.')[0] == 'gym_cloth_amd']; assert not own, own; "
            "assert m.pack_mlp and m.mlp_forward and m.mlp_backward; "
            "import importlib; [importlib.import_module('gym_cloth_amd.' + k) for k in %r]; "
            "assert 'torch' not in sys.modules, 'torch was imported'"
            % (ROOT, os.path.join(ROOT, "gym_cloth_amd", "mlp.py"), MODULES))
    subprocess.check_call([sys.executable, "-c", code])
