"""ctypes binding of libclothhip.so (include/clothhip.h).

The HIP library is the ONLY compute path of this package: there is no CPU fallback. If the shared object
is missing, or no HIP device is visible, the calls below raise -- loudly -- instead of degrading.
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CLOTHHIP_LIB: another build of the same library (A/B kernel comparisons); it must export the same C ABI
LIB_PATH = os.environ.get("CLOTHHIP_LIB") or os.path.join(_HERE, "libclothhip.so")

F64, F32 = 0, 1
REST_SHARED, KEEP_TEAR = 1, 2           # clothhip_set_state flags
FORK_STATE_ONLY = 1                     # clothhip_fork flags
ABI_VERSION = 7

OK, EINVAL, ENODEV, EHIP, ENOMEM, ESTATE = 0, -1, -2, -3, -4, -5


class ClothHipError(RuntimeError):
    """A HIP runtime failure or a missing device/library (no reference counterpart)."""


class ClothParams(C.Structure):
    _fields_ = [("n_side", C.c_int32), ("frames_per_sec", C.c_int32), ("simulation_steps", C.c_int32),
                ("_pad", C.c_int32), ("width", C.c_double), ("height", C.c_double),
                ("density", C.c_double), ("ks", C.c_double), ("damping", C.c_double),
                ("thickness", C.c_double), ("plane_friction", C.c_double), ("tear_thresh", C.c_double),
                ("gravity", C.c_double), ("minimum_z", C.c_double), ("grip_radius", C.c_double)]


class ClothMaterial(C.Structure):
    """The per-env material (clothhip_set_material): the cfg quantities Cloth.update() reads anew on every call (cloth.pyx:175-186)."""
    _fields_ = [("density", C.c_double), ("ks", C.c_double), ("damping", C.c_double), ("plane_friction", C.c_double),
                ("tear_thresh", C.c_double), ("gravity", C.c_double)]


MATERIAL_FIELDS = ("density", "ks", "damping", "plane_friction", "tear_thresh", "gravity")
MATERIAL_DTYPE = np.dtype([(k, "<f8") for k in MATERIAL_FIELDS])
assert MATERIAL_DTYPE.itemsize == C.sizeof(ClothMaterial) == 48


class ClothSchedule(C.Structure):
    _fields_ = [("n_up_end", C.c_int32), ("n_uprest_end", C.c_int32), ("n_pull_end", C.c_int32),
                ("n_griprest_end", C.c_int32), ("n_total", C.c_int32), ("break_on_tear", C.c_int32),
                ("active", C.c_int32), ("_pad", C.c_int32), ("dz_up", C.c_double),
                ("dx_pull", C.c_double), ("dy_pull", C.c_double), ("dz_pull", C.c_double)]


SCHED_DTYPE = np.dtype([("n_up_end", "<i4"), ("n_uprest_end", "<i4"), ("n_pull_end", "<i4"),
                        ("n_griprest_end", "<i4"), ("n_total", "<i4"), ("break_on_tear", "<i4"),
                        ("active", "<i4"), ("_pad", "<i4"), ("dz_up", "<f8"), ("dx_pull", "<f8"),
                        ("dy_pull", "<f8"), ("dz_pull", "<f8")])
assert SCHED_DTYPE.itemsize == C.sizeof(ClothSchedule) == 64



class ClothEpisodeParams(C.Structure):
    _fields_ = [("max_actions", C.c_int32), ("iters_up_rest", C.c_int32), ("iters_grip_rest", C.c_int32),
                ("iters_rest", C.c_int32), ("clip_act_space", C.c_int32), ("force_grab", C.c_int32),
                ("_pad", C.c_int32 * 2), ("iters_up", C.c_double), ("reduce_factor", C.c_double),
                ("grip_radius", C.c_double), ("radius_inc", C.c_double), ("dz_up", C.c_double),
                ("act_low", C.c_double * 4), ("act_high", C.c_double * 4), ("coverage_done", C.c_double)]


class ClothRenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("cam_pos", C.c_float * 3), ("world_to_cam", C.c_float * 9),
                ("lens_mm", C.c_float), ("sensor_mm", C.c_float), ("front", C.c_float * 3), ("back", C.c_float * 3),
                ("background", C.c_float * 3), ("light_dir", C.c_float * 3), ("ambient", C.c_float), ("energy", C.c_float)]


IMG_RGB, IMG_DEPTH, IMG_RGBD = 0, 1, 2                                  # clothhip_render_obs formats ...
IMG_FORMATS = {'rgb': IMG_RGB, 'depth': IMG_DEPTH, 'rgbd': IMG_RGBD}
OBS_STATE, OBS_SLOTS, OBS_RESETS, OBS_HOST = 0, 1, 2, 3                 # ... and sources
OBS_SOURCES = {'state': OBS_STATE, 'slots': OBS_SLOTS, 'resets': OBS_RESETS, 'host': OBS_HOST}

POLICY_TABLE, POLICY_ORACLE_CORNER, POLICY_HIGHEST_POINT, POLICY_MLP = 0, 1, 2, 3
EXPERTS = {'oracle_corner': POLICY_ORACLE_CORNER, 'highest_point': POLICY_HIGHEST_POINT}   # clothhip_run_actions_expert / clothhip_policy_label
MLP_MAX_LAYERS, MLP_MAX_WIDTH = 4, 256   # clothhip_set_policy_mlp (csrc/cloth_policy_mlp.hpp)
POP_ANTITHETIC = 1                       # clothhip_policy_population_perturb flags (csrc/cloth_policy_population.hpp)
POP_ROW_ALIGN, POP_MAX_G = 64, 65534     # floats a population's row stride is rounded up to; the most perturbations of one call
MT_WORDS = 626                      # per-env RandomState image: key[624], pos, pad (csrc/cloth_rng.hpp)

RESET_PULL_DTYPE = np.dtype([("point", "<i4"), ("need_coverage", "<i4"), ("x", "<f8"), ("y", "<f8"), ("dx", "<f8"),
                             ("dy", "<f8"), ("iters_up", "<f8"), ("coverage_min", "<f8")])
RESET_SCRIPT_DTYPE = np.dtype([("valid", "<i4"), ("n_pulls", "<i4"), ("settle_after", "<i4"), ("_pad", "<i4"),
                               ("pull", RESET_PULL_DTYPE, (3,))])
STEP_RECORD_DTYPE = np.dtype([("action", "<f8", (4,)), ("coverage", "<f8"), ("variance_inv", "<f8"),
                              ("executed", "<i4"), ("n_grabbed", "<i4"), ("iters_pull", "<i4"),
                              ("n_below_half_thickness", "<i4"), ("ran", "u1"), ("oob", "u1"), ("tear", "u1"),
                              ("done", "u1"), ("reset_before", "u1"), ("_pad", "u1", (3,))])
RESET_RECORD_DTYPE = np.dtype([("consumed", "<i4"), ("pulls_run", "<i4"), ("executed", "<i4", (3,)),
                               ("settle_executed", "<i4"), ("tear", "<i4"), ("init_side", "<i4"),
                               ("start_coverage", "<f8"), ("start_variance_inv", "<f8"), ("action", "<f8", (3, 4))])
assert RESET_PULL_DTYPE.itemsize == 56 and RESET_SCRIPT_DTYPE.itemsize == 184
assert STEP_RECORD_DTYPE.itemsize == 72 and RESET_RECORD_DTYPE.itemsize == 144
assert C.sizeof(ClothEpisodeParams) == 144

# ClothBatch._launch, the last episode launch of a batch: T slots and R reset scripts per env (the shapes of the tables it left on the
# device: render_obs('slots' / 'resets'), run_actions_labels), and between run_actions_begin and run_actions_end what the second half needs
# (here, beside the records' dtypes, because batch.py's launches and batch_plan.py's planner both write it)
LastLaunch = namedtuple("LastLaunch", "T R pending")
PendingLaunch = namedtuple("PendingLaunch", "num_steps done have_rst have_obs have_robs rng_states")


class ClothFitParams(C.Structure):
    """clothhip_policy_fit's optimizer: six floats, `optimizer` one of FIT_OPTIMIZERS' codes."""
    _fields_ = [("optimizer", C.c_float), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("momentum", C.c_float)]


FIT_ADAM, FIT_SGD = 0, 1
FIT_OPTIMIZERS = {'adam': FIT_ADAM, 'sgd': FIT_SGD}
FIT_MAX_BATCH = 4096                # CLOTHHIP_FIT_MAX_BATCH: the most rows of one minibatch
FIT_MAX_MEMBER_ROWS = 65536         # CLOTHHIP_FIT_MAX_MEMBER_ROWS: the most members x rows of one grouped call (clothhip_policy_fit_members)
FIT_SRC_SLOTS, FIT_SRC_RESETS, FIT_SRC_HELD = 0, 1, 2   # CLOTHHIP_FIT_SRC_*: where a row of clothhip_fit_hold / _append_launch lies
FIT_LABEL_EXPERT, FIT_LABEL_ACTION = 0, 1               # CLOTHHIP_FIT_LABEL_*: where clothhip_fit_data_append_launch_ex takes a row's label from
FIT_LABELS = {'expert': FIT_LABEL_EXPERT, 'action': FIT_LABEL_ACTION}
FIT_LABEL_ZERO = 3                                      # ... or (0, 0, 0, 0) from no table at all: how a leaf of the actor-critic is appended
FIT_LABEL_ACTION_EXPERT = 4                             # ... or the executed action as the label AND the armed expert's into the expert column (DDPG from demonstrations)
FIT_NO_EXPERT_BITS = 0x7fc00000                         # the expert column's fill: component 0 a NaN means the row has no expert action
FIT_NEXT_TERMINAL, FIT_NEXT_NONE = -1, -2               # CLOTHHIP_FIT_NEXT_*: a row's successor column besides a dataset index
GAE_WRITE_WEIGHTS, GAE_NORMALIZE = 1, 2                 # CLOTHHIP_GAE_*: clothhip_fit_data_gae's flags
assert C.sizeof(ClothFitParams) == 24


class ClothGaeParams(C.Structure):
    """clothhip_fit_data_gae's constants: the discount, GAE's lambda, the scale of the written weights, GAE_* flags."""
    _fields_ = [("gamma", C.c_double), ("lambda_", C.c_double), ("w_scale", C.c_float), ("flags", C.c_int32)]


assert C.sizeof(ClothGaeParams) == 24


class ClothPpoParams(C.Structure):
    """clothhip_policy_fit_ppo*'s constants: the standard deviation of the fixed-sigma Gaussian policy, the clip range epsilon."""
    _fields_ = [("sigma", C.c_double), ("clip", C.c_double)]


PPO_STATS = 3                       # CLOTHHIP_PPO_STATS: loss, clip_fraction, kl
assert C.sizeof(ClothPpoParams) == 16


class ClothPpoSigmaParams(C.Structure):
    """clothhip_policy_fit_ppo_sigma*'s constants: the clip range epsilon, the coefficient of the entropy bonus (sigma is the handle's head)."""
    _fields_ = [("clip", C.c_double), ("ent_coef", C.c_double)]


PPO_SIGMA_STATS = 4                 # CLOTHHIP_PPO_SIGMA_STATS: loss, clip_fraction, kl, entropy
assert C.sizeof(ClothPpoSigmaParams) == 16


class ClothDdpgParams(C.Structure):
    """The DDPG entries' constants: the discount, the soft-update rate of the targets, the action bound of the clamp (inf: none), flags (0)."""
    _fields_ = [("gamma", C.c_double), ("tau", C.c_double), ("act_bound", C.c_float), ("flags", C.c_int32)]


Q_STATS, DPG_STATS, DDPG_STATS = 3, 3, 6      # CLOTHHIP_*_STATS: loss, mean q, mean y; -mean q, gated fraction, mean |dL/da|; both
assert C.sizeof(ClothDdpgParams) == 24


class ClothBcParams(C.Structure):
    """The constants of DDPG from demonstrations: the coefficients of the policy gradient and of the behaviour-cloning term, BC_* flags, 0."""
    _fields_ = [("q_coef", C.c_float), ("bc_coef", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


BC_QFILTER = 1                                # CLOTHHIP_BC_QFILTER: the cloning term counts only where the critic rates the expert's action above the policy's
DPG_BC_STATS, DDPG_BC_STATS = 6, 9            # CLOTHHIP_DPG_BC_STATS: DPG's three, then bc_loss, labelled share, filter-pass share; the critic's three in front
assert C.sizeof(ClothBcParams) == 16


class ClothPlanParams(C.Structure):
    """clothhip_plan_cem's planner constants (clothhip.h: PLAN ACTIONS ON THE DEVICE)."""
    _fields_ = [("horizon", C.c_int32), ("n_candidates", C.c_int32), ("n_elite", C.c_int32), ("n_iters", C.c_int32),
                ("seed", C.c_uint64), ("iter0", C.c_uint32), ("_pad", C.c_int32), ("alpha", C.c_double), ("penalty", C.c_double),
                ("min_std", C.c_double * 4)]


PLAN_MAX_H, PLAN_MAX_K = 8, 1024    # csrc/cloth_plan.hpp: the longest horizon, the most candidates per env
assert C.sizeof(ClothPlanParams) == 80

# every symbol include/clothhip.h declares: (name, restype, argtypes)
_vp, _dp, _u8p, _i32p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
_PP = C.POINTER(ClothParams)
SYMBOLS = [
    ("clothhip_last_error", C.c_char_p, []),
    ("clothhip_abi_version", C.c_int, []),
    ("clothhip_device_count", C.c_int, []),
    ("clothhip_create", C.c_int, [_PP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    ("clothhip_destroy", C.c_int, [_vp]),
    ("clothhip_num_points", C.c_int, [_vp]),
    ("clothhip_num_springs", C.c_int, [_vp]),
    ("clothhip_num_envs", C.c_int, [_vp]),
    ("clothhip_precision", C.c_int, [_vp]),
    ("clothhip_init_grid", C.c_int, [_PP, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    ("clothhip_spring_topology", C.c_int, [_PP, _i32p, _i32p, _u8p]),
    ("clothhip_set_state", C.c_int, [_vp, C.c_int32, C.c_int32, _dp, _dp, _u8p, _dp, C.c_int32]),
    ("clothhip_get_state", C.c_int, [_vp, C.c_int32, C.c_int32, _dp, _dp, _u8p]),
    ("clothhip_get_rest", C.c_int, [_vp, C.c_int32, C.c_int32, _dp]),
    ("clothhip_reset_flat", C.c_int, [_vp, _u8p]),
    ("clothhip_get_tear", C.c_int, [_vp, _u8p]),
    ("clothhip_set_tear", C.c_int, [_vp, _u8p]),
    ("clothhip_grab_top", C.c_int, [_vp, _dp, _dp, _u8p, _i32p]),
    ("clothhip_grab", C.c_int, [_vp, _dp, _dp, _u8p, _i32p]),
    ("clothhip_release", C.c_int, [_vp, _u8p]),
    ("clothhip_pin_points", C.c_int, [_vp, C.c_int32, _i32p, C.c_int32]),
    ("clothhip_run", C.c_int, [_vp, _vp, _i32p]),
    ("clothhip_run_async", C.c_int, [_vp, _vp]),
    ("clothhip_sync", C.c_int, [_vp, _i32p]),
    ("clothhip_fused_supported", C.c_int, [_vp]),
    ("clothhip_run_actions_begin", C.c_int, [_vp, C.POINTER(ClothEpisodeParams), C.c_int32, C.c_int32, _vp, C.c_int32, _i32p,
                                             _vp, C.c_int32, _i32p, _u8p, _vp, C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_double]),
    ("clothhip_run_actions_end", C.c_int, [_vp, _i32p, _u8p, _vp, _vp, _vp, _vp, _vp]),
    ("clothhip_run_actions_op_ticks", C.c_int, [_vp, _vp]),
    ("clothhip_run_actions_summary", C.c_int, [_vp, _dp, C.POINTER(_vp)]),
    ("clothhip_run_actions", C.c_int, [_vp, C.POINTER(ClothEpisodeParams), C.c_int32, C.c_int32, _vp, C.c_int32, _i32p, _vp,
                                       C.c_int32, _i32p, _u8p, _vp, _vp, _vp, _vp, C.c_double]),
    ("clothhip_set_policy_mlp", C.c_int, [_vp, C.c_int32, _i32p, C.POINTER(C.c_float), C.c_size_t]),
    ("clothhip_policy_eval", C.c_int, [_vp, C.POINTER(C.c_float), C.c_int64, _dp]),
    ("clothhip_set_policy_population", C.c_int, [_vp, C.c_int32, _i32p, C.POINTER(C.c_float), C.c_int32, _i32p]),
    ("clothhip_set_policy_members", C.c_int, [_vp, _i32p]),
    ("clothhip_get_policy_mlp", C.c_int, [_vp, C.c_int64, C.POINTER(C.c_float), C.c_size_t]),
    ("clothhip_policy_eval_members", C.c_int, [_vp, C.POINTER(C.c_float), C.c_int64, _i32p, _dp]),
    ("clothhip_policy_population_perturb", C.c_int, [_vp, C.c_int32, _i32p, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_uint64,
                                                     C.c_int32, _i32p]),
    ("clothhip_policy_population_combine", C.c_int, [_vp, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float)]),
    ("clothhip_run_actions_expert", C.c_int, [_vp, C.c_int32, C.c_int32, _u8p, _i32p]),
    ("clothhip_run_actions_labels", C.c_int, [_vp, _dp, C.POINTER(_vp)]),
    ("clothhip_policy_label", C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int64, _i32p, _i32p, _dp]),
    ("clothhip_fit_data_append", C.c_int, [_vp, C.POINTER(C.c_float), _dp, C.c_int64]),
    ("clothhip_fit_data_clear", C.c_int, [_vp]),
    ("clothhip_fit_data_size", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("clothhip_fit_data_get", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("clothhip_fit_data_set_weights", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_fit_data_get_weights", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_fit_data_append_weighted", C.c_int, [_vp, C.POINTER(C.c_float), _dp, C.POINTER(C.c_float), C.c_int64]),
    ("clothhip_fit_hold", C.c_int, [_vp, _i32p]),
    ("clothhip_fit_data_append_launch", C.c_int, [_vp, _i32p, C.c_int64]),
    ("clothhip_fit_data_append_launch_ex", C.c_int, [_vp, _i32p, C.c_int64, C.c_int32, C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_predict", C.c_int, [_vp, _i32p, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_predict_members", C.c_int, [_vp, _i32p, C.c_int32, _i32p, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_grad", C.c_int, [_vp, _i32p, C.c_int32, C.POINTER(C.c_float), _dp]),
    ("clothhip_policy_fit_loss", C.c_int, [_vp, _i32p, C.c_int64, _dp]),
    ("clothhip_policy_fit", C.c_int, [_vp, C.POINTER(ClothFitParams), _i32p, C.c_int32, C.c_int32, _dp]),
    ("clothhip_policy_fit_reset", C.c_int, [_vp]),
    ("clothhip_policy_fit_grad_members", C.c_int, [_vp, _i32p, C.c_int32, _i32p, C.c_int32, C.POINTER(C.c_float), _dp]),
    ("clothhip_policy_fit_members", C.c_int, [_vp, C.POINTER(ClothFitParams), _i32p, C.c_int32, _i32p, C.c_int32, C.c_int32, _dp]),
    ("clothhip_policy_fit_reset_members", C.c_int, [_vp, _i32p, C.c_int32]),
    ("clothhip_set_value_mlp", C.c_int, [_vp, C.c_int32, _i32p, C.POINTER(C.c_float), C.c_size_t]),
    ("clothhip_get_value_mlp", C.c_int, [_vp, C.POINTER(C.c_float), C.c_size_t]),
    ("clothhip_fit_data_set_transitions", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float), _i32p]),
    ("clothhip_fit_data_get_transitions", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float), _i32p]),
    ("clothhip_fit_data_set_returns", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_fit_data_get_returns", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_value_fit_grad", C.c_int, [_vp, _i32p, C.c_int32, C.POINTER(C.c_float), _dp]),
    ("clothhip_value_fit", C.c_int, [_vp, C.POINTER(ClothFitParams), _i32p, C.c_int32, C.c_int32, _dp]),
    ("clothhip_value_fit_reset", C.c_int, [_vp]),
    ("clothhip_value_predict", C.c_int, [_vp, _i32p, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_fit_data_gae", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(ClothGaeParams), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("clothhip_fit_data_snapshot_policy", C.c_int, [_vp, C.c_int64, C.c_int64]),
    ("clothhip_fit_data_set_old_means", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_fit_data_get_old_means", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_ppo_grad", C.c_int, [_vp, C.POINTER(ClothPpoParams), _i32p, C.c_int32, C.POINTER(C.c_float), _dp, C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_ppo", C.c_int, [_vp, C.POINTER(ClothFitParams), C.POINTER(ClothPpoParams), _i32p, C.c_int32, C.c_int32, _dp]),
    ("clothhip_set_policy_log_sigma", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("clothhip_get_policy_log_sigma", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("clothhip_fit_data_set_old_log_sigma", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_fit_data_get_old_log_sigma", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_ppo_sigma_grad", C.c_int, [_vp, C.POINTER(ClothPpoSigmaParams), _i32p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), _dp,
                                                     C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_ppo_sigma", C.c_int, [_vp, C.POINTER(ClothFitParams), C.POINTER(ClothPpoSigmaParams), _i32p, C.c_int32, C.c_int32, _dp,
                                                C.POINTER(C.c_float)]),
    ("clothhip_fit_data_snapshot_policy_members", C.c_int, [_vp, C.c_int64, C.c_int64, _i32p]),
    ("clothhip_policy_fit_ppo_grad_members", C.c_int, [_vp, C.POINTER(ClothPpoParams), _i32p, C.c_int32, _i32p, C.c_int32, C.POINTER(C.c_float), _dp,
                                                       C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_ppo_members", C.c_int, [_vp, C.POINTER(ClothFitParams), C.POINTER(ClothPpoParams), _i32p, C.c_int32, _i32p, C.c_int32, C.c_int32,
                                                  _dp]),
    ("clothhip_policy_noise_fill", C.c_int, [_vp, C.c_uint64, C.c_int32, C.POINTER(C.c_int64), _dp, C.c_int32, C.POINTER(_vp)]),
    ("clothhip_policy_noise_get", C.c_int, [_vp, C.c_int32, _dp]),
    ("clothhip_set_q_mlp", C.c_int, [_vp, C.c_int32, _i32p, C.POINTER(C.c_float), C.c_size_t]),
    ("clothhip_get_q_mlp", C.c_int, [_vp, C.POINTER(C.c_float), C.c_size_t]),
    ("clothhip_ddpg_sync_targets", C.c_int, [_vp]),
    ("clothhip_ddpg_get_targets", C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("clothhip_ddpg_set_targets", C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("clothhip_q_fit_grad", C.c_int, [_vp, C.POINTER(ClothDdpgParams), _i32p, C.c_int32, C.POINTER(C.c_float), _dp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("clothhip_q_fit", C.c_int, [_vp, C.POINTER(ClothFitParams), C.POINTER(ClothDdpgParams), _i32p, C.c_int32, C.c_int32, _dp]),
    ("clothhip_q_fit_reset", C.c_int, [_vp]),
    ("clothhip_policy_fit_dpg_grad", C.c_int, [_vp, C.POINTER(ClothDdpgParams), _i32p, C.c_int32, C.POINTER(C.c_float), _dp, C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_dpg", C.c_int, [_vp, C.POINTER(ClothFitParams), C.POINTER(ClothDdpgParams), _i32p, C.c_int32, C.c_int32, _dp]),
    ("clothhip_ddpg_polyak", C.c_int, [_vp, C.c_double]),
    ("clothhip_ddpg_last_tables", C.c_int, [_vp, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("clothhip_ddpg_fit", C.c_int, [_vp, C.POINTER(ClothFitParams), C.POINTER(ClothFitParams), C.POINTER(ClothDdpgParams), _i32p, C.c_int32, C.c_int32, _dp]),
    ("clothhip_fit_data_set_expert", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_fit_data_get_expert", C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_dpg_bc_grad", C.c_int, [_vp, C.POINTER(ClothDdpgParams), C.POINTER(ClothBcParams), _i32p, C.c_int32, C.POINTER(C.c_float), _dp,
                                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("clothhip_policy_fit_dpg_bc", C.c_int, [_vp, C.POINTER(ClothFitParams), C.POINTER(ClothDdpgParams), C.POINTER(ClothBcParams), _i32p, C.c_int32, C.c_int32, _dp]),
    ("clothhip_ddpg_fit_bc", C.c_int, [_vp, C.POINTER(ClothFitParams), C.POINTER(ClothFitParams), C.POINTER(ClothDdpgParams), C.POINTER(ClothBcParams), _i32p, C.c_int32,
                                       C.c_int32, _dp]),
    ("clothhip_plan_cem", C.c_int, [_vp, _vp, C.POINTER(ClothEpisodeParams), C.POINTER(ClothPlanParams), _i32p, _u8p, _dp, _dp, _dp, _dp,
                                    _dp, _dp]),
    ("clothhip_plan_sample", C.c_int, [_vp, C.POINTER(ClothPlanParams), _dp, _dp, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    ("clothhip_plan_refit", C.c_int, [_vp, C.POINTER(ClothPlanParams), C.c_int32, _dp, _dp, _u8p, _dp, _dp, _u8p, _i32p]),
    ("clothhip_update", C.c_int, [_vp, C.c_int32, _dp]),
    ("clothhip_metrics", C.c_int, [_vp, _dp, _dp, _u8p, _u8p]),
    ("clothhip_metrics_ex", C.c_int, [_vp, _dp, _dp, _u8p, _u8p, _i32p]),
    ("clothhip_hull_area", C.c_double, [_dp, C.c_int32]),
    ("clothhip_write_obs_f32_device", C.c_int, [_vp, _vp]),
    ("clothhip_run_device_sched_async", C.c_int, [_vp, _vp]),
    ("clothhip_render", C.c_int, [_vp, C.POINTER(ClothRenderParams), _u8p, _u8p, C.POINTER(C.c_float)]),
    ("clothhip_render_obs", C.c_int, [_vp, C.POINTER(ClothRenderParams), C.c_int32, C.POINTER(C.c_float), C.c_int64, _u8p, _u8p,
                                      C.c_int32, _u8p, _vp]),
    ("clothhip_device_alloc", C.c_int, [_vp, C.c_uint64, C.POINTER(_vp)]),
    ("clothhip_device_free", C.c_int, [_vp, _vp]),
    ("clothhip_device_upload", C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    ("clothhip_device_download", C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    ("clothhip_stream", _vp, [_vp]),
    ("clothhip_last_kernel_ms", C.c_double, [_vp]),
    ("clothhip_debug_stats", C.c_int, [_vp, _i32p]),
    ("clothhip_last_variant", C.c_int, [_vp, _i32p]),
    ("clothhip_last_dispatches", C.c_int, [_vp, _i32p]),
    ("clothhip_last_specialised", C.c_int, [_vp, _i32p]),
    ("clothhip_set_relaxed_order", C.c_int, [_vp, C.c_int32]),
    ("clothhip_set_material", C.c_int, [_vp, C.c_int32, C.c_int32, _vp]),
    ("clothhip_get_material", C.c_int, [_vp, C.c_int32, C.c_int32, _vp]),
    ("clothhip_fork", C.c_int, [_vp, _i32p, _vp, _i32p, C.c_int32, C.c_int32]),
    ("clothhip_in_flight", C.c_int, [_vp, _u8p]),
    ("clothhip_get_pin_counts", C.c_int, [_vp, C.c_int32, C.c_int32, _u8p]),
    ("clothhip_selftest_material", C.c_int, [_PP, C.POINTER(ClothMaterial), C.c_int32, _dp]),
    ("clothhip_selftest_windows", C.c_int, [_PP, _i32p, _i32p, _i32p, _i32p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_int32]),
    ("clothhip_selftest_layout", C.c_int, [_PP, C.c_int32, C.c_int32, C.c_int32, _i32p, C.c_int32]),
    ("clothhip_selftest_rng", C.c_int, [_vp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, _dp]),
    ("clothhip_selftest_depth8", C.c_int, [C.POINTER(C.c_float), C.c_int32, C.c_int64, _u8p]),
    ("clothhip_selftest_exp_fixed", C.c_int, [_dp, C.c_int64, _dp]),
    ("clothhip_selftest_normal_fixed", C.c_int, [C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_int64, _dp]),
    ("clothhip_selftest_render_plan", C.c_int, [_PP, C.c_int32, C.c_int32, _i32p]),
    ("clothhip_selftest_arith", C.c_int, [C.c_int32, C.c_int32, _dp, _dp, _dp, C.c_int64]),
]

_lib = None


def load():
    """dlopen libclothhip.so and bind every declared symbol. Raises ClothHipError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ClothHipError(
            "libclothhip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C gym_cloth_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    # ROCr keeps a per-queue scratch pool and serves a kernel whose scratch at full occupancy exceeds HSA_SCRATCH_SINGLE_LIMIT
    # (default 140 MB) with a throttled wave count -- and, measured on MI355X / ROCm 7.2, a process that has once run such a kernel
    # may then run a LATER stepper variant below its residency too (two 50x50 cloths per CU became 1.33: 5.0 -> 3.3 M substeps/s).
    # The stepper variants with a VGPR cap spill a few registers in their cold episode code, so they all own some scratch. Unless
    # the caller has set the limit, raise it (512 MB) before the HIP runtime comes up; a runtime that is already up ignores this.
    os.environ.setdefault("HSA_SCRATCH_SINGLE_LIMIT", str(512 << 20))
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise ClothHipError("cannot load %s: %s" % (LIB_PATH, e))
    for name, res, args in SYMBOLS:
        fn = getattr(L, name)          # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if L.clothhip_abi_version() != ABI_VERSION:
        raise ClothHipError("libclothhip ABI version %d, expected %d" % (L.clothhip_abi_version(), ABI_VERSION))
    _lib = L
    return L


def check(rc):
    """Map a negative status to the Python exception the reference would raise for that condition."""
    if rc >= 0:
        return rc
    msg = load().clothhip_last_error().decode("utf8", "replace")
    if rc == EINVAL:
        raise ValueError(msg)
    if rc == ENOMEM:
        raise MemoryError(msg)
    raise ClothHipError("[%d] %s" % (rc, msg))


def dp(a):
    return None if a is None else a.ctypes.data_as(_dp)


def u8p(a):
    return None if a is None else a.ctypes.data_as(_u8p)


def i32p(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def vp(a):
    return None if a is None else a.ctypes.data_as(_vp)


def params_from_cfg(cfg, gravity=-9.8, minimum_z=0.0):
    """cfg: the dict ClothEnv loads from cfg/*.yaml (cloth_env.py:87-118, cloth.pyx:53-56,175-186)."""
    c = cfg["cloth"]
    if c["num_width_points"] != c["num_height_points"]:
        raise AssertionError("height == width (cloth.pyx:91)")
    p = ClothParams()
    p.n_side = int(c["num_width_points"])
    p.frames_per_sec = int(cfg["frames_per_sec"])
    p.simulation_steps = int(cfg["simulation_steps"])
    p.width = float(c["width"]); p.height = float(c["height"])
    p.density = float(c["density"]); p.ks = float(c["ks"]); p.damping = float(c["damping"])
    p.thickness = float(c["thickness"]); p.plane_friction = float(c["plane_friction"])
    p.tear_thresh = float(c["tear_thresh"])
    p.gravity = float(gravity); p.minimum_z = float(minimum_z)
    p.grip_radius = float(cfg.get("env", {}).get("grip_radius", 0.003))
    return p
