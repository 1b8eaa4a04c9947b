"""Host side of the drop-in: the gym `ClothEnv.step()/reset()` surface of the reference
(gym_cloth/envs/cloth_env.py) driving the HIP stepper, vectorised over E independent cloths.

ClothVecEnv  E envs on one GPU (new: the reference is one env per process, analysis/README.md:8-13)
ClothEnv     the reference's single-env API (cloth_env.py:55) = a ClothVecEnv with E = 1

What is mirrored here is exactly what sits between the gym API and the physics hot path:
  action clipping / un-clipping / direction / iters_pull        cloth_env.py:396-470
  phase schedule + per-iteration adjust -> update -> tear?      cloth_env.py:352-367, :472-515
  reset procedures of the three tiers and their RNG sequence    cloth_env.py:717-987, cloth.pyx:75,101
  reward / terminal / out-of-bounds / coverage / variance       cloth_env.py:536-715, :1020-1098
Blender observations, the OpenGL viewer, logging-to-file and pickle I/O are out of scope;
obs_type is forced to the '1d' observation (cloth_env.py:196-200).
"""
import collections
import copy
import time

import numpy as np
import yaml

from . import _lib, seeding
from .batch import ClothBatch, make_schedules
from .reset_streams import ScriptChain, domrand_draws, export_mt, import_mt, prevent_oob, randval_minabs

_REWARD_THRESHOLDS = {           # cloth_env.py:42-50
    'coverage': 0.92, 'coverage-delta': 0.92, 'height': 0.85, 'height-delta': 0.85,
    'variance': 2, 'variance-delta': 2, 'folding-number': 0,
}
_EPS = 1e-5                      # cloth_env.py:52

# What step_many's arguments come to (ClothVecEnv._parse_launch): the policy code, T, the actions / noise table (or the DeviceNoise that makes it), policy_arg, the expert
# and its tables, the reset capacity R and where resets come from, what to return.
_Launch = collections.namedtuple('_Launch', 'pol T actions actions_device_ptr policy_arg expert expert_mix expert_choices R dev_reset '
                                            'use_rng want_obs images image_kw time_budget_ms device_noise')
# What goes to the device with a launch and comes back changed in place (ClothVecEnv._export_streams): reset scripts or MT19937
# images (+ their copy from before, export_mt's token), the envs' step counters and episode-over flags.
_Flight = collections.namedtuple('_Flight', 'scripts mt mt_before mt_token nsteps done_io')


def _is_device_noise(x):
    """policies.DeviceNoise (or anything with its fill / advance): noise made on the device, not an ndarray table."""
    return hasattr(x, 'fill') and hasattr(x, 'advance')


class Box(object):
    """Minimal stand-in for gym.spaces.Box (gym is not a dependency of the hot path)."""

    def __init__(self, low, high, dtype=np.float64):
        self.low = np.asarray(low, dtype=dtype)
        self.high = np.asarray(high, dtype=dtype)
        self.shape = self.low.shape
        self.dtype = dtype
        self.np_random = np.random.RandomState()

    def seed(self, seed=None):
        self.np_random.seed(seed)

    def sample(self):
        return self.np_random.uniform(low=self.low, high=self.high)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))


def slot_start_obs(out, obs_before):
    """float32[T, E, 3P]: the observation each slot's policy saw in a step_many(want_obs=True) launch without a time budget. Slot (t, e)
    began on reset_obs[e, reset_before - 1] where an in-kernel reset preceded it (reset_before[t, e] > 0), else on obs_before[e] --
    the observation before the launch -- for t = 0, else on obs_t[t - 1, e]. Rows of slots that did not run are whatever that rule gives."""
    obs_t = np.asarray(out['obs_t'], dtype=np.float32)
    T, E = obs_t.shape[:2]
    start = np.empty_like(obs_t)
    start[0] = np.asarray(obs_before, dtype=np.float32).reshape(E, -1)
    start[1:] = obs_t[:-1]
    rb = np.asarray(out['reset_before']).astype(np.int64)
    t_, e_ = np.nonzero(rb > 0)
    if len(t_):
        start[t_, e_] = np.asarray(out['reset_obs'])[e_, rb[t_, e_] - 1]
    return start


def _reset_capacity(out):
    """R of the launch `out` came from: the row stride of its reset-observation table per env."""
    if out.get('reset_obs') is not None:
        return int(np.asarray(out['reset_obs']).shape[1])
    return int(out.get('reset_capacity', 0))


def slot_start_sources(out, held_valid=True):
    """int32[T, E, 2]: slot_start_obs's rule stated as indices -- the (source, row) of the observation each slot began on, as
    ClothBatch.fit_append_launch and fit_hold name rows that lie on the device (_lib.FIT_SRC_*). Slot (t, e) began on RESETS row
    e * R + reset_before - 1 where an in-kernel reset preceded it, else on HELD row e -- what the env showed before the launch, kept by
    fit_hold -- for t = 0, else on SLOTS row (t - 1) * E + e. `out` is step_many's dict (want_obs='device' or True); held_valid (bool or
    bool[E]) False marks an env without a held row: its t = 0 entry is (-1, -1), which the library refuses. Unlike slot_start_obs this
    holds for time-sliced launches too, given hold_sources between them: an action a slice cut is recorded in slot 0 of the launch that
    completes it, and was planned on exactly the row held then."""
    rb = np.asarray(out['reset_before']).astype(np.int64)
    T, E = rb.shape
    R = _reset_capacity(out)
    e_ = np.arange(E, dtype=np.int64)
    src = np.empty((T, E, 2), dtype=np.int64)
    src[1:, :, 0] = _lib.FIT_SRC_SLOTS
    src[1:, :, 1] = (np.arange(T - 1, dtype=np.int64)[:, None] * E + e_[None, :])
    ok = np.broadcast_to(np.asarray(held_valid, dtype=bool), (E,))
    src[0, :, 0] = np.where(ok, _lib.FIT_SRC_HELD, -1)
    src[0, :, 1] = np.where(ok, e_, -1)
    t_, k_ = np.nonzero(rb > 0)
    if len(t_):
        src[t_, k_, 0] = _lib.FIT_SRC_RESETS
        src[t_, k_, 1] = k_ * R + rb[t_, k_] - 1
    return src.astype(np.int32)


def hold_sources(out):
    """int32[E, 2]: what every env's held row becomes after the launch `out` (ClothBatch.fit_hold's table) -- the last thing that
    completed in it. That is the reset observation of the env's last fully consumed reset when no record carries it as reset_before
    (out['n_resets'][e] > max_t reset_before[t, e]: a time slice ended right after the reset), else the row of its last executed slot,
    else the row it holds already. `out` needs 'ran', 'reset_before' and 'n_resets' (step_many(want_obs='device') gives it)."""
    ran = np.asarray(out['ran'], dtype=bool)
    rb = np.asarray(out['reset_before']).astype(np.int64)
    T, E = ran.shape
    R = _reset_capacity(out)
    n_res = np.asarray(out['n_resets']).astype(np.int64)
    e_ = np.arange(E, dtype=np.int64)
    src = np.stack([np.full(E, _lib.FIT_SRC_HELD, dtype=np.int64), e_], axis=1)
    any_ran = ran.any(axis=0)
    last = T - 1 - np.argmax(ran[::-1], axis=0)
    src[any_ran, 0] = _lib.FIT_SRC_SLOTS
    src[any_ran, 1] = (last * E + e_)[any_ran]
    tail = n_res > rb.max(axis=0)
    src[tail, 0] = _lib.FIT_SRC_RESETS
    src[tail, 1] = (e_ * R + n_res - 1)[tail]
    return src.astype(np.int32)


def load_cfg(cfg):
    if isinstance(cfg, dict):
        return copy.deepcopy(cfg)
    with open(cfg, 'r') as fh:                       # cloth_env.py:87-88
        return yaml.safe_load(fh)


def decode_actions(actions, low, high, clip_act_space, delta_actions, reduce_factor, iters_up, iters_up_rest,
                   iters_pull_max, iters_grip_rest, iters_rest):
    """The action -> schedule arithmetic of ClothEnv.step (cloth_env.py:396-475), vectorised over envs.

    actions [E,4]; iters_up scalar or [E] (tier 3 draws a float per env, cloth_env.py:960).
    Returns dict(x, y, x_dir_r, y_dir_r, iters_pull, bounds[E,5]); bounds are the integer ceilings of the
    cumulative phase boundaries (`i < b` for integer i is `i < ceil(b)`), formed left to right as the reference
    writes them (cloth_env.py:472-475).
    """
    a = np.asarray(actions, dtype=np.float64)
    E = a.shape[0]
    a = np.maximum(np.minimum(a, np.asarray(high)[None, :]), np.asarray(low)[None, :])    # :402-415
    x_coord, y_coord, c2, c3 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    if clip_act_space:                                                                  # :417-426
        x_coord = (x_coord / 2.0) + 0.5
        y_coord = (y_coord / 2.0) + 0.5
        if not delta_actions:
            c2 = (c2 / 2.0) + 0.5
            c3 = c3 * np.pi
    if delta_actions:                                                                   # :448-453
        total_length = np.sqrt((c2) ** 2 + (c3) ** 2)
        x_dir = c2 / (total_length + _EPS)
        y_dir = c3 / (total_length + _EPS)
    else:
        x_dir = np.cos(c3)
        y_dir = np.sin(c3)
    x_dir_r = x_dir * reduce_factor                                                     # :455-456
    y_dir_r = y_dir * reduce_factor
    if delta_actions:                                                                   # :460-468
        step = np.sqrt((x_dir_r) ** 2 + (y_dir_r) ** 2)
        cur = np.zeros(E)
        ii = np.zeros(E, dtype=np.int64)
        alive = np.ones(E, dtype=bool)
        guard = 0
        while alive.any():
            cur = cur + step
            alive &= ~(cur >= total_length)
            ii[alive] += 1
            guard += 1
            if guard > 1000000:
                raise FloatingPointError("iters_pull does not terminate (non-finite action?)")
        iters_pull = ii
    else:
        iters_pull = (iters_pull_max * c2).astype(np.int64)                             # :470
    iu = np.broadcast_to(np.asarray(iters_up, dtype=np.float64), (E,))
    b1 = iu
    b2 = iu + iters_up_rest
    b3 = iu + iters_up_rest + iters_pull
    b4 = iu + iters_up_rest + iters_pull + iters_grip_rest
    b5 = iu + iters_up_rest + iters_pull + iters_grip_rest + iters_rest
    bounds = np.ceil(np.stack([b1, b2, b3, b4, b5], axis=1)).astype(np.int64)
    return dict(x=x_coord, y=y_coord, x_dir_r=x_dir_r, y_dir_r=y_dir_r, iters_pull=iters_pull, bounds=bounds)


_REWARD_CONSTS = dict(neg_living_rew=0.0, nogrip_penalty=-0.01, tear_penalty=0.0, oob_penalty=0.0, cover_success=5.,
                      act_bound_factor=1.0, act_pen_limit=3.0)            # cloth_env.py:132-141


def compute_reward(reward_type, actions, exit_early, cov, vinv, oob, mask, have_tear, prev_reward, height=None,
                   clip_act_space=True, act_low=None, act_high=None, consts=_REWARD_CONSTS):
    """ClothEnv._reward (cloth_env.py:536-683) as a pure function of its inputs, vectorised over n cloths: nothing is read from or
    written to an env, so the branches of a lookahead can be rewarded without touching the env they started from.

    have_tear is the flag AFTER the action, prev_reward what the '-delta' types subtract (the env's _prev_reward), height the
    fraction of points below half the thickness (only the 'height' types read it). Returns (rew[n], tracked): rew is 0 where mask is
    False; tracked is the value _prev_reward takes for the envs in mask ('-delta' types), or None."""
    n = len(cov)
    rew = np.zeros(n)
    rew += np.where(have_tear, consts['tear_penalty'], np.where(oob, consts['oob_penalty'], 0.0))   # :557-562
    rew += np.where(exit_early, consts['nogrip_penalty'], 0.0)                                      # :563-565
    if not clip_act_space:                                                                          # :579-593
        a = np.asarray(actions, dtype=np.float64).reshape(n, 4)
        diff = np.where(a < act_low, act_low - a, np.where(a > act_high, a - act_high, 0.0))
        pen = -np.minimum(diff ** 2, consts['act_pen_limit']) * consts['act_bound_factor']
        rew += pen.sum(axis=1)
    rew += np.where(cov > _REWARD_THRESHOLDS['coverage'], consts['cover_success'], 0.0)             # :648-650
    rew += consts['neg_living_rew']
    tracked = None
    rt = reward_type                                                                                # :656-679
    if rt == 'coverage':
        rew += cov
    elif rt == 'coverage-delta':
        tracked = cov
    elif rt == 'height':
        rew += height
    elif rt == 'height-delta':
        tracked = height
    elif rt == 'variance':
        rew += vinv
    elif rt == 'variance-delta':
        tracked = vinv
    elif rt == 'folding-number':
        raise NotImplementedError()
    else:
        raise ValueError(rt)
    if tracked is not None:
        rew += tracked - prev_reward
    return np.where(mask, rew, 0.0), tracked


def compute_terminal(reward_type, max_actions, num_steps, have_tear, oob, current_coverage, mask):
    """ClothEnv._terminal (cloth_env.py:684-715) as a pure function: num_steps, have_tear and current_coverage AFTER the action."""
    done = (num_steps >= max_actions) | have_tear | oob                                             # :692-703
    done = done | (current_coverage > _REWARD_THRESHOLDS[reward_type])                              # :706-710
    return done & mask


class ClothSnapshot(object):
    """What ClothVecEnv.snapshot() returns: opaque. `batch` holds the E cloths on the device, `host` the per-env host state."""

    def __init__(self, batch, host):
        self.batch, self.host = batch, host

    def close(self):
        self.batch.close()


class ClothVecEnv(object):
    metadata = {'render.modes': ['human']}

    def __init__(self, cfg_file, n_envs=1, device=0, precision='f32', consume_domrand_draws=True):
        cfg = load_cfg(cfg_file)
        self.cfg, self.cfg_file = cfg, cfg_file
        e = cfg['env']
        self.max_actions = e['max_actions']
        self.iters_up = e['iters_up']
        self.iters_up_rest = e['iters_up_rest']
        self.iters_pull_max = e['iters_pull_max']
        self.iters_grip_rest = e['iters_grip_rest']
        self.iters_rest = e['iters_rest']
        self.reduce_factor = e['reduce_factor']
        self.grip_radius = e['grip_radius']
        self._init_type = cfg['init']['type']
        self._clip_act_space = e['clip_act_space']
        self._delta_actions = e['delta_actions']
        self._force_grab = e['force_grab']
        self._radius_inc = 0.02
        self.bounds = (1, 1, 1)
        self.reward_type = e['reward_type']
        assert 'coverage' in self.reward_type                       # cloth_env.py:130
        self._neg_living_rew = 0.0
        self._nogrip_penalty = -0.01
        self._tear_penalty = 0.0
        self._oob_penalty = 0.0
        self._cover_success = 5.
        self._act_bound_factor = 1.0
        self._act_pen_limit = 3.0
        self._slack = 0.25
        self.num_w = cfg['cloth']['num_width_points']
        self.num_h = cfg['cloth']['num_height_points']
        self.num_points = self.num_w * self.num_h
        self.obslow = np.ones((3 * self.num_points,)) * -100
        self.obshigh = np.ones((3 * self.num_points,)) * 100
        self.observation_space = Box(self.obslow, self.obshigh)
        b0, b1 = self.bounds[0], self.bounds[1]
        if self._clip_act_space:                                     # cloth_env.py:162-181
            self.action_space = Box([-1., -1., -1., -1.], [1., 1., 1., 1.])
        elif self._delta_actions:
            self.action_space = Box([0., 0., -1., -1.], [1., 1., 1., 1.])
        else:
            self.action_space = Box([-self._slack, -self._slack, 0.0, -np.pi],
                                    [b0 + self._slack, b1 + self._slack, 1.0, np.pi])
        self._wd = self._hd = 224
        self._consume_domrand = consume_domrand_draws

        self.E = int(n_envs)
        self.batch = ClothBatch(cfg, n_envs=self.E, device=device, precision=precision)
        self.P = self.batch.P
        E = self.E
        self.np_randoms = [None] * E
        self.seed(None)
        self.init_side = np.zeros(E, dtype=bool)
        self.num_steps = np.zeros(E, dtype=np.int64)
        self.num_sim_steps = np.zeros(E, dtype=np.int64)
        self.have_tear = np.zeros(E, dtype=bool)
        self._prev_reward = np.zeros(E)
        self._start_coverage = np.zeros(E)
        self._start_variance_inv = np.zeros(E)
        self._current_coverage = np.zeros(E)
        self._iters_up_env = np.full(E, float(self.iters_up))       # tier 3 overrides it per env during reset
        self.last_executed = np.zeros(E, dtype=np.int64)
        self.last_grabbed = np.zeros(E, dtype=np.int64)
        self.last_iters_pull = np.zeros(E, dtype=np.int64)
        self._ep_done = np.zeros(E, dtype=bool)                      # episode over, reset pending (step_many's auto-reset)
        self._pending = [None] * E                                   # pre-drawn reset scripts of step_many: a ScriptChain per env, or None
        self.total_substeps = 0                                      # executed update() calls, all envs
        self._version = 0                                            # counts the calls that change the env (commit checks it)
        self._policy_mlp = None                                      # the network on the batch (set_policy): an MLPPolicy or its layers
        self._scratch = None                                         # lookahead's ClothBatch of E*K cloths
        self._look = None                                            # the last lookahead, for commit
        self._plan_scratch = None                                    # plan's ClothBatch of E*K cloths (its own, not lookahead's)

    def close(self):
        self.batch.close()
        if self._scratch is not None:
            self._scratch.close()
            self._scratch = None
        if getattr(self, '_plan_scratch', None) is not None:
            self._plan_scratch.close()
            self._plan_scratch = None

    # ------------------------------------------------------------------------------------------------
    def seed(self, seed=None):
        """cloth_env.py:332-341, one RandomState per env. `seed` may be None, an int (env e gets
        seed + e) or a sequence of E ints."""
        if seed is None or isinstance(seed, (int, np.integer)):
            seeds = [None if seed is None else int(seed) + e for e in range(self.E)]
        else:
            seeds = list(seed)
            assert len(seeds) == self.E
        out = []
        for e, s in enumerate(seeds):
            self.np_randoms[e], s2 = seeding.np_random(s)
            out.append(s2)
        self._version = getattr(self, '_version', 0) + 1
        self._pending = [None] * self.E                                # reset scripts pre-drawn from the old generators
        return out

    # ---- per-env materials (physics domain randomisation, material sweeps) ------------------------------------
    @property
    def material(self):
        """Every env's material, a read-only structured array [E] with the fields density, ks, damping, plane_friction,
        tear_thresh, gravity (the cfg's values for envs never given one)."""
        m = self.batch.get_material()
        m.flags.writeable = False
        return m

    def _env_indices(self, envs):
        idx = np.arange(self.E) if envs is None else np.atleast_1d(np.asarray(envs))
        if idx.dtype == bool:
            if idx.shape != (self.E,):
                raise ValueError("a boolean env mask must have shape (%d,)" % self.E)
            idx = np.nonzero(idx)[0]
        idx = idx.astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= self.E):
            raise ValueError("env index outside [0, %d)" % self.E)
        return idx

    def set_material(self, envs=None, **fields):
        """Change the material of the chosen envs (None: all; indices or a boolean mask): the named fields -- scalars or arrays,
        broadcast over the chosen envs -- are set, the others keep their current value. It belongs to the env slot and survives
        resets; the particle state is not touched. What Cloth.update() reads from the cfg on every call (cloth.pyx:175-186)."""
        unknown = [k for k in fields if k not in _lib.MATERIAL_FIELDS]
        if unknown:
            raise ValueError("unknown material field(s) %s; a material has %s" % (unknown, _lib.MATERIAL_FIELDS))
        idx = self._env_indices(envs)
        if idx.size == 0:
            return
        self._version += 1
        lo, hi = int(idx.min()), int(idx.max()) + 1             # only the touched range of envs is read and rewritten
        m = self.batch.get_material(lo, hi - lo)
        for k, v in fields.items():
            m[k][idx - lo] = np.broadcast_to(np.asarray(v, dtype=np.float64), idx.shape)
        self.batch.set_material(m, env0=lo)

    def randomize_material(self, ranges, seed=None, envs=None):
        """Draw the fields named in `ranges` ({field: (low, high)}, uniform) for the chosen envs, from a RandomState of its own
        seeded by `seed`: the envs' np_randoms do not advance (the reset streams stay the reference's), and the same seed gives the
        same materials. Returns the new material table. Call it between launches to resample."""
        unknown = [k for k in ranges if k not in _lib.MATERIAL_FIELDS]
        if unknown:
            raise ValueError("unknown material field(s) %s; a material has %s" % (unknown, _lib.MATERIAL_FIELDS))
        rng = np.random.RandomState(seed)
        idx = self._env_indices(envs)
        draws = {}
        for k in _lib.MATERIAL_FIELDS:                # drawn in the fixed field order, whatever order `ranges` names them in
            if k in ranges:
                lo, hi = ranges[k]
                draws[k] = rng.uniform(float(lo), float(hi), size=idx.shape)
        self.set_material(idx, **draws)
        return self.material

    @property
    def state(self):
        """'1d' observation of every env, [E, 3P] (cloth_env.py:196-200)."""
        return self.batch.positions().reshape(self.E, 3 * self.P)

    def image_obs(self, use_depth=False, rgbd=False, **render_kw):
        """Image observations without Blender (the reference's obs_type 'blender', cloth_env.py:196-209, :212-330), rendered
        by the library's own rasteriser from the device-resident particles: uint8 [E, H, W, 3] colour, or with use_depth the
        depth image replicated to 3 channels (the Z pass normalised over the image, get_image_rep_279.py:390-406, minus the 50
        grey levels of cloth_env.py:301-302), or with rgbd [E, H, W, 4] = colour + depth channel (:202-205). The camera /
        colour parameters follow the reference's Blender script; the pixels are not Blender's (no smoothing filter, no
        domain randomisation, own shading)."""
        swap = (~self.init_side).astype(np.uint8) if self._init_type == 'tier2' else None      # get_image_rep_279.py:235-239
        rgb, dep = self.batch.render(want_rgb=(rgbd or not use_depth), want_depth=(rgbd or use_depth), swap_sides=swap,
                                     **render_kw)
        d8 = None
        if dep is not None:
            lo = dep.min(axis=(1, 2), keepdims=True); hi = dep.max(axis=(1, 2), keepdims=True)
            nz = np.where(hi > lo, (dep - lo) / np.where(hi > lo, hi - lo, 1.0), 0.0)
            d8 = np.uint8(np.maximum(0.0, np.rint(nz * 255.0) - 50.0))
        if rgbd:
            return np.concatenate([rgb, d8[..., None]], axis=-1)
        return np.repeat(d8[..., None], 3, axis=-1) if use_depth else rgb

    def render_observations(self, obs1d, fmt='rgbd', swap_sides=None, **render_kw):
        """Stored '1d' observations [n, 3P] (or one, [3P]) as finished images, uint8 [n, H, W, C]: what image_obs returns for a
        cloth at those float32 positions (fmt 'rgb' = image_obs(), 'depth' = use_depth, 'rgbd' = rgbd), rendered and finished
        on the device in one call (ClothBatch.render_obs, source 'host'). Turns a '1d' demonstration file into an image set.
        swap_sides[n]: the side swap of a tier-2 cloth dropped with init_side False (~init_side), which a '1d' row does not
        record."""
        obs1d = np.asarray(obs1d, dtype=np.float32).reshape(-1, 3 * self.P)
        return self.batch.render_obs('host', obs=obs1d, swap_sides=swap_sides, fmt=fmt, **render_kw)

    # ---- action decoding (cloth_env.py:396-475) -------------------------------------------------------
    def decode_actions(self, actions, iters_up=None):
        """-> dict(x, y, x_dir_r, y_dir_r, iters_pull, bounds[E,5])."""
        return decode_actions(actions, self.action_space.low, self.action_space.high, self._clip_act_space,
                              self._delta_actions, self.reduce_factor,
                              self._iters_up_env if iters_up is None else iters_up, self.iters_up_rest,
                              self.iters_pull_max, self.iters_grip_rest, self.iters_rest)

    # ---- one action for every (active) env ----------------------------------------------------------------
    def step(self, actions, initialize=False, active=None, auto_reset=False):
        """ClothEnv.step (cloth_env.py:369-534) for all envs at once.
        Returns (obs[E,3P], rew[E], done[E], info dict of arrays); with initialize=True returns None.
        auto_reset: envs that finish their episode in this step are reset before the call returns, as the
        reference's episode loop does (`while not done: step` then `env.reset()`, examples/analytic.py:872-882);
        their row of `obs` is then the first observation of the new episode, info['terminal_observation'] holds
        the last one of the finished episode and info['reset_mask'] says which envs were reset."""
        self._version += 1
        act_mask = np.ones(self.E, dtype=bool) if active is None else np.asarray(active, dtype=bool).copy()
        r = self._run_action(self.batch, actions, self._iters_up_env, act_mask)
        return self._finish_step(actions, r, act_mask, initialize, auto_reset)

    def _run_action(self, batch, actions, iters_up, act_mask):
        """The device half of step() on `batch` (the env's own, or the scratch batch of lookahead: n = batch.E cloths): decode with
        the given per-cloth iters_up, grab_top with the force_grab radius loop, the schedule, the metrics. Touches no env state."""
        n = batch.E
        d = self.decode_actions(actions, iters_up=iters_up)
        xy = np.stack([d['x'], d['y']], axis=1)
        n_grab = batch.grab_top(xy, active=act_mask).astype(np.int64)                   # :431
        if self._force_grab:                                                            # :434-444
            radius = np.full(n, float(self.grip_radius))
            need = act_mask & (n_grab == 0)
            while need.any():
                radius[need] += self._radius_inc
                n2 = batch.grab_top(xy, radius=radius, active=need)
                n_grab[need] = n2[need]
                need = need & (n_grab == 0)
        exit_early = act_mask & (n_grab == 0)                                           # :490-493
        run_mask = act_mask & ~exit_early
        s = make_schedules(n, break_on_tear=1, dz_up=0.0025)                            # :359
        b = d['bounds']
        s['n_up_end'], s['n_uprest_end'], s['n_pull_end'] = b[:, 0], b[:, 1], b[:, 2]
        s['n_griprest_end'], s['n_total'] = b[:, 3], b[:, 4]
        s['dx_pull'], s['dy_pull'] = d['x_dir_r'], d['y_dir_r']
        s['active'] = run_mask
        executed = batch.run(s).astype(np.int64)
        executed[~run_mask] = 0
        if self.reward_type.startswith('height'):
            cov, vinv, oob, tear, height = batch.metrics(want_height=True)
        else:
            (cov, vinv, oob, tear), height = batch.metrics(), None
        return dict(executed=executed, n_grabbed=n_grab, iters_pull=d['iters_pull'], exit_early=exit_early, run_mask=run_mask,
                    cov=cov, vinv=vinv, oob=oob, tear=tear, height=height)

    def _finish_step(self, actions, r, act_mask, initialize, auto_reset):
        """The host half of step(): counters, reward, terminal test, info, auto-reset -- from the results `r` of _run_action (step),
        or of the adopted branches of a lookahead (commit)."""
        executed, n_grab, oob, vinv = r['executed'], r['n_grabbed'], r['oob'], r['vinv']
        self.total_substeps += int(executed.sum())
        self.last_executed, self.last_grabbed, self.last_iters_pull = executed, n_grab, r['iters_pull']
        self.have_tear |= (r['run_mask'] & r['tear'])                                   # :511-514
        if initialize:                                                                  # :517-518
            return None
        self.num_sim_steps[act_mask] += executed[act_mask]
        self.num_steps[act_mask] += 1
        rew = self._reward(actions, r['exit_early'], r['cov'], vinv, oob, act_mask, height=r['height'])
        term = self._terminal(oob, act_mask)
        self._ep_done = np.where(act_mask, term, self._ep_done)
        info = {
            'num_steps': self.num_steps.copy(), 'num_sim_steps': self.num_sim_steps.copy(),
            'actual_coverage': self._current_coverage.copy(), 'start_coverage': self._start_coverage.copy(),
            'variance_inv': vinv, 'start_variance_inv': self._start_variance_inv.copy(),
            'have_tear': self.have_tear.copy(), 'out_of_bounds': oob,
            'executed': executed.copy(), 'n_grabbed': n_grab.copy(),      # (not in the reference's info) this action's update() calls
        }
        obs = self.state
        if auto_reset and term.any():
            info['terminal_observation'] = obs
            info['reset_mask'] = term.copy()
            obs = self.reset(mask=term)
        return obs, rew, term, info

    # ---- forks of the device state: snapshot / restore, action lookahead (clothhip_fork) ---------------------------------
    _SNAP_ARRAYS = ('num_steps', 'num_sim_steps', 'have_tear', '_prev_reward', '_start_coverage', '_start_variance_inv',
                    '_current_coverage', '_iters_up_env', 'init_side', '_ep_done', 'last_executed', 'last_grabbed', 'last_iters_pull')

    def set_policy(self, mlp):
        """Upload a policies.MLPPolicy's network (or a list of (W, b) layers) to this env's batch for step_many(policy='mlp') and
        policy_actions; None clears it. That network belongs to the batch, not to an env slot. A policies.MLPPopulation puts ONE NETWORK
        PER ENV SLOT there instead (its present generation, made on the device). Either way snapshot / restore, forks, the lookahead's
        scratch batch and resets neither carry nor touch networks. On several GPUs every rank sets it itself (dist.py broadcasts no
        weights)."""
        from .policies import MLPPopulation
        from .trainers import MLPEnsemble
        if isinstance(mlp, (MLPPopulation, MLPEnsemble)):      # (an MLPEnsemble: its G networks as uploaded rows, one per env slot)
            self._policy_mlp = None                # a failed upload leaves the batch without a network
            mlp._upload(self.batch)
            self._policy_mlp = mlp
            return
        layers = None if mlp is None else getattr(mlp, 'layers', mlp)
        if layers:
            from .mlp import pack_mlp
            pack_mlp(layers, n_in=3 * self.P)      # a malformed network is refused here and the earlier one stays ...
        self._policy_mlp = None                    # ... a failed upload leaves the batch without one (clothhip_set_policy_mlp)
        self.batch.set_policy_mlp(layers)
        self._policy_mlp = mlp if layers else None

    def policy_actions(self, obs=None):
        """The network's actions float64[E, 4] (before noise and clipping) for '1d' observations obs [E, 3P], or with obs=None for
        every env's present state, computed on the device (ClothBatch.policy_eval; with an MLPPopulation every env under its own
        network, ClothBatch.policy_eval_members)."""
        if self._policy_mlp is None:
            raise ValueError("no policy network: call set_policy(MLPPolicy(...)) first")
        rows = None if obs is None else np.asarray(obs).reshape(self.E, -1).astype(np.float32)
        member = getattr(self._policy_mlp, 'member', None)
        if member is not None:
            return self.batch.policy_eval_members(rows, member)
        return self.batch.policy_eval(rows)

    def expert_actions(self, expert, obs=None, choices=None, init_side=None):
        """What the analytic policy `expert` ('oracle_corner' | 'highest_point') does, float64[n, 4] as step_many(policy=expert) records its
        actions (unclipped; in clip space when the env clips): for float32 '1d' observations obs [n, 3P] -- rows collect_demos or
        step_many(want_obs=True) wrote -- or with obs=None for every env's present state, computed on the device with the launch's
        arithmetic (ClothBatch.policy_label). choices int[n]: which of the highest points ('highest_point'). init_side bool[n]: on tier
        2, the side each row's cloth was dropped from (default with obs=None: the envs' own; with rows it must be given)."""
        if obs is None:
            rows, n = None, self.E
        else:
            rows = np.asarray(obs, dtype=np.float32)
            rows = rows.reshape(-1, rows.shape[-1])
            n = rows.shape[0]
        side = None
        if self._init_type == 'tier2':
            if init_side is None:
                if obs is not None:
                    raise ValueError("tier 2: init_side bool[n] says which side each row's cloth was dropped from")
                init_side = self.init_side
            side = np.where(np.asarray(init_side, dtype=bool).reshape(n), 2, 1).astype(np.int32)      # as step_many's policy_arg
        elif init_side is not None:
            raise ValueError("init_side goes with tier 2")
        if choices is not None:
            choices = np.asarray(choices).reshape(n)
        return self.batch.policy_label(expert, rows, side=side, choices=choices, clip_act_space=self._clip_act_space)

    def _require_whole_actions(self, what):
        if self.batch.in_flight().any():
            raise RuntimeError("%s: a time-sliced step_many left operations in flight on env(s) %s; take it between whole actions "
                               "(finish them with another step_many launch first)" % (what, np.nonzero(self.batch.in_flight())[0].tolist()))

    def snapshot(self):
        """Keep the env as it is now, to come back to with restore(): an opaque ClothSnapshot holding a device-resident copy of all E
        cloths (a private ClothBatch filled by ONE fork: particles, pin bytes, tear flags, rest lengths, materials -- no host staging)
        and everything the host keeps per env (step counters, tear flags, reward bookkeeping, per-env iters_up, init_side, episode-over
        flags, the last_* arrays, every env's RandomState and the reset scripts pre-drawn for step_many). Snapshots are taken between
        whole actions: it raises if a time-sliced step_many left operations in flight."""
        self._require_whole_actions("snapshot")
        b = ClothBatch(self.cfg, n_envs=self.E, device=self.batch.device, precision=self.batch.precision)
        b.fork_from(self.batch, np.arange(self.E))
        host = {k: np.array(getattr(self, k), copy=True) for k in self._SNAP_ARRAYS}
        host['rng'] = [r.get_state() for r in self.np_randoms]
        host['pending'] = copy.deepcopy(self._pending)
        host['built_pos0'] = copy.deepcopy(getattr(self, '_built_pos0', None))
        return ClothSnapshot(b, host)

    def restore(self, snap, envs=None):
        """Put the chosen envs (None: all; indices or a boolean mask) back to where `snap` = snapshot() saw them: the device state
        (materials included) by one fork, and the host state. Afterwards they behave bit for bit as they did after snapshot(),
        including the reset draws of later step_many launches; the other envs stay where they are. A snapshot can be restored any
        number of times."""
        if snap.batch.E != self.E or snap.batch.P != self.P or snap.batch.precision != self.batch.precision:
            raise ValueError("the snapshot was taken from another env")
        idx = self._env_indices(envs)
        self._version += 1
        if idx.size == 0:
            return
        self.batch.fork_from(snap.batch, idx, idx)
        for k in self._SNAP_ARRAYS:
            a = np.array(getattr(self, k), copy=True)
            a[idx] = snap.host[k][idx]
            setattr(self, k, a)
        for e in idx:
            self.np_randoms[e].set_state(snap.host['rng'][e])
            self._pending[e] = copy.deepcopy(snap.host['pending'][e])
        if 0 in idx:
            self._built_pos0 = copy.deepcopy(snap.host['built_pos0'])

    def lookahead(self, actions):
        """What would step(a) return? -- for K candidate actions per env at once, WITHOUT changing the env. actions: float [E, K, 4].
        One fork copies env e into slots e*K .. e*K+K-1 of a scratch ClothBatch of E*K cloths (created on first use, kept for the next
        call with the same K; materials included), which then runs exactly the device half of step() -- decode with the env's own
        iters_up, grab_top with the force_grab radius loop, the schedule, the metrics. Returns a dict of [E, K] arrays: `rew` and
        `done` as step() would return them for that action, and actual_coverage, variance_inv, out_of_bounds, have_tear, executed,
        n_grabbed as in its info. commit() adopts one branch per env."""
        a = np.ascontiguousarray(actions, dtype=np.float64)
        if a.ndim != 3 or a.shape[0] != self.E or a.shape[2] != 4 or a.shape[1] < 1:
            raise ValueError("actions must have shape (%d, K, 4)" % self.E)
        self._require_whole_actions("lookahead")
        E, K = self.E, a.shape[1]
        if self._scratch is None or self._scratch.E != E * K:
            if self._scratch is not None:
                self._scratch.close()
            self._scratch = ClothBatch(self.cfg, n_envs=E * K, device=self.batch.device, precision=self.batch.precision)
        self._look = None
        rep = np.repeat(np.arange(E), K)
        self._scratch.fork_from(self.batch, rep)
        flat = a.reshape(E * K, 4)
        mask = np.ones(E * K, dtype=bool)
        r = self._run_action(self._scratch, flat, self._iters_up_env[rep], mask)
        have_tear = self.have_tear[rep] | (r['run_mask'] & r['tear'])
        rew, _ = compute_reward(self.reward_type, flat, r['exit_early'], r['cov'], r['vinv'], r['oob'], mask, have_tear,
                                self._prev_reward[rep], height=r['height'], clip_act_space=self._clip_act_space,
                                act_low=self.action_space.low, act_high=self.action_space.high, consts=self._reward_consts())
        done = compute_terminal(self.reward_type, self.max_actions, self.num_steps[rep] + 1, have_tear, r['oob'], r['cov'], mask)
        self._look = dict(K=K, version=self._version, actions=a.copy(), r=r)
        sh = lambda v: np.asarray(v).reshape(E, K).copy()
        return dict(rew=sh(rew), done=sh(done), actual_coverage=sh(r['cov']), variance_inv=sh(r['vinv']), out_of_bounds=sh(r['oob']),
                    have_tear=sh(have_tear), executed=sh(r['executed']), n_grabbed=sh(r['n_grabbed']))

    def commit(self, choice, auto_reset=False):
        """Adopt branch choice[e] of the LAST lookahead() for every env e: returns (obs, rew, done, info) exactly as
        step(actions[e, choice[e]], auto_reset=auto_reset) would have. The state is forked back from the scratch batch; the action is
        not simulated again. Raises if anything changed the env since that lookahead -- step, step_many, reset, restore, seed,
        set_material, another commit. Changes accepted in between: none (a further lookahead replaces the one to commit)."""
        L = self._look
        if L is None:
            raise RuntimeError("commit: no lookahead to adopt a branch of")
        if L['version'] != self._version:
            self._look = None
            raise RuntimeError("commit: the env changed since the last lookahead; its branches no longer start from the env's state")
        E, K = self.E, L['K']
        c = np.asarray(choice)
        if c.shape != (E,) or c.dtype.kind not in 'iu' or (c < 0).any() or (c >= K).any():
            raise ValueError("choice must be int[%d] with values in [0, %d)" % (E, K))
        sel = np.arange(E) * K + c.astype(np.int64)
        self._look = None
        self._version += 1
        self.batch.fork_from(self._scratch, sel, np.arange(E))
        r = {k: (None if v is None else np.array(v[sel], copy=True)) for k, v in L['r'].items()}
        return self._finish_step(L['actions'][np.arange(E), c], r, np.ones(E, dtype=bool), False, auto_reset)

    def plan(self, horizon, n_candidates, n_elite, n_iters, mean=None, std=None, init_std=0.5, min_std=0.01, alpha=1.0, penalty=1.0,
             seed=0, iter0=0, want_scores=False, want_candidates=False):
        """Search for good actions with the simulator itself as the model: the cross-entropy method over action sequences of
        `horizon` actions, WITHOUT changing the env (clothhip_plan_cem; include/clothhip.h has the definition). Per iteration,
        n_candidates sequences per env are sampled around (mean, std) on the device -- candidate 0 is the clipped mean itself --, env
        e is forked into n_candidates slots of a scratch ClothBatch of E * n_candidates cloths (this method's own, kept for the next
        call with the same n_candidates), all branches run `horizon` actions in ONE episode launch exactly as step_many(actions,
        auto_reset=False) would run them, each is scored by the coverage after its last executed action minus `penalty` if it tore or
        left the bounds, and (mean, std) are refit to the n_elite best (mean <- alpha mu + (1 - alpha) mean, std likewise, not below
        min_std). mean, std: float64 [E, horizon, 4] in the action space (clip space with clip_act_space); None = zeros / init_std.
        The noise is a function of (seed, iter0 + iteration, table index): the same arguments give the same plan.
        An env whose episode is over (reset pending) is not planned. Returns a dict: actions [E, H, 4] and score [E] of the best
        sequence seen over all iterations (NaN where not planned), mean, std [E, H, 4] after the last refit, planned bool[E], and with
        want_scores / want_candidates scores [n_iters, E, K] / candidates [n_iters, H, E K, 4]. Like lookahead, it is taken between
        whole actions: it raises if a time-sliced step_many left operations in flight."""
        if not self._delta_actions:
            raise NotImplementedError("non-delta actions are decoded on the host only (cos/sin, cloth_env.py:452-453)")
        E, K, H = self.E, int(n_candidates), int(horizon)
        kw = dict(horizon=H, n_candidates=K, n_elite=n_elite, n_iters=n_iters, alpha=alpha, penalty=penalty, min_std=min_std, seed=seed,
                  iter0=iter0)
        ClothBatch.plan_params(**kw)                                   # refuse bad arguments before anything is created
        mean = np.zeros((E, H, 4)) if mean is None else mean
        std = np.broadcast_to(np.asarray(init_std, dtype=np.float64), (E, H, 4)) if std is None else std
        planned = ~np.asarray(self._ep_done, dtype=bool)
        m, s = ClothBatch._plan_dist(mean, std, E, H)
        if not (np.isfinite(m[planned]).all() and np.isfinite(s[planned]).all() and (s[planned] >= 0).all()):
            raise ValueError("mean must be finite, std finite and >= 0")
        self._require_whole_actions("plan")
        if self._plan_scratch is None or self._plan_scratch.E != E * K:
            if self._plan_scratch is not None:
                self._plan_scratch.close()
            self._plan_scratch = ClothBatch(self.cfg, n_envs=E * K, device=self.batch.device, precision=self.batch.precision)
        out = self._plan_scratch.plan_cem(self.batch, self._episode_params(), self.num_steps, ~planned, m, s, want_scores=want_scores,
                                          want_candidates=want_candidates, **kw)
        out['planned'] = planned
        return out

    # ---- whole episodes on the device (clothhip_run_actions) ------------------------------------------------------
    def _episode_params(self):
        from ._lib import ClothEpisodeParams
        ep = ClothEpisodeParams()
        ep.max_actions = int(self.max_actions)
        ep.iters_up_rest, ep.iters_grip_rest, ep.iters_rest = int(self.iters_up_rest), int(self.iters_grip_rest), int(self.iters_rest)
        ep.clip_act_space, ep.force_grab = int(bool(self._clip_act_space)), int(bool(self._force_grab))
        ep.iters_up = float(self.iters_up)
        ep.reduce_factor, ep.grip_radius = float(self.reduce_factor), float(self.grip_radius)
        ep.radius_inc, ep.dz_up = float(self._radius_inc), 0.0025
        for k in range(4):
            ep.act_low[k], ep.act_high[k] = float(self.action_space.low[k]), float(self.action_space.high[k])
        ep.coverage_done = float(_REWARD_THRESHOLDS[self.reward_type])
        return ep

    @property
    def _tier(self):
        """1, 2, 3 for init type 'tier1' .. 'tier3', 0 for anything else."""
        return {'tier1': 1, 'tier2': 2, 'tier3': 3}.get(self._init_type, 0)

    def _drop_pending(self, e):
        """Give back the draws of the env's pre-drawn reset scripts (the RNG is parked at the first one's start)."""
        self._pending[e] = None

    def _extend_chain(self, e, n):
        """Make env e's ScriptChain of pre-drawn resets at least n long (see _prepare_scripts); the RandomState stays parked."""
        if self._pending[e] is None:
            self._pending[e] = ScriptChain(self._tier, self.P, self.iters_up, (self._wd, self._hd) if self._consume_domrand else None)
        self._pending[e].extend(self.np_randoms[e], n)
        return self._pending[e]

    def _prepare_scripts(self, n_scripts):
        """The next `n_scripts` resets of every env, [E, R] (reset_streams.ScriptChain). Scripts that were not consumed stay cached
        for the next launch; each env's RandomState stays parked where its first pending script starts."""
        R = int(n_scripts)
        scripts = np.zeros((self.E, R), dtype=_lib.RESET_SCRIPT_DTYPE)
        self._script_sides = np.zeros((self.E, R), dtype=bool)        # Cloth.init_side of each scripted reset (cloth.pyx:75)
        for e in range(self.E):
            scripts[e], self._script_sides[e] = self._extend_chain(e, R).take(R)
        return scripts

    def _apply_reset_records(self, ie, rb, rst, n_consumed, substeps_out, device_rng):
        """ClothEnv.reset bookkeeping (cloth_env.py:717-790) for the envs `ie` whose rb[e]-th reset of this launch ran."""
        if not len(ie):
            return
        k = rb[ie] - 1
        q = rst[ie, k]
        self.init_side[ie] = (q['init_side'] != 0) if device_rng else self._script_sides[ie, k]
        n_consumed[ie] = k + 1
        sub = q['executed'].sum(axis=1).astype(np.int64) + q['settle_executed']
        substeps_out[ie] = sub
        self.total_substeps += int(sub.sum())
        self.num_steps[ie] = 0; self.num_sim_steps[ie] = 0
        self.have_tear[ie] = q['tear'] != 0
        self._prev_reward[ie] = q['start_coverage']
        self._start_coverage[ie] = q['start_coverage']
        self._start_variance_inv[ie] = q['start_variance_inv']
        self._current_coverage[ie] = 0.0
        self._ep_done[ie] = False

    def step_many(self, actions=None, n_actions=None, policy=None, auto_reset=True, want_obs=False, reset_tail=False,
                  actions_device_ptr=None, max_resets=None, time_budget_ms=0.0, device_rng=True, policy_choices=None,
                  images=None, image_kw=None, policy_noise=None, expert=None, expert_mix=None, expert_choices=None):
        """T consecutive `step(a_t, auto_reset=auto_reset)` calls for every env in ONE device launch
        (clothhip_run_actions): decoding, grab, the substep loop, metrics, the terminal test and the episode resets all
        run in the kernel, envs never wait for each other, and the host only does the reward / info bookkeeping below.

        actions: float64[T, E, 4], or policy='oracle_corner' (examples/analytic.py's oracle, evaluated on the device)
        with n_actions=T, or policy='highest_point' (analytic.py:723-808 on the device) with n_actions=T and
        policy_choices int[T, E]: which of the highest points (0 = the highest; the reference draws randint(5)) the env
        pulls in its t-th slot, or policy='mlp' (the network of set_policy, evaluated in the kernel on the cloth's '1d' observation when
        the slot begins -- after an in-kernel reset on the new episode's first state) with n_actions=T and optionally policy_noise
        float64[T, E, 4], added to the network's output of that slot before clipping (exploration noise comes from the caller's table, so
        the launch stays deterministic; with a time budget the caller passes the unused rows again, as for actions), or a
        policies.DeviceNoise: the table of this launch's T slots is filled on the device in front of the launch (ClothBatch.policy_noise_fill),
        row t of env e being that env's slot slot_base[e] + t, and slot_base then moves on by the slots each env ran -- with a time budget
        the next launch continues every env's own stream, nothing is passed again. With auto_reset=False an env whose episode ends idles for the rest of the launch (`ran` False). Up to `max_resets` (default min(T, 255), the
        launch's limit) resets per env and launch; an env that has used them idles until the launch ends. The resets are drawn on the device from
        each env's numpy RandomState stream (device_rng=True: the states are uploaded before and read back after the
        launch; csrc/cloth_rng.hpp reproduces numpy's MT19937 draws bit for bit; all three tiers, tier 2 rebuilding the
        env's noisy sheet and rest lengths in the kernel), or, with device_rng=False (tiers 1 and 3), pre-drawn
        on the host as a chain of scripts -- then, when tier 1's coverage-conditional third reset pull runs, that env's
        later scripts are void (the RNG stream forked) and it idles after its next episode until the launch ends.
        An episode that ends in the last slot is reset by the NEXT launch, or here on the host with reset_tail=True (then
        the returned obs is what T sequential steps return).

        expert='oracle_corner' | 'highest_point' (beside actions or policy='mlp' only) runs that analytic policy as a silent second policy
        of the launch: when a slot begins it is evaluated where the acting policy is, on the same state, and out['expert_actions']
        float64[T, E, 4] holds what a launch with policy=expert would have recorded as that slot's action (NaN where `ran` is False) --
        the DAgger label of every state the learner reached. expert_mix bool[T, E] lets it act: where True the label IS the slot's action
        (no policy_noise added, the network not evaluated); out['expert_took'] bool[T, E] says where that happened. expert_choices
        int[T, E]: which of the highest points, for 'highest_point' (as policy_choices). out['init_side_t'] bool[T, E] is init_side as it
        stood when each slot began (tier 2: what expert_actions needs beside stored rows). With a time budget the caller passes the unused
        expert_mix / expert_choices rows again, as for policy_noise, and arms every launch of the sequence.

        time_budget_ms > 0 turns the launch into a time slice: an env starts no further action once the launch has run that
        long, so envs advance at their own pace instead of waiting for the one with the most work (episode resets make
        the work per env very uneven). out['ran'][:, e] is then True for the first n_e slots only, and the caller passes
        actions[n_e:, e] again in the next call. Results do not depend on how an env's actions are split into launches.

        Returns a dict of arrays [T, E] (rew, done, ran, executed, n_grabbed, reset_before, and the info keys of step())
        plus 'obs' [E, 3P] (state after the launch), 'actions' [T, E, 4], with want_obs 'obs_t' [T, E, 3P], and the launch's time
        accounting 'op_ticks' / 'op_substeps' uint64[E, 4] (ClothBatch.op_ticks). want_obs='device' writes both observation tables as
        True does but leaves them on the device until the next launch and downloads neither: no 'obs_t' / 'reset_obs', instead
        'n_resets' int[E] (the resets of this launch each env consumed completely) and 'reset_capacity' (the reset table's rows per env) --
        what slot_start_sources and hold_sources need to name the rows for ClothBatch.fit_append_launch / fit_hold.

        images='rgb' | 'depth' | 'rgbd' (implies want_obs) adds the image observation of every slot, rendered on the device from
        the launch's resident observation tables after the bookkeeping (ClothBatch.render_obs; image_kw: render parameters, as
        image_obs takes them): 'img_t' uint8 [T, E, H, W, C], what image_obs would have returned after that step, zeros where
        `ran` is False, and 'reset_img' [E, R, H, W, C] beside 'reset_obs' (None without in-kernel resets), zeros for the resets
        the launch did not consume. A tier-2 image swaps the side colours by the init_side its episode was dropped with."""
        self._version += 1
        tp = [time.perf_counter()]
        prof = self.__dict__.setdefault('host_prof', {})

        def _lap(name):
            now = time.perf_counter()
            prof[name] = prof.get(name, 0.0) + now - tp[0]
            tp[0] = now
        a = self._parse_launch(actions, n_actions, policy, auto_reset, want_obs, actions_device_ptr, max_resets, time_budget_ms,
                               device_rng, policy_choices, images, image_kw, policy_noise, expert, expert_mix, expert_choices)
        fl = self._export_streams(a)
        _lap('prepare_resets')
        self._launch(a, fl)
        _lap('launch')
        if a.dev_reset and not a.use_rng:                             # while the kernel runs: draw ahead for the NEXT launch
            for e in range(self.E):
                self._extend_chain(e, 2 * a.R)
        _lap('draw_ahead(overlapped)')
        rec, rst, obs_t, robs = self.batch.run_actions_end()
        op = self.batch.op_ticks()
        labels = self.batch.run_actions_labels(a.T) if a.expert is not None else None
        _lap('wait+download')
        out, n_consumed, side_t = self._account_launch(rec, rst, fl.nsteps, fl.done_io, a.dev_reset, a.use_rng, op, labels, a.expert_mix)
        _lap('bookkeeping')
        if a.device_noise is not None:
            a.device_noise.advance(out['ran'])                        # every env's next launch goes on with its own next slot
        self._commit_streams(a, fl, rst, n_consumed)
        _lap('rng_commit')
        if a.images is not None:                                      # the launch's tables are still on the device
            self._render_launch(a, out, rst, robs is not None or (a.want_obs == 'device' and a.dev_reset), n_consumed, side_t)
            _lap('images')
        obs = self.state
        _lap('obs_download')
        if reset_tail and auto_reset and self._ep_done.any():
            obs = self.reset(mask=self._ep_done.copy())
        out['obs'] = obs
        if expert is not None:                                        # (an un-armed launch returns exactly the keys it always did)
            out['init_side_t'] = side_t                               # tier 2: the side each slot's cloth was dropped from (expert_actions on stored rows)
        if a.want_obs == 'device':                                    # both tables stay on the device; what names their rows instead
            out['n_resets'] = n_consumed                              # resets of this launch each env consumed completely
            out['reset_capacity'] = a.R if a.dev_reset else 0         # the reset table's rows per env
        elif a.want_obs:
            out['obs_t'], out['reset_obs'] = obs_t, robs
        return out

    # ---- the stages of step_many: parse, begin (export streams, launch), account, commit streams, images ------------------------
    def _parse_launch(self, actions, n_actions, policy, auto_reset, want_obs, actions_device_ptr, max_resets, time_budget_ms,
                      device_rng, policy_choices, images, image_kw, policy_noise, expert, expert_mix, expert_choices):
        """step_many's arguments -> a _Launch; every refusal, in a fixed order. The ORDER IS BEHAVIOUR: callers get a ValueError for bad
        arguments before anything reaches a device, so up to and including batch._expert_tables this reads nothing of the env but E,
        _policy_mlp, num_points and _delta_actions, and of the batch nothing but E (tests/test_dagger_host.py's _bare_env has no
        more); _init_type and init_side are read only after the refusals that need neither."""
        E = self.E
        device_noise = None
        if policy in (None, 'table'):
            pol = _lib.POLICY_TABLE
            if actions_device_ptr is None:
                actions = np.ascontiguousarray(actions, dtype=np.float64)
                T = actions.shape[0]
            else:
                T = int(n_actions)
        elif policy == 'oracle_corner':
            pol, T = _lib.POLICY_ORACLE_CORNER, int(n_actions)
            assert self._delta_actions and self.num_points == 625                        # analytic.py:103-106
        elif policy == 'highest_point':                                                  # analytic.py:723-808, evaluated on the device
            pol, T = _lib.POLICY_HIGHEST_POINT, int(n_actions)
            policy_choices = np.asarray(policy_choices, dtype=np.int32)                  # [T, E]: 0 = the highest point, 1 = the next ...
            if policy_choices.shape != (T, E):
                raise ValueError("policy_choices must have shape (%d, %d)" % (T, E))
        elif policy == 'mlp':
            pol, T = _lib.POLICY_MLP, int(n_actions)
            if self._policy_mlp is None:
                raise ValueError("policy='mlp' needs a network: call set_policy(MLPPolicy(...)) first")
            if actions is not None or actions_device_ptr is not None:
                raise ValueError("policy='mlp' takes no actions: the network gives them; exploration noise goes into policy_noise")
            if _is_device_noise(policy_noise):                                           # policies.DeviceNoise: the table is made on the device (_launch)
                device_noise = policy_noise
            elif policy_noise is not None:
                actions = np.ascontiguousarray(policy_noise, dtype=np.float64)
                if actions.shape != (T, E, 4):
                    raise ValueError("policy_noise must have shape (%d, %d, 4)" % (T, E))
        else:
            raise ValueError(policy)
        if policy_noise is not None and policy != 'mlp':
            raise ValueError("policy_noise goes with policy='mlp'")
        if expert is not None and pol not in (_lib.POLICY_TABLE, _lib.POLICY_MLP):
            raise ValueError("an expert runs beside actions or policy='mlp' only (got policy=%r)" % (policy,))
        if expert == 'oracle_corner' and self.num_points != 625:
            raise ValueError("the oracle-corner expert is defined for 25x25 cloths only (analytic.py:106)")
        expert_mix, expert_choices = self.batch._expert_tables(expert, expert_mix, expert_choices, T)
        if not self._delta_actions:
            raise NotImplementedError("non-delta actions are decoded on the host only (cos/sin, cloth_env.py:452-453)")
        if images is not None:
            if images not in _lib.IMG_FORMATS:
                raise ValueError("images must be None, 'rgb', 'depth' or 'rgbd' (got %r)" % (images,))
            want_obs = want_obs or True
        dev_reset = bool(auto_reset and (self._tier in (1, 3) or (self._tier == 2 and device_rng)))
        R = min(T, 255) if max_resets is None else int(max_resets)      # clothhip_run_actions: n_scripts in [1, 255]
        if dev_reset and not 1 <= R <= 255:
            raise ValueError("max_resets must be in [1, 255] (got %d)" % R)
        parg = None
        if (pol != _lib.POLICY_TABLE or expert is not None) and self._tier == 2:
            parg = np.where(self.init_side, 2, 1).astype(np.int32)                       # analytic.py:108-114, :781-788
        if pol == _lib.POLICY_HIGHEST_POINT:
            parg = np.concatenate([(np.zeros(E, dtype=np.int32) if parg is None else parg)[None, :], policy_choices], axis=0)
        return _Launch(pol, T, actions, actions_device_ptr, parg, expert, expert_mix, expert_choices, R, dev_reset,
                       bool(dev_reset and device_rng), want_obs, images, dict(image_kw or {}), time_budget_ms, device_noise)

    def _export_streams(self, a):
        """Where the launch's resets come from, ready for the device: the next R scripts of every env (host-drawn), or every env's
        numpy stream as RandomState.get_state() has it (device-drawn; pending scripts give their draws back first). -> _Flight."""
        scripts = mt = mt_before = token = None
        if a.use_rng:
            if self._tier == 2:
                self.batch.ensure_per_env_rest()                      # the kernel rebuilds each env's rest lengths at a reset
            self._pending = [None] * self.E
            mt, token = export_mt(self.np_randoms)
            mt_before = mt.copy()
        elif a.dev_reset:
            scripts = self._prepare_scripts(a.R)
        return _Flight(scripts, mt, mt_before, token, np.ascontiguousarray(self.num_steps, dtype=np.int32),
                       np.ascontiguousarray(self._ep_done, dtype=np.uint8))

    def _launch(self, a, fl):
        ptr = a.actions_device_ptr
        if a.device_noise is not None:                                # this launch's T slots of every env, filled on the batch's stream in front of the launch
            ptr = a.device_noise.fill(self.batch, a.T)
        self.batch.run_actions_begin(self._episode_params(), a.T, fl.nsteps, fl.done_io, actions=a.actions, policy=a.pol,
                                     policy_arg=a.policy_arg, scripts=fl.scripts, want_obs=a.want_obs,
                                     actions_device_ptr=ptr, time_budget_ms=a.time_budget_ms,
                                     rng_states=fl.mt, rng_tier=self._tier,
                                     domrand_words=2 * (3 + self._wd * self._hd * 3) if self._consume_domrand else 0,
                                     reset_capacity=a.R, expert=a.expert, expert_mix=a.expert_mix, expert_choices=a.expert_choices)

    def _account_launch(self, rec, rst, nsteps, done_io, dev_reset, use_rng, op, labels=None, expert_mix=None):
        """The host's bookkeeping of a launch, from what it returned alone (no device access, no call on self.batch): the step records
        rec[T, E] and reset records rst[E, R] (or None) of run_actions_end, the counters nsteps[E] / flags done_io[E] it updated, op =
        op_ticks(), the expert's labels and mix table. Advances the env's host arrays and returns (out, n_consumed[E]: resets of
        the launch the host has accounted, side_t[T, E]: init_side as it stood at each slot)."""
        if (rec['ran'] == 2).any():
            raise FloatingPointError("iters_pull does not terminate (non-finite action?)")
        T, E = rec.shape[0], self.E
        out = {k: np.zeros((T, E)) for k in ('rew', 'actual_coverage', 'start_coverage', 'variance_inv', 'start_variance_inv')}
        for k in ('done', 'ran', 'have_tear', 'out_of_bounds'):
            out[k] = np.zeros((T, E), dtype=bool)
        for k in ('executed', 'n_grabbed', 'num_steps', 'num_sim_steps', 'reset_before', 'reset_substeps'):
            out[k] = np.zeros((T, E), dtype=np.int64)
        out['actions'] = rec['action'].copy()
        if labels is not None:
            ran_ = rec['ran'] == 1
            out['expert_actions'] = np.where(ran_[:, :, None], labels, np.nan)
            out['expert_took'] = ran_ & (expert_mix != 0 if expert_mix is not None else False)
        # per env: 100 MHz ticks of this launch spent in {actions, reset pulls, reset settling, the rest} and the update() calls of each
        out['op_ticks'], out['op_substeps'] = op
        n_consumed = np.zeros(E, dtype=np.int64)
        side_t = np.zeros((T, E), dtype=bool)                         # init_side as it stands at each slot (images of tier 2)
        for t in range(T):
            self._account_slot(t, rec[t], rst, out, n_consumed, side_t, use_rng)
        if dev_reset:                                                 # a time slice may end right after a reset
            tail = np.nonzero((rst['consumed'] == 1).sum(axis=1) > n_consumed)[0]
            if len(tail):
                rb = np.zeros(E, dtype=np.int64)
                rb[tail] = n_consumed[tail] + 1
                out['tail_reset_substeps'] = np.zeros(E, dtype=np.int64)
                out['tail_reset_index'] = rb.copy()                   # 1-based index into reset_obs[e] of that reset, 0 = none
                self._apply_reset_records(tail, rb, rst, n_consumed, out['tail_reset_substeps'], use_rng)
        # the device's view of the episode state must be the host's, except where a time slice cut a reset in the middle (the
        # device has already zeroed that env's counters; the host learns of the reset from the launch that completes it)
        settled = np.ones(E, dtype=bool) if rst is None else ~(rst['consumed'] == 2).any(axis=1)
        assert np.array_equal(self.num_steps.astype(np.int32)[settled], nsteps[settled])
        assert np.array_equal(self._ep_done[settled], (done_io != 0)[settled])
        return out, n_consumed, side_t

    def _account_slot(self, t, r, rst, out, n_consumed, side_t, use_rng):
        """Slot t of a launch, r = rec[t]: the resets that preceded it, then what step() does on the host after an action -- for the envs
        whose slot ran."""
        rb = r['reset_before'].astype(np.int64)
        self._apply_reset_records(np.nonzero(rb)[0], rb, rst, n_consumed, out['reset_substeps'][t], use_rng)
        side_t[t] = self.init_side
        ran = r['ran'] == 1
        executed = np.where(ran, r['executed'], 0).astype(np.int64)
        self.total_substeps += int(executed.sum())
        self.have_tear |= ran & (r['tear'] != 0)
        self.num_sim_steps[ran] += executed[ran]
        self.num_steps[ran] += 1
        oob = r['oob'] != 0
        rew = self._reward(r['action'], ran & (r['n_grabbed'] == 0), r['coverage'], r['variance_inv'], oob, ran,
                           height=r['n_below_half_thickness'] / float(self.P))
        term = self._terminal(oob, ran)
        if not np.array_equal(term[ran], (r['done'] != 0)[ran]):
            raise RuntimeError("device and host disagree on the terminal test")
        self._ep_done = np.where(ran, term, self._ep_done)
        self.last_executed = np.where(ran, executed, self.last_executed)
        self.last_grabbed = np.where(ran, r['n_grabbed'], self.last_grabbed)
        self.last_iters_pull = np.where(ran, r['iters_pull'], self.last_iters_pull)
        out['rew'][t], out['done'][t], out['ran'][t] = rew, term, ran
        out['executed'][t], out['n_grabbed'][t], out['reset_before'][t] = executed, r['n_grabbed'], rb
        out['num_steps'][t], out['num_sim_steps'][t] = self.num_steps, self.num_sim_steps
        out['actual_coverage'][t], out['start_coverage'][t] = self._current_coverage, self._start_coverage
        out['variance_inv'][t], out['start_variance_inv'][t] = r['variance_inv'], self._start_variance_inv
        out['have_tear'][t], out['out_of_bounds'][t] = self.have_tear, oob

    def _commit_streams(self, a, fl, rst, n_consumed):
        """Move every env's RandomState past the draws the launch consumed: the streams as the device left them (a reset cut by the
        time slice has drawn too, before any record of it is complete), or the scripts it ran (ScriptChain.commit)."""
        if a.use_rng:
            import_mt(self.np_randoms, fl.mt, fl.mt_before, fl.mt_token)
        elif a.dev_reset:
            for e in np.nonzero(n_consumed)[0]:
                c = int(n_consumed[e])
                self._pending[e].commit(self.np_randoms[e], c, rst[e, c - 1]['pulls_run'])

    def _render_launch(self, a, out, rst, have_reset_obs, n_consumed, side_t):
        """out['img_t'] / out['reset_img']: every slot's and every consumed reset's image, from the launch's tables on the device."""
        tier2 = self._tier == 2
        img = self.batch.render_obs('slots', valid=out['ran'].reshape(-1), swap_sides=(~side_t).reshape(-1) if tier2 else None,
                                    fmt=a.images, **a.image_kw)
        out['img_t'] = img.reshape((a.T, self.E) + img.shape[1:])
        out['reset_img'] = None
        if have_reset_obs:
            sides = (rst['init_side'] != 0) if a.use_rng else self._script_sides
            rimg = self.batch.render_obs('resets', valid=(np.arange(a.R)[None, :] < n_consumed[:, None]).reshape(-1),
                                         swap_sides=(~sides).reshape(-1) if tier2 else None, fmt=a.images, **a.image_kw)
            out['reset_img'] = rimg.reshape((self.E, a.R) + rimg.shape[1:])

    # ---- reward / terminal (cloth_env.py:536-715) ------------------------------------------------------------
    def _height_fraction(self):
        """compute_height (cloth_env.py:603-609): the count comes from the device metrics kernel."""
        return self.batch.metrics(want_height=True)[4]

    def _reward(self, actions, exit_early, cov, vinv, oob, mask, height=None):
        """compute_reward on the env's own state, then the two updates ClothEnv._reward makes (_current_coverage, :647; _prev_reward
        of the '-delta' types, :656-679)."""
        if height is None and self.reward_type.startswith('height'):
            height = self._height_fraction()
        rew, tracked = compute_reward(self.reward_type, actions, exit_early, cov, vinv, oob, mask, self.have_tear, self._prev_reward,
                                      height=height, clip_act_space=self._clip_act_space, act_low=self.action_space.low,
                                      act_high=self.action_space.high, consts=self._reward_consts())
        self._current_coverage = np.where(mask, cov, self._current_coverage)                         # :647
        if tracked is not None:
            self._prev_reward = np.where(mask, tracked, self._prev_reward)
        return rew

    def _reward_consts(self):
        return dict(neg_living_rew=self._neg_living_rew, nogrip_penalty=self._nogrip_penalty, tear_penalty=self._tear_penalty,
                    oob_penalty=self._oob_penalty, cover_success=self._cover_success, act_bound_factor=self._act_bound_factor,
                    act_pen_limit=self._act_pen_limit)

    def _terminal(self, oob, mask):
        return compute_terminal(self.reward_type, self.max_actions, self.num_steps, self.have_tear, oob, self._current_coverage, mask)

    def _compute_coverage(self):
        return self.batch.metrics()[0]

    def _compute_variance(self):
        return self.batch.metrics()[1]

    def _out_of_bounds(self):
        return self.batch.metrics()[2]

    def _convert_action_to_clip_space(self, a):                     # cloth_env.py:1207-1215, vectorised
        a = np.asarray(a, dtype=np.float64)
        if not self._clip_act_space:
            return a
        out = a.copy()
        out[..., 0] = (a[..., 0] - 0.5) * 2
        out[..., 1] = (a[..., 1] - 0.5) * 2
        if not self._delta_actions:
            out[..., 2] = (a[..., 2] - 0.5) * 2
            out[..., 3] = a[..., 3] / np.pi
        return out

    def get_random_action(self, atype='over_xy_plane'):
        """cloth_env.py:989-1018; [E,4]. NB the reference samples from the action space's own, unseeded RNG."""
        if atype == 'over_xy_plane':
            return np.stack([self.action_space.sample() for _ in range(self.E)])
        raise ValueError(atype)

    # ---- reset (cloth_env.py:717-987; cloth.pyx:75, :94-130) -------------------------------------------------
    def _update_masked(self, n, mask):
        s = make_schedules(self.E, n_griprest_end=n, n_total=n, break_on_tear=0)
        s['active'] = mask
        ex = self.batch.run(s)
        self.total_substeps += int(ex[mask].sum())

    def reset(self, mask=None):
        """Reset the envs selected by `mask` (default all) and return the '1d' observation of ALL envs."""
        E, P = self.E, self.P
        self._version += 1
        m = np.ones(E, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        idx = np.nonzero(m)[0]
        tier = self._tier
        if not tier:
            raise ValueError(self._init_type)                         # cloth.pyx:131-132
        if not self._delta_actions:
            raise NotImplementedError()                               # cloth_env.py:862, :917, :968
        for e in idx:                                                 # scripts pre-drawn for step_many: re-drawn below
            self._drop_pending(e)
        # ---- Cloth(...) construction: RNG draws in the reference's order (cloth.pyx:75, :101) --------------
        if tier == 2:
            pos_all = np.empty((len(idx), P, 3))
            rest_all = np.empty((len(idx), self.batch.S))
            for k, e in enumerate(idx):
                rng = self.np_randoms[e]
                self.init_side[e] = rng.rand() > 0.5
                draws = rng.rand(P)                                   # one rand() per point, r-major
                pos_all[k], rest_all[k] = self.batch.init_grid(2, self.init_side[e], draws)
                if e == 0:
                    self._built_pos0 = pos_all[k].copy()              # what env 0's cloth was built with (Point.orig_*, the façade's view)
            zeros_pin = np.zeros((len(idx), P), dtype=np.uint8)
            k = 0
            while k < len(idx):                                       # one upload per run of consecutive envs
                j = k
                while j + 1 < len(idx) and idx[j + 1] == idx[j] + 1:
                    j += 1
                self.batch.set_state(pos_all[k:j + 1], pos_all[k:j + 1], zeros_pin[k:j + 1], rest_all[k:j + 1],
                                     env0=int(idx[k]), n=j + 1 - k, rest_shared=False)
                k = j + 1
        else:
            for e in idx:
                self.init_side[e] = self.np_randoms[e].rand() > 0.5
            self.batch.reset_flat(None if len(idx) == E else m)       # flat grid, nothing pinned, no tear: on the device
            if m[0]:
                self._built_pos0 = None                                # the flat grid (ClothEnv.reset asks init_grid for it)
        self.num_steps[m] = 0
        self.num_sim_steps[m] = 0
        self.have_tear[m] = False
        self._ep_done[m] = False
        self._iters_up_env[m] = float(self.iters_up)
        self._reset_actions(m, idx, tier)
        cov, vinv, _, _ = self.batch.metrics()                        # cloth_env.py:780-782
        self._prev_reward = np.where(m, cov, self._prev_reward)
        self._start_coverage = np.where(m, cov, self._start_coverage)
        self._start_variance_inv = np.where(m, vinv, self._start_variance_inv)
        self._current_coverage = np.where(m, 0.0, self._current_coverage)
        if self._consume_domrand:                                     # cloth_env.py:786-789 advance the env RNG
            for e in idx:
                domrand_draws(self.np_randoms[e], self._wd, self._hd)
        return self.state

    _randval_minabs = staticmethod(randval_minabs)                    # cloth_env.py:824-832
    _prevent_oob = staticmethod(prevent_oob)                          # cloth_env.py:834-840

    def _reset_actions(self, m, idx, tier):
        E = self.E
        acts = np.zeros((E, 4))
        if tier == 1:                                                 # cloth_env.py:843-891
            lim = 0.20
            for pull in range(3):
                if pull < 2:
                    who = idx
                else:
                    cov = self.batch.metrics()[0]
                    who = np.array([e for e in idx if cov[e] >= 0.90], dtype=np.int64)
                    if len(who) == 0:
                        break
                pos = self.batch.positions()
                sel = np.zeros(E, dtype=bool)
                for e in who:
                    rng = self.np_randoms[e]
                    p = pos[e, rng.randint(self.P)]
                    dx0 = self._randval_minabs(rng, -lim, lim, 0.08)
                    dy0 = self._randval_minabs(rng, -lim, lim, 0.08)
                    dx0 = self._prevent_oob(p[0], dx0)
                    dy0 = self._prevent_oob(p[1], dy0)
                    acts[e] = (p[0], p[1], dx0, dy0)
                    sel[e] = True
                self.step(self._convert_action_to_clip_space(acts), initialize=True, active=sel)
        elif tier == 2:                                               # cloth_env.py:893-949
            self._update_masked(1500, m)
            pos = self.batch.positions()
            choice = {}
            sel = np.zeros(E, dtype=bool)
            for e in idx:
                rng = self.np_randoms[e]
                side = 1 if self.init_side[e] else -1
                pi = -25 if rng.rand() < 0.5 else -1
                choice[e] = pi
                p0 = pos[e, pi]
                dx0 = rng.uniform(0.30, 0.50) * side
                dy0 = rng.uniform(0.30, 0.60) if pi == -25 else rng.uniform(-0.60, -0.30)
                acts[e] = (p0[0], p0[1], dx0, dy0)
                sel[e] = True
            self.step(self._convert_action_to_clip_space(acts), initialize=True, active=sel)
            pos = self.batch.positions()
            for e in idx:
                rng = self.np_randoms[e]
                side = 1 if self.init_side[e] else -1
                if choice[e] == -25:
                    p1 = pos[e, -19]
                    dx1 = rng.uniform(0.30, 0.60) * side
                    dy1 = rng.uniform(-0.30, -0.60)
                else:
                    p1 = pos[e, -7]
                    dx1 = rng.uniform(0.30, 0.60) * side
                    dy1 = rng.uniform(0.30, 0.60)
                acts[e] = (p1[0], p1[1], dx1, dy1)
            self.step(self._convert_action_to_clip_space(acts), initialize=True, active=sel)
            self._update_masked(500, m)
        elif tier == 3:                                               # cloth_env.py:951-982
            lim = 0.25
            sel = np.zeros(E, dtype=bool)
            for e in idx:
                rng = self.np_randoms[e]
                self._iters_up_env[e] = rng.uniform(low=200, high=280)
                p0x = self._randval_minabs(rng, 0.30, 0.70)
                p0y = self._randval_minabs(rng, 0.30, 0.70)
                dx0 = self._randval_minabs(rng, -lim, lim, 0.10)
                dy0 = self._randval_minabs(rng, -lim, lim, 0.10)
                dx0 = self._prevent_oob(p0x, dx0)
                dy0 = self._prevent_oob(p0y, dy0)
                acts[e] = (p0x, p0y, dx0, dy0)
                sel[e] = True
            self.step(self._convert_action_to_clip_space(acts), initialize=True, active=sel)
            self._update_masked(800, m)
            self._iters_up_env[m] = float(self.iters_up)


class ClothEnv(object):
    """The reference's single-environment API (cloth_env.py:55): same constructor signature, seed/reset/
    step/state/get_random_action, same return types (scalars, dict of scalars)."""
    metadata = {'render.modes': ['human']}

    def __init__(self, cfg_file, subrank=None, start_state_path=None, device=0, precision='f32'):
        self._vec = ClothVecEnv(cfg_file, n_envs=1, device=device, precision=precision)
        v = self._vec
        self.cfg, self.cfg_file = v.cfg, cfg_file
        self._logger_idx = subrank
        self._start_state = None
        if start_state_path is not None:                              # npz instead of the reference's pickle
            with np.load(start_state_path) as d:
                self._start_state = {k: d[k] for k in d.files}
        for k in ('max_actions', 'iters_up', 'iters_up_rest', 'iters_pull_max', 'iters_grip_rest', 'iters_rest',
                  'reduce_factor', 'grip_radius', 'bounds', 'reward_type', 'num_w', 'num_h', 'num_points',
                  'observation_space', 'action_space', 'obslow', 'obshigh'):
            setattr(self, k, getattr(v, k))
        from .physics import Cloth, Gripper
        self.cloth = Cloth(batch=v.batch, env=0, owner=v)
        self.gripper = Gripper(self.cloth, self.grip_radius, self.cfg['cloth']['height'],
                               self.cfg['cloth']['thickness'])

    def close(self):
        self._vec.close()

    @property
    def np_random(self):
        return self._vec.np_randoms[0]

    def seed(self, seed=None):
        return self._vec.seed([seed])

    @property
    def state(self):
        return self._vec.state[0]

    @property
    def num_steps(self):
        return int(self._vec.num_steps[0])

    @property
    def num_sim_steps(self):
        return int(self._vec.num_sim_steps[0])

    @property
    def have_tear(self):
        return bool(self._vec.have_tear[0])

    def reset(self):
        self.cloth._invalidate()
        if self._start_state is not None:                             # cloth_env.py:736-741, :771-772
            s = self._start_state
            v = self._vec
            rng = v.np_randoms[0]
            v.init_side[0] = rng.rand() > 0.5                          # Cloth(state=...) still draws init_side, cloth.pyx:75
            self.cloth.init_side = bool(v.init_side[0])
            v.batch.set_state(s['pos'][None], s['prev'][None], s['pinned'][None],
                              s['rest'] if 'rest' in s else None, rest_shared=True if 'rest' in s else None)
            v.num_steps[:] = 0; v.num_sim_steps[:] = 0; v.have_tear[:] = False
            self.cloth._rebuilt(s['pos'])                              # the new Cloth's springs / colour set / orig_* 
            cov, vinv, _, _ = v.batch.metrics()
            v._prev_reward[:] = cov; v._start_coverage[:] = cov; v._start_variance_inv[:] = vinv
            v._current_coverage[:] = 0.0
            if v._consume_domrand:                                     # cloth_env.py:786-789, as in the normal reset
                domrand_draws(rng, v._wd, v._hd)
            return self.state
        obs = self._vec.reset()[0]
        self.cloth.init_side = bool(self._vec.init_side[0])
        built = getattr(self._vec, "_built_pos0", None)
        self.cloth._rebuilt(built if built is not None else self._vec.batch.init_grid(1)[0])
        return obs

    def step(self, action, initialize=False):
        self.cloth._invalidate()
        out = self._vec.step(np.asarray(action, dtype=np.float64)[None], initialize=initialize)
        if out is None:
            return None
        obs, rew, done, info = out
        info1 = {k: (v[0].item() if hasattr(v[0], 'item') else v[0]) for k, v in info.items()}
        return obs[0], float(rew[0]), bool(done[0]), info1

    def get_random_action(self, atype='over_xy_plane'):
        if atype == 'over_xy_plane':
            return self.action_space.sample()
        raise ValueError(atype)

    def snapshot(self):
        """ClothVecEnv.snapshot of the single env."""
        return self._vec.snapshot()

    def restore(self, snap):
        """Back to where snapshot() saw the env (ClothVecEnv.restore)."""
        self.cloth._invalidate()
        self._vec.restore(snap)
        self.cloth.init_side = bool(self._vec.init_side[0])

    def set_material(self, **fields):
        """The env's material: density, ks, damping, plane_friction, tear_thresh, gravity (ClothVecEnv.set_material)."""
        self._vec.set_material(None, **fields)

    @property
    def material(self):
        return self._vec.material[0]

    def save_state(self, cloth_file):
        """cloth_env.py:343-350 (npz of SoA arrays instead of a pickle of Python objects)."""
        pos, prev, pin = self._vec.batch.get_state()
        np.savez(cloth_file, pos=pos[0], prev=prev[0], pinned=pin[0], rest=self._vec.batch.get_rest(0, 1)[0])

    def _compute_coverage(self):
        return float(self._vec._compute_coverage()[0])

    def _compute_variance(self):
        return float(self._vec._compute_variance()[0])

    def _out_of_bounds(self):
        return bool(self._vec._out_of_bounds()[0])

    def _convert_action_to_clip_space(self, a):
        return tuple(self._vec._convert_action_to_clip_space(np.asarray(a, dtype=np.float64)))

    def render(self, *a, **k):
        """The OpenGL viewer / Blender renderer are out of scope (components 7, 13)."""
        return None
