"""ClothBatch: E independent cloths resident on one MI355X, stepped by libclothhip.

This is the batched counterpart of the reference's `Cloth` + `Gripper` pair (gym_cloth/physics/cloth.pyx:21,
gripper.pyx:8); the single-cloth façade with the reference's attribute names lives in physics.py.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import F32, F64, SCHED_DTYPE, check

# ClothBatch._launch, the last episode launch of a batch: T slots and R reset scripts per env (the shapes of the tables it left on the
# device: render_obs('slots' / 'resets'), run_actions_labels), and between run_actions_begin and run_actions_end what the second half needs
LastLaunch = namedtuple("LastLaunch", "T R pending")
PendingLaunch = namedtuple("PendingLaunch", "num_steps done have_rst have_obs have_robs rng_states")


def make_schedules(n, **fields):
    """A zeroed ClothSchedule[n] numpy record array with `fields` broadcast in."""
    s = np.zeros(n, dtype=SCHED_DTYPE)
    for k, v in fields.items():
        s[k] = v
    return s


def schedule_bounds(iters_up, iters_up_rest, iters_pull, iters_grip_rest, iters_rest):
    """Integer phase boundaries of ClothEnv.step (cloth_env.py:472-475) / _pull (:352-367).

    The reference compares an int `i` with cumulative sums that may be floats (tier 3 draws a float
    iters_up, cloth_env.py:960); `i < b` for integer i is `i < ceil(b)`, so the ceilings are exact.
    The sums are formed left to right exactly as the reference writes them.
    """
    b1 = iters_up
    b2 = iters_up + iters_up_rest
    b3 = iters_up + iters_up_rest + iters_pull
    b4 = iters_up + iters_up_rest + iters_pull + iters_grip_rest
    b5 = iters_up + iters_up_rest + iters_pull + iters_grip_rest + iters_rest
    return tuple(int(np.ceil(b)) for b in (b1, b2, b3, b4, b5))


class ClothBatch(object):
    def __init__(self, cfg, n_envs=1, device=0, precision="f32", gravity=-9.8, minimum_z=0.0):
        self._L = _lib.load()
        self.cfg = cfg
        self.params = _lib.params_from_cfg(cfg, gravity=gravity, minimum_z=minimum_z)
        self.precision = {"f64": F64, "f32": F32, F64: F64, F32: F32}[precision]
        h = C.c_void_p()
        check(self._L.clothhip_create(C.byref(self.params), int(n_envs), int(device), self.precision, C.byref(h)))
        self._h = h
        self.E = int(n_envs)
        self.P = self._L.clothhip_num_points(h)
        self.S = self._L.clothhip_num_springs(h)
        self.N = self.params.n_side
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.clothhip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # ---- construction helpers (host, double) ---------------------------------------------------------
    def init_grid(self, tier=1, init_side=False, rand_draws=None):
        """(pos[P,3], rest[S]) of a freshly constructed Cloth (cloth.pyx:92-146, :411-417)."""
        pos = np.empty((self.P, 3)); rest = np.empty(self.S)
        rd = None if rand_draws is None else np.ascontiguousarray(rand_draws, dtype=np.float64)
        check(self._L.clothhip_init_grid(C.byref(self.params), int(tier), int(bool(init_side)),
                                         _lib.dp(rd), _lib.dp(pos), _lib.dp(rest)))
        return pos, rest

    def topology(self):
        a = np.empty(self.S, dtype=np.int32); b = np.empty(self.S, dtype=np.int32)
        t = np.empty(self.S, dtype=np.uint8)
        check(self._L.clothhip_spring_topology(C.byref(self.params), _lib.i32p(a), _lib.i32p(b), _lib.u8p(t)))
        return a, b, t

    # ---- state -----------------------------------------------------------------------------------------
    def set_state(self, pos=None, prev=None, pinned=None, rest=None, env0=0, n=None, rest_shared=None,
                  keep_tear=False):
        """Upload state of envs [env0, env0+n). keep_tear: a write into a live cloth (the reference's tear flag is
        sticky, cloth.pyx:272-273); without it the call is the Cloth(...) rebuild of a reset and clears the flag."""
        n = self.E - env0 if n is None else n
        f = lambda a, shp: None if a is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(a, dtype=np.float64), shp))
        pos = f(pos, (n, self.P, 3)); prev = f(prev, (n, self.P, 3))
        pin = None if pinned is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(pinned, dtype=np.uint8), (n, self.P)))
        if rest is not None:
            rest = np.asarray(rest, dtype=np.float64)
            if rest_shared is None:
                rest_shared = rest.ndim == 1
            rest = np.ascontiguousarray(rest if rest_shared else np.broadcast_to(rest, (n, self.S)))
        flags = (_lib.REST_SHARED if rest_shared else 0) | (_lib.KEEP_TEAR if keep_tear else 0)
        check(self._L.clothhip_set_state(self._h, env0, n, _lib.dp(pos), _lib.dp(prev), _lib.u8p(pin),
                                         _lib.dp(rest), flags))

    # ---- per-env materials -----------------------------------------------------------------------------
    def set_material(self, material=None, env0=0, n=None):
        """Give envs [env0, env0+n) a material of their own (clothhip_set_material): density, ks, damping, plane_friction,
        tear_thresh, gravity -- what Cloth.update() reads from the cfg on every call (cloth.pyx:175-186). `material`: a structured
        array of _lib.MATERIAL_DTYPE, or a dict with all six fields (scalars or arrays, broadcast over the n envs); None: these envs go
        back to the handle's parameters. n defaults to the array's length, else to every env from env0 on. The material stays with the
        env slot through set_state, reset_flat and episode resets."""
        if n is None and material is not None and not isinstance(material, dict) and np.ndim(material) == 1:
            n = len(material)
        n = self.E - env0 if n is None else int(n)
        if material is None:
            check(self._L.clothhip_set_material(self._h, int(env0), n, None))
            return
        if isinstance(material, dict):
            missing = [k for k in _lib.MATERIAL_FIELDS if k not in material]
            extra = [k for k in material if k not in _lib.MATERIAL_FIELDS]
            if missing or extra:
                raise ValueError("a material has exactly the fields %s (missing %s, unknown %s)" % (_lib.MATERIAL_FIELDS, missing, extra))
            m = np.empty(n, dtype=_lib.MATERIAL_DTYPE)
            for k in _lib.MATERIAL_FIELDS:
                m[k] = np.broadcast_to(np.asarray(material[k], dtype=np.float64), (n,))
        else:
            m = np.asarray(material)
            if m.dtype.names is None or set(m.dtype.names) != set(_lib.MATERIAL_FIELDS):
                raise ValueError("material must be a structured array with the fields %s" % (_lib.MATERIAL_FIELDS,))
            src = np.broadcast_to(m, (n,))
            m = np.empty(n, dtype=_lib.MATERIAL_DTYPE)
            for k in _lib.MATERIAL_FIELDS:                # by NAME: numpy converts structured dtypes by position
                m[k] = src[k]
        m = np.ascontiguousarray(m)
        check(self._L.clothhip_set_material(self._h, int(env0), n, m.ctypes.data_as(C.c_void_p)))

    def get_material(self, env0=0, n=None):
        """The effective materials of envs [env0, env0+n), _lib.MATERIAL_DTYPE[n] (the handle's parameters where none was set)."""
        n = self.E - env0 if n is None else int(n)
        m = np.zeros(n, dtype=_lib.MATERIAL_DTYPE)
        check(self._L.clothhip_get_material(self._h, int(env0), n, m.ctypes.data_as(C.c_void_p)))
        return m

    # ---- device-side copies of whole cloths ---------------------------------------------------------------
    def fork_from(self, src_batch, src_env, dst_env=None, state_only=False):
        """Make env dst_env[j] of THIS batch a copy of env src_env[j] of `src_batch`, on the device (clothhip_fork): positions,
        previous positions, the pin bytes as they are (grab multiplicities, pinned-from-outside), the tear flag, the rest lengths
        and -- unless state_only -- the material. One source may feed many destinations. dst_env None: envs 0 .. len(src_env)-1.
        The batches must agree in device, precision and grid; src_batch may be this batch when the two lists are disjoint."""
        src = np.ascontiguousarray(np.atleast_1d(src_env), dtype=np.int32)
        dst = np.arange(len(src), dtype=np.int32) if dst_env is None else np.ascontiguousarray(np.atleast_1d(dst_env), dtype=np.int32)
        if src.ndim != 1 or dst.shape != src.shape:
            raise ValueError("src_env and dst_env must be index lists of one length")
        check(self._L.clothhip_fork(self._h, _lib.i32p(dst), src_batch._h, _lib.i32p(src), len(src),
                                    _lib.FORK_STATE_ONLY if state_only else 0))

    def pin_counts(self, env0=0, n=None):
        """The raw pin byte of every point, uint8[n, P] (clothhip_get_pin_counts): bits 0-6 how many times the gripper holds the
        point, bit 7 pinned from outside (pin_points). get_state's `pinned` is this != 0."""
        n = self.E - env0 if n is None else int(n)
        c = np.empty((n, self.P), dtype=np.uint8)
        check(self._L.clothhip_get_pin_counts(self._h, int(env0), n, _lib.u8p(c)))
        return c

    def in_flight(self):
        """bool[E]: the env holds an operation that a time-sliced episode launch cut and the next launch continues
        (clothhip_in_flight)."""
        p = np.zeros(self.E, dtype=np.uint8)
        check(self._L.clothhip_in_flight(self._h, _lib.u8p(p)))
        return p.astype(bool)

    def get_rest(self, env0=0, n=None):
        """Spring.rest_length per env in reference list order, [n, S]."""
        n = self.E - env0 if n is None else n
        rest = np.empty((n, self.S))
        check(self._L.clothhip_get_rest(self._h, env0, n, _lib.dp(rest)))
        return rest

    def ensure_per_env_rest(self):
        """Give every env its own rest-length table (what tier 2 needs: cloth.pyx:417 measures them on the noisy sheet);
        a no-op once done. The tables start as copies of the current ones."""
        if not getattr(self, "_per_env_rest", False):
            self.set_state(rest=self.get_rest(), rest_shared=False)
            self._per_env_rest = True

    def reset_flat(self, mask=None):
        """Cloth(...) rebuild of the flat tiers (1, 3) on the device for the masked envs (None = all)."""
        m = None if mask is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mask, dtype=np.uint8), (self.E,)))
        check(self._L.clothhip_reset_flat(self._h, _lib.u8p(m)))

    def get_state(self, env0=0, n=None, want_prev=True, want_pinned=True):
        n = self.E - env0 if n is None else n
        pos = np.empty((n, self.P, 3))
        prev = np.empty((n, self.P, 3)) if want_prev else None
        pin = np.empty((n, self.P), dtype=np.uint8) if want_pinned else None
        check(self._L.clothhip_get_state(self._h, env0, n, _lib.dp(pos), _lib.dp(prev), _lib.u8p(pin)))
        return pos, prev, pin

    def positions(self, env0=0, n=None):
        return self.get_state(env0, n, want_prev=False, want_pinned=False)[0]

    @property
    def tear(self):
        t = np.empty(self.E, dtype=np.uint8)
        check(self._L.clothhip_get_tear(self._h, _lib.u8p(t)))
        return t.astype(bool)

    @tear.setter
    def tear(self, v):
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.uint8), (self.E,)))
        check(self._L.clothhip_set_tear(self._h, _lib.u8p(t)))

    def metrics(self, want_height=False):
        """(coverage[E], variance_inv[E], out_of_bounds[E], tear[E]) as ClothEnv computes them
        (cloth_env.py:1020-1098); with want_height also the 'height' reward's fraction of points with
        z < thickness/2 (cloth_env.py:603-609)."""
        cov = np.empty(self.E); vinv = np.empty(self.E)
        oob = np.empty(self.E, dtype=np.uint8); tear = np.empty(self.E, dtype=np.uint8)
        nlow = np.empty(self.E, dtype=np.int32) if want_height else None
        check(self._L.clothhip_metrics_ex(self._h, _lib.dp(cov), _lib.dp(vinv), _lib.u8p(oob), _lib.u8p(tear),
                                          _lib.i32p(nlow)))
        if want_height:
            return cov, vinv, oob.astype(bool), tear.astype(bool), nlow / float(self.P)
        return cov, vinv, oob.astype(bool), tear.astype(bool)

    # ---- headless rendering ---------------------------------------------------------------
    @staticmethod
    def camera_matrix(cam_deg=(0.0, 0.0, 0.0)):
        """world -> camera rotation for Blender's `rotation_euler` (XYZ order, degrees) of the reference's camera
        (get_image_rep_279.py:119-122): camera-to-world = Rz Ry Rx, returned transposed as float32[9]."""
        ax, ay, az = np.deg2rad(np.asarray(cam_deg, dtype=np.float64))
        cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
        m = np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                      [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                      [-sy, cy * sx, cy * cx]])
        return np.ascontiguousarray(m.T.reshape(9), dtype=np.float32)

    RENDER_DEFAULTS = dict(width=224, height=224, cam_pos=(0.5, 0.5, 1.45), cam_deg=(0.0, 0.0, 0.0), lens_mm=40.0,
                           sensor_mm=36.0, front=(0.070, 0.050, 0.600), back=(0.070, 0.300, 0.900),
                           background=(1.0, 1.0, 1.0), light_dir=(0.5169, 0.0730, 0.8530), ambient=0.05, energy=1.5)

    def render_params(self, **kw):
        """_lib.ClothRenderParams of the reference's scene (get_image_rep_279.py: camera :114-122, lens :273-276, side colours
        :249-257, bed :172, lamp energy :450; light_dir = the direction from the cloth centre to Blender's default lamp);
        any field can be overridden, cam_deg instead of world_to_cam."""
        d = dict(self.RENDER_DEFAULTS); d.update(kw)
        p = _lib.ClothRenderParams()
        p.width, p.height = int(d["width"]), int(d["height"])
        w2c = d["world_to_cam"] if "world_to_cam" in d else self.camera_matrix(d["cam_deg"])
        for k in range(9):
            p.world_to_cam[k] = float(w2c[k])
        for name in ("cam_pos", "front", "back", "background", "light_dir"):
            for k in range(3):
                getattr(p, name)[k] = float(d[name][k])
        p.lens_mm, p.sensor_mm, p.ambient, p.energy = float(d["lens_mm"]), float(d["sensor_mm"]), float(d["ambient"]), float(d["energy"])
        return p

    def render(self, want_rgb=True, want_depth=True, swap_sides=None, params=None, **kw):
        """Rasterise every env's cloth mesh (cloth_env.py:212-330 without Blender): (rgb uint8 [E, H, W, 3] or None,
        depth float32 [E, H, W] camera-space distance or None)."""
        p = params if params is not None else self.render_params(**kw)
        rgb = np.empty((self.E, p.height, p.width, 3), dtype=np.uint8) if want_rgb else None
        dep = np.empty((self.E, p.height, p.width), dtype=np.float32) if want_depth else None
        sw = None if swap_sides is None else np.ascontiguousarray(np.broadcast_to(np.asarray(swap_sides, dtype=np.uint8), (self.E,)))
        check(self._L.clothhip_render(self._h, C.byref(p), _lib.u8p(sw), _lib.u8p(rgb),
                                      _lib.fp(dep)))
        return rgb, dep

    def render_obs(self, source, obs=None, valid=None, swap_sides=None, fmt='rgbd', params=None, out_device_ptr=None, **render_kw):
        """Finished image observations of many cloths in one call (clothhip_render_obs): uint8 [n, H, W, C], C = 4 for
        fmt 'rgbd', 3 for 'rgb' and 'depth' (the 8-bit depth replicated). source: 'state' (this batch's particles, n = E),
        'slots' / 'resets' (the obs_t / reset_obs tables the last run_actions launch left on the device, n = T * E in [t][e]
        order / E * R in [e][k] order) or 'host' (obs: float32 [n, 3P] '1d' observations). valid[n]: False = not rendered,
        all bytes zero; swap_sides[n]: swap the two side colours of that image. out_device_ptr: also keep the images in
        that device buffer (n * H * W * C bytes). The pixels are those of render() for the same float32 positions."""
        p = params if params is not None else self.render_params(**render_kw)
        src = _lib.OBS_SOURCES[source] if isinstance(source, str) else int(source)
        f = _lib.IMG_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)
        if src == _lib.OBS_HOST:
            obs = np.ascontiguousarray(obs, dtype=np.float32)
            if obs.ndim != 2 or obs.shape[1] != 3 * self.P:
                raise ValueError("obs must have shape (n, %d)" % (3 * self.P))
            n = obs.shape[0]
        elif src == _lib.OBS_STATE:
            n = self.E
        else:
            last = getattr(self, '_launch', None)                     # the last run_actions launch
            n = 0 if last is None else (last.T * self.E if src == _lib.OBS_SLOTS else self.E * last.R)
        flag = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a).astype(bool).astype(np.uint8), (n,)))
        v, sw = flag(valid), flag(swap_sides)
        out = np.empty((n, p.height, p.width, 4 if f == _lib.IMG_RGBD else 3), dtype=np.uint8)
        check(self._L.clothhip_render_obs(self._h, C.byref(p), src, _lib.fp(obs),
                                          n, _lib.u8p(v), _lib.u8p(sw), f, _lib.u8p(out),
                                          None if out_device_ptr is None else C.c_void_p(int(out_device_ptr))))
        return out

    # ---- gripper ---------------------------------------------------------------------------------------
    def _grab(self, fn, xy, radius, active):
        xy = np.ascontiguousarray(np.broadcast_to(np.asarray(xy, dtype=np.float64), (self.E, 2)))
        rad = None if radius is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.E,)))
        act = None if active is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(active, dtype=np.uint8), (self.E,)))
        n = np.zeros(self.E, dtype=np.int32)
        check(fn(self._h, _lib.dp(xy), _lib.dp(rad), _lib.u8p(act), _lib.i32p(n)))
        return n

    def grab_top(self, xy, radius=None, active=None):
        return self._grab(self._L.clothhip_grab_top, xy, radius, active)

    def grab(self, xy, radius=None, active=None):
        return self._grab(self._L.clothhip_grab, xy, radius, active)

    def release(self, active=None):
        act = None if active is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(active, dtype=np.uint8), (self.E,)))
        check(self._L.clothhip_release(self._h, _lib.u8p(act)))

    def pin_points(self, env, idx):
        idx = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int32)
        check(self._L.clothhip_pin_points(self._h, int(env), _lib.i32p(idx), len(idx)))

    # ---- stepping --------------------------------------------------------------------------------------
    def run(self, sched):
        """Run ClothSchedule[E] (see include/clothhip.h); returns executed update() counts [E]."""
        sched = np.ascontiguousarray(sched, dtype=SCHED_DTYPE)
        if sched.shape != (self.E,):
            raise ValueError("sched must have shape (%d,)" % self.E)
        ex = np.zeros(self.E, dtype=np.int32)
        check(self._L.clothhip_run(self._h, sched.ctypes.data_as(C.c_void_p), _lib.i32p(ex)))
        return ex

    def run_async(self, sched):
        sched = np.ascontiguousarray(sched, dtype=SCHED_DTYPE)
        if sched.shape != (self.E,):
            raise ValueError("sched must have shape (%d,)" % self.E)
        check(self._L.clothhip_run_async(self._h, sched.ctypes.data_as(C.c_void_p)))

    def sync(self, want_executed=True):
        ex = np.zeros(self.E, dtype=np.int32) if want_executed else None
        check(self._L.clothhip_sync(self._h, _lib.i32p(ex)))
        return ex

    @property
    def fused_supported(self):
        return bool(check(self._L.clothhip_fused_supported(self._h)))

    def run_actions_begin(self, ep, n_actions, num_steps, done, actions=None, policy=None, policy_arg=None, scripts=None,
                          want_resets=True, want_obs=False, actions_device_ptr=None, time_budget_ms=0.0,
                          rng_states=None, rng_tier=0, domrand_words=0, reset_capacity=0, expert=None, expert_mix=None,
                          expert_choices=None):
        """First half of clothhip_run_actions (see include/clothhip.h): upload + launch, returns while the kernel runs.
        ep: _lib.ClothEpisodeParams; scripts: RESET_SCRIPT_DTYPE[E, R], each env's next R resets in order.
        expert ('oracle_corner' | 'highest_point' or its CLOTHHIP_POLICY_* code) arms this launch with a silent expert
        (clothhip_run_actions_expert): expert_mix bool[T, E] (None: it never acts), expert_choices int[T, E] (highest point);
        run_actions_labels() gives its labels after run_actions_end(). want_obs='device' writes the observation tables as True does but
        keeps them on the device (run_actions_end returns None for them): render_obs('slots' / 'resets') and fit_append_launch read them."""
        T = int(n_actions)
        keep = isinstance(want_obs, str)
        if keep and want_obs != 'device':
            raise ValueError("want_obs must be False, True or 'device' (got %r)" % (want_obs,))
        mix, cho = self._expert_tables(expert, expert_mix, expert_choices, T)
        pol = _lib.POLICY_TABLE if policy is None else int(policy)
        on_dev = 0
        ap = None
        if pol == _lib.POLICY_TABLE or (pol == _lib.POLICY_MLP and (actions is not None or actions_device_ptr is not None)):
            if actions_device_ptr is not None:
                ap, on_dev = C.c_void_p(int(actions_device_ptr)), 1
            else:
                actions = np.ascontiguousarray(actions, dtype=np.float64)
                if actions.shape != (T, self.E, 4):
                    raise ValueError("actions must have shape (%d, %d, 4)" % (T, self.E))
                ap = actions.ctypes.data_as(C.c_void_p)
        assert num_steps.dtype == np.int32 and num_steps.shape == (self.E,) and num_steps.flags['C_CONTIGUOUS']
        assert done.dtype == np.uint8 and done.shape == (self.E,) and done.flags['C_CONTIGUOUS']
        parg = None if policy_arg is None else np.ascontiguousarray(policy_arg, dtype=np.int32)
        if pol == _lib.POLICY_HIGHEST_POINT and (parg is None or parg.shape != (1 + T, self.E)):
            raise ValueError("the highest-point policy needs policy_arg int32[1 + %d, %d]: construction codes, then which of "
                             "the highest points every env pulls in every slot" % (T, self.E))
        if pol != _lib.POLICY_HIGHEST_POINT and parg is not None and parg.shape != (self.E,):
            raise ValueError("policy_arg must have shape (%d,)" % self.E)
        if scripts is not None:
            scripts = np.ascontiguousarray(scripts, dtype=_lib.RESET_SCRIPT_DTYPE)
            if scripts.ndim != 2 or scripts.shape[0] != self.E:
                raise ValueError("scripts must have shape (%d, R)" % self.E)
        if rng_states is not None:                       # resets drawn on the device from the envs' numpy streams
            assert scripts is None and rng_states.dtype == np.uint32 and rng_states.shape == (self.E, _lib.MT_WORDS)
            assert rng_states.flags['C_CONTIGUOUS']
        have_src = scripts is not None or rng_states is not None
        R = scripts.shape[1] if scripts is not None else (int(reset_capacity) if rng_states is not None else 0)
        have_rst = bool(want_resets and have_src)
        have_robs = bool(want_obs and have_src)
        if expert is not None:                           # (the library copies both tables; the arming is for the very next launch alone)
            check(self._L.clothhip_run_actions_expert(self._h, _lib.EXPERTS.get(expert, expert), T, _lib.u8p(mix), _lib.i32p(cho)))
        check(self._L.clothhip_run_actions_begin(self._h, C.byref(ep), T, pol, ap, on_dev, _lib.i32p(parg), _lib.vp(scripts), R,
                                                 _lib.i32p(num_steps), _lib.u8p(done), _lib.vp(rng_states), int(rng_tier),
                                                 int(domrand_words), int(have_rst), 2 if keep else int(bool(want_obs)),
                                                 2 if keep and have_robs else int(have_robs), float(time_budget_ms)))
        self._launch = LastLaunch(T, R, PendingLaunch(num_steps, done, have_rst, bool(want_obs) and not keep, have_robs and not keep, rng_states))

    def run_actions_end(self):
        """Second half: wait for the launch and fetch its outputs. num_steps / done given to _begin are updated in place.
        rng_states given to _begin (uint32[E, 626]) now hold the advanced streams.
        Returns (records[T, E], resets[E, R] or None, obs float32[T, E, 3P] or None, reset_obs float32[E, R, 3P] or None:
        the first observation of every episode started inside the launch)."""
        (T, R, p), vp = self._launch, _lib.vp
        self._launch = LastLaunch(T, R, None)                # (the shapes stay: the tables the launch leaves on the device have them)
        rec = np.zeros((T, self.E), dtype=_lib.STEP_RECORD_DTYPE)
        rst = np.zeros((self.E, R), dtype=_lib.RESET_RECORD_DTYPE) if p.have_rst else None
        obs = np.empty((T, self.E, 3 * self.P), dtype=np.float32) if p.have_obs else None
        robs = np.empty((self.E, R, 3 * self.P), dtype=np.float32) if p.have_robs else None
        check(self._L.clothhip_run_actions_end(self._h, _lib.i32p(p.num_steps), _lib.u8p(p.done), vp(rec), vp(rst), vp(obs),
                                               vp(robs), vp(p.rng_states)))
        return rec, rst, obs, robs

    def _expert_tables(self, expert, expert_mix, expert_choices, T):
        """(mix uint8[T, E] or None, choices int32[T, E] or None) as clothhip_run_actions_expert takes them. ValueError for an unknown
        expert, tables without an expert, a wrong shape, and expert_choices with or without expert='highest_point' as it must not / must be."""
        if expert is None:
            if expert_mix is not None or expert_choices is not None:
                raise ValueError("expert_mix / expert_choices go with expert='oracle_corner' or 'highest_point'")
            return None, None
        code = _lib.EXPERTS.get(expert, expert)
        if code not in _lib.EXPERTS.values():
            raise ValueError("expert must be None, 'oracle_corner' or 'highest_point' (got %r)" % (expert,))
        mix = cho = None
        if expert_mix is not None:
            mix = np.asarray(expert_mix)
            if mix.shape != (T, self.E):
                raise ValueError("expert_mix must have shape (%d, %d) (got %r)" % (T, self.E, mix.shape))
            mix = np.ascontiguousarray(mix != 0, dtype=np.uint8)
        if (expert_choices is not None) != (code == _lib.POLICY_HIGHEST_POINT):
            raise ValueError("expert_choices int[T, E] goes with expert='highest_point', and only with it")
        if expert_choices is not None:
            cho = np.asarray(expert_choices)
            if cho.shape != (T, self.E) or not np.issubdtype(cho.dtype, np.integer):
                raise ValueError("expert_choices must be integers of shape (%d, %d)" % (T, self.E))
            cho = np.ascontiguousarray(cho, dtype=np.int32)
        return mix, cho

    def run_actions_labels(self, n_actions=None):
        """float64[T, E, 4]: the expert's labels of the last, armed episode launch (clothhip_run_actions_labels), NaN where the slot's
        `ran` is 0. ClothHipError when that launch was not armed."""
        T = int(self._launch.T if n_actions is None else n_actions)
        out = np.zeros((T, self.E, 4), dtype=np.float64)
        check(self._L.clothhip_run_actions_labels(self._h, _lib.dp(out), None))
        return out

    def policy_label(self, expert, obs=None, side=None, choices=None, clip_act_space=True):
        """The analytic expert ('oracle_corner' | 'highest_point') on float32 '1d' observations obs [n, 3P], or with obs=None on every
        env's present state: float64 [n, 4], what an episode launch with that policy records as its action (unclipped; in clip space
        with clip_act_space) -- clothhip_policy_label. side int[n]: 0 flat tiers, 1 / 2 tier 2 with init_side False / True (None: 0);
        choices int[n]: which of the highest points."""
        code = _lib.EXPERTS.get(expert, expert)
        if code not in _lib.EXPERTS.values():
            raise ValueError("expert must be 'oracle_corner' or 'highest_point' (got %r)" % (expert,))
        if obs is None:
            n, ptr = self.E, None
        else:
            obs = np.ascontiguousarray(obs, dtype=np.float32)
            if obs.ndim != 2 or obs.shape[1] != 3 * self.P:
                raise ValueError("obs must have shape (n, %d)" % (3 * self.P))
            n, ptr = obs.shape[0], _lib.fp(obs)
        tabs = []
        for name, a in (('side', side), ('choices', choices)):
            if a is not None:
                a = np.asarray(a)
                if a.shape != (n,):
                    raise ValueError("%s must have shape (%d,)" % (name, n))
                a = np.ascontiguousarray(a, dtype=np.int32)
            tabs.append(a)
        if (tabs[1] is not None) != (code == _lib.POLICY_HIGHEST_POINT):
            raise ValueError("choices int[n] goes with expert='highest_point', and only with it")
        out = np.zeros((n, 4), dtype=np.float64)
        check(self._L.clothhip_policy_label(self._h, code, int(bool(clip_act_space)), ptr, n, _lib.i32p(tabs[0]), _lib.i32p(tabs[1]), _lib.dp(out)))
        return out

    def run_summary(self):
        """float64[E, 4] written by the last episode launch: actions executed, episode over, coverage after the env's last
        action / reset of the launch (NaN: none), update() calls of its actions (clothhip_run_actions_summary)."""
        out = np.zeros((self.E, 4))
        check(self._L.clothhip_run_actions_summary(self._h, _lib.dp(out), None))
        return out

    @property
    def run_summary_device_ptr(self):
        """Device address of that table (for an in-place all-gather on the handle's stream)."""
        p = C.c_void_p()
        check(self._L.clothhip_run_actions_summary(self._h, None, C.byref(p)))
        return p.value

    def op_ticks(self):
        """Where the time of the last episode launch went, per env (clothhip_run_actions_op_ticks): (ticks uint64[E, 4] in 100 MHz
        ticks, substeps uint64[E, 4]) for the classes {actions, reset pulls, reset settling, the rest}."""
        raw = np.zeros((self.E, 8), dtype=np.uint64)
        check(self._L.clothhip_run_actions_op_ticks(self._h, raw.ctypes.data_as(C.c_void_p)))
        return raw[:, :4].copy(), raw[:, 4:].copy()

    def run_actions(self, *a, **k):
        """clothhip_run_actions: `n_actions` whole ClothEnv.step calls per env in one launch (begin + end)."""
        self.run_actions_begin(*a, **k)
        return self.run_actions_end()

    def set_policy_mlp(self, layers):
        """The handle's policy network (clothhip_set_policy_mlp): `layers` is a list of (W, b) with W [out, in] (torch.nn.Linear.weight's
        layout) and b [out], ReLU between them, the first `in` = 3 P, the last `out` = 4; None or [] clears it. The values are
        uploaded as float32; every env of the batch evaluates the same network. ValueError for shapes the library refuses."""
        self._mlp_n_params = 0                     # (fit_grad sizes its result by it: the shared network's parameters, 0 without one)
        self._pop_shape = None                     # (a shared network replaces a population)
        if not layers:
            check(self._L.clothhip_set_policy_mlp(self._h, 0, None, None, 0))
            return
        from .policies import pack_mlp
        widths, blob = pack_mlp(layers)
        check(self._L.clothhip_set_policy_mlp(self._h, len(widths) - 1, _lib.i32p(widths), blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size))
        self._mlp_n_params = int(blob.size)

    def policy_eval(self, obs=None):
        """The handle's network on float32 '1d' observations obs [n, 3P], or with obs=None on every env's present state: float64
        [n, 4], the network's output before noise and clipping, computed by the device function the episode launch runs
        (clothhip_policy_eval) -- the same bits."""
        if obs is None:
            n, ptr = self.E, None
        else:
            obs = np.ascontiguousarray(obs, dtype=np.float32)
            if obs.ndim != 2 or obs.shape[1] != 3 * self.P:
                raise ValueError("obs must have shape (n, %d)" % (3 * self.P))
            n, ptr = obs.shape[0], obs.ctypes.data_as(C.POINTER(C.c_float))
        out = np.zeros((n, 4), dtype=np.float64)
        check(self._L.clothhip_policy_eval(self._h, ptr, n, _lib.dp(out)))
        return out

    def _member_map(self, member, rows):
        """member as int32[E], checked against [0, rows): what the library would refuse is refused here first."""
        m = np.asarray(member)
        if m.shape != (self.E,):
            raise ValueError("member must have shape (%d,) (got %r)" % (self.E, m.shape))
        if not np.issubdtype(m.dtype, np.integer):
            raise ValueError("member must hold integers")
        if m.size and (m.min() < 0 or m.max() >= rows):
            raise ValueError("member values must lie in [0, %d)" % rows)
        return np.ascontiguousarray(m, dtype=np.int32)

    def set_policy_population(self, members, member):
        """A network per env slot (clothhip_set_policy_population): `members` is a list of G networks of ONE shape, each a list of (W, b)
        layers as set_policy_mlp takes them, `member` int[E] with env e running members[member[e]]. None or [] clears the handle's
        network. Replaces a shared network (and set_policy_mlp replaces a population). The networks belong to the env slots: resets and
        uploads leave them alone; forks and snapshots do not carry them."""
        self._pop_shape = None                     # (fit_grad_members sizes its result by it: (rows, n_params) of the population)
        if not members:
            check(self._L.clothhip_set_policy_population(self._h, 0, None, None, 0, None))
            return
        from .policies import pack_population
        widths, blob = pack_population(members, n_in=3 * self.P)
        m = self._member_map(member, blob.shape[0])
        check(self._L.clothhip_set_policy_population(self._h, len(widths) - 1, _lib.i32p(widths), _lib.fp(blob), blob.shape[0], _lib.i32p(m)))
        self._pop_shape = (int(blob.shape[0]), int(blob.shape[1]))

    def set_policy_members(self, member):
        """The map alone (clothhip_set_policy_members): member int[E], each below the population's number of rows."""
        m = np.asarray(member)
        if m.shape != (self.E,) or not np.issubdtype(m.dtype, np.integer):
            raise ValueError("member must be %d integers" % self.E)
        check(self._L.clothhip_set_policy_members(self._h, _lib.i32p(np.ascontiguousarray(m, dtype=np.int32))))

    def get_policy_mlp(self, g, n_params):
        """Blob g of the handle's population (g = 0: a shared network) as float32[n_params], downloaded (clothhip_get_policy_mlp). For a
        population n_params may be the row stride (policies.population_stride): the row with its pad."""
        out = np.zeros(int(n_params), dtype=np.float32)
        check(self._L.clothhip_get_policy_mlp(self._h, int(g), _lib.fp(out), out.size))
        return out

    def policy_eval_members(self, obs, members):
        """policy_eval with a network per row: row r under blob members[r] (clothhip_policy_eval_members); obs=None: every env's present
        state, members int[E]. float64 [n, 4], the bits the episode launch computes for an env slot that runs that blob."""
        m = np.ascontiguousarray(members, dtype=np.int32)
        if obs is None:
            n, ptr = self.E, None
        else:
            obs = np.ascontiguousarray(obs, dtype=np.float32)
            if obs.ndim != 2 or obs.shape[1] != 3 * self.P:
                raise ValueError("obs must have shape (n, %d)" % (3 * self.P))
            n, ptr = obs.shape[0], _lib.fp(obs)
        if m.shape != (n,):
            raise ValueError("members must have shape (%d,)" % n)
        out = np.zeros((n, 4), dtype=np.float64)
        check(self._L.clothhip_policy_eval_members(self._h, ptr, n, _lib.i32p(m), _lib.dp(out)))
        return out

    def population_perturb(self, center_layers, n_members, sigma, seed, antithetic=True, member=None):
        """G = n_members perturbed copies of one network made on the device (clothhip_policy_population_perturb;
        csrc/cloth_policy_population.hpp defines the noise): rows 2k, 2k + 1 = theta +- sigma eps_k with antithetic=True (G even), else row
        g = theta + sigma eps_g; row G = theta. member int[E] in [0, G], default e % (G + 1). sigma is rounded to float32; seed is an
        integer in [0, 2^64). Returns (widths, n_params)."""
        from .policies import pack_mlp
        widths, blob = pack_mlp(center_layers, n_in=3 * self.P)
        G = int(n_members)
        if not 1 <= G <= _lib.POP_MAX_G:
            raise ValueError("n_members = %d outside [1, %d]" % (G, _lib.POP_MAX_G))
        if antithetic and G % 2:
            raise ValueError("n_members = %d: antithetic perturbations come in pairs, n_members must be even" % G)
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must lie in [0, 2^64)")
        if not np.isfinite(np.float32(sigma)):
            raise ValueError("sigma is not finite")
        m = self._member_map(np.arange(self.E) % (G + 1) if member is None else member, G + 1)
        check(self._L.clothhip_policy_population_perturb(self._h, len(widths) - 1, _lib.i32p(widths), _lib.fp(blob), G, float(np.float32(sigma)),
                                                         int(seed), _lib.POP_ANTITHETIC if antithetic else 0, _lib.i32p(m)))
        self._pop_n_params = blob.size
        self._pop_shape = (G + 1, int(blob.size))
        return widths, blob.size

    def population_combine(self, coef):
        """float32[n_params] of the last population_perturb: sum_k coef[k] eps_k, accumulated in float64 in ascending k, eps made again on the device from the seed of
        the last population_perturb (clothhip_policy_population_combine). len(coef) = G / 2 with antithetic, else G."""
        c = np.ascontiguousarray(coef, dtype=np.float32)
        if c.ndim != 1:
            raise ValueError("coef must be one-dimensional")
        out = np.zeros(getattr(self, '_pop_n_params', 0), dtype=np.float32)      # (set by the last perturb that succeeded: the one the library sums, or it refuses before it writes)
        check(self._L.clothhip_policy_population_combine(self._h, _lib.fp(c), c.size, _lib.fp(out)))
        return out

    @staticmethod
    def _fit_weights(weights, n, what="weights"):
        """A table of per-row loss weights (or, by `what`, another float32 column of the dataset) as float32[n], finite (any sign, zero
        allowed); None stays None: 1 for every row."""
        if weights is None:
            return None
        w64 = np.asarray(weights, dtype=np.float64)
        if w64.shape != (n,):
            raise ValueError("%s must have shape (%d,) (got %r)" % (what, n, w64.shape))
        with np.errstate(over='ignore'):                  # (a double past float32's range becomes inf, refused below)
            w = np.ascontiguousarray(w64, dtype=np.float32)
        if not np.isfinite(w).all():
            raise ValueError("%s must be finite (float32)" % what)
        return w

    def fit_append(self, obs, labels, weights=None):
        """Append (observation row, action label) pairs to the handle's device-resident dataset (clothhip_fit_data_append): obs [n, 3P]
        (stored as float32), labels [n, 4] (stored as float32), weights [n] (the rows' loss weights, float32, any finite value; None:
        1 for every row -- clothhip_fit_data_append_weighted). ValueError for other shapes or non-finite values (dagger_rollout gives
        NaN labels where a slot did not run: pass the [ran] rows); nothing is appended then. Returns the dataset's size."""
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        lab = np.ascontiguousarray(labels, dtype=np.float64)
        if obs.ndim != 2 or obs.shape[1] != 3 * self.P:
            raise ValueError("obs must have shape (n, %d)" % (3 * self.P))
        if lab.shape != (obs.shape[0], 4):
            raise ValueError("labels must have shape (%d, 4)" % obs.shape[0])
        if not (np.isfinite(obs).all() and np.isfinite(lab).all() and (np.abs(lab) <= np.finfo(np.float32).max).all()):
            raise ValueError("obs and labels must be finite (float32)")
        w = self._fit_weights(weights, obs.shape[0])
        if w is None:
            check(self._L.clothhip_fit_data_append(self._h, _lib.fp(obs), _lib.dp(lab), obs.shape[0]))
        else:
            check(self._L.clothhip_fit_data_append_weighted(self._h, _lib.fp(obs), _lib.dp(lab), _lib.fp(w), obs.shape[0]))
        return self.fit_size()

    def fit_set_weights(self, weights, first=0):
        """Write the loss weights of the stored rows [first, first + len(weights)) (clothhip_fit_data_set_weights): any finite float32,
        negative and zero allowed. The weight is the one column of a stored row that can be rewritten -- a row is appended when its
        observation exists, its return is known when its episode ends."""
        w = self._fit_weights(weights, len(weights))
        check(self._L.clothhip_fit_data_set_weights(self._h, int(first), w.size, _lib.fp(w)))

    def fit_get_weights(self, first=0, n=None):
        """float32[n]: the loss weights of the stored rows [first, first + n), n=None: to the end (clothhip_fit_data_get_weights)."""
        first, n = self._fit_range(first, n)
        w = np.zeros(n, dtype=np.float32)
        check(self._L.clothhip_fit_data_get_weights(self._h, first, n, _lib.fp(w)))
        return w

    def fit_hold(self, src=None):
        """Fill the handle's held rows (clothhip_fit_hold): src=None -> held[e] = the float32 '1d' observation of env e's present state;
        src int[E, 2] = (source, row) with _lib.FIT_SRC_* -> held[e] = that row of the last launch's tables ((FIT_SRC_HELD, e) keeps it)."""
        if src is not None:
            src = np.asarray(src)
            if src.shape != (self.E, 2) or not np.issubdtype(src.dtype, np.integer):
                raise ValueError("src must be integers of shape (%d, 2)" % self.E)
            src = np.ascontiguousarray(src, dtype=np.int32)
        check(self._L.clothhip_fit_hold(self._h, _lib.i32p(src)))

    def fit_append_launch(self, rows, labels="expert", weights=None):
        """Append pairs that lie on the device (clothhip_fit_data_append_launch_ex): rows int[n, 3] = (source, row, label_row) -- the
        observation is that row of the last launch's tables or of the held rows; the label is row label_row = t * E + e of the last
        armed launch's labels (labels="expert"), or the action that slot of the last launch EXECUTED, (float32)out['actions'][t, e] read
        from the launch's records on the device (labels="action": for policy='mlp' the network's output plus the caller's noise; no
        expert needed), or with labels="zero" (0, 0, 0, 0) and label_row ignored: a leaf of the actor-critic, appended for its state alone.
        weights [n]: the rows' loss weights, None: 1. ValueError when a named value is not finite (a slot that did not
        run); nothing is appended then. Returns the dataset's size."""
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != 3 or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError("rows must be integers of shape (n, 3)")
        if labels != "zero" and labels not in _lib.FIT_LABELS:
            raise ValueError("labels must be one of %r or 'zero' (got %r)" % (sorted(_lib.FIT_LABELS), labels))
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        w = self._fit_weights(weights, rows.shape[0])
        src = _lib.FIT_LABEL_ZERO if labels == "zero" else _lib.FIT_LABELS[labels]
        check(self._L.clothhip_fit_data_append_launch_ex(self._h, _lib.i32p(rows), rows.shape[0], src, _lib.fp(w)))
        return self.fit_size()

    def fit_data(self, first=0, n=None):
        """(obs float32[n, 3P], labels float32[n, 4]): the stored rows [first, first + n), n=None: to the end (clothhip_fit_data_get)."""
        first, n = self._fit_range(first, n)
        obs = np.zeros((n, 3 * self.P), dtype=np.float32)
        lab = np.zeros((n, 4), dtype=np.float32)
        check(self._L.clothhip_fit_data_get(self._h, first, n, _lib.fp(obs), _lib.fp(lab)))
        return obs, lab

    def fit_loss(self, idx):
        """The MSE of the handle's shared network over the dataset rows idx [n], any n >= 1 (a held-out split by index), forward only
        (clothhip_policy_fit_loss); for n <= FIT_MAX_BATCH it is fit_grad's loss bit for bit."""
        ix = self._fit_rows(idx)
        self._fit_n_params()
        loss = np.zeros(1, dtype=np.float64)
        check(self._L.clothhip_policy_fit_loss(self._h, _lib.i32p(ix), ix.size, _lib.dp(loss)))
        return float(loss[0])

    def fit_predict(self, idx, members=None):
        """The trainer's forward on the stored rows idx [n], any n >= 1, nothing updated: float32[n, 4] of the shared network
        (clothhip_policy_fit_predict), or with members (distinct population rows) float32[n_m, n, 4], the same rows under every member
        (clothhip_policy_fit_predict_members). Row r is bit for bit the y fit_grad forms for dataset row idx[r] -- what the loss and its
        gradient are made of, so weights computed from it (residuals, trust regions, an ensemble's disagreement) describe the fit itself."""
        ix = self._fit_rows(idx)
        if members is None:
            self._fit_n_params()
            y = np.zeros((ix.size, 4), dtype=np.float32)
            check(self._L.clothhip_policy_fit_predict(self._h, _lib.i32p(ix), ix.size, _lib.fp(y)))
            return y
        m, _ = self._fit_members(members)
        y = np.zeros((m.size, ix.size, 4), dtype=np.float32)
        check(self._L.clothhip_policy_fit_predict_members(self._h, _lib.i32p(m), m.size, _lib.i32p(ix), ix.size, _lib.fp(y)))
        return y

    def fit_clear(self):
        """Empty the dataset (clothhip_fit_data_clear); the device memory stays with the handle."""
        check(self._L.clothhip_fit_data_clear(self._h))

    def fit_size(self):
        """Rows in the dataset (clothhip_fit_data_size)."""
        n = C.c_int64(0)
        check(self._L.clothhip_fit_data_size(self._h, C.byref(n)))
        return int(n.value)

    @staticmethod
    def _fit_rows(idx):
        """Any number >= 1 of dataset rows as int32: a 1-d integer list (fit_loss, fit_predict, value_predict)."""
        a = np.asarray(idx)
        if a.ndim != 1 or a.size < 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("idx must be a non-empty 1-d integer array")
        if a.min() < 0 or a.max() > np.iinfo(np.int32).max:
            raise ValueError("idx must hold row numbers of the dataset")
        return np.ascontiguousarray(a, dtype=np.int32)

    @staticmethod
    def _fit_idx(idx, ndim):
        """A minibatch index table as int32, C order: integers, `ndim` dimensions, at least one row per step, at most FIT_MAX_BATCH."""
        a = np.asarray(idx)
        if a.ndim != ndim or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("idx must be a %d-d integer array" % ndim)
        if not 1 <= a.shape[-1] <= _lib.FIT_MAX_BATCH:
            raise ValueError("a minibatch has 1 to %d rows (got %d)" % (_lib.FIT_MAX_BATCH, a.shape[-1]))
        if a.size and (a.min() < 0 or a.max() > np.iinfo(np.int32).max):
            raise ValueError("idx must hold row numbers of the dataset")
        return np.ascontiguousarray(a, dtype=np.int32)

    def fit_grad(self, idx):
        """(loss float, grad float32[n_params] in the blob's layout) of the handle's shared network over the dataset rows idx [B]
        (repeats count as often), at the present weights; nothing is updated (clothhip_policy_fit_grad). The loss is
        1 / (4 B) sum (y - label)^2, torch.nn.MSELoss()."""
        ix = self._fit_idx(idx, 1)
        n_params = self._fit_n_params()
        grad = np.zeros(n_params, dtype=np.float32)
        loss = np.zeros(1, dtype=np.float64)
        check(self._L.clothhip_policy_fit_grad(self._h, _lib.i32p(ix), ix.size, _lib.fp(grad), _lib.dp(loss)))
        return float(loss[0]), grad

    def _fit_n_params(self):
        n = getattr(self, '_mlp_n_params', 0)
        if not n:
            raise _lib.ClothHipError("no shared network on this batch: call set_policy_mlp first")
        return n

    @staticmethod
    def _fit_params(hyper, n_m):
        """_lib.ClothFitParams[n_m] from a dict with fit's keywords (optimizer, lr, beta1, beta2, eps, momentum), each value a scalar for
        all members or a sequence of n_m, rounded to float32; what the library would refuse is a ValueError here first."""
        hyper = dict(hyper or {})
        optimizer = hyper.pop('optimizer', 'adam')
        if optimizer not in _lib.FIT_OPTIMIZERS:
            raise ValueError("optimizer must be one of %r (got %r)" % (sorted(_lib.FIT_OPTIMIZERS), optimizer))
        vals = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0)
        unknown = sorted(set(hyper) - set(vals))
        if unknown:
            raise ValueError("unknown hyper-parameters %r" % unknown)
        vals.update(hyper)
        p = (_lib.ClothFitParams * n_m)()
        for k, v in vals.items():
            v = np.asarray(v, dtype=np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.size != n_m):
                raise ValueError("%s must be a scalar or %d values, one per member" % (k, n_m))
            v = np.broadcast_to(v, (n_m,)).astype(np.float32)
            if not (np.isfinite(v).all() and (v >= 0.0).all()) or (k.startswith('beta') and (v >= 1.0).any()):
                raise ValueError("%s = %r: hyper-parameters are finite and >= 0, the betas below 1" % (k, vals[k]))
            for j in range(n_m):
                setattr(p[j], k, float(v[j]))
        for j in range(n_m):
            p[j].optimizer = float(_lib.FIT_OPTIMIZERS[optimizer])
        return p

    def fit(self, idx_table, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        """n_steps optimizer steps on the handle's shared network, in place on the device (clothhip_policy_fit): step s uses the dataset
        rows idx_table[s] (int [n_steps, B]). optimizer 'adam' (lr, beta1, beta2, eps) or 'sgd' (lr, momentum); the hyper-parameters are
        rounded to float32. The moments and the step count persist across calls (fit_reset, or a new network, restarts them). Returns
        float64[n_steps]: each step's loss BEFORE its update. The next step_many(policy='mlp') runs the fitted weights."""
        ix = self._fit_idx(idx_table, 2)
        p = self._fit_params(dict(optimizer=optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum), 1)
        self._fit_n_params()
        loss = np.zeros(ix.shape[0], dtype=np.float64)
        check(self._L.clothhip_policy_fit(self._h, p, _lib.i32p(ix), ix.shape[0], ix.shape[1], _lib.dp(loss)))
        return loss

    def fit_reset(self):
        """Zero the optimizer's moments and its step count (clothhip_policy_fit_reset)."""
        check(self._L.clothhip_policy_fit_reset(self._h))

    # ---- the grouped trainer: rows of the population fitted in the launches of one network (clothhip_policy_fit*_members) ----------
    def _fit_members(self, members):
        """members as int32[n_m]: distinct rows of the batch's population ((rows, n_params) from the call that made it)."""
        shape = getattr(self, '_pop_shape', None)
        if shape is None:
            raise _lib.ClothHipError("no population on this batch: call set_policy_population or population_perturb first")
        m = np.asarray(members)
        if m.ndim != 1 or m.size < 1 or not np.issubdtype(m.dtype, np.integer):
            raise ValueError("members must be a non-empty 1-d integer array")
        if m.min() < 0 or m.max() >= shape[0]:
            raise ValueError("members must lie in [0, %d)" % shape[0])
        if np.unique(m).size != m.size:
            raise ValueError("members must be distinct: a call fits a row once")
        return np.ascontiguousarray(m, dtype=np.int32), shape[1]

    def _fit_members_idx(self, idx, n_m, ndim):
        ix = self._fit_idx(idx, ndim)
        if ix.shape[-2] != n_m:
            raise ValueError("idx must have %d rows of minibatch per step, one per member (got shape %r)" % (n_m, ix.shape))
        if n_m * ix.shape[-1] > _lib.FIT_MAX_MEMBER_ROWS:
            raise ValueError("%d members x %d rows in one call, at most %d" % (n_m, ix.shape[-1], _lib.FIT_MAX_MEMBER_ROWS))
        return ix

    def fit_grad_members(self, members, idx):
        """(loss float64[n_m], grad float32[n_m, n_params]) of the population rows `members` (distinct ints) over their own minibatches
        idx [n_m, B] of the batch's one dataset, at the present weights; nothing is updated (clothhip_policy_fit_grad_members). Member
        j's result is bit for bit fit_grad's on a batch that carries row members[j] as its shared network."""
        m, n_params = self._fit_members(members)
        ix = self._fit_members_idx(idx, m.size, 2)
        grad = np.zeros((m.size, n_params), dtype=np.float32)
        loss = np.zeros(m.size, dtype=np.float64)
        check(self._L.clothhip_policy_fit_grad_members(self._h, _lib.i32p(m), m.size, _lib.i32p(ix), ix.shape[1], _lib.fp(grad), _lib.dp(loss)))
        return loss, grad

    def fit_members(self, members, idx_table, hyper=None):
        """n_steps optimizer steps on the population rows `members`, in place on the device, all members in the launches of one
        (clothhip_policy_fit_members): step s of member j uses the dataset rows idx_table[s, j] (int [n_steps, n_m, B]). hyper: a dict
        with fit's keywords (optimizer, lr, beta1, beta2, eps, momentum), each value a scalar for all members or a sequence of n_m;
        the optimizer is one for the call. Every row keeps its own moments and step count across calls (fit_reset_members, or a new
        population, restarts them). Returns float64[n_steps, n_m]: each member's loss BEFORE each step's update -- the bits fit gives
        on a batch that carries the row as its shared network."""
        m, _ = self._fit_members(members)
        ix = self._fit_members_idx(idx_table, m.size, 3)
        p = self._fit_params(hyper, m.size)
        loss = np.zeros((ix.shape[0], m.size), dtype=np.float64)
        check(self._L.clothhip_policy_fit_members(self._h, p, _lib.i32p(m), m.size, _lib.i32p(ix), ix.shape[0], ix.shape[2], _lib.dp(loss)))
        return loss

    def fit_reset_members(self, members=None):
        """Zero the moments and the step count of the population rows `members`, None: of all rows (clothhip_policy_fit_reset_members)."""
        if members is None:
            check(self._L.clothhip_policy_fit_reset_members(self._h, None, 0))
            return
        m, _ = self._fit_members(members)
        check(self._L.clothhip_policy_fit_reset_members(self._h, _lib.i32p(m), m.size))

    # ---- actor-critic from reward: the value network, the transition columns, the critic's fit, GAE (clothhip.h: ACTOR-CRITIC FROM REWARD) ----
    def set_value_mlp(self, layers):
        """The handle's value network (clothhip_set_value_mlp): `layers` as set_policy_mlp takes them with a last `out` of 1; None or []
        drops it. It lives beside the policy network or population and independent of it; no launch evaluates it."""
        self._val_n_params = 0
        if not layers:
            check(self._L.clothhip_set_value_mlp(self._h, 0, None, None, 0))
            return
        from .policies import pack_mlp
        widths, blob = pack_mlp(layers, n_out=1)
        check(self._L.clothhip_set_value_mlp(self._h, len(widths) - 1, _lib.i32p(widths), _lib.fp(blob), blob.size))
        self._val_n_params = int(blob.size)

    def _value_n_params(self):
        n = getattr(self, '_val_n_params', 0)
        if not n:
            raise _lib.ClothHipError("no value network on this batch: call set_value_mlp first")
        return n

    def get_value_mlp(self):
        """The value network's blob as the device holds it, float32[n_params] (clothhip_get_value_mlp)."""
        out = np.zeros(self._value_n_params(), dtype=np.float32)
        check(self._L.clothhip_get_value_mlp(self._h, _lib.fp(out), out.size))
        return out

    def _fit_range(self, first, n):
        first = int(first)
        n = self.fit_size() - first if n is None else int(n)
        if first < 0 or n < 0:
            raise ValueError("first and n must be >= 0 and lie within the dataset")
        return first, n

    def fit_set_transitions(self, rew, next, first=0):
        """Write the reward and the successor of the stored rows [first, first + len(rew)) (clothhip_fit_data_set_transitions): rew
        finite float32, next int: the dataset index of the row with the successor state (greater than the row's own), or
        _lib.FIT_NEXT_TERMINAL (the episode ended), or _lib.FIT_NEXT_NONE (a leaf: the row has no transition, it only bootstraps)."""
        r = self._fit_weights(rew, len(rew), "rew")
        nx = np.asarray(next)
        if nx.shape != r.shape or not np.issubdtype(nx.dtype, np.integer):
            raise ValueError("next must hold %d integers" % r.size)
        if nx.size and (nx.min() < _lib.FIT_NEXT_NONE or nx.max() > np.iinfo(np.int32).max):
            raise ValueError("next must hold row numbers of the dataset, FIT_NEXT_TERMINAL or FIT_NEXT_NONE")
        nx = np.ascontiguousarray(nx, dtype=np.int32)
        check(self._L.clothhip_fit_data_set_transitions(self._h, int(first), r.size, _lib.fp(r), _lib.i32p(nx)))

    def fit_get_transitions(self, first=0, n=None):
        """(rew float32[n], next int32[n]) of the stored rows [first, first + n), n=None: to the end (clothhip_fit_data_get_transitions)."""
        first, n = self._fit_range(first, n)
        rew, nx = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
        check(self._L.clothhip_fit_data_get_transitions(self._h, first, n, _lib.fp(rew), _lib.i32p(nx)))
        return rew, nx

    def fit_set_returns(self, ret, first=0):
        """Write the value targets of the stored rows [first, first + len(ret)) (clothhip_fit_data_set_returns): finite float32."""
        r = self._fit_weights(ret, len(ret), "ret")
        check(self._L.clothhip_fit_data_set_returns(self._h, int(first), r.size, _lib.fp(r)))

    def fit_get_returns(self, first=0, n=None):
        """float32[n]: the value targets of the stored rows [first, first + n), n=None: to the end (clothhip_fit_data_get_returns)."""
        first, n = self._fit_range(first, n)
        ret = np.zeros(n, dtype=np.float32)
        check(self._L.clothhip_fit_data_get_returns(self._h, first, n, _lib.fp(ret)))
        return ret

    def value_grad(self, idx):
        """(loss float, grad float32[n_params] in the blob's layout) of the value network over the dataset rows idx [B], at the present
        weights; nothing is updated (clothhip_value_fit_grad). The loss is 1 / (2 B) sum (v - ret)^2, unweighted."""
        ix = self._fit_idx(idx, 1)
        grad = np.zeros(self._value_n_params(), dtype=np.float32)
        loss = np.zeros(1, dtype=np.float64)
        check(self._L.clothhip_value_fit_grad(self._h, _lib.i32p(ix), ix.size, _lib.fp(grad), _lib.dp(loss)))
        return float(loss[0]), grad

    def value_fit(self, idx_table, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        """fit for the value network (clothhip_value_fit): n_steps optimizer steps in place on the device, step s on the dataset rows
        idx_table[s] (int [n_steps, B]), with its own moments and step count (value_fit_reset, or a new value network, restarts them).
        Returns float64[n_steps]: each step's loss BEFORE its update. The policy's network and optimizer keep their bits."""
        ix = self._fit_idx(idx_table, 2)
        p = self._fit_params(dict(optimizer=optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum), 1)
        self._value_n_params()
        loss = np.zeros(ix.shape[0], dtype=np.float64)
        check(self._L.clothhip_value_fit(self._h, p, _lib.i32p(ix), ix.shape[0], ix.shape[1], _lib.dp(loss)))
        return loss

    def value_predict(self, idx):
        """float32[n]: the value network on the stored rows idx [n], any n >= 1, nothing updated (clothhip_value_predict) -- row r is bit
        for bit the v value_grad forms for dataset row idx[r]."""
        ix = self._fit_rows(idx)
        self._value_n_params()
        v = np.zeros(ix.size, dtype=np.float32)
        check(self._L.clothhip_value_predict(self._h, _lib.i32p(ix), ix.size, _lib.fp(v)))
        return v

    def value_fit_reset(self):
        """Zero the value network's moments and its step count (clothhip_value_fit_reset)."""
        check(self._L.clothhip_value_fit_reset(self._h))

    def fit_gae(self, gamma, lam, first=0, n=None, write_weights=True, normalize=False, w_scale=1.0, want=True):
        """Generalised advantage estimation over the stored rows [first, first + n) ON THE DEVICE (clothhip_fit_data_gae): the value
        network's forward over the range, then per non-leaf row A = sum_k (gamma lam)^k delta_k along its chain of successors,
        delta = rew + gamma V(next) - V (V(next) = 0 at a terminal row, the critic's value at a leaf); the value-target column gets
        (float32)(A + V), a leaf's gets V. write_weights: the weight column gets (float32)(w_scale A), or with normalize
        w_scale (A - mean) / (std + 1e-8) over the non-leaf rows; a leaf gets 0. Returns (adv float32[n], ret float32[n]), or None
        with want=False (nothing is downloaded). policies.gae_reference states the arithmetic."""
        first, n = self._fit_range(first, n)
        g, l, ws = float(gamma), float(lam), float(np.float32(w_scale))
        if not (np.isfinite(g) and np.isfinite(l) and np.isfinite(ws)) or not (0.0 <= g <= 1.0 and 0.0 <= l <= 1.0):
            raise ValueError("gamma and lam lie in [0, 1], w_scale is a finite float32 (got %r, %r, %r)" % (gamma, lam, w_scale))
        self._value_n_params()
        p = _lib.ClothGaeParams(g, l, ws, (_lib.GAE_WRITE_WEIGHTS if write_weights else 0) | (_lib.GAE_NORMALIZE if normalize else 0))
        adv = np.zeros(n, dtype=np.float32) if want else None
        ret = np.zeros(n, dtype=np.float32) if want else None
        check(self._L.clothhip_fit_data_gae(self._h, first, n, C.byref(p), _lib.fp(adv), _lib.fp(ret)))
        return (adv, ret) if want else None

    # ---- PPO: the old means and the clipped surrogate (clothhip.h: PPO ON THE DEVICE) ----------------------------------------------
    def fit_snapshot_policy(self, first=0, n=None):
        """Write the shared network's present output on the stored rows [first, first + n) (n=None: to the end) into the dataset's
        old-mean column, on the device (clothhip_fit_data_snapshot_policy): the bytes fit_predict returns for these rows, never
        downloaded. The rows then have an old mean, which fit_ppo / fit_ppo_grad need of every row they name."""
        first, n = self._fit_range(first, n)
        self._fit_n_params()
        check(self._L.clothhip_fit_data_snapshot_policy(self._h, first, n))

    def fit_set_old_means(self, mu, first=0):
        """Write the old means of the stored rows [first, first + len(mu)) from the host (clothhip_fit_data_set_old_means): mu [n, 4],
        finite float32."""
        m = np.asarray(mu, dtype=np.float64)
        if m.ndim != 2 or m.shape[1] != 4:
            raise ValueError("mu must have shape (n, 4)")
        if not (np.isfinite(m).all() and (np.abs(m) <= np.finfo(np.float32).max).all()):
            raise ValueError("mu must be finite (float32)")
        m = np.ascontiguousarray(m, dtype=np.float32)
        check(self._L.clothhip_fit_data_set_old_means(self._h, int(first), m.shape[0], _lib.fp(m)))

    def fit_get_old_means(self, first=0, n=None):
        """float32[n, 4]: the old means of the stored rows [first, first + n), n=None: to the end (clothhip_fit_data_get_old_means);
        zeros for a row that has none."""
        first, n = self._fit_range(first, n)
        mu = np.zeros((n, 4), dtype=np.float32)
        check(self._L.clothhip_fit_data_get_old_means(self._h, first, n, _lib.fp(mu)))
        return mu

    @staticmethod
    def _ppo_params(sigma, clip):
        s, c = float(sigma), float(clip)
        if not (np.isfinite(s) and s > 0.0 and s * s > 0.0 and np.isfinite(1.0 / (s * s))):
            raise ValueError("sigma = %r: the policy's standard deviation is finite and > 0" % (sigma,))
        if not (np.isfinite(c) and 0.0 <= c < 1.0):
            raise ValueError("clip = %r: the clip range lies in [0, 1)" % (clip,))
        return _lib.ClothPpoParams(s, c)

    def fit_ppo_grad(self, idx, sigma, clip=0.2):
        """(stats float64[3] = loss, clip_fraction, kl; grad float32[n_params] in the blob's layout; ratio float32[B]) of PPO's clipped
        surrogate over the dataset rows idx [B] at the present weights; nothing is updated (clothhip_policy_fit_ppo_grad). The policy
        is Gaussian with the fixed standard deviation sigma around the shared network's output; a row's action is its label, its
        advantage its weight, its old mean what fit_snapshot_policy / fit_set_old_means stored. policies.ppo_reference is the float64
        yardstick, policies.ppo_loss_reference the kernel's arithmetic."""
        ix = self._fit_idx(idx, 1)
        q = self._ppo_params(sigma, clip)
        grad = np.zeros(self._fit_n_params(), dtype=np.float32)
        stats = np.zeros(_lib.PPO_STATS, dtype=np.float64)
        ratio = np.zeros(ix.size, dtype=np.float32)
        check(self._L.clothhip_policy_fit_ppo_grad(self._h, C.byref(q), _lib.i32p(ix), ix.size, _lib.fp(grad), _lib.dp(stats), _lib.fp(ratio)))
        return stats, grad, ratio

    def fit_ppo(self, idx_table, sigma, clip=0.2, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        """fit with PPO's clipped surrogate as the loss (clothhip_policy_fit_ppo): n_steps optimizer steps on the shared network in
        place, step s on the dataset rows idx_table[s] (int [n_steps, B]), every row with an old mean. The optimizer is the policy's:
        fit and fit_ppo share the moments and the step count, fit_reset restarts both. Returns float64[n_steps, 3]: each step's
        (loss, clip_fraction, kl) BEFORE its update."""
        ix = self._fit_idx(idx_table, 2)
        p = self._fit_params(dict(optimizer=optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum), 1)
        q = self._ppo_params(sigma, clip)
        self._fit_n_params()
        stats = np.zeros((ix.shape[0], _lib.PPO_STATS), dtype=np.float64)
        check(self._L.clothhip_policy_fit_ppo(self._h, p, C.byref(q), _lib.i32p(ix), ix.shape[0], ix.shape[1], _lib.dp(stats)))
        return stats

    # ---- the cross-entropy planner over forked cloths (clothhip_plan_*) ------------------------------------------
    @staticmethod
    def plan_params(horizon, n_candidates, n_elite=1, n_iters=1, alpha=1.0, penalty=1.0, min_std=0.0, seed=0, iter0=0):
        """_lib.ClothPlanParams from keyword values; what the library would refuse (clothhip.h: BOUNDS) is a ValueError here first."""
        H, K, M, n = int(horizon), int(n_candidates), int(n_elite), int(n_iters)
        if not 1 <= H <= _lib.PLAN_MAX_H:
            raise ValueError("horizon = %d outside [1, %d]" % (H, _lib.PLAN_MAX_H))
        if not 2 <= K <= _lib.PLAN_MAX_K:
            raise ValueError("n_candidates = %d outside [2, %d]" % (K, _lib.PLAN_MAX_K))
        if not 1 <= M <= K:
            raise ValueError("n_elite = %d outside [1, n_candidates = %d]" % (M, K))
        if n < 1:
            raise ValueError("n_iters = %d < 1" % n)
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must lie in [0, 2^64)")
        if int(iter0) < 0 or int(iter0) + n > 2 ** 31:
            raise ValueError("iter0 >= 0 and iter0 + n_iters <= 2^31")
        if not 0.0 < float(alpha) <= 1.0:
            raise ValueError("alpha = %r outside (0, 1]" % (alpha,))
        if not np.isfinite(float(penalty)):
            raise ValueError("penalty is not finite")
        ms = np.broadcast_to(np.asarray(min_std, dtype=np.float64), (4,))
        if not (np.isfinite(ms).all() and (ms >= 0).all()):
            raise ValueError("min_std must be finite and >= 0")
        p = _lib.ClothPlanParams()
        p.horizon, p.n_candidates, p.n_elite, p.n_iters = H, K, M, n
        p.seed, p.iter0, p.alpha, p.penalty = int(seed), int(iter0), float(alpha), float(penalty)
        for a in range(4):
            p.min_std[a] = float(ms[a])
        return p

    @staticmethod
    def _plan_dist(mean, std, E, H):
        """(mean, std) as fresh float64 [E, H, 4] arrays the library may write into: mean finite, std finite and >= 0."""
        m = np.array(np.broadcast_to(np.asarray(mean, dtype=np.float64), (E, H, 4)), order='C')
        s = np.array(np.broadcast_to(np.asarray(std, dtype=np.float64), (E, H, 4)), order='C')
        return m, s

    def plan_cem(self, src_batch, ep, num_steps, done, mean, std, want_scores=False, want_candidates=False, **plan_kw):
        """The whole cross-entropy loop on the device (clothhip_plan_cem), with THIS batch as the scratch handle of src_batch.E * K cloths:
        n_iters x { sample K action sequences per env around (mean, std), fork src_batch's env e into slots e K .. e K + K - 1, run
        all of them for `horizon` actions in one episode launch, score each branch from its records, refit (mean, std) to the
        n_elite best }. ep: _lib.ClothEpisodeParams; num_steps int[E], done bool[E] of the source (a done env is not planned);
        mean, std: float64 [E, H, 4] (broadcast). plan_kw: plan_params' keywords. src_batch is only read. Returns a dict: mean, std
        (after the last refit), actions [E, H, 4] and score [E] of the best candidate seen (NaN for an env that was not planned),
        with want_scores scores [n_iters, E, K], with want_candidates candidates [n_iters, H, E K, 4] (the clipped tables)."""
        p = self.plan_params(**plan_kw)
        E, K, H, n = src_batch.E, p.n_candidates, p.horizon, p.n_iters
        m, s = self._plan_dist(mean, std, E, H)
        ns = np.ascontiguousarray(np.broadcast_to(np.asarray(num_steps), (E,)), dtype=np.int32)
        dn = np.ascontiguousarray(np.broadcast_to(np.asarray(done).astype(bool), (E,)), dtype=np.uint8)
        best_a = np.full((E, H, 4), np.nan)
        best_s = np.full(E, np.nan)
        sc = np.zeros((n, E, K)) if want_scores else None
        cd = np.zeros((n, H, E * K, 4)) if want_candidates else None
        check(self._L.clothhip_plan_cem(self._h, src_batch._h, C.byref(ep), C.byref(p), _lib.i32p(ns), _lib.u8p(dn), _lib.dp(m), _lib.dp(s),
                                        _lib.dp(best_a), _lib.dp(best_s), _lib.dp(sc), _lib.dp(cd)))
        self._launch = LastLaunch(H, 0, None)                # (the planner's last launch, ended on the device: H slots, no reset source)
        out = dict(mean=m, std=s, actions=best_a, score=best_s)
        if want_scores:
            out['scores'] = sc
        if want_candidates:
            out['candidates'] = cd
        return out

    def plan_sample(self, mean, std, act_low, act_high, it=0, n_envs=None, **plan_kw):
        """The sampling kernel alone on host tables (clothhip_plan_sample; the batch gives the device only): mean, std [E, H, 4] -> the
        clipped action table float64 [H, E K, 4] of iteration `it` (seed, iter0, horizon, n_candidates from plan_kw)."""
        p = self.plan_params(**plan_kw)
        E = int(np.shape(mean)[0] if n_envs is None else n_envs)
        m, s = self._plan_dist(mean, std, E, p.horizon)
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(act_low, dtype=np.float64), (4,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(act_high, dtype=np.float64), (4,)))
        x = np.zeros((p.horizon, E * p.n_candidates, 4))
        check(self._L.clothhip_plan_sample(self._h, C.byref(p), _lib.dp(lo), _lib.dp(hi), E, int(it), _lib.dp(m), _lib.dp(s), _lib.dp(x)))
        return x

    def plan_refit(self, x, scores, mean, std, done=None, **plan_kw):
        """The refit kernel alone on host tables (clothhip_plan_refit): the action table x [H, E K, 4] and scores [E, K] -> (mean, std
        [E, H, 4] after the refit, elite bool[E, K], top int[E]: the best candidate's k, -1 for an env with done set)."""
        sc = np.ascontiguousarray(scores, dtype=np.float64)
        if sc.ndim != 2:
            raise ValueError("scores must have shape (E, K)")
        E, K = sc.shape
        p = self.plan_params(n_candidates=K, **plan_kw)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (p.horizon, E * K, 4):
            raise ValueError("x must have shape (%d, %d, 4)" % (p.horizon, E * K))
        m, s = self._plan_dist(mean, std, E, p.horizon)
        dn = None if done is None else np.ascontiguousarray(np.broadcast_to(np.asarray(done).astype(bool), (E,)), dtype=np.uint8)
        elite = np.zeros((E, K), dtype=np.uint8)
        top = np.zeros(E, dtype=np.int32)
        check(self._L.clothhip_plan_refit(self._h, C.byref(p), E, _lib.dp(x), _lib.dp(sc), _lib.u8p(dn), _lib.dp(m), _lib.dp(s),
                                          _lib.u8p(elite), _lib.i32p(top)))
        return m, s, elite.astype(bool), top

    def update(self, n=1, delta=None):
        """n x Cloth.update() (cloth.pyx:169), each preceded by Gripper.adjust(*delta) if delta is given."""
        d = None if delta is None else np.ascontiguousarray(delta, dtype=np.float64)
        check(self._L.clothhip_update(self._h, int(n), _lib.dp(d)))

    def debug_stats(self):
        """[E,16]: [0..3] strain sweeps run, windows walked, passes, passes that corrected (last run);
        [4..15] per-phase shader cycles/64 when CLOTHHIP_DEBUG_PHASES has bit 32 set."""
        st = np.zeros((self.E, 16), dtype=np.int32)
        check(self._L.clothhip_debug_stats(self._h, _lib.i32p(st)))
        return st

    def last_variant(self):
        """Which compiled stepper variant the last launch of this handle ran (clothhip_last_variant): a dict with the template
        parameters, whether the LEAN arithmetic ran, LDS bytes per cloth, resident cloths per CU and the device's CU count, plus a
        one-line `name`."""
        v = np.zeros(10, dtype=np.int32)
        check(self._L.clothhip_last_variant(self._h, _lib.i32p(v)))
        d = dict(threads=int(v[0]), particles_per_thread=int(v[1]), table_mode=int(v[2]), rest_reg=int(v[3]), lean=bool(v[4]),
                 fused=int(v[5]), lds_bytes=int(v[6]), cloths_per_cu=int(v[7]), n_cus=int(v[8]), precision="f32" if v[9] else "f64")
        d["name"] = "k_run_schedule<%s,%d,%d,%d,%s,%d>%s: %d B LDS, %d cloths per CU" % (
            "float" if v[9] else "double", v[0], v[1], v[2], "true" if v[3] else "false", v[5], " (LEAN)" if v[4] else "", v[6], v[7])
        n = np.zeros(1, dtype=np.int32)
        check(self._L.clothhip_last_dispatches(self._h, _lib.i32p(n)))
        d["dispatches"] = int(n[0])            # kernel dispatches the launch went out as (one per generation of a time-sliced launch)
        check(self._L.clothhip_last_specialised(self._h, _lib.i32p(n)))
        d["spec_n_side"] = int(n[0])           # 25: the grid-specialised build of that variant ran (25x25 at compile time); 0: the generic build
        if n[0]:
            d["name"] = d["name"].replace(">", ",N%d>" % n[0], 1)
        return d

    def set_relaxed_order(self, on=True):
        """MEASUREMENT ONLY (bench.py's labelled companion): this handle's episode launches run the relaxed-order kernel -- Jacobi
        self-collision, coloured strain limit; NOT the reference's trajectories (clothhip_set_relaxed_order). Per handle."""
        check(self._L.clothhip_set_relaxed_order(self._h, 1 if on else 0))

    @property
    def last_kernel_ms(self):
        return float(self._L.clothhip_last_kernel_ms(self._h))

    # ---- device-resident paths (multi-GPU driver) --------------------------------------------------------
    def run_device_sched_async(self, d_sched_ptr):
        check(self._L.clothhip_run_device_sched_async(self._h, C.c_void_p(int(d_sched_ptr))))

    def write_obs_f32_device(self, d_out_ptr):
        check(self._L.clothhip_write_obs_f32_device(self._h, C.c_void_p(int(d_out_ptr))))

    @property
    def stream(self):
        return self._L.clothhip_stream(self._h)

    def device_alloc(self, nbytes):
        p = C.c_void_p()
        check(self._L.clothhip_device_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value

    def device_free(self, ptr):
        check(self._L.clothhip_device_free(self._h, C.c_void_p(ptr)))

    def device_upload(self, ptr, arr):
        a = np.ascontiguousarray(arr)
        check(self._L.clothhip_device_upload(self._h, C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def device_download(self, out, ptr):
        assert out.flags['C_CONTIGUOUS']
        check(self._L.clothhip_device_download(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes))
        return out
