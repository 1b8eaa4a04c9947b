"""ClothBatch's bindings of the policy networks on the handle (clothhip.h, csrc/api_policy.hip): the shared MLP, a population with one
network per env slot, their evaluation and the perturbations made on the device. A mixin of batch.ClothBatch: it reads self._L,
self._h, self.E and self.P and keeps no state but what the methods below say."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .mlp import pack_mlp, pack_population


class PolicyBindings(object):
    def set_policy_mlp(self, layers):
        """The handle's policy network (clothhip_set_policy_mlp): `layers` is a list of (W, b) with W [out, in] (torch.nn.Linear.weight's
        layout) and b [out], ReLU between them, the first `in` = 3 P, the last `out` = 4; None or [] clears it. The values are
        uploaded as float32; every env of the batch evaluates the same network. ValueError for shapes the library refuses."""
        self._mlp_n_params = 0                     # (fit_grad sizes its result by it: the shared network's parameters, 0 without one)
        self._pop_shape = None                     # (a shared network replaces a population)
        if not layers:
            check(self._L.clothhip_set_policy_mlp(self._h, 0, None, None, 0))
            return
        widths, blob = pack_mlp(layers)
        check(self._L.clothhip_set_policy_mlp(self._h, len(widths) - 1, _lib.i32p(widths), blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size))
        self._mlp_n_params = int(blob.size)

    def set_policy_log_sigma(self, log_sigma):
        """The head of a learned standard deviation (clothhip_set_policy_log_sigma): log_sigma [4] float32, one per action component,
        finite and within [-10, 10]; None drops it. It lies beside the shared network (setting a network leaves it alone), no launch
        reads it, fit_ppo_sigma trains it; setting it restarts the head's optimizer state and nothing else."""
        if log_sigma is None:
            check(self._L.clothhip_set_policy_log_sigma(self._h, None))
            return
        ls64 = np.asarray(log_sigma, dtype=np.float64)
        if ls64.shape != (4,):
            raise ValueError("log_sigma must have shape (4,) (got %r)" % (ls64.shape,))
        if not (np.isfinite(ls64).all() and (np.abs(ls64) <= 10.0).all()):
            raise ValueError("log_sigma must be finite and lie in [-10, 10] (got %r)" % (ls64.tolist(),))
        ls = np.ascontiguousarray(ls64, dtype=np.float32)
        check(self._L.clothhip_set_policy_log_sigma(self._h, _lib.fp(ls)))

    def get_policy_log_sigma(self):
        """float32[4]: the head as the device holds it now (clothhip_get_policy_log_sigma); ClothHipError without one."""
        out = np.zeros(4, dtype=np.float32)
        check(self._L.clothhip_get_policy_log_sigma(self._h, _lib.fp(out)))
        return out

    def policy_noise_fill(self, seed, n_actions, sigma=None, slot_base=None):
        """Fill the handle's exploration-noise table float64 [n_actions, E, 4] on the device (clothhip_policy_noise_fill) and return
        where it lies, an int: what run_actions_begin(policy=POLICY_MLP, actions_device_ptr=...) takes. [t, e, k] = sigma[e, k] *
        z_k(seed, e, slot_base[e] + t), z the standard normals of references.normal_fixed_reference -- policy_noise_reference restates
        the table bit for bit. sigma: a scalar, [4] or [E, 4], finite and >= 0; None: the log-sigma head of set_policy_log_sigma, read
        where it lies as exp_fixed of its float32 values (ClothHipError without one). slot_base int[E] >= 0, None: zeros. The fill runs
        on the batch's stream, so the launch that follows needs no synchronisation; the table belongs to the batch and stays valid
        until the next fill. Refused (ClothHipError) while a launch is in flight."""
        seed, T = int(seed), int(n_actions)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed must lie in [0, 2^64)")
        if T < 1 or T * self.E > 2 ** 31 - 1:
            raise ValueError("n_actions = %d: at least 1, and n_actions * E at most 2^31 - 1" % T)
        sg, rows = None, 0
        if sigma is not None:
            sg = np.asarray(sigma, dtype=np.float64)
            if sg.ndim == 0:
                sg = np.full(4, float(sg))
            if sg.shape not in ((4,), (self.E, 4)):
                raise ValueError("sigma must be a scalar, [4] or [%d, 4] (got shape %r)" % (self.E, sg.shape))
            if not np.isfinite(sg).all() or (sg < 0.0).any():
                raise ValueError("sigma must be finite and >= 0")
            rows = 1 if sg.ndim == 1 else self.E
            sg = np.ascontiguousarray(sg)
        base = None
        if slot_base is not None:
            b = np.asarray(slot_base)
            if b.shape != (self.E,) or not np.issubdtype(b.dtype, np.integer):
                raise ValueError("slot_base must be %d integers" % self.E)
            if b.size and (int(b.min()) < 0 or int(b.max()) > 2 ** 63 - 1 - T):
                raise ValueError("slot_base must be >= 0 (and slot_base + n_actions below 2^63)")
            base = np.ascontiguousarray(b, dtype=np.int64)
        ptr = C.c_void_p()
        check(self._L.clothhip_policy_noise_fill(self._h, seed, T, None if base is None else base.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 _lib.dp(sg), rows, C.byref(ptr)))
        self._noise_T = T
        return int(ptr.value)

    def policy_noise_get(self):
        """float64 [n_actions, E, 4]: the table of the last policy_noise_fill, downloaded (clothhip_policy_noise_get). ValueError before
        any fill."""
        T = getattr(self, '_noise_T', 0)
        if T < 1:
            raise ValueError("no noise table on this batch: call policy_noise_fill first")
        out = np.zeros((T, self.E, 4), dtype=np.float64)
        check(self._L.clothhip_policy_noise_get(self._h, T, _lib.dp(out)))
        return out

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
