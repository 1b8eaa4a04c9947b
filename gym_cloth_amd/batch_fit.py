"""ClothBatch's bindings of the trainer on the handle (clothhip.h, csrc/api_fit_data.hip, api_fit.hip, api_fit_rollout.hip and api_fit_ddpg.hip): the device-resident dataset
and its columns, the fit of the shared network and of population rows, the value network, GAE and PPO. A mixin of batch.ClothBatch: it
reads self._L, self._h, self.E and self.P, and the sizes batch_policy.py's setters leave (_mlp_n_params, _pop_shape)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .mlp import pack_mlp


class FitBindings(object):
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
        expert needed), or with labels="zero" (0, 0, 0, 0) and label_row ignored: a leaf of the actor-critic, appended for its state alone,
        or with labels="action+expert" the executed action as the label AND the armed launch's label into the row's expert column (DDPG
        from demonstrations: fit_expert, dpg_bc_fit).
        weights [n]: the rows' loss weights, None: 1. ValueError when a named value is not finite (a slot that did not
        run); nothing is appended then. Returns the dataset's size."""
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != 3 or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError("rows must be integers of shape (n, 3)")
        other = {"zero": _lib.FIT_LABEL_ZERO, "action+expert": _lib.FIT_LABEL_ACTION_EXPERT}
        if labels not in other and labels not in _lib.FIT_LABELS:
            raise ValueError("labels must be one of %r, 'zero' or 'action+expert' (got %r)" % (sorted(_lib.FIT_LABELS), labels))
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        w = self._fit_weights(weights, rows.shape[0])
        src = other[labels] if labels in other else _lib.FIT_LABELS[labels]
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

    # ---- PPO for a population: the snapshot by member and the grouped surrogate (clothhip.h: PPO FOR A POPULATION) --------------------
    def fit_snapshot_policy_members(self, member_of_row, first=0):
        """Write into the old-mean column of the stored rows [first, first + len(member_of_row)) the present output of the population
        row that ACTED there, on the device (clothhip_fit_data_snapshot_policy_members): member_of_row int[n] names a population row
        per stored row, -1 skips the row (its bytes and its mark stay). A named row gets the bytes fit_predict([row], [g]) returns and
        then has an old mean; nothing is downloaded."""
        m = np.asarray(member_of_row)
        if m.ndim != 1 or not (np.issubdtype(m.dtype, np.integer) or m.size == 0):
            raise ValueError("member_of_row must be a 1-d integer array")
        shape = getattr(self, '_pop_shape', None)
        if shape is None:
            raise _lib.ClothHipError("no population on this batch: call set_policy_population or population_perturb first")
        if m.size and (m.min() < -1 or m.max() >= shape[0]):
            raise ValueError("member_of_row must hold -1 or population rows in [0, %d)" % shape[0])
        if int(first) < 0:
            raise ValueError("first must be >= 0 and lie within the dataset")
        m = np.ascontiguousarray(m, dtype=np.int32)
        check(self._L.clothhip_fit_data_snapshot_policy_members(self._h, int(first), m.size, _lib.i32p(m)))

    @classmethod
    def _ppo_params_members(cls, sigma, clip, n_m):
        """_lib.ClothPpoParams[n_m] from sigma and clip, each a scalar for all members or n_m values."""
        q = (_lib.ClothPpoParams * n_m)()
        vals = {}
        for k, v in (('sigma', sigma), ('clip', clip)):
            v = np.asarray(v, dtype=np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.size != n_m):
                raise ValueError("%s must be a scalar or %d values, one per member" % (k, n_m))
            vals[k] = np.broadcast_to(v, (n_m,))
        for j in range(n_m):
            one = cls._ppo_params(vals['sigma'][j], vals['clip'][j])
            q[j].sigma, q[j].clip = one.sigma, one.clip
        return q

    def fit_ppo_grad_members(self, members, idx, sigma, clip=0.2):
        """(stats float64[n_m, 3] = loss, clip_fraction, kl; grad float32[n_m, n_params]; ratio float32[n_m, B]) of PPO's clipped
        surrogate of the population rows `members` over their own minibatches idx [n_m, B], member j under its own sigma[j] and clip[j]
        (scalars: the same for all); nothing is updated (clothhip_policy_fit_ppo_grad_members). Member j's result is bit for bit
        fit_ppo_grad's on a batch that carries row members[j] as its shared network over the same dataset, weights and old means."""
        m, n_params = self._fit_members(members)
        ix = self._fit_members_idx(idx, m.size, 2)
        q = self._ppo_params_members(sigma, clip, m.size)
        grad = np.zeros((m.size, n_params), dtype=np.float32)
        stats = np.zeros((m.size, _lib.PPO_STATS), dtype=np.float64)
        ratio = np.zeros((m.size, ix.shape[1]), dtype=np.float32)
        check(self._L.clothhip_policy_fit_ppo_grad_members(self._h, q, _lib.i32p(m), m.size, _lib.i32p(ix), ix.shape[1], _lib.fp(grad), _lib.dp(stats),
                                                           _lib.fp(ratio)))
        return stats, grad, ratio

    def fit_ppo_members(self, members, idx_table, sigma, clip=0.2, hyper=None):
        """fit_members with PPO's clipped surrogate as the loss (clothhip_policy_fit_ppo_members): n_steps optimizer steps on the
        population rows `members` in place, all members in the launches of one, step s of member j on the dataset rows
        idx_table[s, j] (int [n_steps, n_m, B]), every row with an old mean; sigma and clip are scalars or n_m values, hyper as
        fit_members takes it. The optimizer state is the rows' own: fit_members and fit_ppo_members share a row's moments and step
        count, fit_reset_members restarts both. Returns float64[n_steps, n_m, 3]: each member's (loss, clip_fraction, kl) BEFORE each
        step's update -- the bits fit_ppo gives on a batch that carries the row as its shared network."""
        m, _ = self._fit_members(members)
        ix = self._fit_members_idx(idx_table, m.size, 3)
        p = self._fit_params(hyper, m.size)
        q = self._ppo_params_members(sigma, clip, m.size)
        stats = np.zeros((ix.shape[0], m.size, _lib.PPO_STATS), dtype=np.float64)
        check(self._L.clothhip_policy_fit_ppo_members(self._h, p, q, _lib.i32p(m), m.size, _lib.i32p(ix), ix.shape[0], ix.shape[2], _lib.dp(stats)))
        return stats

    # ---- PPO with a learned sigma: the old log sigma and the surrogate over the handle's head (clothhip.h: PPO WITH A LEARNED SIGMA) ----
    def fit_set_old_log_sigma(self, log_sigma, first=0):
        """Write the old log sigma of the stored rows [first, first + len(log_sigma)) from the host
        (clothhip_fit_data_set_old_log_sigma): log_sigma [n, 4], finite float32. (fit_snapshot_policy writes the present head on the
        device when the batch has one.)"""
        m = np.asarray(log_sigma, dtype=np.float64)
        if m.ndim != 2 or m.shape[1] != 4:
            raise ValueError("log_sigma must have shape (n, 4)")
        if not (np.isfinite(m).all() and (np.abs(m) <= np.finfo(np.float32).max).all()):
            raise ValueError("log_sigma must be finite (float32)")
        m = np.ascontiguousarray(m, dtype=np.float32)
        check(self._L.clothhip_fit_data_set_old_log_sigma(self._h, int(first), m.shape[0], _lib.fp(m)))

    def fit_get_old_log_sigma(self, first=0, n=None):
        """float32[n, 4]: the old log sigma of the stored rows [first, first + n), n=None: to the end
        (clothhip_fit_data_get_old_log_sigma); zeros for a row that has none."""
        first, n = self._fit_range(first, n)
        ls = np.zeros((n, 4), dtype=np.float32)
        check(self._L.clothhip_fit_data_get_old_log_sigma(self._h, first, n, _lib.fp(ls)))
        return ls

    @staticmethod
    def _ppo_sigma_params(clip, ent_coef):
        c, e = float(clip), float(ent_coef)
        if not (np.isfinite(c) and 0.0 <= c < 1.0):
            raise ValueError("clip = %r: the clip range lies in [0, 1)" % (clip,))
        if not (np.isfinite(e) and e >= 0.0):
            raise ValueError("ent_coef = %r: the entropy coefficient is finite and >= 0" % (ent_coef,))
        return _lib.ClothPpoSigmaParams(c, e)

    def fit_ppo_sigma_grad(self, idx, clip=0.2, ent_coef=0.0):
        """(stats float64[4] = loss, clip_fraction, kl, entropy; grad float32[n_params] in the blob's layout; grad_ls float32[4], the
        head's gradient; ratio float32[B]) of PPO's clipped surrogate minus ent_coef times the entropy, over the dataset rows idx [B]
        at the present weights and the present head; nothing is updated (clothhip_policy_fit_ppo_sigma_grad). The policy is Gaussian
        around the shared network's output with the standard deviation exp(head); every row needs an old mean and an old log sigma
        (fit_snapshot_policy stores both). policies.ppo_sigma_reference is the float64 yardstick, policies.ppo_sigma_loss_reference the
        kernel's arithmetic."""
        ix = self._fit_idx(idx, 1)
        q = self._ppo_sigma_params(clip, ent_coef)
        grad = np.zeros(self._fit_n_params(), dtype=np.float32)
        grad_ls = np.zeros(4, dtype=np.float32)
        stats = np.zeros(_lib.PPO_SIGMA_STATS, dtype=np.float64)
        ratio = np.zeros(ix.size, dtype=np.float32)
        check(self._L.clothhip_policy_fit_ppo_sigma_grad(self._h, C.byref(q), _lib.i32p(ix), ix.size, _lib.fp(grad), _lib.fp(grad_ls), _lib.dp(stats),
                                                         _lib.fp(ratio)))
        return stats, grad, grad_ls, ratio

    def fit_ppo_sigma(self, idx_table, clip=0.2, ent_coef=0.0, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        """fit_ppo with the learned head in the place of a fixed sigma (clothhip_policy_fit_ppo_sigma): n_steps optimizer steps on the
        shared network AND on the head, step s on the dataset rows idx_table[s] (int [n_steps, B]). The network's optimizer is the
        policy's (shared with fit and fit_ppo); the head has its own moments and step count under the same hyper-parameters
        (fit_reset restarts both, set_policy_log_sigma the head's alone). Returns (float64[n_steps, 4]: each step's loss,
        clip_fraction, kl, entropy; float32[n_steps, 4]: the head) -- both BEFORE that step's update."""
        ix = self._fit_idx(idx_table, 2)
        p = self._fit_params(dict(optimizer=optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum), 1)
        q = self._ppo_sigma_params(clip, ent_coef)
        self._fit_n_params()
        stats = np.zeros((ix.shape[0], _lib.PPO_SIGMA_STATS), dtype=np.float64)
        heads = np.zeros((ix.shape[0], 4), dtype=np.float32)
        check(self._L.clothhip_policy_fit_ppo_sigma(self._h, p, C.byref(q), _lib.i32p(ix), ix.shape[0], ix.shape[1], _lib.dp(stats), _lib.fp(heads)))
        return stats, heads

    # ---- DDPG: a Q critic, target networks, the deterministic policy gradient (clothhip.h: DDPG ON THE DEVICE) ------------------------
    def set_q_mlp(self, layers):
        """The handle's Q network (clothhip_set_q_mlp): `layers` as set_value_mlp takes them, with an input width of 3P + 4 -- a row is the
        '1d' observation followed by the four action components -- and a last `out` of 1; None or [] drops it. It lives beside the
        policy, the value network and the head, independent of them; a new one drops the target Q and restarts its optimizer."""
        self._q_n_params = 0
        if not layers:
            check(self._L.clothhip_set_q_mlp(self._h, 0, None, None, 0))
            return
        widths, blob = pack_mlp(layers, n_out=1)
        check(self._L.clothhip_set_q_mlp(self._h, len(widths) - 1, _lib.i32p(widths), _lib.fp(blob), blob.size))
        self._q_n_params = int(blob.size)

    def _q_params(self):
        n = getattr(self, '_q_n_params', 0)
        if not n:
            raise _lib.ClothHipError("no Q network on this batch: call set_q_mlp first")
        return n

    def get_q_mlp(self):
        """The Q network's blob as the device holds it, float32[n_params] (clothhip_get_q_mlp)."""
        out = np.zeros(self._q_params(), dtype=np.float32)
        check(self._L.clothhip_get_q_mlp(self._h, _lib.fp(out), out.size))
        return out

    def q_fit_reset(self):
        """Zero the Q network's moments and its step count (clothhip_q_fit_reset)."""
        check(self._L.clothhip_q_fit_reset(self._h))

    def ddpg_sync_targets(self):
        """Copy the present shared policy network and Q network into the target copies, on the device (clothhip_ddpg_sync_targets)."""
        check(self._L.clothhip_ddpg_sync_targets(self._h))

    def ddpg_targets(self):
        """(policy float32[n_params], q float32[n_params]): the two target blobs by download (clothhip_ddpg_get_targets)."""
        pol, q = np.zeros(self._fit_n_params(), dtype=np.float32), np.zeros(self._q_params(), dtype=np.float32)
        check(self._L.clothhip_ddpg_get_targets(self._h, _lib.fp(pol), _lib.fp(q)))
        return pol, q

    def ddpg_set_targets(self, policy_layers=None, q_layers=None):
        """Upload target copies from the host, as a checkpoint restores them (clothhip_ddpg_set_targets): each a list of (W, b) of the
        shape of the network it shadows, None: that target stays as it is."""
        pol = q = None
        if policy_layers is not None:
            pol = pack_mlp(policy_layers, n_in=3 * self.P)[1]
            if pol.size != self._fit_n_params():
                raise ValueError("the target policy has %d parameters, the policy network %d" % (pol.size, self._fit_n_params()))
        if q_layers is not None:
            q = pack_mlp(q_layers, n_in=3 * self.P + 4, n_out=1)[1]
            if q.size != self._q_params():
                raise ValueError("the target Q network has %d parameters, the Q network %d" % (q.size, self._q_params()))
        check(self._L.clothhip_ddpg_set_targets(self._h, _lib.fp(pol), _lib.fp(q)))

    @staticmethod
    def _ddpg_params(gamma, tau, act_bound):
        g, t, b = float(gamma), float(tau), float(np.float32(act_bound))
        if not (np.isfinite(g) and np.isfinite(t) and 0.0 <= g <= 1.0 and 0.0 <= t <= 1.0):
            raise ValueError("gamma and tau lie in [0, 1] (got %r, %r)" % (gamma, tau))
        if not b > 0.0:
            raise ValueError("act_bound = %r: the action bound is > 0 (inf: no clamp)" % (act_bound,))
        return _lib.ClothDdpgParams(g, t, b, 0)

    def q_grad(self, idx, gamma, act_bound=1.0):
        """(stats float64[3] = loss, mean q, mean y; grad float32[n_params] of the Q network in the blob's layout; y float32[B], the TD
        targets; q float32[B], the critic on [s, clamp(label)]) over the dataset rows idx [B] at the present weights and targets;
        nothing is updated (clothhip_q_fit_grad). y = rew + gamma Q'(s', clamp(mu'(s'))) through a row's successor, 0 behind a
        terminal row; no row may be a leaf. references.q_fit_reference is the float64 yardstick, td_loss_reference the kernel's arithmetic."""
        ix = self._fit_idx(idx, 1)
        p = self._ddpg_params(gamma, 0.0, act_bound)
        grad = np.zeros(self._q_params(), dtype=np.float32)
        stats = np.zeros(_lib.Q_STATS, dtype=np.float64)
        y, q = np.zeros(ix.size, dtype=np.float32), np.zeros(ix.size, dtype=np.float32)
        check(self._L.clothhip_q_fit_grad(self._h, C.byref(p), _lib.i32p(ix), ix.size, _lib.fp(grad), _lib.dp(stats), _lib.fp(y), _lib.fp(q)))
        return stats, grad, y, q

    def q_fit(self, idx_table, gamma, act_bound=1.0, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        """n_steps optimizer steps of the Q network on the TD loss, in place (clothhip_q_fit): step s on the dataset rows idx_table[s]
        (int [n_steps, B]), with the Q network's own moments and step count. No target moves. Returns float64[n_steps, 3]: each step's
        (loss, mean q, mean y) BEFORE its update."""
        ix = self._fit_idx(idx_table, 2)
        p = self._fit_params(dict(optimizer=optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum), 1)
        q = self._ddpg_params(gamma, 0.0, act_bound)
        self._q_params()
        stats = np.zeros((ix.shape[0], _lib.Q_STATS), dtype=np.float64)
        check(self._L.clothhip_q_fit(self._h, p, C.byref(q), _lib.i32p(ix), ix.shape[0], ix.shape[1], _lib.dp(stats)))
        return stats

    def dpg_grad(self, idx, act_bound=1.0):
        """(stats float64[3] = loss -mean Q, gated fraction, mean |dL/da|; grad float32[n_params] of the POLICY in the blob's layout; da
        float32[B, 4] = dL/da, the critic's input gradient at the action columns) of the deterministic policy gradient over the dataset
        rows idx [B]; nothing is updated (clothhip_policy_fit_dpg_grad). references.dpg_reference is the float64 yardstick."""
        ix = self._fit_idx(idx, 1)
        p = self._ddpg_params(0.0, 0.0, act_bound)
        self._q_params()
        grad = np.zeros(self._fit_n_params(), dtype=np.float32)
        stats = np.zeros(_lib.DPG_STATS, dtype=np.float64)
        da = np.zeros((ix.size, 4), dtype=np.float32)
        check(self._L.clothhip_policy_fit_dpg_grad(self._h, C.byref(p), _lib.i32p(ix), ix.size, _lib.fp(grad), _lib.dp(stats), _lib.fp(da)))
        return stats, grad, da

    def dpg_fit(self, idx_table, act_bound=1.0, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        """n_steps optimizer steps of the shared policy network on -mean Q(s, clamp(mu(s))), the critic held fixed
        (clothhip_policy_fit_dpg): the policy's optimizer state, shared with fit and fit_ppo. Returns float64[n_steps, 3]."""
        ix = self._fit_idx(idx_table, 2)
        p = self._fit_params(dict(optimizer=optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum), 1)
        q = self._ddpg_params(0.0, 0.0, act_bound)
        self._q_params()
        self._fit_n_params()
        stats = np.zeros((ix.shape[0], _lib.DPG_STATS), dtype=np.float64)
        check(self._L.clothhip_policy_fit_dpg(self._h, p, C.byref(q), _lib.i32p(ix), ix.shape[0], ix.shape[1], _lib.dp(stats)))
        return stats

    def ddpg_polyak(self, tau):
        """The soft update of both targets: target = (1 - tau) target + tau network, in float32 on the device (clothhip_ddpg_polyak)."""
        self._ddpg_params(0.0, tau, 1.0)
        check(self._L.clothhip_ddpg_polyak(self._h, float(tau)))

    def ddpg_last_tables(self, B, want_qn=True):
        """(x float32[B, 3P + 4], qn float32[B] or None, q float32[B]): what the last DDPG call of minibatches of B rows left in the Q
        passes' scratch (clothhip_ddpg_last_tables) -- the critic's input rows of its last concat, the target critic's values (a
        critic's call only: want_qn), the critic's output of its last forward. For tests of the elementwise kernels."""
        x = np.zeros((int(B), 3 * self.P + 4), dtype=np.float32)
        qn, q = (np.zeros(int(B), dtype=np.float32) if want_qn else None), np.zeros(int(B), dtype=np.float32)
        check(self._L.clothhip_ddpg_last_tables(self._h, int(B), _lib.fp(x), _lib.fp(qn), _lib.fp(q)))
        return x, qn, q

    def ddpg_fit(self, idx_table, gamma, tau, act_bound=1.0, policy_hyper=None, q_hyper=None, bc=None):
        """n_steps DDPG steps in one call (clothhip_ddpg_fit): per step the critic's step on idx_table[s] (int [n_steps, B]), the actor's
        step against the updated critic, the soft update of both targets by tau. policy_hyper and q_hyper are dicts with fit's
        keywords (optimizer, lr, beta1, beta2, eps, momentum). By bytes what q_fit, dpg_fit and ddpg_polyak give one call at a time.
        Returns float64[n_steps, 6]: the critic's (loss, mean q, mean y), then the actor's (loss, gated fraction, mean |dL/da|).
        bc = dict(q_coef=, bc_coef=, q_filter=): the actor's step of DDPG from demonstrations (clothhip_ddpg_fit_bc; dpg_bc_fit has
        the loss); returns float64[n_steps, 9] then, the actor's six behind the critic's three."""
        ix = self._fit_idx(idx_table, 2)
        pp, pq = self._fit_params(policy_hyper, 1), self._fit_params(q_hyper, 1)
        q = self._ddpg_params(gamma, tau, act_bound)
        self._q_params()
        self._fit_n_params()
        if bc is not None:
            b = bc_params(**bc)
            stats = np.zeros((ix.shape[0], _lib.DDPG_BC_STATS), dtype=np.float64)
            check(self._L.clothhip_ddpg_fit_bc(self._h, pp, pq, C.byref(q), C.byref(b), _lib.i32p(ix), ix.shape[0], ix.shape[1], _lib.dp(stats)))
            return stats
        stats = np.zeros((ix.shape[0], _lib.DDPG_STATS), dtype=np.float64)
        check(self._L.clothhip_ddpg_fit(self._h, pp, pq, C.byref(q), _lib.i32p(ix), ix.shape[0], ix.shape[1], _lib.dp(stats)))
        return stats

    # ---- DDPG from demonstrations (clothhip.h: DDPG FROM DEMONSTRATIONS) --------------------------------------------------
    def fit_set_expert(self, actions, first=0):
        """Write the expert actions of the stored rows [first, first + len(actions)) from the host (clothhip_fit_data_set_expert):
        actions [n, 4]; a row of four finite float32 sets the row's expert action, a row of four NaNs clears it; a row that mixes the
        two, or an infinity, is a ValueError and nothing is written (expert_rows)."""
        a = expert_rows(actions)
        check(self._L.clothhip_fit_data_set_expert(self._h, int(first), a.shape[0], _lib.fp(a)))

    def fit_expert(self, first=0, n=None):
        """float32[n, 4]: the expert actions of the stored rows [first, first + n), n=None: to the end (clothhip_fit_data_get_expert);
        a row without one is four NaNs of the pattern _lib.FIT_NO_EXPERT_BITS (has_expert tells which rows have one)."""
        first, n = self._fit_range(first, n)
        a = np.zeros((n, 4), dtype=np.float32)
        check(self._L.clothhip_fit_data_get_expert(self._h, first, n, _lib.fp(a)))
        return a

    def dpg_bc_grad(self, idx, act_bound=1.0, q_coef=1.0, bc_coef=0.0, q_filter=True):
        """dict(stats float64[6] = -mean Q, gated fraction, mean |dL/da|, bc_loss, labelled share, filter-pass share; grad float32[n_params]
        of the POLICY; da float32[B, 4]; dz float32[B, 4], the dZ of the policy's last layer; q float32[B], the critic on the policy's
        action; qe float32[B] or None, the critic on the expert's action -- q_filter only) of the actor's loss of DDPG from
        demonstrations over the dataset rows idx [B]; nothing is updated (clothhip_policy_fit_dpg_bc_grad).
        references.dpg_bc_reference is the float64 yardstick, dpg_bc_dz_reference the kernel's arithmetic."""
        ix = self._fit_idx(idx, 1)
        p, b = self._ddpg_params(0.0, 0.0, act_bound), bc_params(q_coef, bc_coef, q_filter)
        self._q_params()
        grad = np.zeros(self._fit_n_params(), dtype=np.float32)
        stats = np.zeros(_lib.DPG_BC_STATS, dtype=np.float64)
        da, dz = np.zeros((ix.size, 4), dtype=np.float32), np.zeros((ix.size, 4), dtype=np.float32)
        q, qe = np.zeros(ix.size, dtype=np.float32), (np.zeros(ix.size, dtype=np.float32) if q_filter else None)
        check(self._L.clothhip_policy_fit_dpg_bc_grad(self._h, C.byref(p), C.byref(b), _lib.i32p(ix), ix.size, _lib.fp(grad), _lib.dp(stats), _lib.fp(da),
                                                      _lib.fp(dz), _lib.fp(q), _lib.fp(qe)))
        return dict(stats=stats, grad=grad, da=da, dz=dz, q=q, qe=qe)

    def dpg_bc_fit(self, idx_table, act_bound=1.0, q_coef=1.0, bc_coef=0.0, q_filter=True, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                   momentum=0.0):
        """n_steps optimizer steps of the shared policy network on q_coef (-mean Q(s, clamp(mu(s)))) + bc_coef / (4 B) sum over the rows
        that carry an expert action (and, q_filter, where Q(s, a_E) > Q(s, mu(s))) of |mu - clamp(a_E)|^2, the critic held fixed
        (clothhip_policy_fit_dpg_bc). Returns float64[n_steps, 6]."""
        ix = self._fit_idx(idx_table, 2)
        p = self._fit_params(dict(optimizer=optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum), 1)
        q, b = self._ddpg_params(0.0, 0.0, act_bound), bc_params(q_coef, bc_coef, q_filter)
        self._q_params()
        self._fit_n_params()
        stats = np.zeros((ix.shape[0], _lib.DPG_BC_STATS), dtype=np.float64)
        check(self._L.clothhip_policy_fit_dpg_bc(self._h, p, C.byref(q), C.byref(b), _lib.i32p(ix), ix.shape[0], ix.shape[1], _lib.dp(stats)))
        return stats


def bc_params(q_coef=1.0, bc_coef=0.0, q_filter=True):
    """ClothBcParams of the two coefficients (each finite and >= 0 as a float32, not both 0) and the Q-filter."""
    with np.errstate(over='ignore'):                      # (a double past float32's range becomes inf, refused below)
        qc, bc = float(np.float32(q_coef)), float(np.float32(bc_coef))
    if not (np.isfinite(qc) and np.isfinite(bc) and qc >= 0.0 and bc >= 0.0):
        raise ValueError("q_coef and bc_coef are finite and >= 0 (got %r, %r)" % (q_coef, bc_coef))
    if qc == 0.0 and bc == 0.0:
        raise ValueError("q_coef and bc_coef are both 0: the step has no loss")
    return _lib.ClothBcParams(qc, bc, _lib.BC_QFILTER if q_filter else 0, 0)


def expert_rows(actions):
    """float32[n, 4] as clothhip_fit_data_set_expert stores it: a row of four finite float32 values stays, a row of four NaNs becomes four
    times the fill pattern _lib.FIT_NO_EXPERT_BITS ("no expert action"); ValueError for another shape, a row that mixes NaN and finite
    values, or an infinity (as a float32)."""
    a = np.asarray(actions, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("actions must have shape (n, 4)")
    with np.errstate(over="ignore"):
        a = np.ascontiguousarray(a, dtype=np.float32)
    if np.isinf(a).any():
        raise ValueError("an expert action is infinite (float32)")
    nan = np.isnan(a)
    if (nan.any(axis=1) != nan.all(axis=1)).any():
        raise ValueError("a row mixes NaN and finite values: a row is four finite values, or four NaNs (no expert action)")
    bits = a.view(np.uint32).copy()
    bits[nan] = _lib.FIT_NO_EXPERT_BITS
    return bits.view(np.float32)


def has_expert(actions):
    """bool[n]: which rows of an expert column float32[n, 4] carry an expert action -- component 0 not a NaN, by its bits."""
    bits = np.ascontiguousarray(actions, dtype=np.float32).view(np.uint32).reshape(-1, 4)[:, 0]
    return (bits & np.uint32(0x7fffffff)) <= np.uint32(0x7f800000)
