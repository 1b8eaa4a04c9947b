"""ClothBatch's bindings of the cross-entropy planner (clothhip.h: PLAN ACTIONS ON THE DEVICE; csrc/api_plan.hip): the whole loop on a
scratch batch of forked cloths, and its sampling and refit kernels alone on host tables. A mixin of batch.ClothBatch: it reads self._L
and self._h and, as an episode launch does, leaves self._launch."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LastLaunch, check


class PlanBindings(object):
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
