"""Workload drivers: vectorised counterparts of the scripted policies of the reference's examples/analytic.py
that BASELINE configs name (oracle-corner, random), plus highest-point. They read the '1d' observation
(positions) only, so they work on a ClothVecEnv batch without touching per-particle Python objects.

OracleCornerPolicy   examples/analytic.py:70-155  (distance method, delta actions, inset corners 26/48/576/598)
HighestPointPolicy   examples/analytic.py:723-808
RandomPolicy         examples/analytic.py:811-823 (the reference samples from an UNSEEDED space RNG,
                     cloth_env.py:1004; here each env gets its own RandomState so runs are reproducible)
                     Both also run on the device as an EXPERT beside another acting policy (ClothVecEnv.step_many(expert=...): labels for
                     every state a learner reaches, DAgger's beta-mixture per slot) and stand-alone on stored observations
                     (ClothVecEnv.expert_actions); demos.dagger_rollout is the data-collection pass built on that
LookaheadPolicy      no reference counterpart: one-step greedy action selection over K candidates per env, evaluated on
                     device-side forks of the env's state (ClothVecEnv.lookahead)
MLPPolicy            no reference counterpart: a small fully-connected network over the '1d' observation, evaluated on the device -- by
                     the host loop through ClothBatch.policy_eval, or inside the episode launch (ClothVecEnv.step_many(policy='mlp'))
MLPPopulation        no reference counterpart: one MLP per env slot -- G perturbed copies of a centre network made on the device
                     (ClothBatch.population_perturb), rolled out in ONE episode launch, and the evolution-strategies update summed on
                     the device (ClothBatch.population_combine)
CEMPolicy            no reference counterpart: model-predictive control with the simulator as the model -- the cross-entropy method over action
                     sequences, every candidate rolled out on a device-side fork of the env (ClothVecEnv.plan, clothhip_plan_cem);
                     plan_sample_reference / plan_refit_reference / cem_reference restate the planner in numpy, bit for bit
DeviceNoise          no reference counterpart: the Gaussian exploration noise of an MLP policy made on the device, a pure function of
                     (seed, env, that env's slot number) -- step_many(policy='mlp', policy_noise=DeviceNoise(seed, sigma)) and the
                     collections of demos.py; normal_fixed_reference / policy_noise_reference restate it in numpy, bit for bit

The rest lives beside this module and is re-exported here under its old name: mlp.py packs a network for the library and holds the one
float64 pass of the numpy references; references.py holds those references (fit, value, GAE, exp_fixed, PPO, Adam, SGD, Philox, the
planner, the exploration noise); trainers.py holds MLPTrainer, ValueTrainer and MLPEnsemble, the drivers of the fit on the device.
"""
import numpy as np

from .mlp import MLP_MAX_LAYERS, MLP_MAX_WIDTH, mlp_float64, mlp_forward, pack_mlp, pack_population, population_stride, unpack_mlp  # noqa: F401
from .references import (NEXT_NONE, NEXT_TERMINAL, _house_sum, _plan_clip, adam_reference, cem_reference, exp_fixed_reference,  # noqa: F401
                         fit_reference, gae_reference, log_fixed_reference, normal_fixed_reference, philox4x32_10, philox_eps,
                         plan_refit_reference, plan_sample_reference, plan_score_reference, policy_noise_reference, ppo_loss_reference, ppo_reference, ppo_sigma_loss_reference, ppo_sigma_reference, sgd_reference,
                         value_fit_reference)
from .references import concat_reference, dpg_dz_reference, dpg_reference, polyak_reference, q_fit_reference, td_loss_reference  # noqa: F401
from .trainers import MLPEnsemble, MLPTrainer, QTrainer, ValueTrainer, ensemble_disagreement  # noqa: F401


def _data_delta(x, y, targx, targy, shrink=True):
    """examples/analytic.py:45-67: clip-space grasp point, delta towards the target (x0.9), distance."""
    cx = (x - 0.5) * 2.0
    cy = (y - 0.5) * 2.0
    dx = targx - x
    dy = targy - y
    dist = np.sqrt((x - targx) ** 2 + (y - targy) ** 2)
    if shrink:
        dx = dx * 0.90
        dy = dy * 0.90
    return cx, cy, dx, dy, dist, x, y


class OracleCornerPolicy(object):
    """Pull the (inset) cloth corner that is farthest from its target plane corner."""

    def __init__(self, env):
        self.env = env
        assert env.cfg['env']['delta_actions']
        assert env.num_points == 625, env.num_points                     # analytic.py:106

    def get_action(self, obs, t=0):
        E = self.env.E
        pos = np.asarray(obs, dtype=np.float64).reshape(E, -1, 3)
        tier2 = self.env.cfg['init']['type'] == 'tier2'
        acts = np.zeros((E, 4))
        for e in range(E):
            if tier2 and not self.env.init_side[e]:                      # analytic.py:108-114
                ll, ul, lr, ur = 576, 598, 26, 48
            else:
                ll, ul, lr, ur = 26, 48, 576, 598
            cands = [_data_delta(pos[e, ur, 0], pos[e, ur, 1], 1, 1), _data_delta(pos[e, lr, 0], pos[e, lr, 1], 1, 0),
                     _data_delta(pos[e, ll, 0], pos[e, ll, 1], 0, 0), _data_delta(pos[e, ul, 0], pos[e, ul, 1], 0, 1)]
            maxdist = max(c[4] for c in cands)
            for c in cands:                                              # first match wins (analytic.py:143-150)
                if c[4] == maxdist:
                    cx, cy, dx, dy, _, x, y = c
                    break
            if self.env.cfg['env']['clip_act_space']:                   # analytic.py:151-154
                acts[e] = (cx, cy, dx, dy)
            else:
                acts[e] = (x, y, dx, dy)
        return acts


class HighestPointPolicy(object):
    """Pick one of the top-k highest points at random and pull it to where it sits on the flat cloth
    (examples/analytic.py:723-808; the reference draws the pick from the global numpy stream, here every env has its own
    RandomState(seed + e) so that runs are reproducible and the device evaluation, ClothVecEnv.step_many(policy=
    'highest_point'), can be fed the same picks)."""

    def __init__(self, env, top_k=5, seed=0):
        self.env, self.top_k = env, top_k
        self.rngs = [np.random.RandomState(seed + e) for e in range(env.E)]
        self.orig = env.batch.init_grid(1)[0]                            # pt.orig_x/y of tiers 1 and 3 (cloth.pyx:122-124)
        n = int(round(np.sqrt(env.P)))
        r, c = np.divmod(np.arange(env.P), n)
        self.orig_y2 = c * (1.0 / (n - 1))                               # tier 2 (cloth.pyx:109-110): orig_y, orig_z
        self.orig_z2 = r * (1.0 / (n - 1))

    def draw(self, e):
        """The next pick of env e: which of the highest points (0 = the highest)."""
        return int(self.rngs[e].randint(self.top_k))

    def target(self, e, i):
        """analytic.py:742-789: (orig_x, orig_y) on the flat tiers; tier 2: (orig_z, orig_y) or (1 - orig_z, orig_y)."""
        if self.env._init_type == 'tier2':
            z = self.orig_z2[i]
            return (z if self.env.init_side[e] else 1.0 - z), self.orig_y2[i]
        return self.orig[i, 0], self.orig[i, 1]

    def get_action(self, obs, t=0):
        E = self.env.E
        pos = np.asarray(obs, dtype=np.float64).reshape(E, -1, 3)
        acts = np.zeros((E, 4))
        for e in range(E):
            order = np.argsort(-pos[e, :, 2], kind="stable")             # sorted(..., key=z, reverse=True)
            i = int(order[self.draw(e)])
            tx, ty = self.target(e, i)
            cx, cy, dx, dy, _, x, y = _data_delta(pos[e, i, 0], pos[e, i, 1], tx, ty)
            acts[e] = (cx, cy, dx, dy) if self.env.cfg['env']['clip_act_space'] else (x, y, dx, dy)
        return acts


class RandomPolicy(object):
    """Uniform actions over the action space ('over_xy_plane', cloth_env.py:1003-1004), one RNG per env."""

    def __init__(self, env, seed=2000):
        self.env = env
        self.rngs = [np.random.RandomState(seed + e) for e in range(env.E)]

    def get_action(self, obs=None, t=0):
        sp = self.env.action_space
        return np.stack([r.uniform(low=sp.low, high=sp.high) for r in self.rngs])


class LookaheadPolicy(object):
    """Greedy one-step lookahead: K candidate actions per env, each tried from the env's current state on a fork of it
    (ClothVecEnv.lookahead -- the env itself does not move), the candidate with the highest reward wins; ties go to the lowest
    candidate index. The candidates are uniform over the action space, drawn from ONE RandomState(seed) of the policy's own (the
    envs' np_randoms, i.e. the reset streams, do not advance; the same seed gives the same candidate stream); with `include`, another
    policy's proposal is candidate 0, so the lookahead never does worse in one-step reward than that policy. After get_action,
    last_candidates [E, K, 4], last_lookahead (the dict lookahead returned) and last_choice [E] describe the decision, and
    env.commit(last_choice) adopts the winning branches without simulating them again (step(action) does the same from scratch)."""

    def __init__(self, env, n_candidates=16, seed=0, include=None):
        if int(n_candidates) < 1:
            raise ValueError("n_candidates must be >= 1")
        self.env, self.K, self.include = env, int(n_candidates), include
        self.rng = np.random.RandomState(seed)
        self.last_candidates = self.last_lookahead = self.last_choice = None

    def candidates(self, obs=None, t=0):
        """The next [E, K, 4] candidate table (advances the policy's stream)."""
        sp = self.env.action_space
        cand = self.rng.uniform(low=sp.low, high=sp.high, size=(self.env.E, self.K, 4))
        if self.include is not None:
            cand[:, 0] = np.asarray(self.include.get_action(obs, t), dtype=np.float64)
        return cand

    @staticmethod
    def choose(rew):
        """arg-max over the candidates of every env, the lowest index among equals: rew [E, K] -> int64[E]."""
        return np.argmax(np.asarray(rew), axis=1).astype(np.int64)

    def get_action(self, obs=None, t=0):
        cand = self.candidates(obs, t)
        out = self.env.lookahead(cand)
        best = self.choose(out['rew'])
        self.last_candidates, self.last_lookahead, self.last_choice = cand, out, best
        return cand[np.arange(self.env.E), best]


class MLPPolicy(object):
    """A fully-connected network over the '1d' observation: `layers` = [(W, b), ...] numpy arrays, W [out, in] as torch.nn.Linear
    holds it -- from a torch.nn.Sequential of Linear and ReLU modules:
        [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in net if hasattr(m, 'weight')]
    ReLU follows every layer but the last; the env's decode clips the action to the action space. The weights are held as float32.

    get_action evaluates the network ON THE DEVICE (ClothBatch.policy_eval on the float32 observation), with the device function
    the episode launch runs, so that ClothVecEnv.step(policy.get_action(obs)) and step_many(policy='mlp') compute the same bits;
    reference(obs) is a float64 numpy evaluation of the same float32 weights, for tests. noise_std > 0 adds N(0, noise_std^2)
    exploration noise to every action component, drawn from one RandomState(seed + e) per env: draw(e) is the next [4] of env e, which
    collect_demos(on_device=True) hands to the launch slot by slot (step_many(policy_noise=...)). noise_std may be a length-4 vector,
    one standard deviation per action component (MLPTrainer.sigma() of a learned head): the unit draws are those of a scalar, scaled
    per component, and the policy is noisy when any component is > 0. The constructor uploads the network
    to env's batch (ClothVecEnv.set_policy); on several GPUs every rank does so itself."""

    def __init__(self, env, layers, noise_std=0.0, seed=0):
        self.env = env
        self.layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)) for W, b in layers]
        self.widths, self._blob = pack_mlp(self.layers, n_in=3 * env.P)
        std = np.asarray(noise_std, dtype=np.float64)
        if std.shape not in ((), (4,)) or not np.isfinite(std).all() or (std < 0.0).any():
            raise ValueError("noise_std must be a finite scalar or 4 values >= 0 (got %r)" % (noise_std,))
        self.noise_std = float(std) if std.ndim == 0 else float(std.max())      # (what collect_demos asks: is there noise at all)
        self._noise_scale = self.noise_std if std.ndim == 0 else std.copy()
        self.rngs = [np.random.RandomState(seed + e) for e in range(env.E)]
        env.set_policy(self)

    def pack(self):
        """(widths int32[L + 1], blob float32): the network as clothhip_set_policy_mlp takes it."""
        return self.widths.copy(), self._blob.copy()

    def reference(self, obs):
        """float64 evaluation of the float32 weights on obs [n, 3P] (rounded to float32 first, as the device reads it): [n, 4]."""
        x = np.asarray(obs, dtype=np.float32).astype(np.float64).reshape(-1, int(self.widths[0]))
        return mlp_forward(*mlp_float64(self.layers), x)[-1]

    def draw(self, e):
        """The next noise vector [4] of env e (zeros without noise; the stream then does not advance)."""
        if self.noise_std <= 0.0:
            return np.zeros(4)
        return self.rngs[e].normal(size=4) * self._noise_scale

    def get_action(self, obs, t=0):
        E = self.env.E
        if self.env._policy_mlp is not self:       # another network was set on the env since: put this one back, never answer with the other's
            self.env.set_policy(self)
        act = self.env.batch.policy_eval(np.asarray(obs).reshape(E, -1).astype(np.float32))
        if self.noise_std > 0.0:
            act = act + np.stack([self.draw(e) for e in range(E)])
        return act


class DeviceNoise(object):
    """Gaussian exploration noise made ON THE DEVICE (ClothBatch.policy_noise_fill, clothhip_policy_noise_fill) instead of an ndarray
    policy_noise: the noise of env e in ITS slot s is sigma[e] * z(seed, e, s), a pure function of (seed, env, slot number) --
    references.policy_noise_reference restates the table bit for bit. sigma is a scalar, [4] (one per action component), [E, 4] (one
    row per env: with an MLPEnsemble, DeviceNoise(seed, sigma=sigma_g[ens.member]) gives every member its own), or None: the handle's
    log-sigma head, read where it lies as exp_fixed of its float32 values -- the sigma PPO's surrogate differentiates; nothing is
    downloaded. slot_base int64[E] (zeros at first, made on first use) numbers the next slot of every env: step_many fills a launch's
    T rows from it and then advances it by the slots each env RAN, so successive launches continue one stream per env; the
    collections of demos.py (dagger_collect, reward_collect, actor_critic_collect) number the slots of one collection 0 .. n_actions - 1
    themselves and leave slot_base alone. A value object: it holds no device memory, the table belongs to the batch."""

    def __init__(self, seed, sigma=None):
        self.seed = int(seed)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must lie in [0, 2^64)")
        if sigma is not None:
            sigma = np.array(sigma, dtype=np.float64)
            if sigma.ndim > 2 or (sigma.ndim >= 1 and sigma.shape[-1] != 4):
                raise ValueError("sigma must be a scalar, [4] or [E, 4] (got shape %r)" % (sigma.shape,))
            if not np.isfinite(sigma).all() or (sigma < 0.0).any():
                raise ValueError("sigma must be finite and >= 0")
        self.sigma = sigma
        self.slot_base = None

    def base(self, E):
        """slot_base as int64[E], zeros before the first launch."""
        if self.slot_base is None:
            self.slot_base = np.zeros(int(E), dtype=np.int64)
        if self.slot_base.shape != (int(E),):
            raise ValueError("this DeviceNoise has numbered the slots of %d envs, the batch holds %d" % (self.slot_base.size, E))
        return self.slot_base

    def fill(self, batch, T, slot_base=None):
        """Fill batch's table for T slots from slot_base (None: the running one) and return the device pointer."""
        return batch.policy_noise_fill(self.seed, T, sigma=self.sigma, slot_base=self.base(batch.E) if slot_base is None else slot_base)

    def advance(self, ran):
        """ran bool[T, E] of a launch: every env's slot_base moves on by the slots it ran."""
        r = np.asarray(ran, dtype=bool)
        self.slot_base = self.base(r.shape[1]) + r.sum(axis=0).astype(np.int64)


def es_coefficients(fitness, sigma, antithetic=True, shaping="centered_rank"):
    """The coefficients w_k of the evolution-strategies estimate g = sum_k w_k eps_k from the G members' fitness (float64 arithmetic,
    returned as float32 -- what ClothBatch.population_combine takes).
      shaping 'centered_rank': u_g = rank_g / (G - 1) - 1/2, rank 0 for the lowest fitness (equal values rank in member order; G = 1: 0);
              'raw':           u_g = fitness_g, unchanged.
      plain:       g = 1 / (G sigma) sum_g u_g eps_g                          -> w_g = u_g / (G sigma), K = G
      antithetic:  rows 2k, 2k + 1 carry +eps_k, -eps_k, so the same estimate -> w_k = (u_2k - u_2k+1) / (G sigma), K = G / 2."""
    f = np.asarray(fitness, dtype=np.float64).reshape(-1)
    G = f.size
    if G < 1 or not np.isfinite(f).all():
        raise ValueError("fitness must hold one finite value per member")
    if antithetic and G % 2:
        raise ValueError("antithetic perturbations come in pairs: %d fitness values" % G)
    if not float(sigma) > 0.0:
        raise ValueError("sigma must be > 0")
    if shaping == "centered_rank":
        rank = np.empty(G, dtype=np.float64)
        rank[np.argsort(f, kind="stable")] = np.arange(G)
        u = rank / (G - 1) - 0.5 if G > 1 else np.zeros(1)
    elif shaping == "raw":
        u = f
    else:
        raise ValueError(shaping)
    w = (u[0::2] - u[1::2]) if antithetic else u
    return (w / (G * float(sigma))).astype(np.float32)


class MLPPopulation(object):
    """G = n_members perturbed copies of ONE centre network, one per env slot, for gradient-free learners (evolution strategies, CEM over
    parameters, checkpoints side by side): the copies are made on the device, all E cloths roll out under their own network in one
    step_many(policy='mlp') launch, and the update sum_k w_k eps_k is summed on the device as well -- no normal variate is drawn on
    the host and no blob crosses PCIe but the centre.

    The device holds G + 1 rows: with antithetic=True (G even) rows 2k and 2k + 1 are theta + sigma eps_k and theta - sigma eps_k, else
    row g is theta + sigma eps_g; row G is theta, the unperturbed centre. `member` int[E] says which row env e runs (default
    e % (G + 1)). eps is defined in csrc/cloth_policy_population.hpp (Philox4x32-10; zero mean, unit variance, symmetric, |eps| <= 3.47:
    a sum of four uniforms, NOT a Gaussian). THE SEED OF GENERATION n IS seed + n (mod 2^64): perturb(n) makes that generation's rows,
    the same bits every time. sigma is held as float32.

    The networks belong to the env slots of env's batch: resets and uploads leave them alone; snapshots, forks and the lookahead's
    scratch batch do not carry them. The constructor makes generation 0 (ClothVecEnv.set_policy(self))."""

    noise_std = 0.0        # (collect_demos: no exploration noise on top of the parameter noise)

    def __init__(self, env, center_layers, n_members, sigma, seed, antithetic=True, member=None):
        self.env = env
        self.center = [(np.array(W, dtype=np.float32), np.array(b, dtype=np.float32)) for W, b in center_layers]
        self.widths, self._blob = pack_mlp(self.center, n_in=3 * env.P)
        self.G = int(n_members)
        self.antithetic = bool(antithetic)
        if self.G < 1:
            raise ValueError("n_members = %d: a population has at least one member" % self.G)
        if self.antithetic and self.G % 2:
            raise ValueError("n_members = %d: antithetic perturbations come in pairs, n_members must be even" % self.G)
        self.sigma = float(np.float32(sigma))
        if not (np.isfinite(self.sigma) and self.sigma > 0.0):
            raise ValueError("sigma must be a finite float32 > 0")
        self.seed = int(seed)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must lie in [0, 2^64)")
        m = np.arange(env.E) % (self.G + 1) if member is None else np.asarray(member)
        if m.shape != (env.E,):
            raise ValueError("member must have shape (%d,) (got %r)" % (env.E, m.shape))
        if not np.issubdtype(m.dtype, np.integer) or m.min() < 0 or m.max() > self.G:
            raise ValueError("member must hold integers in [0, %d]" % self.G)
        self.member = m.astype(np.int32)
        self.generation = 0
        env.set_policy(self)

    @property
    def n_params(self):
        return int(self._blob.size)

    def generation_seed(self, generation):
        return (self.seed + int(generation)) % 2 ** 64

    def _upload(self, batch):
        batch.population_perturb(self.center, self.G, self.sigma, self.generation_seed(self.generation), antithetic=self.antithetic,
                                 member=self.member)

    def perturb(self, generation):
        """Make generation `generation`'s G + 1 rows around the present centre (seed + generation) and put them on the env."""
        self.generation = int(generation)
        self.env.set_policy(self)

    def set_members(self, member):
        """Another map env -> row, without touching the rows (ClothBatch.set_policy_members)."""
        m = np.asarray(member)
        if m.shape != (self.env.E,) or not np.issubdtype(m.dtype, np.integer) or m.min() < 0 or m.max() > self.G:
            raise ValueError("member must be %d integers in [0, %d]" % (self.env.E, self.G))
        self._on_env()
        self.env.batch.set_policy_members(m)
        self.member = m.astype(np.int32)

    def _on_env(self):
        if self.env._policy_mlp is not self:       # another network was set on the env since: put this generation back (the same bits)
            self.env.set_policy(self)

    def members(self):
        """The G + 1 rows as the device holds them: a list of layer lists, by download."""
        self._on_env()
        return [unpack_mlp(self.widths, self.env.batch.get_policy_mlp(g, self.n_params)) for g in range(self.G + 1)]

    def get_action(self, obs, t=0):
        """float64[E, 4]: env e's row on obs[e], on the device (ClothBatch.policy_eval_members) -- the bits the launch computes."""
        self._on_env()
        return self.env.batch.policy_eval_members(np.asarray(obs).reshape(self.env.E, -1).astype(np.float32), self.member)

    def fitness(self, out):
        """float64[G + 1] from a step_many result: per row the mean, over the envs that ran it, of the rewards the env collected in
        the launch (slots it did not run count nothing); NaN for a row no env ran."""
        ret = np.where(out["ran"], out["rew"], 0.0).sum(axis=0)
        return np.array([ret[self.member == g].mean() if (self.member == g).any() else np.nan for g in range(self.G + 1)])

    def coefficients(self, fitness, shaping="centered_rank"):
        """es_coefficients of the G members' fitness (a [G + 1] vector's last entry, the centre's, is left out)."""
        f = np.asarray(fitness, dtype=np.float64).reshape(-1)
        if f.size == self.G + 1:
            f = f[:self.G]
        if f.size != self.G:
            raise ValueError("fitness must hold %d (or %d) values" % (self.G, self.G + 1))
        return es_coefficients(f, self.sigma, self.antithetic, shaping)

    def gradient(self, fitness, shaping="centered_rank"):
        """The evolution-strategies estimate of d E[fitness] / d theta as a float32 blob [n_params]: the coefficients on the host
        (es_coefficients), their sum over this generation's eps on the device (ClothBatch.population_combine)."""
        w = self.coefficients(fitness, shaping)
        self._on_env()
        return self.env.batch.population_combine(w)

    def apply(self, delta):
        """centre += delta (float32 [n_params], one float32 addition per parameter, on the host), then the next generation's rows."""
        d = np.asarray(delta, dtype=np.float32).reshape(-1)
        if d.size != self.n_params or not np.isfinite(d).all():
            raise ValueError("delta must hold %d finite values" % self.n_params)
        self._blob = (self._blob + d).astype(np.float32)
        self.center = unpack_mlp(self.widths, self._blob)
        self.perturb(self.generation + 1)


class CEMPolicy(object):
    """Model-predictive control by the cross-entropy method, the simulator itself as the model: every get_action plans `horizon`
    actions ahead on device-side forks of the env's present state (ClothVecEnv.plan: n_iters iterations of n_candidates action
    sequences per env, refit to the n_elite best) and returns the first action of the best sequence seen. The env does not move.
    warm_start: another policy (get_action(obs, t)) whose proposal becomes mean[:, 0]; candidate 0 of iteration 0 is the clipped
    mean itself, so the plan's score is never below what that proposal (followed by the rest of the mean) scores. Between calls the
    mean is the last plan's mean shifted by one action with the last row repeated, std goes back to init_std, and iter0 advances by
    n_iters (fresh noise each call, the same stream for the same seed). last_plan keeps the dict plan() returned. An env whose
    episode is over is not planned; it gets the clipped mean's first action."""

    def __init__(self, env, horizon=1, n_candidates=16, n_elite=4, n_iters=2, init_std=0.5, min_std=0.01, alpha=1.0, penalty=1.0, seed=0,
                 warm_start=None):
        from .batch import ClothBatch
        ClothBatch.plan_params(horizon, n_candidates, n_elite, n_iters, alpha=alpha, penalty=penalty, min_std=min_std, seed=seed)
        self.env, self.warm_start = env, warm_start
        self.horizon, self.n_candidates, self.n_elite, self.n_iters = int(horizon), int(n_candidates), int(n_elite), int(n_iters)
        self.init_std, self.min_std, self.alpha, self.penalty, self.seed = init_std, min_std, float(alpha), float(penalty), int(seed)
        self.iter0 = 0
        self.mean = np.zeros((env.E, self.horizon, 4))
        self.last_plan = None

    def get_action(self, obs=None, t=0):
        E, H = self.env.E, self.horizon
        mean = self.mean.copy()
        if self.warm_start is not None:
            mean[:, 0] = np.asarray(self.warm_start.get_action(obs, t), dtype=np.float64)
        std = np.array(np.broadcast_to(np.asarray(self.init_std, dtype=np.float64), (E, H, 4)))
        plan = self.env.plan(H, self.n_candidates, self.n_elite, self.n_iters, mean=mean, std=std, min_std=self.min_std, alpha=self.alpha,
                             penalty=self.penalty, seed=self.seed, iter0=self.iter0)
        self.iter0 += self.n_iters
        self.last_plan = plan
        m = plan['mean']
        self.mean = np.concatenate([m[:, 1:], m[:, -1:]], axis=1)
        sp = self.env.action_space
        fallback = _plan_clip(mean[:, 0], sp.low, sp.high)
        return np.where(plan['planned'][:, None], plan['actions'][:, 0], fallback)
