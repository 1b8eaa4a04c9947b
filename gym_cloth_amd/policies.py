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
MLPTrainer           no reference counterpart: the supervised refit of the shared network on the device (ClothBatch.fit_*), Adam or SGD over a
                     device-resident dataset of (observation, label) rows; fit_reference is its float64 numpy yardstick
MLPEnsemble          no reference counterpart: G networks, one per env slot, fitted together on the device in the launches of one
                     (ClothBatch.fit_members): a bootstrapped ensemble whose disagreement is a novelty signal, a learning-rate sweep
"""
import math

import numpy as np


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


MLP_MAX_LAYERS, MLP_MAX_WIDTH = 4, 256


def pack_mlp(layers, n_in=None, n_out=4):
    """[(W, b), ...] -> (widths int32[L + 1], blob float32): for every layer W [out, in] row-major (torch.nn.Linear.weight's layout),
    then b [out] -- what clothhip_set_policy_mlp takes. ValueError for anything the library would refuse: no or more than four layers,
    a W that is not 2-d or a b that is not [out], widths that do not chain, an input width other than n_in (when given), a last width
    other than 4 (n_out: 1 for a value network, clothhip_set_value_mlp), a hidden width outside [1, 256], non-finite values."""
    layers = list(layers)
    if not 1 <= len(layers) <= MLP_MAX_LAYERS:
        raise ValueError("an MLP policy has 1 to %d weight layers (got %d)" % (MLP_MAX_LAYERS, len(layers)))
    widths, parts = [], []
    for l, wb in enumerate(layers):
        if len(wb) != 2:
            raise ValueError("layer %d must be a (W, b) pair" % l)
        W, b = np.asarray(wb[0], dtype=np.float32), np.asarray(wb[1], dtype=np.float32)
        if W.ndim != 2 or W.shape[0] < 1 or W.shape[1] < 1:
            raise ValueError("layer %d: W must be a non-empty [out, in] matrix (got shape %r)" % (l, W.shape))
        if b.shape != (W.shape[0],):
            raise ValueError("layer %d: b must have shape (%d,) (got %r)" % (l, W.shape[0], b.shape))
        if l and W.shape[1] != widths[-1]:
            raise ValueError("layer %d takes %d inputs, layer %d gives %d" % (l, W.shape[1], l - 1, widths[-1]))
        if not (np.isfinite(W).all() and np.isfinite(b).all()):
            raise ValueError("layer %d holds non-finite values" % l)
        if not l:
            widths.append(int(W.shape[1]))
        widths.append(int(W.shape[0]))
        parts += [np.ascontiguousarray(W).reshape(-1), b]
    if n_in is not None and widths[0] != int(n_in):
        raise ValueError("the network's input width is %d, the '1d' observation has %d values" % (widths[0], int(n_in)))
    if widths[-1] != int(n_out):
        raise ValueError("the network's output width is %d, %s" % (widths[-1], "an action has 4 values" if int(n_out) == 4 else "this network has %d" % int(n_out)))
    for l in range(1, len(widths) - 1):
        if not 1 <= widths[l] <= MLP_MAX_WIDTH:
            raise ValueError("hidden width %d (layer %d) outside [1, %d]" % (widths[l], l, MLP_MAX_WIDTH))
    return np.asarray(widths, dtype=np.int32), np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


class MLPPolicy(object):
    """A fully-connected network over the '1d' observation: `layers` = [(W, b), ...] numpy arrays, W [out, in] as torch.nn.Linear
    holds it -- from a torch.nn.Sequential of Linear and ReLU modules:
        [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in net if hasattr(m, 'weight')]
    ReLU follows every layer but the last; the env's decode clips the action to the action space. The weights are held as float32.

    get_action evaluates the network ON THE DEVICE (ClothBatch.policy_eval on the float32 observation), with the device function
    the episode launch runs, so that ClothVecEnv.step(policy.get_action(obs)) and step_many(policy='mlp') compute the same bits;
    reference(obs) is a float64 numpy evaluation of the same float32 weights, for tests. noise_std > 0 adds N(0, noise_std^2)
    exploration noise to every action component, drawn from one RandomState(seed + e) per env: draw(e) is the next [4] of env e, which
    collect_demos(on_device=True) hands to the launch slot by slot (step_many(policy_noise=...)). The constructor uploads the network
    to env's batch (ClothVecEnv.set_policy); on several GPUs every rank does so itself."""

    def __init__(self, env, layers, noise_std=0.0, seed=0):
        self.env = env
        self.layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)) for W, b in layers]
        self.widths, self._blob = pack_mlp(self.layers, n_in=3 * env.P)
        self.noise_std = float(noise_std)
        self.rngs = [np.random.RandomState(seed + e) for e in range(env.E)]
        env.set_policy(self)

    def pack(self):
        """(widths int32[L + 1], blob float32): the network as clothhip_set_policy_mlp takes it."""
        return self.widths.copy(), self._blob.copy()

    def reference(self, obs):
        """float64 evaluation of the float32 weights on obs [n, 3P] (rounded to float32 first, as the device reads it): [n, 4]."""
        x = np.asarray(obs, dtype=np.float32).astype(np.float64).reshape(-1, int(self.widths[0]))
        for l, (W, b) in enumerate(self.layers):
            x = x @ W.astype(np.float64).T + b.astype(np.float64)
            if l + 1 < len(self.layers):
                x = np.maximum(x, 0.0)
        return x

    def draw(self, e):
        """The next noise vector [4] of env e (zeros without noise; the stream then does not advance)."""
        if self.noise_std <= 0.0:
            return np.zeros(4)
        return self.rngs[e].normal(size=4) * self.noise_std

    def get_action(self, obs, t=0):
        E = self.env.E
        if self.env._policy_mlp is not self:       # another network was set on the env since: put this one back, never answer with the other's
            self.env.set_policy(self)
        act = self.env.batch.policy_eval(np.asarray(obs).reshape(E, -1).astype(np.float32))
        if self.noise_std > 0.0:
            act = act + np.stack([self.draw(e) for e in range(E)])
        return act


def unpack_mlp(widths, blob):
    """The inverse of pack_mlp: [(W, b), ...] float32 copies out of one blob."""
    layers, o = [], 0
    for l in range(len(widths) - 1):
        n_in, n_out = int(widths[l]), int(widths[l + 1])
        W = np.array(blob[o:o + n_out * n_in], dtype=np.float32).reshape(n_out, n_in); o += n_out * n_in
        b = np.array(blob[o:o + n_out], dtype=np.float32); o += n_out
        layers.append((W, b))
    if o != len(blob):
        raise ValueError("the blob holds %d values, these widths %d" % (len(blob), o))
    return layers


def pack_population(members, n_in=None):
    """[network, ...] (each a list of (W, b) layers, all of ONE shape) -> (widths int32[L + 1], float32 [G, n_params]): what
    clothhip_set_policy_population takes. ValueError for what pack_mlp refuses, and for networks of different shapes."""
    members = list(members)
    if not members:
        raise ValueError("a population has at least one network")
    widths, rows = None, []
    for g, layers in enumerate(members):
        w, blob = pack_mlp(layers, n_in=n_in)
        if widths is not None and not np.array_equal(w, widths):
            raise ValueError("network %d has widths %r, network 0 has %r: a population has one shape" % (g, w.tolist(), widths.tolist()))
        widths = w
        rows.append(blob)
    return widths, np.ascontiguousarray(np.stack(rows), dtype=np.float32)


def population_stride(n_params):
    """Floats between two rows of a population on the device: n_params rounded up to 64, so that every row is 256-byte aligned."""
    return (int(n_params) + 63) // 64 * 64


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


def fit_reference(layers, obs, labels, idx, weights=None):
    """Pure-numpy float64 loss and gradient of the trainer's objective, for tests and for users who want to check a fit:
    L = 1 / (4 B) sum_r w_r sum_k (y_rk - a_rk)^2 over the rows idx [B] of (obs [n, in], labels [n, 4], weights [n] or None: all 1 --
    then torch.nn.MSELoss()) with ReLU after every layer but the last and ReLU' = 1 where the pre-activation is > 0, else 0. The
    normaliser is B, whatever the weights sum to. obs, labels, the per-row weights and the network's weights are rounded to float32
    first (what the device stores), the arithmetic is float64. Returns (loss, [(dW, db), ...]) in `layers`' shapes."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    Ws = [np.asarray(W, dtype=np.float32).astype(np.float64) for W, _ in layers]
    bs = [np.asarray(b, dtype=np.float32).astype(np.float64) for _, b in layers]
    x = np.asarray(obs, dtype=np.float32).astype(np.float64)[ix]
    a = np.asarray(labels, dtype=np.float64).astype(np.float32).astype(np.float64)[ix]
    B, L = len(ix), len(Ws)
    hs = [x]
    for l in range(L):
        z = hs[-1] @ Ws[l].T + bs[l]
        hs.append(np.maximum(z, 0.0) if l + 1 < L else z)
    d = hs[-1] - a
    if weights is None:
        loss = float((d * d).sum() / (4.0 * B))
        g = d / (2.0 * B)
    else:
        w = np.asarray(weights, dtype=np.float64).astype(np.float32).astype(np.float64).reshape(-1)[ix][:, None]
        loss = float((w * (d * d)).sum() / (4.0 * B))
        g = w * d / (2.0 * B)
    grads = [None] * L
    for l in range(L - 1, -1, -1):
        grads[l] = (g.T @ hs[l], g.sum(axis=0))
        if l:
            g = (g @ Ws[l]) * (hs[l] > 0.0)
    return loss, grads


def value_fit_reference(layers, obs, ret, idx):
    """Pure-numpy float64 loss and gradient of the critic's objective (clothhip_value_fit_grad): L_V = 1 / (2 B) sum_r (v_r - ret_r)^2
    over the rows idx [B] of (obs [n, in], ret [n]), UNWEIGHTED, the network as fit_reference takes it with a last width of 1. obs, ret
    and the network's weights are rounded to float32 first (what the device stores), the arithmetic is float64. Returns
    (loss, [(dW, db), ...]) in `layers`' shapes."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    Ws = [np.asarray(W, dtype=np.float32).astype(np.float64) for W, _ in layers]
    bs = [np.asarray(b, dtype=np.float32).astype(np.float64) for _, b in layers]
    if Ws[-1].shape[0] != 1:
        raise ValueError("a value network ends in ONE output (got %d)" % Ws[-1].shape[0])
    x = np.asarray(obs, dtype=np.float32).astype(np.float64)[ix]
    a = np.asarray(ret, dtype=np.float64).astype(np.float32).astype(np.float64).reshape(-1)[ix][:, None]
    B, L = len(ix), len(Ws)
    hs = [x]
    for l in range(L):
        z = hs[-1] @ Ws[l].T + bs[l]
        hs.append(np.maximum(z, 0.0) if l + 1 < L else z)
    d = hs[-1] - a
    loss = float((d * d).sum() / (2.0 * B))
    g = d / float(B)
    grads = [None] * L
    for l in range(L - 1, -1, -1):
        grads[l] = (g.T @ hs[l], g.sum(axis=0))
        if l:
            g = (g @ Ws[l]) * (hs[l] > 0.0)
    return loss, grads


NEXT_TERMINAL, NEXT_NONE = -1, -2          # _lib.FIT_NEXT_*: a row's successor column besides a row number


def _house_sum(x):
    """The device's reduction order over x [n] float64: thread t of 256 adds elements t, t + 256, ... in ascending order from +0.0, then a
    halving tree adds the 256 sums. (Elements that do not take part are passed as +0.0: s + 0.0 keeps the bits of a sum that began at +0.0.)"""
    x = np.asarray(x, dtype=np.float64)
    k = (len(x) + 255) // 256
    tab = np.zeros((max(k, 1), 256))
    tab.reshape(-1)[:len(x)] = x
    red = np.zeros(256)
    for row in tab:
        red = red + row
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return red[0]


def gae_reference(v, rew, next, gamma, lam, w_scale=1.0, normalize=False):
    """clothhip_fit_data_gae restated in float64 numpy, operation by operation (include/clothhip.h: ADVANTAGES AND VALUE TARGETS ON THE
    DEVICE): v [n] float32 the critic on the rows of a range, rew [n] float32, next [n] int with successors as indices INTO THE RANGE
    (the dataset's column minus `first` where it is >= 0), NEXT_TERMINAL or NEXT_NONE (a leaf). For a non-leaf row the chain r, next[r],
    ... stops after a row whose next is TERMINAL or whose successor is a leaf; delta = (rew + gamma nv) - v, A = sum (gamma lam)^k
    delta_k accumulated for k ascending with coef = coef c. Returns (adv float32[n], ret float32[n], w float32[n]): adv = (float)A,
    ret = (float)(A + v), w = (float)((float32)w_scale A^) with A^ = A, or normalised (A - mean) / (std + 1e-8) over the non-leaf rows in
    the device's reduction order; a leaf has adv 0, ret v, w 0. Bit for bit what the device writes."""
    v64 = np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1)
    r64 = np.asarray(rew, dtype=np.float32).astype(np.float64).reshape(-1)
    nx = np.asarray(next).astype(np.int64).reshape(-1)
    n = len(v64)
    if not (len(r64) == len(nx) == n):
        raise ValueError("v, rew and next must have one length")
    if ((nx >= 0) & ((nx <= np.arange(n)) | (nx >= n))).any() or (nx < NEXT_NONE).any():
        raise ValueError("a successor lies behind its row and inside the range (or is NEXT_TERMINAL / NEXT_NONE)")
    gamma, c = float(gamma), float(gamma) * float(lam)
    leaf = nx == NEXT_NONE
    A = np.zeros(n)
    for r in np.nonzero(~leaf)[0]:
        acc, coef, cur = 0.0, 1.0, int(r)
        while True:
            k = int(nx[cur])
            nv = 0.0 if k < 0 else v64[k]
            delta = (r64[cur] + gamma * nv) - v64[cur]
            acc = acc + coef * delta
            coef = coef * c
            if k < 0 or leaf[k]:
                break
            cur = k
        A[r] = acc
    with np.errstate(over='ignore'):
        adv = A.astype(np.float32)
        ret = np.where(leaf, v64, A + v64).astype(np.float32)
    hat = A
    cnt = int((~leaf).sum())
    if normalize and cnt:
        mean = _house_sum(np.where(leaf, 0.0, A)) / float(cnt)
        d = A - mean
        std = np.sqrt(_house_sum(np.where(leaf, 0.0, d * d)) / float(cnt))
        hat = d / (std + 1e-8)
    with np.errstate(over='ignore', invalid='ignore'):
        w = np.where(leaf, 0.0, float(np.float32(w_scale)) * hat).astype(np.float32)
    return adv, ret, w


_LOG2E, _LN2_HI, _LN2_LO = float.fromhex('0x1.71547652b82fep+0'), float.fromhex('0x1.62e42feep-1'), float.fromhex('0x1.a39ef35793c76p-33')
_EXP_COEF = [1.0 / math.factorial(i) for i in range(14)]      # correctly rounded quotients of exact integers, as the compiler folds them


def exp_fixed_reference(x):
    """The device's exponential restated in float64 numpy, operation by operation (include/clothhip.h: PPO ON THE DEVICE; csrc/
    cloth_policy_fit.hpp exp_fixed): x clamped to [-40, 40], k = rint(x log2e), r = (x - k ln2_hi) - k ln2_lo with fdlibm's constants,
    Horner over 1 / i! for i = 13 .. 0 with a rounded product and a rounded sum per step, the result scaled by 2^k exactly. Bit for bit
    what the kernel and clothhip_selftest_exp_fixed compute; within 2.2e-16 relative of math.exp, and exactly 1.0 at 0."""
    x = np.minimum(np.maximum(np.asarray(x, dtype=np.float64), -40.0), 40.0)
    k = np.rint(x * _LOG2E)
    r = (x - k * _LN2_HI) - k * _LN2_LO
    p = np.full_like(x, _EXP_COEF[13])
    for i in range(12, -1, -1):
        p = p * r + _EXP_COEF[i]
    return np.ldexp(p, k.astype(np.int64))


def ppo_loss_reference(y, actions, old, adv, sigma, clip, B):
    """k_fit_loss_ppo restated in float64 numpy from a given float32 y, bit for bit, reduction order included (include/clothhip.h: PPO
    ON THE DEVICE): y, actions, old [B, 4] and adv [B] are the minibatch's rows in order (the network's output, the stored labels, old
    means and weights, all float32). Returns (stats float64[3] = loss, clip_fraction, kl; dz float32[B, 4]; ratio float32[B]; active
    bool[B])."""
    f64 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
    mu, a, mo, A = f64(y).reshape(-1, 4), f64(actions).reshape(-1, 4), f64(old).reshape(-1, 4), f64(adv).reshape(-1)
    if not (len(mu) == len(a) == len(mo) == len(A) == int(B)):
        raise ValueError("y, actions, old [B, 4] and adv [B] must hold the B rows of the minibatch")
    inv_s2 = 1.0 / (float(sigma) * float(sigma))
    half, lo, hi, Bd = 0.5 * inv_s2, 1.0 - float(clip), 1.0 + float(clip), float(int(B))
    q, kl = np.zeros(len(A)), np.zeros(len(A))
    for k in range(4):
        d_old, d_new, e = a[:, k] - mo[:, k], a[:, k] - mu[:, k], mu[:, k] - mo[:, k]
        q = q + (d_old * d_old - d_new * d_new)
        kl = kl + e * e
    rho = exp_fixed_reference(q * half)
    s1, s2 = rho * A, np.minimum(np.maximum(rho, lo), hi) * A
    active = s1 <= s2
    with np.errstate(over='ignore'):
        dz = np.where(active[:, None], (((s1[:, None] * (mu - a)) * inv_s2) / Bd).astype(np.float32), np.float32(0.0)).astype(np.float32)
    stats = np.array([-_house_sum(np.where(active, s1, s2)) / Bd, _house_sum(np.where(active, 0.0, 1.0)) / Bd, _house_sum(kl * half) / Bd])
    return stats, dz, rho.astype(np.float32), active


def ppo_reference(layers, obs, actions, old, adv, idx, sigma, clip):
    """Pure-numpy float64 loss and gradient of PPO's clipped surrogate for a Gaussian policy of fixed standard deviation sigma whose
    mean is the network's output, beside fit_reference and with its conventions (obs [n, in], actions [n, 4], old [n, 4] the old
    means, adv [n] the advantages, all rounded to float32 first; idx [B] the minibatch; math.exp):
        rho_r = exp((|a - mu_old|^2 - |a - mu|^2) / (2 sigma^2))   (the exponent clamped to [-40, 40], as the device does),
        L = -1 / B sum_r min(rho_r A_r, clip(rho_r, 1 - eps, 1 + eps) A_r),
    a row is ACTIVE when rho A <= clip(rho) A (the first term is the minimum: its gradient counts; inside the interval both are equal),
    dL/dmu_rk = A rho (mu_rk - a_rk) / (sigma^2 B) on active rows, else 0. Returns (stats, [(dW, db), ...], rho float64[B], active
    bool[B]) with stats = (loss, clip_fraction = share of rows not active, kl = 1 / B sum_r |mu - mu_old|^2 / (2 sigma^2))."""
    ix = np.asarray(idx, dtype=np.int64).reshape(-1)
    Ws = [np.asarray(W, dtype=np.float32).astype(np.float64) for W, _ in layers]
    bs = [np.asarray(b, dtype=np.float32).astype(np.float64) for _, b in layers]
    f64 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    x, a, mo, A = f64(obs)[ix], f64(actions)[ix], f64(old)[ix], f64(adv).reshape(-1)[ix]
    B, L = len(ix), len(Ws)
    hs = [x]
    for l in range(L):
        z = hs[-1] @ Ws[l].T + bs[l]
        hs.append(np.maximum(z, 0.0) if l + 1 < L else z)
    mu = hs[-1]
    inv_s2 = 1.0 / (float(sigma) * float(sigma))
    q = ((a - mo) ** 2 - (a - mu) ** 2).sum(axis=1)
    rho = np.array([math.exp(min(max(v, -40.0), 40.0)) for v in q * (0.5 * inv_s2)])
    s1, s2 = rho * A, np.clip(rho, 1.0 - float(clip), 1.0 + float(clip)) * A
    active = s1 <= s2
    stats = (float(-np.where(active, s1, s2).sum() / B), float((~active).sum() / float(B)), float((((mu - mo) ** 2).sum(axis=1) * (0.5 * inv_s2)).sum() / B))
    g = np.where(active[:, None], (s1[:, None] * (mu - a)) * inv_s2 / B, 0.0)
    grads = [None] * L
    for l in range(L - 1, -1, -1):
        grads[l] = (g.T @ hs[l], g.sum(axis=0))
        if l:
            g = (g @ Ws[l]) * (hs[l] > 0.0)
    return stats, grads, rho, active


def adam_reference(theta, m, v, g, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """The device's Adam step restated in numpy float32, operation by operation (include/clothhip.h, clothhip_policy_fit): t is the
    1-based step count. Returns the new (theta, m, v), float32."""
    f = np.float32
    b1, b2, g = f(beta1), f(beta2), np.asarray(g, dtype=f)
    a_t = f(float(f(lr)) * np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t))
    omb1, omb2 = f(1.0 - float(b1)), f(1.0 - float(b2))
    m = (b1 * np.asarray(m, dtype=f)).astype(f) + (omb1 * g).astype(f)
    v = (b2 * np.asarray(v, dtype=f)).astype(f) + (omb2 * (g * g).astype(f)).astype(f)
    q = m / (np.sqrt(v).astype(f) + f(eps)).astype(f)
    return (np.asarray(theta, dtype=f) - (a_t * q.astype(f)).astype(f)).astype(f), m.astype(f), v.astype(f)


def sgd_reference(theta, u, g, lr=1e-3, momentum=0.0):
    """The device's SGD step in numpy float32: u = fl(fl(mu u) + g), theta = fl(theta - fl(lr u)). Returns the new (theta, u)."""
    f = np.float32
    u = ((f(momentum) * np.asarray(u, dtype=f)).astype(f) + np.asarray(g, dtype=f)).astype(f)
    return (np.asarray(theta, dtype=f) - (f(lr) * u).astype(f)).astype(f), u


class MLPTrainer(object):
    """Supervised training of the env's shared network ON THE DEVICE (no reference counterpart; ClothBatch.fit_*): a mean-squared-error
    fit of (observation row, action label) pairs by Adam or SGD with momentum, the refit half of a DAgger / behaviour-cloning iteration.
    `policy_or_layers` is a policies.MLPPolicy or a list of (W, b) layers; the constructor puts it on the env (ClothVecEnv.set_policy,
    which also restarts the optimizer). The dataset lives on the device and grows by append (DAgger's D <- D u D_i); step trains the
    network in place, so the next step_many(policy='mlp') and policy_actions run the fitted weights with no download and no upload;
    layers() downloads them. Whoever puts another network on the env afterwards replaces the fitted one.

    The minibatches are a table: step(n_steps, batch_size, seed) draws RandomState(seed).randint(0, n, size=(n_steps, batch_size)) as
    int32 -- a function of (seed, n, n_steps, batch_size) alone."""

    def __init__(self, env, policy_or_layers, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        from . import _lib
        if optimizer not in _lib.FIT_OPTIMIZERS:
            raise ValueError("optimizer must be one of %r (got %r)" % (sorted(_lib.FIT_OPTIMIZERS), optimizer))
        self.env = env
        self.hyper = dict(optimizer=optimizer, lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(eps), momentum=float(momentum))
        layers = getattr(policy_or_layers, 'layers', policy_or_layers)
        self.widths, blob = pack_mlp(layers, n_in=3 * env.P)
        self.n_params = int(blob.size)
        env.set_policy(policy_or_layers)
        env.batch.fit_clear()

    @staticmethod
    def index_table(n, n_steps, batch_size, seed):
        """int32[n_steps, batch_size] rows of a dataset of n: RandomState(seed).randint(0, n, size=(n_steps, batch_size))."""
        if int(n) < 1 or int(n_steps) < 0 or int(batch_size) < 1:
            raise ValueError("index_table needs n >= 1, n_steps >= 0, batch_size >= 1")
        return np.random.RandomState(seed).randint(0, int(n), size=(int(n_steps), int(batch_size))).astype(np.int32)

    def append(self, obs, labels, weights=None):
        """Add rows to the dataset (obs [n, 3P], labels [n, 4], finite; weights [n]: their loss weights, None: 1); returns its size."""
        return self.env.batch.fit_append(obs, labels, weights)

    def append_launch(self, rows, labels="expert", weights=None):
        """Add rows that lie on the device (ClothBatch.fit_append_launch): rows int[n, 3] = (source, row, label_row) into the last
        launch's tables and the held rows, as envs.slot_start_sources names them; labels="expert": the last armed launch's label,
        labels="action": the action that slot executed; weights [n]: the rows' loss weights, None: 1. Returns the dataset's size."""
        return self.env.batch.fit_append_launch(rows, labels, weights)

    def data(self, first=0, n=None):
        """(obs float32[n, 3P], labels float32[n, 4]): the stored rows [first, first + n) by download, n=None: to the end."""
        return self.env.batch.fit_data(first, n)

    def set_weights(self, weights, first=0):
        """Write the loss weights of the stored rows [first, first + len(weights)): any finite float32 (ClothBatch.fit_set_weights)."""
        self.env.batch.fit_set_weights(weights, first)

    def weights(self, first=0, n=None):
        """float32[n]: the loss weights of the stored rows [first, first + n), n=None: to the end."""
        return self.env.batch.fit_get_weights(first, n)

    def predict(self, idx):
        """float32[n, 4]: the trainer's forward on the dataset rows idx at the present weights -- the y of grad and step, bit for bit."""
        return self.env.batch.fit_predict(idx)

    def loss(self, idx):
        """The MSE over the dataset rows idx (any number: a held-out split by index) at the present weights, forward only."""
        return self.env.batch.fit_loss(idx)

    def size(self):
        return self.env.batch.fit_size()

    def clear(self):
        self.env.batch.fit_clear()

    def step(self, n_steps, batch_size, seed):
        """n_steps optimizer steps on minibatches of batch_size rows drawn by index_table(size(), n_steps, batch_size, seed); returns
        float64[n_steps], each step's loss before its update."""
        n = self.size()
        if n < 1:
            raise ValueError("the dataset is empty: append first")
        return self.env.batch.fit(self.index_table(n, n_steps, batch_size, seed), **self.hyper)

    def grad(self, idx):
        """(loss, [(dW, db), ...]) over the dataset rows idx at the present weights, float32 from the device; nothing is updated."""
        loss, g = self.env.batch.fit_grad(idx)
        return loss, unpack_mlp(self.widths, g)

    def snapshot_old(self, first=0, n=None):
        """Store the network's present output on the dataset rows [first, first + n) (n=None: to the end) as their OLD MEANS, on the
        device (ClothBatch.fit_snapshot_policy): what ppo_step's probability ratios are taken against. Call it after a collection and
        before the first policy step on it."""
        self.env.batch.fit_snapshot_policy(first, n)

    @staticmethod
    def ppo_epoch_tables(rows, n_epochs, batch_size, seed):
        """The minibatches of ppo_step: a list of n_epochs int32 tables [n_minibatches, B]. ONE RandomState(seed) draws a permutation of
        `rows` (int [m]) per epoch, which is cut into minibatches of batch_size in order; the short tail is dropped when there is more
        than one minibatch, and m < batch_size gives one minibatch of all m rows. A function of the arguments alone."""
        rows = np.asarray(rows)
        if rows.ndim != 1 or rows.size < 1 or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError("rows must be a non-empty 1-d integer array")
        if int(n_epochs) < 0 or int(batch_size) < 1:
            raise ValueError("ppo_epoch_tables needs n_epochs >= 0, batch_size >= 1")
        m, B = rows.size, min(int(batch_size), rows.size)
        r = np.random.RandomState(seed)
        return [rows[r.permutation(m)][:(m // B) * B].reshape(m // B, B).astype(np.int32) for _ in range(int(n_epochs))]

    def ppo_step(self, n_epochs, batch_size, seed, sigma, clip=0.2, target_kl=None, rows=None):
        """PPO on the device (ClothBatch.fit_ppo): up to n_epochs epochs over `rows` (int [m] dataset rows, None: all), each the
        minibatches of ppo_epoch_tables in ONE fit_ppo call -- optimizer steps on the clipped surrogate with the advantages in the
        weight column and the old means of snapshot_old, under this trainer's optimizer (shared with step). sigma is the standard
        deviation of the noise the rows' actions were drawn with, clip the range epsilon. With target_kl the loop stops after the first
        epoch whose mean kl exceeds it. Returns (stats float64[steps, 3]: loss, clip_fraction, kl of every step before its update;
        epochs run)."""
        if rows is None:
            n = self.size()
            if n < 1:
                raise ValueError("the dataset is empty: append first")
            rows = np.arange(n)
        out, epochs = [], 0
        for table in self.ppo_epoch_tables(rows, n_epochs, batch_size, seed):
            stats = self.env.batch.fit_ppo(table, sigma, clip, **self.hyper)
            out.append(stats)
            epochs += 1
            if target_kl is not None and float(np.mean(stats[:, 2])) > float(target_kl):
                break
        return (np.concatenate(out) if out else np.zeros((0, 3))), epochs

    def layers(self):
        """The network as the device holds it now: [(W, b), ...] float32, by download (clothhip_get_policy_mlp)."""
        return unpack_mlp(self.widths, self.env.batch.get_policy_mlp(0, self.n_params))

    def reset(self):
        """Zero the optimizer's moments and step count; the weights and the dataset stay."""
        self.env.batch.fit_reset()


class ValueTrainer(object):
    """The critic of an actor-critic ON THE DEVICE (no reference counterpart; ClothBatch.value_*): a network V(s) with ONE output over
    the rows of the env's dataset -- the dataset an MLPTrainer on the same env fills --, fitted to the column of value targets
    (ClothBatch.fit_set_returns, or fit_gae's ret) by the trainer's kernels under L_V = 1 / (2 B) sum (v - ret)^2, unweighted. `layers`
    is a list of (W, b) with a last width of 1; the constructor puts it on the env's batch beside the policy, which it leaves alone (as
    every step here does, and the policy's steps leave the critic alone). The dataset is not cleared."""

    def __init__(self, env, layers, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        from . import _lib
        if optimizer not in _lib.FIT_OPTIMIZERS:
            raise ValueError("optimizer must be one of %r (got %r)" % (sorted(_lib.FIT_OPTIMIZERS), optimizer))
        self.env = env
        self.hyper = dict(optimizer=optimizer, lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(eps), momentum=float(momentum))
        self.widths, blob = pack_mlp(layers, n_in=3 * env.P, n_out=1)
        self.n_params = int(blob.size)
        env.batch.set_value_mlp(layers)

    def step(self, n_steps, batch_size, seed, rows=None):
        """n_steps optimizer steps on minibatches of batch_size rows drawn by MLPTrainer.index_table(n, n_steps, batch_size, seed) with n
        the dataset's size, or with rows (int [m]: a subset of the dataset, e.g. its non-leaf rows) n = m and the table's entries name
        rows[...]. Returns float64[n_steps], each step's loss before its update."""
        if rows is None:
            n = self.env.batch.fit_size()
            if n < 1:
                raise ValueError("the dataset is empty: append first")
            table = MLPTrainer.index_table(n, n_steps, batch_size, seed)
        else:
            rows = np.asarray(rows)
            if rows.ndim != 1 or rows.size < 1 or not np.issubdtype(rows.dtype, np.integer):
                raise ValueError("rows must be a non-empty 1-d integer array")
            table = rows.astype(np.int32)[MLPTrainer.index_table(rows.size, n_steps, batch_size, seed)]
        return self.env.batch.value_fit(table, **self.hyper)

    def predict(self, idx):
        """float32[n]: the critic on the dataset rows idx at the present weights -- the v of grad and step, bit for bit."""
        return self.env.batch.value_predict(idx)

    def grad(self, idx):
        """(loss, [(dW, db), ...]) over the dataset rows idx at the present weights, float32 from the device; nothing is updated."""
        loss, g = self.env.batch.value_grad(idx)
        return loss, unpack_mlp(self.widths, g)

    def layers(self):
        """The critic as the device holds it now: [(W, b), ...] float32, by download (clothhip_get_value_mlp)."""
        return unpack_mlp(self.widths, self.env.batch.get_value_mlp())

    def reset(self):
        """Zero the critic's moments and step count; its weights, the policy's optimizer and the dataset stay."""
        self.env.batch.value_fit_reset()


def ensemble_disagreement(actions):
    """float64[n] from actions [G, n, 4]: the mean over the four action components of the population variance over the G members
    (numpy float64, var with ddof = 0) -- the novelty signal of a bootstrapped ensemble."""
    a = np.asarray(actions, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1:
        raise ValueError("actions must have shape (G, n, 4) (got %r)" % (a.shape,))
    return a.var(axis=0).mean(axis=1)


class MLPEnsemble(object):
    """G networks of ONE shape, one per env slot, FITTED TOGETHER ON THE DEVICE (no reference counterpart; ClothBatch.fit_*_members): a
    bootstrapped ensemble for DAgger (disagreement(obs) is the novelty signal), a learning-rate sweep, population-based training.
    `members_layers` is a list of G networks, each a list of (W, b) layers as MLPPolicy takes them; the constructor puts them on the env
    as a population (ClothVecEnv.set_policy -> ClothBatch.set_policy_population, which also restarts every row's optimizer) and empties
    the dataset. `member` int[E] says which network env e runs (default e % G). step_many(policy='mlp'), collect_demos(on_device=True)
    and an armed launch take it as they take an MLPPopulation. The dataset is the env's ONE device-resident dataset, with MLPTrainer's
    methods over it, so demos.dagger_fit and demos.dagger_collect take an ensemble where they take a trainer; step trains every member
    on ITS OWN minibatches (the bootstrap), all members in the launches of one network, each row in place: the next launch runs the
    fitted weights with no download and no upload. Member g's weights are bit for bit those of an MLPTrainer that fits network g alone
    on the same rows. Whoever puts another network on the env afterwards replaces the fitted rows (putting THIS ensemble back uploads
    the constructor's weights again, not the fitted ones: keep layers(g) if the fit is to survive that).

    Hyper-parameters (lr, beta1, beta2, eps, momentum) are scalars or sequences of G, one per member; the optimizer is one."""

    noise_std = 0.0        # (collect_demos: no exploration noise)

    def __init__(self, env, members_layers, member=None, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        from . import _lib
        if optimizer not in _lib.FIT_OPTIMIZERS:
            raise ValueError("optimizer must be one of %r (got %r)" % (sorted(_lib.FIT_OPTIMIZERS), optimizer))
        self.env = env
        self.nets = [[(np.array(W, dtype=np.float32), np.array(b, dtype=np.float32)) for W, b in layers] for layers in members_layers]
        self.widths, blob = pack_population(self.nets, n_in=3 * env.P)
        self.G, self.n_params = int(blob.shape[0]), int(blob.shape[1])
        self.hyper = {'optimizer': optimizer}
        for k, v in (('lr', lr), ('beta1', beta1), ('beta2', beta2), ('eps', eps), ('momentum', momentum)):
            v = np.asarray(v, dtype=np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.size != self.G):
                raise ValueError("%s must be a scalar or %d values, one per member" % (k, self.G))
            v32 = v.astype(np.float32)
            if not (np.isfinite(v32).all() and (v32 >= 0.0).all()) or (k.startswith('beta') and (v32 >= 1.0).any()):
                raise ValueError("%s = %r: hyper-parameters are finite and >= 0, the betas below 1" % (k, v.tolist()))
            self.hyper[k] = np.broadcast_to(v, (self.G,)).copy()
        m = np.arange(env.E) % self.G if member is None else np.asarray(member)
        if m.shape != (env.E,):
            raise ValueError("member must have shape (%d,) (got %r)" % (env.E, m.shape))
        if not np.issubdtype(m.dtype, np.integer) or m.min() < 0 or m.max() >= self.G:
            raise ValueError("member must hold integers in [0, %d)" % self.G)
        self.member = m.astype(np.int32)
        env.set_policy(self)
        env.batch.fit_clear()

    def _upload(self, batch):
        batch.set_policy_population(self.nets, self.member)

    def _on_env(self):
        if self.env._policy_mlp is not self:
            raise ValueError("another network was put on the env: the ensemble's fitted rows are gone (env.set_policy(ensemble) uploads "
                             "the constructor's weights again)")

    def _members(self, members):
        """members (None: all G) as a checked int array of distinct rows."""
        m = np.arange(self.G) if members is None else np.asarray(members)
        if m.ndim != 1 or m.size < 1 or not np.issubdtype(m.dtype, np.integer) or m.min() < 0 or m.max() >= self.G:
            raise ValueError("members must be a non-empty 1-d array of integers in [0, %d)" % self.G)
        if np.unique(m).size != m.size:
            raise ValueError("members must be distinct")
        return m.astype(np.int32)

    # the dataset: MLPTrainer's methods over the env's one dataset
    def append(self, obs, labels, weights=None):
        """Add rows to the dataset (obs [n, 3P], labels [n, 4], finite; weights [n]: their loss weights, None: 1); returns its size."""
        return self.env.batch.fit_append(obs, labels, weights)

    def append_launch(self, rows, labels="expert", weights=None):
        """Add rows that lie on the device (ClothBatch.fit_append_launch), as MLPTrainer.append_launch; returns the dataset's size."""
        return self.env.batch.fit_append_launch(rows, labels, weights)

    def data(self, first=0, n=None):
        """(obs float32[n, 3P], labels float32[n, 4]): the stored rows [first, first + n) by download, n=None: to the end."""
        return self.env.batch.fit_data(first, n)

    def set_weights(self, weights, first=0):
        """Write the loss weights of the stored rows [first, first + len(weights)): any finite float32 (ClothBatch.fit_set_weights)."""
        self.env.batch.fit_set_weights(weights, first)

    def weights(self, first=0, n=None):
        """float32[n]: the loss weights of the stored rows [first, first + n), n=None: to the end."""
        return self.env.batch.fit_get_weights(first, n)

    def predict(self, idx, members=None):
        """float32[n_m, n, 4]: the trainer's forward of the rows `members` (None: all G) on the dataset rows idx [n], the same rows for
        every member -- each member's y of grad and step, bit for bit; nothing is updated."""
        m = self._members(members)
        self._on_env()
        return self.env.batch.fit_predict(idx, m)

    def size(self):
        return self.env.batch.fit_size()

    def clear(self):
        self.env.batch.fit_clear()

    def index_table(self, n, n_steps, batch_size, seed, bootstrap=True):
        """int32[n_steps, G, batch_size] rows of a dataset of n, a function of the arguments (and G) alone. bootstrap=True:
        RandomState(seed).randint(0, n, size=(n_steps, G, batch_size)) -- every member draws its own minibatches; bootstrap=False:
        MLPTrainer.index_table(n, n_steps, batch_size, seed) repeated along the member axis -- every member sees the same rows."""
        if int(n) < 1 or int(n_steps) < 0 or int(batch_size) < 1:
            raise ValueError("index_table needs n >= 1, n_steps >= 0, batch_size >= 1")
        if bootstrap:
            return np.random.RandomState(seed).randint(0, int(n), size=(int(n_steps), self.G, int(batch_size))).astype(np.int32)
        one = MLPTrainer.index_table(n, n_steps, batch_size, seed)
        return np.ascontiguousarray(np.repeat(one[:, None, :], self.G, axis=1))

    def step(self, n_steps, batch_size, seed, members=None, bootstrap=True):
        """n_steps optimizer steps of the rows `members` (None: all G) on the minibatches index_table(size(), n_steps, batch_size, seed,
        bootstrap)[:, members]; returns float64[n_steps, n_m], each member's loss before each step's update."""
        n = self.size()
        if n < 1:
            raise ValueError("the dataset is empty: append first")
        m = self._members(members)
        self._on_env()
        table = np.ascontiguousarray(self.index_table(n, n_steps, batch_size, seed, bootstrap)[:, m])
        hyper = {k: (v if k == 'optimizer' else v[m]) for k, v in self.hyper.items()}
        return self.env.batch.fit_members(m, table, hyper)

    def grad(self, idx, members=None):
        """(loss float64[n_m], [[(dW, db), ...] per member]) over the dataset rows idx [n_m, B] at the present weights, float32 from the
        device; nothing is updated."""
        m = self._members(members)
        self._on_env()
        loss, g = self.env.batch.fit_grad_members(m, idx)
        return loss, [unpack_mlp(self.widths, g[j]) for j in range(m.size)]

    def layers(self, g):
        """Network g as the device holds it now: [(W, b), ...] float32, by download (clothhip_get_policy_mlp)."""
        self._on_env()
        return unpack_mlp(self.widths, self.env.batch.get_policy_mlp(int(g), self.n_params))

    def reset(self, members=None):
        """Zero the moments and step counts of the rows `members` (None: all); the weights and the dataset stay."""
        self._on_env()
        self.env.batch.fit_reset_members(None if members is None else self._members(members))

    def get_action(self, obs, t=0):
        """float64[E, 4]: env e's network member[e] on obs[e], on the device -- the bits the launch computes."""
        self._on_env()
        return self.env.batch.policy_eval_members(np.asarray(obs).reshape(self.env.E, -1).astype(np.float32), self.member)

    def actions(self, obs):
        """float64[G, n, 4]: every member on every row of obs [n, 3P], on the device (ClothBatch.policy_eval_members on the rows tiled G
        times)."""
        self._on_env()
        rows = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1, int(self.widths[0]))
        n = rows.shape[0]
        out = self.env.batch.policy_eval_members(np.tile(rows, (self.G, 1)), np.repeat(np.arange(self.G, dtype=np.int32), n))
        return out.reshape(self.G, n, 4)

    def disagreement(self, obs):
        """float64[n]: per row the mean over the action components of the members' variance. obs float[n, 3P]: host rows, through
        ensemble_disagreement(actions(obs)); obs int[n]: rows of the DATASET by index, through predict -- the trainer's forward on rows
        the host need not hold."""
        a = np.asarray(obs)
        if a.ndim == 1 and np.issubdtype(a.dtype, np.integer):
            return ensemble_disagreement(self.predict(a))
        return ensemble_disagreement(self.actions(obs))


# ---- the cross-entropy planner (clothhip.h: PLAN ACTIONS ON THE DEVICE; csrc/cloth_plan.hpp) ----------------------------------------------
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)
_EPS_SCALE = np.array([0x33DDB3D7], dtype=np.uint32).view(np.float32)[0]      # (float)(sqrt(3) / 2^24)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (standard constants). ctr: four arrays of uint32 values of one shape, key: two ints. Returns the four output words
    as uint64 arrays below 2^32."""
    c = list(np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _U32 for x in ctr]))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
        p0, p1 = _PHILOX_M0 * c[0], _PHILOX_M1 * c[2]                  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _U32]
    return c


def philox_eps(seed, k, i):
    """population_eps(seed, k, i) of csrc/cloth_philox.hpp as float32, i an integer array: Philox4x32-10 keyed by the two halves of seed
    on the counter (i lo, i hi, k, 0); the four words' top 24 bits summed and centred, times (float)(sqrt(3) / 2^24). Zero mean, unit
    variance, |eps| <= 3.47 -- the variate of the MLP population and of the planner's candidates."""
    i = np.asarray(i, dtype=np.uint64)
    seed = int(seed)
    r = philox4x32_10((i & _U32, i >> np.uint64(32), np.uint64(int(k) & 0xFFFFFFFF), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))
    S = sum(x >> np.uint64(8) for x in r)
    D = S.astype(np.int64) - (2 ** 25 - 2)
    return D.astype(np.int32).astype(np.float32) * _EPS_SCALE


def _plan_clip(v, lo, hi):
    """clip(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v), lo / hi per action component (the last axis)."""
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def plan_sample_reference(mean, std, act_low, act_high, n_candidates, seed=0, iteration=0):
    """k_plan_sample in numpy, bit for bit: mean, std float64 [E, H, 4] -> the action table [H, E K, 4];
    x[h][e K + k][a] = clip(mean + std * (double)eps(seed, iteration, ((e K + k) H + h) 4 + a)), candidate k = 0 = clip(mean).
    iteration is iter0 + it."""
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    E, H, _ = mean.shape
    K = int(n_candidates)
    lo = np.broadcast_to(np.asarray(act_low, dtype=np.float64), (4,))
    hi = np.broadcast_to(np.asarray(act_high, dtype=np.float64), (4,))
    slot = np.arange(E * K, dtype=np.int64)[None, :, None]
    h = np.arange(H, dtype=np.int64)[:, None, None]
    a = np.arange(4, dtype=np.int64)[None, None, :]
    eps = philox_eps(seed, iteration, (slot * H + h) * 4 + a).astype(np.float64)            # [H, E K, 4]
    m = np.repeat(mean.transpose(1, 0, 2), K, axis=1)                                      # [H, E K, 4]: row e K + k is env e's
    sd = np.repeat(std.transpose(1, 0, 2), K, axis=1)
    step = sd * eps
    v = np.where((slot % K) == 0, m, m + step)
    return np.ascontiguousarray(_plan_clip(v, lo, hi))


def plan_score_reference(records, penalty=1.0):
    """The planner's score of every branch from a launch's records [H, n]: the coverage of the last executed slot (ran != 0), minus
    `penalty` when any executed slot has oob or tear; -inf for a column without an executed slot. float64 [n]."""
    ran = records['ran'] != 0
    H, n = ran.shape
    last = np.where(ran.any(axis=0), H - 1 - np.argmax(ran[::-1], axis=0), -1)
    bad = (ran & ((records['oob'] != 0) | (records['tear'] != 0))).any(axis=0)
    cov = records['coverage'][np.maximum(last, 0), np.arange(n)]
    return np.where(last < 0, -np.inf, np.where(bad, cov - float(penalty), cov))


def plan_refit_reference(x, scores, mean, std, n_elite, alpha=1.0, min_std=0.0, done=None):
    """k_plan_refit in numpy, bit for bit: the action table x [H, E K, 4] and scores [E, K] -> (mean, std after the refit, elite
    bool[E, K], top int32[E]). Candidates are ranked by (score descending, k ascending); per (h, a) the elites are summed in
    ascending k: mu = sum / M, var = sum (x - mu)^2 / M, sd = sqrt(var); mean <- alpha mu + beta mean, std <- max(min_std, alpha sd +
    beta std), beta = 1 - alpha. An env with done set keeps its rows, has no elites and top -1."""
    x = np.asarray(x, dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float64)
    E, K = scores.shape
    H, M = x.shape[0], int(n_elite)
    mean = np.array(np.broadcast_to(np.asarray(mean, dtype=np.float64), (E, H, 4)))
    std = np.array(np.broadcast_to(np.asarray(std, dtype=np.float64), (E, H, 4)))
    ms = np.broadcast_to(np.asarray(min_std, dtype=np.float64), (4,))
    alpha = np.float64(alpha)
    beta = np.float64(1.0) - alpha
    Md = np.float64(M)
    elite = np.zeros((E, K), dtype=bool)
    top = np.full(E, -1, dtype=np.int32)
    for e in range(E):
        if done is not None and done[e]:
            continue
        order = np.lexsort((np.arange(K), -scores[e]))                # score descending, then k ascending
        top[e] = order[0]
        elite[e, order[:M]] = True
        ks = np.nonzero(elite[e])[0]                                  # ascending k
        xe = x[:, e * K + ks, :]                                      # [H, M, 4]
        tot = np.zeros((H, 4))
        for j in range(M):
            tot = tot + xe[:, j, :]
        mu = tot / Md
        sq = np.zeros((H, 4))
        for j in range(M):
            d = xe[:, j, :] - mu
            sq = sq + d * d
        sd = np.sqrt(sq / Md)
        mean[e] = alpha * mu + beta * mean[e]
        ns = alpha * sd + beta * std[e]
        std[e] = np.where(ns < ms, ms, ns)
    return mean, std, elite, top


def cem_reference(env, scratch_batch, horizon, n_candidates, n_elite, n_iters, mean, std, min_std=0.0, alpha=1.0, penalty=1.0, seed=0,
                  iter0=0):
    """clothhip_plan_cem's loop on the host, from its parts: plan_sample_reference, scratch_batch.fork_from(env.batch), the host-table
    run_actions launch on scratch_batch (E K cloths), plan_score_reference, plan_refit_reference, and the best-so-far rule. Returns the
    dict ClothBatch.plan_cem returns with want_scores and want_candidates. On one scratch batch both routes run the same kernels on
    the same states, so every table agrees bit for bit."""
    E, K, H, n = env.E, int(n_candidates), int(horizon), int(n_iters)
    mean = np.array(np.broadcast_to(np.asarray(mean, dtype=np.float64), (E, H, 4)))
    std = np.array(np.broadcast_to(np.asarray(std, dtype=np.float64), (E, H, 4)))
    done = np.asarray(env._ep_done, dtype=bool)
    rep = np.repeat(np.arange(E), K)
    ep = env._episode_params()
    lo, hi = env.action_space.low, env.action_space.high
    best_a, best_s = np.full((E, H, 4), np.nan), np.full(E, np.nan)
    scores, cands = np.zeros((n, E, K)), np.zeros((n, H, E * K, 4))
    for it in range(n):
        x = plan_sample_reference(mean, std, lo, hi, K, seed=seed, iteration=iter0 + it)
        scratch_batch.fork_from(env.batch, rep)
        ns = np.ascontiguousarray(env.num_steps[rep], dtype=np.int32)
        dn = np.ascontiguousarray(done[rep], dtype=np.uint8)
        rec = scratch_batch.run_actions(ep, H, ns, dn, actions=x)[0]
        sc = plan_score_reference(rec, penalty).reshape(E, K)
        mean, std, _, top = plan_refit_reference(x, sc, mean, std, n_elite, alpha=alpha, min_std=min_std, done=done)
        for e in np.nonzero(~done)[0]:
            if it == 0 or sc[e, top[e]] > best_s[e]:
                best_s[e] = sc[e, top[e]]
                best_a[e] = x[:, e * K + top[e], :]
        scores[it], cands[it] = sc, x
    return dict(mean=mean, std=std, actions=best_a, score=best_s, scores=scores, candidates=cands)


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
