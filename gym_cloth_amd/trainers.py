"""The trainers: Python drivers of the fit that runs ON THE DEVICE (no reference counterpart), over the env's one device-resident dataset.
MLPTrainer           the supervised refit of the shared network on the device (ClothBatch.fit_*), Adam or SGD over (observation, label)
                     rows, and PPO's clipped surrogate over the same rows; references.fit_reference / ppo_reference are its yardsticks
ValueTrainer         the critic of an actor-critic (ClothBatch.value_*; references.value_fit_reference, gae_reference)
QTrainer             the critic of DDPG over (state, action) with its target copies (ClothBatch.q_*, ddpg_*; references.q_fit_reference,
                     dpg_reference); MLPTrainer.ddpg_step is the loop's step
MLPEnsemble          G networks, one per env slot, fitted together on the device in the launches of one (ClothBatch.fit_members): a
                     bootstrapped ensemble whose disagreement is a novelty signal, a learning-rate sweep -- also of PPO, every member
                     under its own sigma, clip and optimizer (ClothBatch.fit_ppo_members)"""
import numpy as np

from . import _lib
from .mlp import pack_mlp, pack_population, unpack_mlp


def _hyper(optimizer, **scalars):
    """A trainer's `hyper` dict: the optimizer (ValueError for an unknown one) and the given scalar hyper-parameters as floats."""
    if optimizer not in _lib.FIT_OPTIMIZERS:
        raise ValueError("optimizer must be one of %r (got %r)" % (sorted(_lib.FIT_OPTIMIZERS), optimizer))
    return dict(optimizer=optimizer, **{k: float(v) for k, v in scalars.items()})


def _check_rows(rows):
    """`rows` as an array: a non-empty 1-d list of dataset rows, integers."""
    rows = np.asarray(rows)
    if rows.ndim != 1 or rows.size < 1 or not np.issubdtype(rows.dtype, np.integer):
        raise ValueError("rows must be a non-empty 1-d integer array")
    return rows


class _EnvDataset(object):
    """The env's ONE device-resident dataset as the trainers on `self.env` see it (no state of its own)."""

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

    def size(self):
        return self.env.batch.fit_size()

    def clear(self):
        self.env.batch.fit_clear()


class MLPTrainer(_EnvDataset):
    """Supervised training of the env's shared network ON THE DEVICE (no reference counterpart; ClothBatch.fit_*): a mean-squared-error
    fit of (observation row, action label) pairs by Adam or SGD with momentum, the refit half of a DAgger / behaviour-cloning iteration.
    `policy_or_layers` is a policies.MLPPolicy or a list of (W, b) layers; the constructor puts it on the env (ClothVecEnv.set_policy,
    which also restarts the optimizer). The dataset lives on the device and grows by append (DAgger's D <- D u D_i); step trains the
    network in place, so the next step_many(policy='mlp') and policy_actions run the fitted weights with no download and no upload;
    layers() downloads them. Whoever puts another network on the env afterwards replaces the fitted one.

    The minibatches are a table: step(n_steps, batch_size, seed) draws RandomState(seed).randint(0, n, size=(n_steps, batch_size)) as
    int32 -- a function of (seed, n, n_steps, batch_size) alone."""

    def __init__(self, env, policy_or_layers, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        self.hyper = _hyper(optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum)
        self.env = env
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

    def predict(self, idx):
        """float32[n, 4]: the trainer's forward on the dataset rows idx at the present weights -- the y of grad and step, bit for bit."""
        return self.env.batch.fit_predict(idx)

    def loss(self, idx):
        """The MSE over the dataset rows idx (any number: a held-out split by index) at the present weights, forward only."""
        return self.env.batch.fit_loss(idx)

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
        before the first policy step on it. With a head on the batch (set_log_sigma) the same call stores the present head as the
        rows' OLD LOG SIGMA."""
        self.env.batch.fit_snapshot_policy(first, n)

    @staticmethod
    def ppo_epoch_tables(rows, n_epochs, batch_size, seed):
        """The minibatches of ppo_step: a list of n_epochs int32 tables [n_minibatches, B]. ONE RandomState(seed) draws a permutation of
        `rows` (int [m]) per epoch, which is cut into minibatches of batch_size in order; the short tail is dropped when there is more
        than one minibatch, and m < batch_size gives one minibatch of all m rows. A function of the arguments alone."""
        rows = _check_rows(rows)
        if int(n_epochs) < 0 or int(batch_size) < 1:
            raise ValueError("ppo_epoch_tables needs n_epochs >= 0, batch_size >= 1")
        m, B = rows.size, min(int(batch_size), rows.size)
        r = np.random.RandomState(seed)
        return [rows[r.permutation(m)][:(m // B) * B].reshape(m // B, B).astype(np.int32) for _ in range(int(n_epochs))]

    def set_log_sigma(self, log_sigma):
        """Put a head of a learned standard deviation on the env's batch (ClothBatch.set_policy_log_sigma): log_sigma [4] or a scalar
        for all four components; None drops it. Restarts the head's optimizer state alone."""
        self.env.batch.set_policy_log_sigma(None if log_sigma is None else np.broadcast_to(np.asarray(log_sigma, dtype=np.float64), (4,)))

    def log_sigma(self):
        """float32[4]: the head as the device holds it now, by download."""
        return self.env.batch.get_policy_log_sigma()

    def sigma(self):
        """float64[4]: exp(log_sigma()) -- the per-component standard deviation a collection acts with (MLPPolicy(noise_std=...), or
        unit noise times it as step_many's policy_noise)."""
        return np.exp(self.log_sigma().astype(np.float64))

    def device_noise(self, seed):
        """policies.DeviceNoise(seed) under the head: the collection's noise is made on the device from the head where it lies, sigma =
        exp_fixed(log_sigma) as the surrogate forms it -- no sigma and no noise table passes through the host."""
        from .policies import DeviceNoise
        return DeviceNoise(seed)

    def ppo_step(self, n_epochs, batch_size, seed, sigma=None, clip=0.2, target_kl=None, rows=None, ent_coef=0.0):
        """PPO on the device (ClothBatch.fit_ppo): up to n_epochs epochs over `rows` (int [m] dataset rows, None: all), each the
        minibatches of ppo_epoch_tables in ONE fit_ppo call -- optimizer steps on the clipped surrogate with the advantages in the
        weight column and the old means of snapshot_old, under this trainer's optimizer (shared with step). sigma is the standard
        deviation of the noise the rows' actions were drawn with, clip the range epsilon. With target_kl the loop stops after the first
        epoch whose mean kl exceeds it. Returns (stats float64[steps, 3]: loss, clip_fraction, kl of every step before its update;
        epochs run).
        sigma=None: the LEARNED head (set_log_sigma) in the place of a number -- ClothBatch.fit_ppo_sigma trains the network and the
        head on the surrogate minus ent_coef times the entropy, against the old means AND old log sigmas of snapshot_old; stats is then
        float64[steps, 4] (loss, clip_fraction, kl, entropy) and self.last_log_sigma float32[steps, 4] the head before every step."""
        if rows is None:
            n = self.size()
            if n < 1:
                raise ValueError("the dataset is empty: append first")
            rows = np.arange(n)
        if sigma is not None and float(ent_coef) != 0.0:
            raise ValueError("ent_coef belongs to the learned head: pass sigma=None")
        out, heads, epochs = [], [], 0
        for table in self.ppo_epoch_tables(rows, n_epochs, batch_size, seed):
            if sigma is None:
                stats, ls = self.env.batch.fit_ppo_sigma(table, clip, ent_coef, **self.hyper)
                heads.append(ls)
            else:
                stats = self.env.batch.fit_ppo(table, sigma, clip, **self.hyper)
            out.append(stats)
            epochs += 1
            if target_kl is not None and float(np.mean(stats[:, 2])) > float(target_kl):
                break
        if sigma is None:
            self.last_log_sigma = np.concatenate(heads) if heads else np.zeros((0, 4), dtype=np.float32)
        return (np.concatenate(out) if out else np.zeros((0, 3 if sigma is not None else 4))), epochs

    def ddpg_step(self, qcritic, n_steps, batch_size, seed, gamma=0.99, tau=0.005, act_bound=1.0, rows=None, q_coef=1.0, bc_coef=0.0, q_filter=True,
                  table=None):
        """n_steps DDPG steps on the device in ONE call (ClothBatch.ddpg_fit): per step the TD step of `qcritic` (a
        QTrainer on the same env), this network's step up the critic's action gradient, the soft update of both targets -- under this
        trainer's optimizer for the policy and qcritic's for the critic. The minibatches are index_table(m, n_steps, batch_size, seed)
        over `rows` (int [m] dataset rows WITH a transition; None: every non-leaf row of the dataset, old collections included). The
        targets must have been synced (qcritic.sync_targets). Returns float64[n_steps, 6]: the critic's (loss, mean q, mean y), then
        the actor's (loss = -mean q, gated fraction, mean |dL/da|), each before its update.
        bc_coef != 0 or q_coef != 1: the actor's step of DDPG from demonstrations (ClothBatch.dpg_bc_fit has the loss),
        q_filter: its Q-filter; returns float64[n_steps, 9] then, the actor's six behind the critic's three. bc_coef == 0 with
        q_coef == 1 takes the plain path, whatever q_filter says. table (int [n_steps, batch_size] dataset rows): the minibatches
        themselves, in the place of rows and seed."""
        if qcritic.env is not self.env:
            raise ValueError("the Q critic belongs to another env")
        bc = None if (float(bc_coef) == 0.0 and float(q_coef) == 1.0) else dict(q_coef=q_coef, bc_coef=bc_coef, q_filter=q_filter)
        if table is not None:
            return self.env.batch.ddpg_fit(np.asarray(table), gamma, tau, act_bound, policy_hyper=self.hyper, q_hyper=qcritic.hyper, bc=bc)
        if rows is None:
            rows = np.nonzero(self.env.batch.fit_get_transitions()[1] != _lib.FIT_NEXT_NONE)[0]
            if rows.size < 1:
                raise ValueError("the dataset holds no row with a transition: collect first")
        rows = _check_rows(rows)
        table = rows.astype(np.int32)[self.index_table(rows.size, n_steps, batch_size, seed)]
        return self.env.batch.ddpg_fit(table, gamma, tau, act_bound, policy_hyper=self.hyper, q_hyper=qcritic.hyper, bc=bc)

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
        self.hyper = _hyper(optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum)
        self.env = env
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
            rows = _check_rows(rows)
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


class QTrainer(object):
    """The critic of DDPG ON THE DEVICE (no reference counterpart; ClothBatch.q_*): a network Q(s, a) with ONE output
    over rows of 3P + 4 values -- a dataset row's observation followed by an action --, fitted to the TD target
    rew + gamma Q'(s', mu'(s')) through the row's successor, with target copies Q', mu' on the batch. `q_layers` is a list of (W, b)
    with an input width of 3P + 4 and a last width of 1; the constructor puts it on the env's batch beside the policy, which it leaves
    alone, and the dataset is not cleared. The targets exist from sync_targets on; a new policy or Q network drops its target."""

    def __init__(self, env, q_layers, optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0):
        self.hyper = _hyper(optimizer, lr=lr, beta1=beta1, beta2=beta2, eps=eps, momentum=momentum)
        self.env = env
        self.widths, blob = pack_mlp(q_layers, n_in=3 * env.P + 4, n_out=1)
        self.n_params = int(blob.size)
        env.batch.set_q_mlp(q_layers)

    def sync_targets(self):
        """Copy the env's present policy network and this critic into the target copies (ClothBatch.ddpg_sync_targets)."""
        self.env.batch.ddpg_sync_targets()

    def step(self, n_steps, batch_size, seed, gamma=0.99, act_bound=1.0, rows=None):
        """n_steps TD steps of the critic alone (ClothBatch.q_fit) on minibatches drawn as ValueTrainer.step draws them; rows None: the
        non-leaf rows of the dataset. No target moves. Returns float64[n_steps, 3]: loss, mean q, mean y before each update."""
        if rows is None:
            rows = np.nonzero(self.env.batch.fit_get_transitions()[1] != _lib.FIT_NEXT_NONE)[0]
            if rows.size < 1:
                raise ValueError("the dataset holds no row with a transition: collect first")
        rows = _check_rows(rows)
        table = rows.astype(np.int32)[MLPTrainer.index_table(rows.size, n_steps, batch_size, seed)]
        return self.env.batch.q_fit(table, gamma, act_bound, **self.hyper)

    def grad(self, idx, gamma=0.99, act_bound=1.0):
        """(stats float64[3], [(dW, db), ...], y float32[B], q float32[B]) over the dataset rows idx at the present weights and targets,
        from the device; nothing is updated."""
        stats, g, y, q = self.env.batch.q_grad(idx, gamma, act_bound)
        return stats, unpack_mlp(self.widths, g), y, q

    def layers(self):
        """The critic as the device holds it now: [(W, b), ...] float32, by download (clothhip_get_q_mlp)."""
        return unpack_mlp(self.widths, self.env.batch.get_q_mlp())

    def reset(self):
        """Zero the critic's moments and step count; its weights, the targets, the policy's optimizer and the dataset stay."""
        self.env.batch.q_fit_reset()


def ensemble_disagreement(actions):
    """float64[n] from actions [G, n, 4]: the mean over the four action components of the population variance over the G members
    (numpy float64, var with ddof = 0) -- the novelty signal of a bootstrapped ensemble."""
    a = np.asarray(actions, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1:
        raise ValueError("actions must have shape (G, n, 4) (got %r)" % (a.shape,))
    return a.var(axis=0).mean(axis=1)


class MLPEnsemble(_EnvDataset):
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
        self.hyper = _hyper(optimizer)
        self.env = env
        self.nets = [[(np.array(W, dtype=np.float32), np.array(b, dtype=np.float32)) for W, b in layers] for layers in members_layers]
        self.widths, blob = pack_population(self.nets, n_in=3 * env.P)
        self.G, self.n_params = int(blob.shape[0]), int(blob.shape[1])
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

    def device_noise(self, seed, sigma):
        """policies.DeviceNoise for a collection of the ensemble: sigma [G] (or a scalar), one standard deviation per member -- env e
        explores with sigma[member[e]] in all four components, the noise made on the device."""
        from .policies import DeviceNoise
        sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (self.G,))
        return DeviceNoise(seed, sigma=np.repeat(sg[self.member][:, None], 4, axis=1))

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

    def predict(self, idx, members=None):
        """float32[n_m, n, 4]: the trainer's forward of the rows `members` (None: all G) on the dataset rows idx [n], the same rows for
        every member -- each member's y of grad and step, bit for bit; nothing is updated."""
        m = self._members(members)
        self._on_env()
        return self.env.batch.fit_predict(idx, m)

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

    # ---- PPO for the population (ClothBatch.fit_*_members) -------------------------------------------------------------
    def snapshot_old(self, member_of_row, first=0):
        """Store as the OLD MEANS of the dataset rows [first, first + len(member_of_row)) the present output of the member that ACTED
        there, on the device (ClothBatch.fit_snapshot_policy_members): member_of_row int[n] holds a member per row -- for a
        collection ensemble.member[env of the row] -- and -1 for a row to skip (a leaf). What ppo_step's probability ratios are taken
        against: call it after a collection and before the first policy step on it."""
        self._on_env()
        self.env.batch.fit_snapshot_policy_members(member_of_row, first)

    @staticmethod
    def ppo_epoch_tables(rows_by_member, n_epochs, batch_size, seed):
        """The minibatches of ppo_step: int32[n_epochs, steps, G', B] from ONE RandomState(seed). rows_by_member is a list of G' 1-d
        integer arrays, member j's dataset rows. Per epoch, per member in ascending order, one permutation of that member's rows is
        drawn and cut into steps = min_j(len(rows_j)) // B minibatches of B = batch_size in order; the rest of the permutation is
        dropped for that epoch. ValueError for a member with fewer than B rows. A function of the arguments alone."""
        lists = [_check_rows(rows) for rows in rows_by_member]
        B = int(batch_size)
        if not lists or int(n_epochs) < 0 or B < 1:
            raise ValueError("ppo_epoch_tables needs at least one member, n_epochs >= 0, batch_size >= 1")
        for j, rows in enumerate(lists):
            if rows.size < B:
                raise ValueError("member %d of the call has %d rows, fewer than a minibatch of %d" % (j, rows.size, B))
        steps = min(rows.size for rows in lists) // B
        r = np.random.RandomState(seed)
        out = np.zeros((int(n_epochs), steps, len(lists), B), dtype=np.int32)
        for e in range(int(n_epochs)):
            for j, rows in enumerate(lists):
                out[e, :, j, :] = rows[r.permutation(rows.size)][:steps * B].reshape(steps, B)
        return out

    def _per_member(self, v, what):
        """v, a scalar or G values, as float64[G]."""
        v = np.asarray(v, dtype=np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.size != self.G):
            raise ValueError("%s must be a scalar or %d values, one per member" % (what, self.G))
        return np.broadcast_to(v, (self.G,))

    def ppo_step(self, n_epochs, batch_size, seed, sigma, clip=0.2, target_kl=None, rows_by_member=None, members=None):
        """PPO of the rows `members` (None: all G) on the device, all members in the launches of one (ClothBatch.fit_ppo_members): up
        to n_epochs epochs, each ONE fit_ppo_members call over the members still live, on the minibatches
        ppo_epoch_tables(rows_by_member, n_epochs, batch_size, seed) -- rows_by_member[j] the dataset rows of members[j] (None: every
        member takes all rows of the dataset). sigma and clip are a scalar or G values (member g's is the g-th), the optimizer's
        hyper-parameters the ensemble's. With target_kl a member whose mean kl over an epoch exceeds it is RETIRED: later calls name
        the rest, its row stays as that epoch left it. Returns (stats float64[n_epochs * steps, G', 3]: loss, clip_fraction, kl of
        every member before each step's update, NaN where the member did not run; epochs int[G']: the epochs each member ran)."""
        m = self._members(members)
        sig, clp = self._per_member(sigma, "sigma")[m], self._per_member(clip, "clip")[m]
        if rows_by_member is None:
            n = self.size()
            if n < 1:
                raise ValueError("the dataset is empty: append first")
            rows_by_member = [np.arange(n)] * m.size
        if len(rows_by_member) != m.size:
            raise ValueError("rows_by_member must hold %d lists of rows, one per member of the call" % m.size)
        self._on_env()
        tables = self.ppo_epoch_tables(rows_by_member, n_epochs, batch_size, seed)
        steps = tables.shape[1]
        stats = np.full((int(n_epochs) * steps, m.size, 3), np.nan)
        epochs, live = np.zeros(m.size, dtype=np.int64), np.ones(m.size, dtype=bool)
        for e in range(int(n_epochs)):
            if not live.any() or steps == 0:
                break
            hyper = {k: (v if k == 'optimizer' else v[m[live]]) for k, v in self.hyper.items()}
            got = self.env.batch.fit_ppo_members(m[live], np.ascontiguousarray(tables[e][:, live]), sig[live], clp[live], hyper)
            stats[e * steps:(e + 1) * steps, live] = got
            epochs[live] += 1
            if target_kl is not None:
                over = np.zeros(m.size, dtype=bool)
                over[live] = np.mean(got[:, :, 2], axis=0) > float(target_kl)
                live &= ~over
        return stats, epochs

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
