"""Demonstration writer: the data-collection loop of the reference's examples/analytic.py:825-910 (`run(args, policy)`:
reset, act until done, append obs / act / rew / done / info per step, pickle the list of episodes) over a ClothVecEnv.

With the oracle-corner policy the whole loop -- policy, steps, episode resets -- runs on the device
(ClothVecEnv.step_many(policy='oracle_corner')): the host only cuts the per-slot records into episodes. Any other
policy object (gym_cloth_amd/policies.py -- LookaheadPolicy included --, or anything with get_action(obs, t)) is driven through
ClothVecEnv.step.

An episode has the reference's layout (analytic.py:866-882):
    {'obs': [obs_0 (what reset() returned), obs_1, ...], 'act': [...], 'rew': [...], 'done': [...], 'info': [dict, ...]}
with the '1d' observation (cloth_env.py:196-200) as float32[3P] on the device path (float64 on the host path), or, with
obs='rgb' / 'depth' / 'rgbd', the image observation the reference's shipped configurations record (uint8 [H, W, C], rendered on
the device for every slot of a launch: ClothVecEnv.step_many(images=...)).
"""
import copy
import pickle

import numpy as np

_INFO_KEYS = ('num_steps', 'num_sim_steps', 'actual_coverage', 'start_coverage', 'variance_inv', 'start_variance_inv',
              'have_tear', 'out_of_bounds')


def _new_episode(obs0, env_index):
    return {'obs': [obs0], 'act': [], 'rew': [], 'done': [], 'info': [], 'env': int(env_index)}


def _info_at(src, t, e):
    out = {}
    for k in _INFO_KEYS:
        v = src[k][t, e] if t is not None else src[k][e]
        out[k] = v.item() if hasattr(v, 'item') else v
    return out


def _state_images(env, fmt, image_kw):
    """The image observation of every env's present state, finished on the device (what reset() / step() just returned as '1d')."""
    swap = ~env.init_side if env._init_type == 'tier2' else None
    return env.batch.render_obs('state', swap_sides=swap, fmt=fmt, **dict(image_kw or {}))


def collect_demos(env, policy='oracle_corner', max_episodes=10, slots_per_launch=12, path=None, time_budget_ms=0.0,
                  on_device=False, obs='1d', image_kw=None):
    """Run `policy` until `max_episodes` episodes have finished (over all envs of `env`, in order of completion) and return
    them as a list of episode dicts; with `path` the list is also pickled there (analytic.py:900-901).
    `env` must have been seeded; it is reset here. A policies.HighestPointPolicy with on_device=True is evaluated in the
    kernel as well: its per-env pick streams are drawn here and handed to the launch slot by slot. So is a policies.MLPPolicy
    with on_device=True (the network runs inside the launch, ClothVecEnv.step_many(policy='mlp')): its per-env noise streams are
    drawn here, one [4] per slot, and what a time-sliced launch leaves unused goes to the next one. A policies.MLPPopulation goes the
    same way, every env under its own network (it adds no noise).
    obs: '1d', or 'rgb' / 'depth' / 'rgbd' for image observations in the episodes' 'obs' lists (image_kw: render parameters);
    everything else in an episode is the same either way."""
    if obs not in ('1d', 'rgb', 'depth', 'rgbd'):
        raise ValueError("obs must be '1d', 'rgb', 'depth' or 'rgbd' (got %r)" % (obs,))
    fmt = None if obs == '1d' else obs
    episodes = []
    E = env.E
    obs = env.reset()
    from .policies import HighestPointPolicy, MLPPolicy, MLPPopulation
    from .trainers import MLPEnsemble
    hp = policy if (on_device and isinstance(policy, HighestPointPolicy)) else None
    mlp = policy if (on_device and isinstance(policy, (MLPPolicy, MLPPopulation, MLPEnsemble))) else None
    if mlp is not None and not (isinstance(mlp, MLPEnsemble) and env._policy_mlp is mlp):      # (an ensemble on the env holds FITTED rows: an upload would undo the fit)
        env.set_policy(mlp)
    if isinstance(policy, str) or hp is not None or mlp is not None:
        if hp is None and mlp is None and policy != 'oracle_corner':
            raise ValueError(policy)
        first = obs.astype(np.float32) if fmt is None else _state_images(env, fmt, image_kw)
        cur = [_new_episode(first[e], e) for e in range(E)]
        picks = [[] for _ in range(E)]                                # highest point / MLP noise: drawn but not consumed yet
        while len(episodes) < max_episodes:
            if hp is not None:
                for e in range(E):
                    while len(picks[e]) < slots_per_launch:
                        picks[e].append(hp.draw(e))
                tbl = np.array([[picks[e][t] for e in range(E)] for t in range(slots_per_launch)], dtype=np.int32)
                out = env.step_many(policy='highest_point', n_actions=slots_per_launch, policy_choices=tbl, auto_reset=True,
                                    want_obs=True, time_budget_ms=time_budget_ms, images=fmt, image_kw=image_kw)
                for e in range(E):
                    del picks[e][:int(out['ran'][:, e].sum())]
            elif mlp is not None:
                tbl = None
                if mlp.noise_std > 0.0:
                    for e in range(E):
                        while len(picks[e]) < slots_per_launch:
                            picks[e].append(mlp.draw(e))
                    tbl = np.array([[picks[e][t] for e in range(E)] for t in range(slots_per_launch)], dtype=np.float64)
                out = env.step_many(policy='mlp', n_actions=slots_per_launch, policy_noise=tbl, auto_reset=True,
                                    want_obs=True, time_budget_ms=time_budget_ms, images=fmt, image_kw=image_kw)
                for e in range(E):
                    del picks[e][:int(out['ran'][:, e].sum())]
            else:
                out = env.step_many(policy='oracle_corner', n_actions=slots_per_launch, auto_reset=True, want_obs=True,
                                    time_budget_ms=time_budget_ms, images=fmt, image_kw=image_kw)
            obs_t, reset_obs = (out['obs_t'], out['reset_obs']) if fmt is None else (out['img_t'], out['reset_img'])
            for t in range(slots_per_launch):
                for e in np.nonzero(out['ran'][t])[0]:
                    k = int(out['reset_before'][t, e])
                    if k:                                             # a new episode started right before this action
                        cur[e] = _new_episode(reset_obs[e, k - 1].copy(), e)
                    ep = cur[e]
                    ep['obs'].append(obs_t[t, e].copy())
                    ep['act'].append(tuple(out['actions'][t, e]))
                    ep['rew'].append(float(out['rew'][t, e]))
                    ep['done'].append(bool(out['done'][t, e]))
                    ep['info'].append(_info_at(out, t, e))
                    if ep['done'][-1]:
                        episodes.append(ep)
            # a time slice can end right after a completed reset: no action of this launch carries its reset_before mark, the
            # next launch's first action belongs to the NEW episode (analytic.py:866-882: every episode opens with reset()'s obs)
            for e in np.nonzero(out.get('tail_reset_index', np.zeros(E, dtype=np.int64)))[0]:
                cur[e] = _new_episode(reset_obs[e, int(out['tail_reset_index'][e]) - 1].copy(), e)
    else:
        seen = obs if fmt is None else _state_images(env, fmt, image_kw)      # what the episodes record; the policy reads '1d'
        cur = [_new_episode(seen[e].copy(), e) for e in range(E)]
        steps = np.zeros(E, dtype=np.int64)
        while len(episodes) < max_episodes:
            act = np.asarray(policy.get_action(obs, t=int(steps.max())), dtype=np.float64)
            side = env.init_side.copy()
            obs, rew, done, info = env.step(act, auto_reset=True)
            last = info.get('terminal_observation', obs)
            if fmt is not None:                                       # the present states, and the finished episodes' last ones
                seen = _state_images(env, fmt, image_kw)
                last = seen
                if 'terminal_observation' in info:
                    m = np.nonzero(info['reset_mask'])[0]
                    last = seen.copy()
                    last[m] = env.render_observations(info['terminal_observation'][m], fmt=fmt,
                                                      swap_sides=~side[m] if env._init_type == 'tier2' else None, **dict(image_kw or {}))
            else:
                seen = obs
            for e in range(E):
                ep = cur[e]
                ep['obs'].append(last[e].copy())
                ep['act'].append(tuple(act[e]))
                ep['rew'].append(float(rew[e]))
                ep['done'].append(bool(done[e]))
                ep['info'].append(_info_at(info, None, e))
                steps[e] += 1
                if done[e]:
                    episodes.append(ep)
                    cur[e] = _new_episode(seen[e].copy(), e)
                    steps[e] = 0
    episodes = episodes[:max_episodes]
    if path is not None:
        with open(path, 'wb') as fh:
            pickle.dump(episodes, fh)
    return episodes


def dagger_mixture(n_actions, n_envs, beta, seed):
    """DAgger's beta-mixture as a table: bool[T, E], True where the expert takes the action -- Bernoulli(beta) per (t, e) from
    numpy.random.default_rng(seed). beta = 0: all False; beta = 1: all True."""
    if not 0.0 <= float(beta) <= 1.0:
        raise ValueError("beta must lie in [0, 1] (got %r)" % (beta,))
    return np.random.default_rng(seed).random((int(n_actions), int(n_envs))) < float(beta)


def dagger_rollout(env, expert='oracle_corner', n_actions=12, beta=0.5, seed=0, policy_noise=None, expert_choices=None):
    """One DAgger data-collection pass in ONE episode launch: the env's network (set_policy: an MLPPolicy's, or an MLPPopulation, every
    env under its own) drives the cloths for n_actions slots, the expert labels every state they reach, and takes the action over
    where dagger_mixture(n_actions, E, beta, seed) says so (ClothVecEnv.step_many(policy='mlp', expert=..., expert_mix=...)); episodes
    that end are reset inside the launch. Returns dict(obs float32[T, E, 3P]: what each slot's policy saw (envs.slot_start_obs),
    labels float64[T, E, 4]: the expert's action there (NaN where ran is False), took bool[T, E]: the expert acted, ran bool[T, E],
    out: step_many's dict). Nothing is trained here: dagger_fit below aggregates (obs[ran], labels[ran]) and refits on the device."""
    from .envs import slot_start_obs
    mix = dagger_mixture(n_actions, env.E, beta, seed)
    obs_before = np.asarray(env.state, dtype=np.float32).reshape(env.E, -1)
    out = env.step_many(policy='mlp', n_actions=int(n_actions), want_obs=True, policy_noise=policy_noise, expert=expert,
                        expert_mix=mix, expert_choices=expert_choices)
    return {'obs': slot_start_obs(out, obs_before), 'labels': out['expert_actions'], 'took': out['expert_took'], 'ran': out['ran'],
            'out': out}


def dagger_fit(env, trainer, roll, n_steps=100, batch_size=64, seed=0):
    """The refit half of a DAgger iteration, on the device: append the rows of `roll` (dagger_rollout's dict) that ran --
    roll['obs'][ran], roll['labels'][ran] -- to `trainer`'s dataset (policies.MLPTrainer on `env`; D <- D u D_i), then take n_steps
    optimizer steps on minibatches of batch_size rows of everything gathered so far (MLPTrainer.step(n_steps, batch_size, seed)). The
    env's network is updated in place: the next dagger_rollout runs the fitted weights. Returns dict(losses float64[n_steps]: each
    step's loss before its update, rows: the dataset's size, appended: the rows this call added)."""
    if trainer.env is not env:
        raise ValueError("the trainer belongs to another env")
    ran = np.asarray(roll['ran'], dtype=bool)
    rows = trainer.append(roll['obs'][ran], roll['labels'][ran]) if ran.any() else trainer.size()
    return {'losses': trainer.step(n_steps, batch_size, seed), 'rows': rows, 'appended': int(ran.sum())}


def dagger_collect(env, trainer, expert='oracle_corner', n_actions=12, beta=0.5, seed=0, slots_per_launch=12, time_budget_ms=0.0,
                   policy_noise=None, expert_choices=None, max_launches=None):
    """dagger_rollout and dagger_fit's append without the observation tables ever leaving the device, and therefore also in TIME SLICES:
    armed launches of slots_per_launch slots (step_many(policy='mlp', want_obs='device', time_budget_ms=...)) until every env has run
    n_actions slots. Slot i of env e -- counted over the launches -- takes row i of dagger_mixture(n_actions, E, beta, seed), of
    policy_noise [n_actions, E, 4] and of expert_choices [n_actions, E]; what a launch leaves unused goes to the next one. Per launch:
    the rows that ran are appended to `trainer`'s dataset by index (envs.slot_start_sources -> MLPTrainer.append_launch), then every
    env's held row moves on (envs.hold_sources -> ClothBatch.fit_hold); before the first launch the held rows are the present states.
    The env must hold no operation parked by an earlier time-sliced launch (ValueError): the held rows start as the present states, and
    a cloth in the middle of an action does not show the state that action was planned on. max_launches bounds the loop (RuntimeError
    when the envs have not all run n_actions slots by then; None: no bound).
    An env that has its n_actions keeps acting on its last table rows while the others catch up; those slots are not appended.
    Returns dict(appended: rows added, rows: the dataset's size, launches, row_env / row_slot int[appended]: the env and the per-env
    slot number of every appended row in dataset order, count int[E]: slots each env ran (>= n_actions), took: seconds in the launches,
    appends and holds, kernel_ms: of that the launches' kernels, substeps: Cloth.update() calls of the launches' actions and resets,
    op_ticks: per launch step_many's uint64[E, 4] time accounting, records: per launch the [T, E] arrays 'ran',
    'done', 'rew', 'actual_coverage', 'expert_took' and 'slot' (the per-env slot number) for coverage curves, with 'n_resets' int[E] and
    'parked' bool[E]: the env holds an operation the slice cut). Nothing is trained here."""
    mix = dagger_mixture(int(n_actions), env.E, beta, seed)
    choices = None if expert_choices is None else np.asarray(expert_choices)
    if choices is not None and choices.shape != (int(n_actions), env.E):
        raise ValueError("expert_choices must have shape (%d, %d)" % (int(n_actions), env.E))

    def launch_kw(idx, ee):
        return dict(expert=expert, expert_mix=mix[idx, ee], expert_choices=None if choices is None else choices[idx, ee])

    return _collect_loop(env, trainer, n_actions, slots_per_launch, time_budget_ms, policy_noise, max_launches, launch_kw,
                         lambda rows, slot, out: trainer.append_launch(rows), ('expert_took',))


def _collect_loop(env, trainer, n_actions, slots_per_launch, time_budget_ms, policy_noise, max_launches, launch_kw, append, record_keys):
    """The loop dagger_collect and reward_collect share: policy='mlp' launches of slots_per_launch slots that keep their observation
    tables on the device until every env has run n_actions slots; per launch the rows that ran (and lie within the n_actions) go to
    append(rows int32[n, 3] in [t][e] order, slot int[n]: their per-env slot numbers, out: the launch's step_many dict), then the held
    rows move on. launch_kw(idx, ee):
    further step_many keywords for the table rows idx [T, E]; record_keys: further [T, E] arrays of step_many's dict to keep per launch.
    policy_noise: float64 [n_actions, E, 4], or a policies.DeviceNoise -- then every launch's table is filled on the device with
    slot_base = the slots each env has run, so the noise of env e's slot i is the same whatever slots_per_launch and time_budget_ms cut the
    collection into (a slot past n_actions, which is not appended, gets the noise of its own number, not the last row again)."""
    import time
    from .envs import hold_sources, slot_start_sources
    if trainer.env is not env:
        raise ValueError("the trainer belongs to another env")
    E, N, T = env.E, int(n_actions), int(slots_per_launch)
    if N < 1 or T < 1:
        raise ValueError("n_actions and slots_per_launch must be >= 1")
    if env.batch.in_flight().any():
        raise ValueError("an earlier time-sliced launch left operations parked on this env: complete or drop them before collecting")
    device_noise = None
    if hasattr(policy_noise, 'fill') and hasattr(policy_noise, 'advance'):      # policies.DeviceNoise: this collection's slots 0 .. of every env, numbered on
        device_noise, policy_noise = copy.copy(policy_noise), None               # a copy of it -- the caller's running slot_base is left alone
    noise = None if policy_noise is None else np.asarray(policy_noise, dtype=np.float64)
    if noise is not None and noise.shape != (N, E, 4):
        raise ValueError("policy_noise must have shape (%d, %d, 4)" % (N, E))
    used = np.zeros(E, dtype=np.int64)
    ee = np.arange(E)[None, :]
    res = {'appended': 0, 'launches': 0, 'row_env': [], 'row_slot': [], 'took': 0.0, 'substeps': 0, 'kernel_ms': 0.0, 'op_ticks': [], 'records': []}
    before = env.total_substeps
    t0 = time.perf_counter()
    env.batch.fit_hold()
    while (used < N).any():
        if max_launches is not None and res['launches'] >= int(max_launches):
            raise RuntimeError("%d launches and the envs have run %r of %d slots" % (res['launches'], used.tolist(), N))
        slot = used[None, :] + np.arange(T)[:, None]                        # [T, E]: the per-env slot number of every slot of this launch
        idx = np.minimum(slot, N - 1)                                       # past the end: the last row again (not appended)
        if device_noise is not None:
            device_noise.slot_base = used.copy()                                # row t of env e is ITS slot used[e] + t, whatever the launches before ran
        out = env.step_many(policy='mlp', n_actions=T, want_obs='device', time_budget_ms=time_budget_ms,
                            policy_noise=device_noise if noise is None else noise[idx, ee], **launch_kw(idx, ee))
        res['kernel_ms'] += float(env.batch.last_kernel_ms)
        res['op_ticks'].append(out['op_ticks'])
        ran = out['ran']
        keep = ran & (slot < N)
        t_, e_ = np.nonzero(keep)                                           # [t][e] order
        if len(t_):
            rows = np.concatenate([slot_start_sources(out)[t_, e_], (t_ * E + e_)[:, None].astype(np.int32)], axis=1)
            append(rows, slot[t_, e_], out)
            res['row_env'].append(e_); res['row_slot'].append(slot[t_, e_])
            res['appended'] += len(t_)
        env.batch.fit_hold(hold_sources(out))
        used += ran.sum(axis=0)
        res['launches'] += 1
        parked = env.batch.in_flight()                                      # operations the slice cut: the next launch continues them
        rec = {'ran': ran, 'done': out['done'], 'rew': out['rew'], 'actual_coverage': out['actual_coverage'], 'slot': slot,
               'n_resets': out['n_resets'], 'parked': parked}
        rec.update({k: out[k] for k in record_keys})
        res['records'].append(rec)
        if not ran.any() and not parked.any() and not (out['n_resets'] > 0).any():
            raise RuntimeError("a launch made no progress (time_budget_ms = %r too short for one substep?)" % (time_budget_ms,))
    res['took'] = time.perf_counter() - t0
    res['substeps'] = int(env.total_substeps - before)
    res['row_env'] = np.concatenate(res['row_env']) if res['row_env'] else np.zeros(0, dtype=np.int64)
    res['row_slot'] = np.concatenate(res['row_slot']) if res['row_slot'] else np.zeros(0, dtype=np.int64)
    res['count'] = used
    res['rows'] = trainer.size()
    return res


# ---- fitting from reward: returns, per-row weights, the collection that labels rows with the executed action ---------------------------
def returns_to_go(rew, ran, done, reset_before, gamma=1.0, carry=None):
    """(G float64[T, E], complete bool[T, E]) of one launch's record tables [T, E] (step_many's 'rew', 'ran', 'done', 'reset_before'):
    G[t, e] = rew[t, e] + gamma G[t + 1, e] while slot t + 1 of env e continues slot t's episode -- slot t + 1 ran, has
    reset_before == 0, and done[t, e] is False --, else G[t, e] = rew[t, e]; G is 0 where the slot did not run. complete[t, e]: the
    slot's episode reached `done` inside the table(s). carry = (G_next float[E], complete_next bool[E], continues bool[E]) chains the
    table that FOLLOWS this one (returns_carry of it): the last slot of env e that ran, if nothing ran after it in this table and its
    done is False, continues into that table where continues[e] says its first executed slot has reset_before == 0. Without a carry
    such a slot ends an open episode (complete False, G the rewards so far). Plain float64 numpy, one multiplication and one addition
    per slot."""
    rew = np.asarray(rew, dtype=np.float64)
    ran = np.asarray(ran, dtype=bool)
    done = np.asarray(done, dtype=bool)
    rb = np.asarray(reset_before).astype(np.int64)
    if not (rew.ndim == 2 and rew.shape == ran.shape == done.shape == rb.shape):
        raise ValueError("rew, ran, done and reset_before must be [T, E] tables of one shape")
    T, E = rew.shape
    gamma = float(gamma)
    if carry is None:
        nG, nC, nK = np.zeros(E), np.zeros(E, dtype=bool), np.zeros(E, dtype=bool)
    else:
        nG, nC, nK = (np.array(carry[0], dtype=np.float64).reshape(E), np.array(carry[1], dtype=bool).reshape(E),
                      np.array(carry[2], dtype=bool).reshape(E))
    G, complete = np.zeros((T, E)), np.zeros((T, E), dtype=bool)
    tail = np.ones(E, dtype=bool)                                           # nothing has run after slot t in this table
    for t in range(T - 1, -1, -1):
        if t + 1 < T:
            cont = np.where(tail, nK, ran[t + 1] & (rb[t + 1] == 0)) & ~done[t]
        else:
            cont = nK & ~done[t]
        G[t] = np.where(ran[t], rew[t] + np.where(cont, gamma * nG, 0.0), 0.0)
        complete[t] = ran[t] & (done[t] | (cont & nC))
        nG, nC = np.where(ran[t], G[t], nG), np.where(ran[t], complete[t], nC)
        tail &= ~ran[t]
    return G, complete


def returns_carry(G, complete, ran, reset_before, carry=None):
    """What a table gives the table BEFORE it as returns_to_go's carry: per env (G, complete) of its first slot that ran and whether
    that slot continues an episode (reset_before == 0); an env with no slot that ran passes on the carry it was given itself."""
    ran = np.asarray(ran, dtype=bool)
    T, E = ran.shape
    first = np.argmax(ran, axis=0)
    e_ = np.arange(E)
    some = ran.any(axis=0)
    if carry is None:
        carry = (np.zeros(E), np.zeros(E, dtype=bool), np.zeros(E, dtype=bool))
    return (np.where(some, np.asarray(G, dtype=np.float64)[first, e_], carry[0]), np.where(some, np.asarray(complete, dtype=bool)[first, e_], carry[1]),
            np.where(some, np.asarray(reset_before)[first, e_] == 0, carry[2]))


def reward_weights(G, scheme='filter', **kw):
    """float32[n] loss weights from the returns G [n] of completed-episode rows. scheme 'advantage': (G - mean) / (std + 1e-8);
    'exp' (temperature=1.0, w_max=20.0): min(exp((G - mean) / temperature), w_max); 'filter' (q=0.25): 1 where G >= the (1 - q)
    quantile of G (numpy.quantile's linear interpolation; ties at the quantile included), else 0; a callable: scheme(G, **kw). Float64
    arithmetic, rounded once. The trainer divides by the batch size, not by the weights' sum: a scheme that should average to 1 must
    be scaled by the caller."""
    G = np.asarray(G, dtype=np.float64).reshape(-1)
    if callable(scheme):
        w = np.asarray(scheme(G, **kw), dtype=np.float64)
        if w.shape != G.shape:
            raise ValueError("the weighting callable must return one weight per return")
    elif G.size == 0:
        w = np.zeros(0)
    elif scheme == 'advantage':
        _no_kw(scheme, kw, ())
        w = (G - G.mean()) / (G.std() + 1e-8)
    elif scheme == 'exp':
        _no_kw(scheme, kw, ('temperature', 'w_max'))
        temperature, w_max = float(kw.get('temperature', 1.0)), float(kw.get('w_max', 20.0))
        if not temperature > 0.0:
            raise ValueError("temperature must be > 0")
        w = np.minimum(np.exp(np.minimum((G - G.mean()) / temperature, 700.0)), w_max)
    elif scheme == 'filter':
        _no_kw(scheme, kw, ('q',))
        q = float(kw.get('q', 0.25))
        if not 0.0 < q <= 1.0:
            raise ValueError("q must lie in (0, 1]")
        w = (G >= np.quantile(G, 1.0 - q)).astype(np.float64)
    else:
        raise ValueError("scheme must be 'advantage', 'exp', 'filter' or a callable (got %r)" % (scheme,))
    w = w.astype(np.float32)
    if not np.isfinite(w).all():
        raise ValueError("the scheme gave a weight that is not a finite float32")
    return w


def _no_kw(scheme, kw, allowed):
    unknown = sorted(set(kw) - set(allowed))
    if unknown:
        raise ValueError("scheme %r takes no %r" % (scheme, unknown))


def _collection_returns(res, n_actions, gamma, n_envs):
    """(G float64[n], complete bool[n], done bool[n], starts bool[n]) of the slots a _collect_loop run collected (res: its dict, with
    'reset_before' in the records), in the order they were appended: the return-to-go of every slot, whether its episode completed
    inside the collection, whether the slot ended it, whether the slot is the first collected one of its episode."""
    N, carry, per_launch = int(n_actions), None, []
    for rec in reversed(res['records']):                                    # the later launch first: a return looks ahead
        ran = rec['ran'] & (rec['slot'] < N)
        G, complete = returns_to_go(rec['rew'], ran, rec['done'], rec['reset_before'], gamma, carry)
        carry = returns_carry(G, complete, ran, rec['reset_before'], carry)
        t_, e_ = np.nonzero(ran)                                            # the order the rows were appended in
        per_launch.append((G[t_, e_], complete[t_, e_], rec['done'][t_, e_]))
    per_launch.reverse()
    cat = lambda k, dt: np.concatenate([p[k] for p in per_launch]).astype(dt) if per_launch else np.zeros(0, dtype=dt)
    G, complete, done = cat(0, np.float64), cat(1, bool), cat(2, bool)
    # an episode starts at an env's first collected slot and after every slot that ended one (a reset a time slice completed without a
    # record of its own shows in no reset_before)
    ended = np.zeros((N + 1, int(n_envs)), dtype=bool)
    ended[0] = True
    ended[res['row_slot'] + 1, res['row_env']] = done
    return G, complete, done, ended[res['row_slot'], res['row_env']]


def reward_collect(env, trainer, n_actions=12, gamma=1.0, scheme='filter', policy_noise=None, slots_per_launch=12, time_budget_ms=0.0,
                   max_launches=None, **scheme_kw):
    """Collect rows to FIT FROM REWARD: dagger_collect's loop with no expert armed. The env's network (plus policy_noise [n_actions, E,
    4], the exploration) drives the cloths in launches of slots_per_launch slots until every env has run n_actions slots; per launch
    the rows that ran are appended where they lie (envs.slot_start_sources) with the action the slot EXECUTED as the label
    (append_launch(labels="action")) and weight 0, then the held rows move on. A row's return is known when its episode ends, possibly
    launches later: the host keeps the per-launch records, and when the loop ends the returns-to-go of the collection's slots
    (returns_to_go with `gamma`, the launches chained by returns_carry; slots an env ran beyond its n_actions are not part of the
    collection) give reward_weights(G[complete], scheme, **scheme_kw), written over the appended range in ONE set_weights call. Rows of
    episodes still open when the collection ends keep weight 0 and are counted in 'open_rows'. Returns dagger_collect's dict (without
    'expert_took' in the records, with 'reset_before') plus first: the dataset index of the first appended row, returns float64[appended]
    and complete bool[appended] in dataset order, weights float32[appended] as written, open_rows, episode_return float64[episodes]: the
    return from the first collected slot of every episode that completed, t_append / t_set_weights: seconds in those calls. Nothing is
    trained here: reward_fit below steps the trainer."""
    import time
    first = trainer.size()
    spent = {'append': 0.0}

    def append(rows, slot, out):
        t0 = time.perf_counter()
        trainer.append_launch(rows, labels="action", weights=np.zeros(len(rows), dtype=np.float32))
        spent['append'] += time.perf_counter() - t0

    res = _collect_loop(env, trainer, n_actions, slots_per_launch, time_budget_ms, policy_noise, max_launches, lambda idx, ee: {}, append,
                        ('reset_before',))
    G, complete, done, starts = _collection_returns(res, n_actions, gamma, env.E)
    w = np.zeros(len(G), dtype=np.float32)
    w[complete] = reward_weights(G[complete], scheme, **scheme_kw)
    t0 = time.perf_counter()
    if len(w):
        trainer.set_weights(w, first)
    res.update(first=first, returns=G, complete=complete, weights=w, open_rows=int((~complete).sum()), episode_return=G[starts & complete],
               t_append=spent['append'], t_set_weights=time.perf_counter() - t0)
    return res


def reward_fit(env, trainer, col, n_steps=100, batch_size=64, seed=0):
    """The refit after reward_collect, on the device: n_steps optimizer steps on minibatches of batch_size rows of everything in the
    dataset (MLPTrainer.step(n_steps, batch_size, seed)), under the weights `col` (reward_collect's dict) wrote. The env's network is
    updated in place: the next reward_collect rolls out the fitted weights. Returns dict(losses float64[n_steps]: each step's weighted
    loss before its update, rows: the dataset's size, appended: the rows `col` added, weighted: those of them with a non-zero weight)."""
    if trainer.env is not env:
        raise ValueError("the trainer belongs to another env")
    return {'losses': trainer.step(n_steps, batch_size, seed), 'rows': trainer.size(), 'appended': int(col['appended']),
            'weighted': int(np.count_nonzero(col['weights']))}


# ---- actor-critic from reward: the episode structure of a collection, a critic's value targets, GAE weights ------------------
def episode_links(row_env, row_slot, done, n_envs, first):
    """int32[n]: the successor column (ClothBatch.fit_set_transitions' `next`) of a collection's rows in append order, the first of them
    dataset row `first`. row_env / row_slot int[n]: the env and the per-env slot number of every row, done bool[n]: the row's slot ended
    its episode. The rule reward_collect uses for episode starts, read forwards: a row whose slot ended its episode is
    _lib.FIT_NEXT_TERMINAL; otherwise its successor is the same env's NEXT collected row (rows are appended in time order, so it lies
    later; row_slot must ascend per env); the last row of an env, if it is not done, has none: _lib.FIT_NEXT_NONE, a leaf --
    actor_critic_collect appends the state behind an env's last open slot as exactly such a row."""
    from ._lib import FIT_NEXT_NONE, FIT_NEXT_TERMINAL
    env_ = np.asarray(row_env).astype(np.int64).reshape(-1)
    slot = np.asarray(row_slot).astype(np.int64).reshape(-1)
    done = np.asarray(done, dtype=bool).reshape(-1)
    n = len(env_)
    if not (len(slot) == len(done) == n):
        raise ValueError("row_env, row_slot and done must have one length")
    if n and (env_.min() < 0 or env_.max() >= int(n_envs)):
        raise ValueError("row_env must lie in [0, %d)" % int(n_envs))
    nxt = np.full(n, FIT_NEXT_NONE, dtype=np.int64)
    later = np.full(int(n_envs), -1, dtype=np.int64)                        # per env: the row met last, walking backwards
    for i in range(n - 1, -1, -1):
        e, k = env_[i], later[env_[i]]
        if k >= 0 and slot[k] <= slot[i]:
            raise ValueError("the rows of env %d are not in time order" % e)
        if done[i]:
            nxt[i] = FIT_NEXT_TERMINAL
        elif k >= 0:
            nxt[i] = int(first) + k
        later[e] = i
    return nxt.astype(np.int32)


def actor_critic_collect(env, trainer, n_actions=12, policy_noise=None, slots_per_launch=12, time_budget_ms=0.0, max_launches=None, expert=None, beta=0.0,
                         seed=0, expert_choices=None):
    """Collect rows for an ACTOR-CRITIC step: reward_collect's loop (labels = the action the slot executed, weight 0), which also
    writes the transitions. Per launch the rows that ran are appended where they lie; and where an env's LAST collected slot (its slot
    n_actions - 1) left its episode open, the state after that slot -- row t * E + e of that launch's observation table -- is appended
    behind them as a LEAF (labels="zero", weight 0): a row with no transition of its own whose value bootstraps the rows before it. No
    row is discarded. When the loop ends, ONE fit_set_transitions call writes every row's reward and successor (episode_links).
    Returns _collect_loop's dict plus first: the dataset index of the first appended row, ds_env / ds_slot int[n], leaf / done bool[n],
    rew float32[n], next int32[n]: the env, per-env slot number (a leaf: n_actions), kind, reward and successor of every appended row
    in DATASET order (n = appended + open_rows), open_rows: the leaves, nonleaf int[appended]: the dataset indices of the other rows,
    episode_return float64[episodes]: the undiscounted return from the first collected slot of every episode that completed,
    t_append / t_set_transitions: seconds in those calls. Nothing is trained here: actor_critic_fit below does.
    expert (a name as dagger_collect takes it; None: none): the launches are ARMED as dagger_collect arms them -- the expert labels
    every state the learner reaches and takes the action over where dagger_mixture(n_actions, E, beta, seed) says so (beta = 1: pure
    demonstrations; expert_choices [n_actions, E] as there) -- and the rows are appended with labels="action+expert": the executed action
    as the label, the expert's into the row's expert column (DDPG from demonstrations: ddpg_fit(bc_coef=...)). Leaves stay
    labels="zero" and carry no expert action."""
    import time
    from ._lib import FIT_SRC_SLOTS
    first, N, E = trainer.size(), int(n_actions), env.E
    row_labels, launch_kw, keys = "action", (lambda idx, ee: {}), ('reset_before',)
    if expert is not None:
        mix = dagger_mixture(N, E, beta, seed)
        choices = None if expert_choices is None else np.asarray(expert_choices)
        if choices is not None and choices.shape != (N, E):
            raise ValueError("expert_choices must have shape (%d, %d)" % (N, E))
        row_labels, keys = "action+expert", ('reset_before', 'expert_took')
        launch_kw = lambda idx, ee: dict(expert=expert, expert_mix=mix[idx, ee], expert_choices=None if choices is None else choices[idx, ee])
    spent = {'append': 0.0}
    cols = {'env': [], 'slot': [], 'leaf': [], 'done': [], 'rew': []}

    def append(rows, slot, out):
        t_, e_ = rows[:, 2] // E, rows[:, 2] % E
        done = np.asarray(out['done'], dtype=bool)[t_, e_]
        open_ = (slot == N - 1) & ~done
        t0 = time.perf_counter()
        trainer.append_launch(rows, labels=row_labels, weights=np.zeros(len(rows), dtype=np.float32))
        if open_.any():
            leaves = np.stack([np.full(int(open_.sum()), FIT_SRC_SLOTS), rows[open_, 2], np.zeros(int(open_.sum()), dtype=np.int64)], axis=1)
            trainer.append_launch(leaves, labels="zero", weights=np.zeros(len(leaves), dtype=np.float32))
        spent['append'] += time.perf_counter() - t0
        k = int(open_.sum())
        cols['env'] += [e_, e_[open_]]; cols['slot'] += [slot, np.full(k, N)]
        cols['leaf'] += [np.zeros(len(rows), dtype=bool), np.ones(k, dtype=bool)]
        cols['done'] += [done, np.zeros(k, dtype=bool)]
        cols['rew'] += [np.asarray(out['rew'], dtype=np.float64)[t_, e_], np.zeros(k)]

    res = _collect_loop(env, trainer, N, slots_per_launch, time_budget_ms, policy_noise, max_launches, launch_kw, append, keys)
    cat = lambda k, dt: np.concatenate(cols[k]).astype(dt) if cols[k] else np.zeros(0, dtype=dt)
    ds_env, ds_slot, leaf, done, rew = cat('env', np.int64), cat('slot', np.int64), cat('leaf', bool), cat('done', bool), cat('rew', np.float32)
    nxt = episode_links(ds_env, ds_slot, done, E, first)
    t0 = time.perf_counter()
    if len(nxt):
        env.batch.fit_set_transitions(rew, nxt, first)
    G, complete, _, starts = _collection_returns(res, N, 1.0, E)
    res.update(first=first, ds_env=ds_env, ds_slot=ds_slot, leaf=leaf, done=done, rew=rew, next=nxt, open_rows=int(leaf.sum()),
               nonleaf=first + np.nonzero(~leaf)[0], episode_return=G[starts & complete], t_append=spent['append'],
               t_set_transitions=time.perf_counter() - t0, rows=trainer.size())
    return res


def actor_critic_fit(env, trainer, critic, col, gamma=0.99, lam=0.95, n_value_steps=100, n_policy_steps=100, batch_size=64, seed=0,
                     normalize=True, w_scale=1.0):
    """The refit after actor_critic_collect, on the device: ONE fit_gae call over the rows `col` added writes their value targets
    (A + V under the present critic) and their loss weights (w_scale A^, A^ the advantage, normalised over the non-leaf rows with
    normalize; a leaf gets 0); then n_value_steps steps of `critic` (policies.ValueTrainer on `env`) on the NON-LEAF rows of the whole
    dataset, then n_policy_steps steps of `trainer` (policies.MLPTrainer) on everything under the written weights -- advantage-weighted
    regression onto the executed actions. Rows of earlier collections keep the targets and weights their own call wrote. Returns
    dict(adv, ret float32[n]: fit_gae's, value_losses, policy_losses float64: each step's loss before its update, rows)."""
    if trainer.env is not env or critic.env is not env:
        raise ValueError("the trainer or the critic belongs to another env")
    n = int(col['appended']) + int(col['open_rows'])
    adv, ret = env.batch.fit_gae(gamma, lam, first=col['first'], n=n, write_weights=True, normalize=normalize, w_scale=w_scale)
    rew, nxt = env.batch.fit_get_transitions()
    from ._lib import FIT_NEXT_NONE
    rows = np.nonzero(nxt != FIT_NEXT_NONE)[0]
    vl = critic.step(n_value_steps, batch_size, seed, rows=rows) if len(rows) else np.zeros(0)
    pl = trainer.step(n_policy_steps, batch_size, seed)
    return {'adv': adv, 'ret': ret, 'value_losses': vl, 'policy_losses': pl, 'rows': trainer.size()}


def demo_table(replay, labelled, n_steps, batch_size, seed, demo_fraction=None):
    """The minibatches of ddpg_fit, int32[n_steps, batch_size] dataset rows, a pure function of its arguments: replay int[m] the rows
    with a transition, labelled int[k] those of them that carry an expert action. demo_fraction None: replay[MLPTrainer.index_table(m,
    n_steps, batch_size, seed)], what ddpg_fit always drew. Else the first floor(demo_fraction * batch_size) positions of every
    minibatch are labelled[RandomState(seed + 1).randint(0, k, ...)] and the others are the corresponding positions of that table.
    ValueError for a fraction outside [0, 1], or when there are no labelled rows."""
    from .trainers import MLPTrainer
    replay, labelled = np.asarray(replay).reshape(-1), np.asarray(labelled).reshape(-1)
    table = replay.astype(np.int32)[MLPTrainer.index_table(replay.size, n_steps, batch_size, seed)]
    if demo_fraction is None:
        return table
    if not 0.0 <= float(demo_fraction) <= 1.0:
        raise ValueError("demo_fraction must lie in [0, 1] (got %r)" % (demo_fraction,))
    if labelled.size < 1:
        raise ValueError("demo_fraction is set and no row with a transition carries an expert action: collect with an expert first")
    k = int(np.floor(float(demo_fraction) * int(batch_size)))
    if k > 0:
        pick = np.random.RandomState(int(seed) + 1).randint(0, labelled.size, size=(int(n_steps), k))
        table = table.copy()
        table[:, :k] = labelled.astype(np.int32)[pick]
    return table


def ddpg_fit(env, trainer, qcritic, col, gamma=0.99, tau=0.005, n_steps=100, batch_size=64, seed=0, act_bound=1.0, q_coef=1.0, bc_coef=0.0, q_filter=True,
             demo_fraction=None):
    """The refit after actor_critic_collect under DDPG, on the device: n_steps steps of MLPTrainer.ddpg_step with
    `qcritic` (policies.QTrainer on `env`), each a TD step of the critic, a step of the policy up the critic's action gradient and the
    soft update of both targets. The minibatches are drawn from the non-leaf rows of the WHOLE dataset -- the replay buffer: rows of
    earlier collections keep paying --, a function of (the dataset, n_steps, batch_size, seed) alone. The targets are synced on the
    first use of this (trainer, qcritic) pair and whenever a new network dropped one. `col` is the collection that was just added (only
    its row count is reported). Returns dict(stats float64[n_steps, 6]: the critic's loss, mean q, mean y, then the actor's loss,
    gated fraction, mean |dL/da| of every step before its update; rows int32[n_steps, B]: the minibatches; replay: the non-leaf
    rows sampled from; synced: whether this call synced the targets).
    bc_coef != 0 or q_coef != 1: the actor's step is that of DDPG from demonstrations (MLPTrainer.ddpg_step) and stats
    is float64[n_steps, 9]: behind the critic's three the actor's -mean q, gated fraction, mean |dL/da|, bc_loss, labelled share and
    filter-pass share. demo_fraction: that share of every minibatch, rounded down, is drawn from the non-leaf rows that carry an
    expert action (demo_table; ValueError when there are none); the dict then also has labelled: those rows."""
    from ._lib import FIT_NEXT_NONE, ClothHipError
    from .batch_fit import has_expert
    if trainer.env is not env or qcritic.env is not env:
        raise ValueError("the trainer or the Q critic belongs to another env")
    replay = np.nonzero(env.batch.fit_get_transitions()[1] != FIT_NEXT_NONE)[0]
    if replay.size < 1:
        raise ValueError("the dataset holds no row with a transition: collect first")
    synced = False
    try:
        env.batch.ddpg_targets()
    except ClothHipError:
        qcritic.sync_targets()
        synced = True
    labelled = None
    if demo_fraction is not None:
        labelled = replay[has_expert(env.batch.fit_expert())[replay]]
    table = demo_table(replay, labelled if labelled is not None else replay[:0], n_steps, batch_size, seed, demo_fraction)
    stats = trainer.ddpg_step(qcritic, n_steps, batch_size, seed, gamma=gamma, tau=tau, act_bound=act_bound, q_coef=q_coef, bc_coef=bc_coef,
                              q_filter=q_filter, table=table)
    res = {'stats': stats, 'rows': table, 'replay': replay, 'synced': synced, 'collected': int(col['appended']) if col is not None else 0}
    if labelled is not None:
        res['labelled'] = labelled
    return res


def ppo_fit(env, trainer, critic, col, sigma=None, gamma=0.99, lam=0.95, clip=0.2, n_value_steps=100, n_epochs=10, batch_size=64, seed=0,
            target_kl=None, normalize=True, ent_coef=0.0):
    """The refit after actor_critic_collect with PPO's clipped surrogate in the place of actor_critic_fit's weighted regression, on the
    device: ONE fit_gae call over the rows `col` added writes their value targets and, as loss weights with w_scale = 1, their
    advantages (normalised over the non-leaf rows with normalize; a leaf gets 0); ONE trainer.snapshot_old over the same rows stores
    the present policy's means as their old means, BEFORE any policy step; then n_value_steps steps of `critic` on the non-leaf rows of
    the whole dataset; then trainer.ppo_step on the COLLECTION's non-leaf rows: up to n_epochs epochs of minibatches of batch_size,
    stopped by target_kl. Because a row's gradient is switched off once its ratio has left [1 - clip, 1 + clip] in the direction of its
    advantage, many epochs on one collection stay bounded where actor_critic_fit's steps diverge. sigma is the standard deviation of
    the policy_noise the collection ACTED with -- the caller's number: the launch draws the noise, the library does not record it, and
    a wrong sigma gives wrong ratios. Returns dict(adv, ret float32[n]: fit_gae's, value_losses float64, ppo_stats float64[steps, 3]:
    loss, clip_fraction, kl of every policy step before its update, epochs: the epochs run, rows).
    sigma=None: the trainer's LEARNED head (MLPTrainer.set_log_sigma; the collection acted with trainer.sigma()): the one snapshot
    stores the old means and the old log sigmas, the policy steps train network and head on the surrogate minus ent_coef times the
    entropy; ppo_stats is float64[steps, 4] (the entropy last) and the dict also holds log_sigma float32[steps, 4], the head before
    every step, and log_sigma_after float32[4].
    `trainer` an MLPEnsemble (a population): every member learns from the rows ITS OWN envs collected, all members in
    the launches of one. ONE fit_gae call (normalize=False, w_scale=1) under the shared critic; with normalize the advantages are
    normalised per member on the host over that member's non-leaf rows (member_normalize) and ONE set_weights call writes them; ONE
    trainer.snapshot_old call with member_of_row = ensemble.member[col['ds_env']], -1 for a leaf; the critic's steps; then
    trainer.ppo_step on each member's non-leaf rows of the collection. sigma and clip are a scalar or G values, the caller's numbers (a
    collection scales its unit noise by sigma[ensemble.member] per env); sigma=None and ent_coef belong to the shared network's head.
    ppo_stats is then float64[steps, G', 3] with NaN where a retired member did not run, epochs int[G'], and the dict also holds
    members int[G']: the members that have rows in the collection, and member_of_row int[n]."""
    if trainer.env is not env or critic.env is not env:
        raise ValueError("the trainer or the critic belongs to another env")
    if hasattr(trainer, 'member'):
        return _ppo_fit_members(env, trainer, critic, col, sigma, gamma, lam, clip, n_value_steps, n_epochs, batch_size, seed, target_kl, normalize, ent_coef)
    n = int(col['appended']) + int(col['open_rows'])
    adv, ret = env.batch.fit_gae(gamma, lam, first=col['first'], n=n, write_weights=True, normalize=normalize, w_scale=1.0)
    trainer.snapshot_old(col['first'], n)
    rew, nxt = env.batch.fit_get_transitions()
    from ._lib import FIT_NEXT_NONE
    rows = np.nonzero(nxt != FIT_NEXT_NONE)[0]
    vl = critic.step(n_value_steps, batch_size, seed, rows=rows) if len(rows) else np.zeros(0)
    mine = np.asarray(col['nonleaf'], dtype=np.int64)
    if len(mine):
        stats, epochs = trainer.ppo_step(n_epochs, batch_size, seed, sigma, clip=clip, target_kl=target_kl, rows=mine, ent_coef=ent_coef)
    else:
        stats, epochs = np.zeros((0, 3 if sigma is not None else 4)), 0
    out = {'adv': adv, 'ret': ret, 'value_losses': vl, 'ppo_stats': stats, 'epochs': epochs, 'rows': trainer.size()}
    if sigma is None:
        out['log_sigma'] = trainer.last_log_sigma if len(mine) else np.zeros((0, 4), dtype=np.float32)
        out['log_sigma_after'] = trainer.log_sigma()
    return out


def member_normalize(adv, member_of_row):
    """float32[n]: the advantages adv [n] normalised PER MEMBER, over the rows member_of_row [n] gives that member (-1: a leaf, which
    gets 0) -- references.gae_reference's formula on each member's rows, in float64 on the (double) of the float32 values:
    (A - mean) / (std + 1e-8), mean and population standard deviation over the member's rows; rounded once."""
    A = np.asarray(adv, dtype=np.float32).astype(np.float64).reshape(-1)
    mor = np.asarray(member_of_row).astype(np.int64).reshape(-1)
    if mor.shape != A.shape:
        raise ValueError("adv and member_of_row must have one length")
    hat = np.zeros(len(A))
    for g in np.unique(mor[mor >= 0]):
        mine = mor == g
        cnt = int(mine.sum())
        mean = A[mine].sum() / float(cnt)
        d = A[mine] - mean
        std = np.sqrt((d * d).sum() / float(cnt))
        hat[mine] = d / (std + 1e-8)
    return hat.astype(np.float32)


def _ppo_fit_members(env, ens, critic, col, sigma, gamma, lam, clip, n_value_steps, n_epochs, batch_size, seed, target_kl, normalize, ent_coef):
    """ppo_fit for an MLPEnsemble (its docstring has the steps)."""
    if sigma is None or float(ent_coef) != 0.0:
        raise ValueError("a population has no learned head: pass sigma (a scalar or one per member) and ent_coef=0")
    first, n = int(col['first']), int(col['appended']) + int(col['open_rows'])
    adv, ret = env.batch.fit_gae(gamma, lam, first=first, n=n, write_weights=True, normalize=False, w_scale=1.0)
    mor = np.where(np.asarray(col['leaf'], dtype=bool), -1, ens.member[np.asarray(col['ds_env'], dtype=np.int64)]).astype(np.int32)
    if normalize and n:
        ens.set_weights(member_normalize(adv, mor), first)
    ens.snapshot_old(mor, first)
    rew, nxt = env.batch.fit_get_transitions()
    from ._lib import FIT_NEXT_NONE
    rows = np.nonzero(nxt != FIT_NEXT_NONE)[0]
    vl = critic.step(n_value_steps, batch_size, seed, rows=rows) if len(rows) else np.zeros(0)
    members = np.unique(mor[mor >= 0]).astype(np.int32)
    if len(members):
        stats, epochs = ens.ppo_step(n_epochs, batch_size, seed, sigma, clip=clip, target_kl=target_kl,
                                     rows_by_member=[first + np.nonzero(mor == g)[0] for g in members], members=members)
    else:
        stats, epochs = np.zeros((0, 0, 3)), np.zeros(0, dtype=np.int64)
    return {'adv': adv, 'ret': ret, 'value_losses': vl, 'ppo_stats': stats, 'epochs': epochs, 'rows': ens.size(), 'members': members,
            'member_of_row': mor}
