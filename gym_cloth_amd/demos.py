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
    from .policies import HighestPointPolicy, MLPEnsemble, MLPPolicy, MLPPopulation
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
    import time
    from .envs import hold_sources, slot_start_sources
    if trainer.env is not env:
        raise ValueError("the trainer belongs to another env")
    E, N, T = env.E, int(n_actions), int(slots_per_launch)
    if N < 1 or T < 1:
        raise ValueError("n_actions and slots_per_launch must be >= 1")
    if env.batch.in_flight().any():
        raise ValueError("an earlier time-sliced launch left operations parked on this env: complete or drop them before collecting")
    mix = dagger_mixture(N, E, beta, seed)
    noise = None if policy_noise is None else np.asarray(policy_noise, dtype=np.float64)
    if noise is not None and noise.shape != (N, E, 4):
        raise ValueError("policy_noise must have shape (%d, %d, 4)" % (N, E))
    choices = None if expert_choices is None else np.asarray(expert_choices)
    if choices is not None and choices.shape != (N, E):
        raise ValueError("expert_choices must have shape (%d, %d)" % (N, E))
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
        out = env.step_many(policy='mlp', n_actions=T, want_obs='device', time_budget_ms=time_budget_ms,
                            policy_noise=None if noise is None else noise[idx, ee], expert=expert, expert_mix=mix[idx, ee],
                            expert_choices=None if choices is None else choices[idx, ee])
        res['kernel_ms'] += float(env.batch.last_kernel_ms)
        res['op_ticks'].append(out['op_ticks'])
        ran = out['ran']
        keep = ran & (slot < N)
        t_, e_ = np.nonzero(keep)                                           # [t][e] order
        if len(t_):
            rows = np.concatenate([slot_start_sources(out)[t_, e_], (t_ * E + e_)[:, None].astype(np.int32)], axis=1)
            trainer.append_launch(rows)
            res['row_env'].append(e_); res['row_slot'].append(slot[t_, e_])
            res['appended'] += len(t_)
        env.batch.fit_hold(hold_sources(out))
        used += ran.sum(axis=0)
        res['launches'] += 1
        parked = env.batch.in_flight()                                      # operations the slice cut: the next launch continues them
        res['records'].append({'ran': ran, 'done': out['done'], 'rew': out['rew'], 'actual_coverage': out['actual_coverage'],
                               'expert_took': out['expert_took'], 'slot': slot, 'n_resets': out['n_resets'], 'parked': parked})
        if not ran.any() and not parked.any() and not (out['n_resets'] > 0).any():
            raise RuntimeError("a launch made no progress (time_budget_ms = %r too short for one substep?)" % (time_budget_ms,))
    res['took'] = time.perf_counter() - t0
    res['substeps'] = int(env.total_substeps - before)
    res['row_env'] = np.concatenate(res['row_env']) if res['row_env'] else np.zeros(0, dtype=np.int64)
    res['row_slot'] = np.concatenate(res['row_slot']) if res['row_slot'] else np.zeros(0, dtype=np.int64)
    res['count'] = used
    res['rows'] = trainer.size()
    return res
