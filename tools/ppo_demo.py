#!/usr/bin/env python3
"""PPO on the device, end to end and small: tools/actor_critic_demo.py's loop with the clipped surrogate in the place of
the advantage-weighted regression, and MANY policy steps per collection. Per iteration: collect under the present network plus Gaussian
exploration noise (demos.actor_critic_collect) -> ONE clothhip_fit_data_gae call writes the value targets and the normalised advantages
-> ONE clothhip_fit_data_snapshot_policy call stores the present means as the rows' old means -> Adam steps of the critic, then
--epochs epochs of PPO minibatches over the collection (demos.ppo_fit). Beside it, from the same seeds and the same noise, on an env of
its own, demos.actor_critic_fit with the SAME number of policy steps. It prints, per iteration, the mean return of the episodes that
completed in both runs, PPO's clip_fraction and kl per epoch, and how far each run's mean has moved from the executed actions; with
--out FILE it also appends the lines there. profiles/ppo.txt holds a run. The tool claims nothing about learning curves: it says what
came out. What it is for is the other column: the weighted regression under these many steps runs away, the clipped surrogate does not.
With --bench it measures instead: clothhip_fit_data_snapshot_policy over the rows of one --envs x --slots collection, kernels and call,
beside the host route it replaces in the same run (fit_predict with its download, fit_set_old_means with its upload).
With --learn-sigma the PPO run carries a log-sigma head that starts at log(--sigma) and is trained by the same surrogate
minus --ent-coef times the entropy: its collections act with unit noise times the head's present sigma, the one snapshot stores the old
means and the old log sigmas, and every iteration's line adds the sigma it acted with; the weighted regression beside it keeps --sigma.
--bench then also times the snapshot with a head on the handle (one more fill kernel). profiles/ppo_sigma.txt holds runs.
With --device-noise the PPO run's exploration noise is a policies.DeviceNoise: the table is made on the device in front of
the launch, and with --learn-sigma under the head where it lies (MLPTrainer.device_noise) -- an iteration then moves no sigma and no
noise through the host. The run beside it keeps its host noise, so the two no longer act with the same noise. In a sweep
(--members) every member's sigma goes down as one [E, 4] table (MLPEnsemble.device_noise). profiles/policy_noise.txt holds runs.
With --members G it runs a SWEEP instead: G = len(--lrs) x len(--sigmas) x len(--seeds) configurations as the members of
ONE MLPEnsemble on one env of G x --envs cloths, member g on every G-th env. Per iteration ONE collection (unit noise times the member's
sigma per env), one fit_gae under a shared critic, one member snapshot and one grouped PPO fit (demos.ppo_fit with the ensemble); it
prints one return curve per member: the mean return of the episodes its envs completed, per iteration, with the epochs it ran. With
--bench --members G it times the member snapshot of one collection beside the host route. profiles/ppo_members.txt holds runs.
    python3 tools/ppo_demo.py [--envs 64] [--slots 12] [--iters 4] [--epochs 10] [--sigma 0.1] [--clip 0.2] [--target-kl X] [--out FILE]
    python3 tools/ppo_demo.py --learn-sigma [--ent-coef 0.01] [--device-noise] [...]
    python3 tools/ppo_demo.py --bench [--envs 512] [--slots 12] [--out FILE]
    python3 tools/ppo_demo.py --members 8 --lrs 1e-3,3e-4,1e-4,3e-5 --sigmas 0.1 --seeds 0,1 [--envs 64] [--iters 4] [--target-kl X] [--out FILE]
    python3 tools/ppo_demo.py --bench --members 16 [--envs 512] [--slots 12] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402
from gym_cloth_amd.demos import actor_critic_collect, actor_critic_fit, ppo_fit      # noqa: E402
from gym_cloth_amd.envs import ClothVecEnv            # noqa: E402
from gym_cloth_amd.policies import DeviceNoise, MLPEnsemble, MLPPolicy, MLPTrainer, ValueTrainer   # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def make_env(E):
    cfg = bench.bench_cfg(25, 0.02, "tier1")
    cfg["env"]["force_grab"] = True
    return ClothVecEnv(cfg, n_envs=E, precision="f32", consume_domrand_draws=False)


def make_layers(widths, seed=0):
    r = np.random.RandomState(seed)
    return [((r.normal(size=(widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32), np.zeros(widths[l + 1], dtype=np.float32))
            for l in range(len(widths) - 1)]


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return "%.3f ms (min %.3f, max %.3f)" % (np.median(xs), xs.min(), xs.max())


def mean(x):
    return float(np.mean(x)) if len(x) else float("nan")


def moved(trainer, col):
    """Mean |mean - executed action|^2 over the collection's non-leaf rows at the present weights."""
    rows = np.asarray(col["nonleaf"])
    y = trainer.predict(rows).astype(np.float64)
    a = trainer.env.batch.fit_data(int(col["first"]), int(col["appended"]) + int(col["open_rows"]))[1].astype(np.float64)[rows - int(col["first"])]
    return float(((y - a) ** 2).sum(axis=1).mean())


def run(args):
    E, T = args.envs, args.slots
    hidden = [int(w) for w in args.hidden.split(",") if w]
    envs = [make_env(E), make_env(E)]
    widths = [3 * envs[0].P] + hidden
    pol = [MLPTrainer(v, MLPPolicy(v, make_layers(widths + [4])), optimizer="adam", lr=args.lr) for v in envs]
    critic = [ValueTrainer(v, make_layers(widths + [1], seed=1), optimizer="adam", lr=args.lr) for v in envs]
    say("ppo demo: %d cloths 25x25 fp32 tier 1 (force_grab), MLP policy and critic hidden %r, %d slots per iteration in one launch, Gaussian "
        "exploration noise sigma %g; GAE gamma %g lambda %g, normalised advantages; Adam lr %g, %d critic steps, then %d epochs of minibatches "
        "of %d rows over the collection: PPO (clip %g, target_kl %r) beside actor_critic_fit with as many policy steps, same seeds and noise"
        % (E, hidden, T, args.sigma, args.gamma, args.lam, args.lr, args.value_steps, args.epochs, args.batch, args.clip, args.target_kl))
    if args.learn_sigma:
        pol[0].set_log_sigma(np.log(args.sigma))
        say("    --learn-sigma: the PPO run's sigma is a head of four log sigmas that starts at log %g and is trained with the network, entropy "
            "coefficient %g; its collections act with unit noise times the head's sigma" % (args.sigma, args.ent_coef))
    for i in range(args.iters):
        t0 = time.perf_counter()
        unit = np.random.RandomState(100 + i).normal(size=(T, E, 4))
        acted = pol[0].sigma() if args.learn_sigma else np.full(4, args.sigma)
        noises = [unit * acted, unit * args.sigma]
        if args.device_noise:                                                 # the PPO run's noise is made on the device, under the head where there is one
            t0 = time.perf_counter()
            noises[0] = pol[0].device_noise(100 + i) if args.learn_sigma else DeviceNoise(100 + i, sigma=args.sigma)
        prep = time.perf_counter() - t0
        for v in envs:
            v.seed([2000 + e for e in range(E)])                              # every iteration from the same start states
            v.reset()
        try:
            cols = [actor_critic_collect(v, tr, n_actions=T, policy_noise=nz, slots_per_launch=T) for v, tr, nz in zip(envs, pol, noises)]
        except ValueError as e:                                               # a network that ran away acts with values that are not finite
            say("iteration %d: a collection was refused (%s): the run ends here" % (i, e))
            break
        before = [moved(tr, c) for tr, c in zip(pol, cols)]
        t0 = time.perf_counter()
        fit = ppo_fit(envs[0], pol[0], critic[0], cols[0], sigma=None if args.learn_sigma else args.sigma, gamma=args.gamma, lam=args.lam,
                      clip=args.clip, n_value_steps=args.value_steps, n_epochs=args.epochs, batch_size=args.batch, seed=i, target_kl=args.target_kl,
                      ent_coef=args.ent_coef if args.learn_sigma else 0.0)
        dp = time.perf_counter() - t0
        n_mb = max(1, len(cols[1]["nonleaf"]) // args.batch)
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            acf = actor_critic_fit(envs[1], pol[1], critic[1], cols[1], gamma=args.gamma, lam=args.lam, n_value_steps=args.value_steps,
                                   n_policy_steps=args.epochs * n_mb, batch_size=args.batch, seed=i)
            after = [moved(tr, c) for tr, c in zip(pol, cols)]
        da = time.perf_counter() - t0
        say("iteration %d: PPO %4d rows + %d leaves, %3d completed episodes, mean return %.4f | weighted regression %4d rows + %d leaves, %3d "
            "completed episodes, mean return %.4f" % (i, cols[0]["appended"], cols[0]["open_rows"], len(cols[0]["episode_return"]),
                                                      mean(cols[0]["episode_return"]), cols[1]["appended"], cols[1]["open_rows"],
                                                      len(cols[1]["episode_return"]), mean(cols[1]["episode_return"])))
        say("    PPO's exploration noise: %s, %.3f ms on the host before the collection; the collection took %.1f ms (kernels %.1f ms)"
            % ("made on the device in front of the launch (DeviceNoise)" if args.device_noise else "drawn and scaled on the host, uploaded by the launch",
               prep * 1e3, cols[0]["took"] * 1e3, cols[0]["kernel_ms"]))
        n_stats = fit["ppo_stats"].shape[1]
        per = fit["ppo_stats"].reshape(fit["epochs"], -1, n_stats).mean(axis=1) if fit["epochs"] else np.zeros((0, n_stats))
        if args.learn_sigma:
            say("    sigma acted with %s -> after the fit %s; entropy per epoch %s" % (
                " ".join("%.5f" % s for s in acted), " ".join("%.5f" % s for s in pol[0].sigma()), " ".join("%.4f" % h for h in per[:, 3])))
        say("    PPO: %d epochs, %d steps, fit %.0f ms; per epoch clip_fraction %s | kl %s | surrogate loss %s" % (
            fit["epochs"], len(fit["ppo_stats"]), dp * 1e3, " ".join("%.3f" % c for c in per[:, 1]), " ".join("%.4f" % k for k in per[:, 2]),
            " ".join("%.4f" % l for l in per[:, 0])))
        say("    mean |mean - executed action|^2 over the collection: PPO %.5f -> %.5f | weighted regression (%d steps, %.0f ms) %.5f -> %.5g, its "
            "weighted loss %.5g -> %.5g" % (before[0], after[0], len(acf["policy_losses"]), da * 1e3, before[1], after[1], acf["policy_losses"][0],
                                           acf["policy_losses"][-1]))
    for v in envs:
        v.close()


def sweep(args):
    """--members: the configurations lr x sigma x seed as the members of one ensemble; one return curve per member."""
    from gym_cloth_amd.demos import _collection_returns
    lrs, sigmas, seeds = ([t(x) for x in v.split(",") if x] for v, t in ((args.lrs, float), (args.sigmas, float), (args.seeds, int)))
    configs = [(lr, sg, sd) for lr in lrs for sg in sigmas for sd in seeds]
    G = len(configs)
    if G != args.members:
        raise SystemExit("--members %d, but --lrs x --sigmas x --seeds names %d configurations" % (args.members, G))
    per, T = args.envs, args.slots
    E = G * per
    hidden = [int(w) for w in args.hidden.split(",") if w]
    env = make_env(E)
    widths = [3 * env.P] + hidden
    lr, sigma = np.array([c[0] for c in configs]), np.array([c[1] for c in configs])
    ens = MLPEnsemble(env, [make_layers(widths + [4], seed=c[2]) for c in configs], optimizer="adam", lr=lr)
    critic = ValueTrainer(env, make_layers(widths + [1], seed=1), optimizer="adam", lr=args.lr)
    say("ppo sweep: %d members x %d cloths 25x25 fp32 tier 1 (force_grab) on ONE env, member g on envs g, g + %d, ...; policy and shared critic hidden "
        "%r, %d slots per iteration in one launch; GAE gamma %g lambda %g, advantages normalised per member on the host; critic Adam lr %g, %d steps; "
        "then up to %d epochs of minibatches of %d rows per member in grouped launches (clip %g, target_kl %r)"
        % (G, per, G, hidden, T, args.gamma, args.lam, args.lr, args.value_steps, args.epochs, args.batch, args.clip, args.target_kl))
    curves, ran = np.full((G, args.iters), np.nan), np.zeros((G, args.iters), dtype=int)
    for i in range(args.iters):
        unit = np.random.RandomState(100 + i).normal(size=(T, E, 4))
        env.seed([2000 + e // G for e in range(E)])                           # every iteration from the same start states, the same ones for every member
        env.reset()
        try:
            noise = ens.device_noise(100 + i, sigma) if args.device_noise else unit * sigma[ens.member][None, :, None]
            col = actor_critic_collect(env, ens, n_actions=T, policy_noise=noise, slots_per_launch=T)
        except ValueError as e:
            say("iteration %d: the collection was refused (%s): the run ends here" % (i, e))
            break
        Gt, complete, _, starts = _collection_returns(col, T, 1.0, E)
        who = ens.member[col["row_env"]]
        t0 = time.perf_counter()
        fit = ppo_fit(env, ens, critic, col, sigma=sigma, gamma=args.gamma, lam=args.lam, clip=args.clip, n_value_steps=args.value_steps,
                      n_epochs=args.epochs, batch_size=args.batch, seed=i, target_kl=args.target_kl)
        dt = time.perf_counter() - t0
        for j, g in enumerate(fit["members"]):
            curves[g, i], ran[g, i] = mean(Gt[starts & complete & (who == g)]), fit["epochs"][j]
        kl = np.nanmean(fit["ppo_stats"][:, :, 2], axis=0) if len(fit["ppo_stats"]) else np.zeros(0)
        say("iteration %d: %d rows + %d leaves, %d completed episodes, fit %.0f ms (collection %.0f ms); mean kl per member %s"
            % (i, col["appended"], col["open_rows"], len(col["episode_return"]), dt * 1e3, col["took"] * 1e3, " ".join("%.4f" % k for k in kl)))
    for g, (l, sg, sd) in enumerate(configs):
        say("member %2d lr %-8g sigma %-6g seed %d: mean return per iteration %s | epochs %s"
            % (g, l, sg, sd, " ".join("%.4f" % c for c in curves[g]), " ".join("%d" % e for e in ran[g])))
    env.close()


def bench_members_section(args, reps=10):
    """--bench --members G: the member snapshot of one collection beside fit_predict per member plus ONE fit_set_old_means through the host."""
    E, T, G = args.envs, args.slots, args.members
    env = make_env(E)
    for e in range(E):
        env.np_randoms[e] = np.random.RandomState(1000 + e)
    env.reset()
    ens = MLPEnsemble(env, [make_layers([3 * env.P, 64, 64, 4], seed=7 + g) for g in range(G)])
    b = env.batch
    col = actor_critic_collect(env, ens, n_actions=T, slots_per_launch=T)
    n = col["appended"] + col["open_rows"]
    mor = np.where(col["leaf"], -1, ens.member[col["ds_env"]]).astype(np.int32)
    say("member snapshot bench: the %d rows (%d of them leaves, skipped) of one %d x %d-slot collection (25x25, policy hidden [64, 64]) under G = %d "
        "members; %d repetitions each, medians" % (n, col["open_rows"], E, T, G, reps))
    b.fit_snapshot_policy_members(mor)
    kern, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.fit_snapshot_policy_members(mor)
        wall.append(time.perf_counter() - t0)
        kern.append(b.last_kernel_ms * 1e-3)
    say("    clothhip_fit_data_snapshot_policy_members, nothing downloaded: device (the grouped forward + the scatter) %s, call %s" % (stats(kern), stats(wall)))
    dev = b.fit_get_old_means()
    parts = {"predict": [], "upload": [], "all": []}
    lists = [np.nonzero(mor == g)[0] for g in range(G)]
    for _ in range(reps):
        y = np.zeros((n, 4), dtype=np.float32)
        t0 = time.perf_counter()
        for g, mine in enumerate(lists):
            if len(mine):
                y[mine] = b.fit_predict(mine, [g])[0]
        t1 = time.perf_counter()
        b.fit_set_old_means(y)                                               # (the leaves get zeros and a mark on this route)
        t2 = time.perf_counter()
        for k, d in zip(("predict", "upload", "all"), (t1 - t0, t2 - t1, t2 - t0)):
            parts[k].append(d)
    say("    the host route: G fit_predict calls with their downloads %s, fit_set_old_means %s; together %s" % tuple(stats(parts[k]) for k in ("predict", "upload", "all")))
    say("    both routes leave the same bytes in the old-mean column: %s" % (dev.tobytes() == b.fit_get_old_means().tobytes()))
    env.close()


def bench_section(args, reps=10):
    E, T = args.envs, args.slots
    env = make_env(E)
    for e in range(E):
        env.np_randoms[e] = np.random.RandomState(1000 + e)
    env.reset()
    tr = MLPTrainer(env, MLPPolicy(env, make_layers([3 * env.P, 64, 64, 4], seed=7)))
    b = env.batch
    col = actor_critic_collect(env, tr, n_actions=T, slots_per_launch=T)
    n = col["appended"] + col["open_rows"]
    say("snapshot bench: the %d rows (%d of them leaves) of one %d x %d-slot collection (25x25, policy hidden [64, 64]); %d repetitions each, "
        "medians" % (n, col["open_rows"], E, T, reps))
    b.fit_snapshot_policy(0, n)                                               # (allocates the scratch)
    kern, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.fit_snapshot_policy(0, n)
        wall.append(time.perf_counter() - t0)
        kern.append(b.last_kernel_ms * 1e-3)
    say("    clothhip_fit_data_snapshot_policy, nothing downloaded: device (the policy's forward + the copies) %s, call %s" % (stats(kern), stats(wall)))
    dev = b.fit_get_old_means()
    parts = {"predict": [], "upload": [], "all": []}
    idx = np.arange(n)
    for _ in range(reps):
        t0 = time.perf_counter()
        y = b.fit_predict(idx)
        t1 = time.perf_counter()
        b.fit_set_old_means(y)
        t2 = time.perf_counter()
        for k, d in zip(("predict", "upload", "all"), (t1 - t0, t2 - t1, t2 - t0)):
            parts[k].append(d)
    say("    the host route: fit_predict with its download %s, fit_set_old_means %s; together %s" % tuple(stats(parts[k]) for k in ("predict", "upload", "all")))
    say("    both routes leave the same bytes in the old-mean column: %s" % (dev.tobytes() == b.fit_get_old_means().tobytes()))
    # with a head on the handle the same call also fills the old-log-sigma column
    tr.set_log_sigma(np.log(0.1))
    b.fit_snapshot_policy(0, n)
    kern, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.fit_snapshot_policy(0, n)
        wall.append(time.perf_counter() - t0)
        kern.append(b.last_kernel_ms * 1e-3)
    say("    with a log-sigma head (the fill of the old-log-sigma column behind the forward): device %s, call %s; the column holds the head in "
        "every row: %s" % (stats(kern), stats(wall), b.fit_get_old_log_sigma().tobytes() == np.tile(tr.log_sigma(), (n, 1)).tobytes()))
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=10, help="epochs over the collection per iteration; the weighted regression takes as many steps")
    ap.add_argument("--sigma", type=float, default=0.1, help="standard deviation of the exploration noise: the policy's sigma")
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--target-kl", type=float, default=None)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--hidden", default="64,64")
    ap.add_argument("--value-steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--learn-sigma", action="store_true", help="the PPO run trains a log-sigma head that starts at log(--sigma)")
    ap.add_argument("--ent-coef", type=float, default=0.0, help="with --learn-sigma: the coefficient of the entropy bonus")
    ap.add_argument("--device-noise", action="store_true", help="the PPO run's (the sweep's) exploration noise is made on the device: policies.DeviceNoise")
    ap.add_argument("--bench", action="store_true", help="measure the snapshot on the device against the host route")
    ap.add_argument("--members", type=int, default=0, help="run a sweep of this many configurations as the members of one ensemble (--lrs x --sigmas x --seeds)")
    ap.add_argument("--lrs", default="1e-3", help="with --members: the members' Adam learning rates, comma-separated")
    ap.add_argument("--sigmas", default="0.1", help="with --members: the members' exploration sigmas, comma-separated")
    ap.add_argument("--seeds", default="0", help="with --members: the seeds of the members' initial networks, comma-separated")
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    if args.envs is None:
        args.envs = 512 if args.bench else 64
    if args.bench and args.members:
        bench_members_section(args)
    elif args.bench:
        bench_section(args)
    elif args.members:
        sweep(args)
    else:
        run(args)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
