"""Time of the parts of one TRPO epoch (algorithms/trpo.py) at the GridGoal1 script's shape:
batch 24,000, traj_len 1200, policy 2 -> [300, 300] -> 2, cg_iters 20, kl_thresh 0.001.

    python tools/trpo_epoch_bench.py                      JSON to profiles/trpo_epoch_bench.json
    python tools/trpo_epoch_bench.py --batch_size 2400 --traj_len 120 --reps 3
    python tools/trpo_epoch_bench.py --hidden_sizes 300 300 300 \
        --out profiles/trpo_epoch_bench_deep.json
    python tools/trpo_epoch_bench.py --env MountainCarGoal    the goal_rl spec of that name (policy
                                          2 -> [300, 300] -> 1, log_std -0.5; random weights only),
                                          JSON to profiles/trpo_epoch_bench_mc.json
    python tools/trpo_epoch_bench.py --env GridGoalAny        a goal_rl spec whose reward is a
    python tools/trpo_epoch_bench.py --env MountainCarLeft    BatchReward: the "roll out, then cut"
                                          route, JSON to profiles/trpo_epoch_bench_<env>.json
    python tools/trpo_epoch_bench.py --env GridGoal1Cut       GridGoal1 / MountainCarGoal with the
    python tools/trpo_epoch_bench.py --env MountainCarGoalCut goal wrapped in a one-member AnyGoal:
                                          the same episodes on the cut route, like for like
    python tools/trpo_epoch_bench.py --env FourRoomsGoal      the goal_rl spec of that name: the
                                          four-rooms box maze (the kernels' env 2), GridGoal1's
                                          policies and goal
    python tools/trpo_epoch_bench.py --sampling_only          only the two sampling rows

Per epoch, the median [min, max] over --reps epochs after --warmup:
  sample_kernel   collect_sample_batch on the kernel path (rounds of ops.rollout_goal, or of
                  ops.rollout_deep_goal for 3 to 6 hidden layers, + ops.traj_budget; for
                  MountainCarGoal their threshold-goal forms);
  sample_cut      the same on the cut route, for the envs whose reward is a BatchReward (rounds of
                  the un-terminated ops.rollout_mlp / ops.rollout_deep, one reward.batch call,
                  ops.traj_cut, ops.traj_budget): a round always runs traj_len steps;
  sample_host     collect_sample_batch on the reference-shaped host loop in the same process
                  (MEPOL_TRPO_SAMPLER=host): one policy.predict and one env.step per step.  It
                  is the comparison point of the sampler and takes seconds, so it has its own
                  --host_reps and a short warm-up batch;
  process_batch   ops.gae + ops.standardize over the sampled batch (values from the critic);
  trpo_step       the policy update;
  critic_fit      the reference's Adam fit, 5 passes over mini-batches of 64, as _fit_critic runs
                  it: one launch of ops.critic_fit (the row says which path it took);
  critic_fit_host the same fit from the same critic on the reference's DataLoader loop in the
                  same process (MEPOL_CRITIC_FIT=host): one torch step per mini-batch.
Sampling is timed at two policies, since the termination frequency changes the round count: the
pre-trained-like weights of tests/golden/policy_pretrained_gw.npz and a random initialisation.
With --hidden_sizes only the random initialisation is timed (the golden weights are [300, 300]).
The other parts are timed on the random policy's batch.  Wall-clock times between device
synchronisations: every part ends in a host read or is followed by one.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOAL = (5, 5)  # GridGoal1
GAMMA, LAMBD, KL_THRESH, CG_DAMPING = 0.995, 0.98, 0.001, 0.1


ENVS = ("GridGoal1", "MountainCarGoal", "GridGoalAny", "MountainCarLeft", "GridGoal1Cut",
        "MountainCarGoalCut", "FourRoomsGoal")
CUT_ENVS = ENVS[2:6]          # sampled on the cut route
MOUNTAINCAR_ENVS = ("MountainCarGoal", "MountainCarLeft", "MountainCarGoalCut")


def _policies(dev, hidden=None, env_name="GridGoal1"):
    import numpy as np
    import torch

    from mepol_amd.policy import GaussianPolicy

    torch.manual_seed(7)
    if env_name in MOUNTAINCAR_ENVS:
        return {"random": GaussianPolicy(hidden or [300, 300], 2, 1, -0.5).to(dev)}
    random = GaussianPolicy(hidden or [300, 300], 2, 2, -1.5).to(dev)
    if hidden:
        return {"random": random}
    pre = GaussianPolicy([300, 300], 2, 2, -1.5).to(dev)
    z = np.load(os.path.join(HERE, "tests", "golden", "policy_pretrained_gw.npz"))
    pre.load_state_dict({k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("sd.")})
    return {"pretrained": pre, "random": random}


def _wall(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "samples": len(ms)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--batch_size", type=int, default=24000)
    p.add_argument("--traj_len", type=int, default=1200)
    p.add_argument("--cg_iters", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--host_reps", type=int, default=1)
    p.add_argument("--hidden_sizes", type=int, nargs="+", default=None, metavar="N",
                   help="hidden widths of the policy; default [300, 300]")
    p.add_argument("--env", choices=ENVS, default="GridGoal1",
                   help="the goal_rl experiment whose env and policy shape are timed")
    p.add_argument("--sampling_only", action="store_true",
                   help="time only the sampling rows, not the rest of the epoch")
    p.add_argument("--out", default=None,
                   help="default profiles/trpo_epoch_bench.json (MountainCarGoal: "
                        "profiles/trpo_epoch_bench_mc.json, every other env: "
                        "profiles/trpo_epoch_bench_<env>.json)")
    args = p.parse_args(argv)
    if args.out is None:
        suffix = {"GridGoal1": "", "MountainCarGoal": "_mc"}.get(args.env, "_" + args.env)
        args.out = os.path.join(HERE, "profiles", f"trpo_epoch_bench{suffix}.json")
    sys.path.insert(0, HERE)
    import torch

    from mepol_amd.algorithms import trpo as T
    from mepol_amd.envs import AnyGoal, CustomRewardEnv, GridGoal, GridWorldContinuous
    from mepol_amd.experiments.goal_rl import exp_specs

    dev = torch.device("cuda")
    if args.env == "GridGoal1":
        env = CustomRewardEnv(GridWorldContinuous(), GridGoal(GOAL))
    elif args.env in ("GridGoal1Cut", "MountainCarGoalCut"):
        # the in-kernel spec's own goal as a BatchReward: the same episodes on the cut route
        env = exp_specs()[args.env[:-3]]["env_create"]()
        env = CustomRewardEnv(env.env, AnyGoal(env.get_reward))
    else:
        env = exp_specs()[args.env]["env_create"]()
    env.seed(0)
    path = "cut" if args.env in CUT_ENVS else "kernel"
    B, L = args.batch_size, args.traj_len
    rows = {}
    batch = None
    for name, policy in _policies(dev, args.hidden_sizes, args.env).items():
        os.environ["MEPOL_TRPO_SAMPLER"] = "kernel"
        ms, rounds, trajs, dones = [], [], [], []
        for i in range(args.warmup + args.reps):
            t, batch = _wall(lambda: T.collect_sample_batch(env, policy, B, L))
            assert T.SAMPLER_STATS["path"] == path and int(batch[3].sum()) == B
            if i >= args.warmup:
                ms.append(t)
                rounds.append(T.SAMPLER_STATS["rounds"])
                trajs.append(batch[0].shape[0])
                dones.append(int(batch[4].sum()))
        rows[f"sample_{path}/{name}"] = dict(_stats(ms), rounds=statistics.median(rounds),
                                             trajectories=statistics.median(trajs),
                                             terminated=statistics.median(dones))
        os.environ["MEPOL_TRPO_SAMPLER"] = "host"
        if args.host_reps:
            T.collect_sample_batch(env, policy, min(B, 200), L)  # warm-up
        ms, hb = [], None
        for _ in range(args.host_reps):
            t, hb = _wall(lambda: T.collect_sample_batch(env, policy, B, L))
            assert T.SAMPLER_STATS["path"] == "host" and int(hb[3].sum()) == B
            ms.append(t)
        if hb is not None:
            rows[f"sample_host/{name}"] = dict(_stats(ms), trajectories=hb[0].shape[0],
                                               terminated=int(hb[4].sum()))
        os.environ["MEPOL_TRPO_SAMPLER"] = "kernel"
        print(json.dumps({k: v for k, v in rows.items() if k.endswith(name)}), flush=True)

    if not args.sampling_only:
        _rest_of_epoch(args, T, dev, batch, rows)
    result = {"shape": {"batch_size": B, "traj_len": L, "hidden": args.hidden_sizes or [300, 300],
                        "cg_iters": args.cg_iters, "kl_thresh": KL_THRESH},
              "run": {"reps": args.reps, "warmup": args.warmup, "host_reps": args.host_reps},
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.env != "GridGoal1":
        result["shape"]["env"] = args.env
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"{'part':28s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    for k, v in rows.items():
        print(f"{k:28s} {v['median_ms']:10.2f} {v['min_ms']:10.2f} {v['max_ms']:10.2f}")


def _rest_of_epoch(args, T, dev, batch, rows):
    """process_batch, trpo_step and the critic fit on the random policy's last batch."""
    import torch

    from mepol_amd.experiments.goal_rl import create_critic

    B = args.batch_size
    policy = _policies(dev, args.hidden_sizes, args.env)["random"]
    vfunc = create_critic(2).to(device=dev, dtype=torch.float64)
    states, actions, rewards, lens, done = batch
    m, _, nf = states.shape
    theta0 = {k: v.clone() for k, v in policy.state_dict().items()}
    critic0 = {k: v.clone() for k, v in vfunc.state_dict().items()}
    parts = {"process_batch": [], "trpo_step": [], "critic_fit": [], "critic_fit_host": []}
    fit_paths, fit_steps = set(), 5 * (B // 64)
    for i in range(args.warmup + args.reps):
        policy.load_state_dict(theta0)
        vfunc.load_state_dict(critic0)
        opt = torch.optim.Adam(vfunc.parameters(), lr=1e-2)
        with torch.no_grad():
            values = vfunc(states.to(torch.float64).reshape(-1, nf)).reshape(m, -1)
        t_pb, (es, ea, et, eadv) = _wall(lambda: T.process_batch(
            states, actions, rewards, lens, done, values, GAMMA, LAMBD))
        t_step, _ = _wall(lambda: T.trpo_step(policy, es, ea, eadv, KL_THRESH,
                                              cg_iters=args.cg_iters, cg_damping=CG_DAMPING))
        os.environ.pop("MEPOL_CRITIC_FIT", None)
        t_fit, _ = _wall(lambda: T._fit_critic(vfunc, opt, "adam", es, et, 1e-3, 5, 64))
        fit_paths.add(T.CRITIC_FIT_STATS["path"])
        vfunc.load_state_dict(critic0)
        opt = torch.optim.Adam(vfunc.parameters(), lr=1e-2)
        os.environ["MEPOL_CRITIC_FIT"] = "host"
        t_host, _ = _wall(lambda: T._fit_critic(vfunc, opt, "adam", es, et, 1e-3, 5, 64))
        assert T.CRITIC_FIT_STATS["path"] == "host"
        os.environ.pop("MEPOL_CRITIC_FIT", None)
        if i >= args.warmup:
            for k, t in (("process_batch", t_pb), ("trpo_step", t_step), ("critic_fit", t_fit),
                         ("critic_fit_host", t_host)):
                parts[k].append(t)
    rows.update({k: _stats(v) for k, v in parts.items()})
    for k in ("critic_fit", "critic_fit_host"):
        rows[k].update(steps=fit_steps, us_per_step=1e3 * rows[k]["median_ms"] / fit_steps)
    rows["critic_fit"]["path"] = "/".join(sorted(fit_paths))


if __name__ == "__main__":
    main()
