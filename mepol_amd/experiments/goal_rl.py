"""Goal-based RL command line (drop-in for src/experiments/goal_rl.py of the reference): TRPO on
a sparse goal reward, from a random policy or from one pre-trained by the MEPOL command line.

Same flags, defaults and experiment specs (src/experiments/goal_rl.py:17-168); same results
directory layout and log_info.txt.  Runs sampling, batch processing and the policy step on the
GPU (algorithms/trpo.py):

    python -m mepol_amd.experiments.goal_rl --env GridGoal1 --num_epochs 100 \
        --batch_size 24000 --traj_len 1200 --cg_iters 20 --kl_thresh 0.001 \
        --policy_init results/exploration/mepol/<run>/<epoch>-policy

--hidden_sizes N [N ...] (a build extension, as the MEPOL command line's) sets the policy's hidden
widths, so a policy pre-trained with `mepol --hidden_sizes 300 300 300` loads here; policies with
two to six ReLU layers sample on the one-launch goal rollouts.

--env MountainCarGoal (a build extension: the reference has no MountainCar goal) is the hilltop of
the MEPOL command line's MountainCar, CustomRewardEnv(MountainCarContinuous(), ThresholdGoal(0,
0.45)), with that command line's policy ([300, 300], ReLU, log_std_init -0.5), so a policy
pre-trained with `mepol --env MountainCar` loads with --policy_init.  The goal is gym's own `done`
for this env: the wall clips the position to exactly 0.45 with velocity 0 when it is crossed, so
`position >= goal_position and velocity >= 0` is the same condition.  It samples on the one-launch
threshold-goal rollouts.

--env GridGoalAny and --env MountainCarLeft (build extensions) are goals the rollout kernels have
no kind for.  GridGoalAny is the three reference GridWorld goals at once, AnyGoal(GridGoal((5,
5)), GridGoal((2, 5)), GridGoal((5, 2))), with the GridGoal policy; MountainCarLeft is the left
hilltop, BoxGoal((-inf, -inf), (-1.1, inf)): position <= -1.1, with MountainCarGoal's policy, so
`mepol --env MountainCar` checkpoints load.  Both rewards are envs.BatchReward objects (a reward
of the reached state alone, defined for whole batches), and so is any such reward of a user's:
they sample on the un-terminated one-launch rollouts, cut at each trajectory's first done
(algorithms/trpo.py).  A plain function reward keeps the reference's one-env host loop.

--env FourRoomsGoal (a build extension) is the far corner of the four-rooms maze of
`mepol --env FourRooms`, CustomRewardEnv(BoxMazeContinuous.four_rooms(), GridGoal((5, 5))), with
the GridGoal policy, so that command line's checkpoints load.  It samples on the one-launch goal
rollouts, as every GridGoal, ThresholdGoal or BatchReward over a BoxMazeContinuous does.

MuJoCo goals (AntEscape, AntNavigate, AntJump, HumanoidUp) keep their specs but need mujoco-py,
which is outside this build's scope.
"""
import argparse
import os
import sys
from datetime import datetime

import numpy as np
import torch
import torch.nn as nn


def build_parser():
    p = argparse.ArgumentParser(description="Goal-Based Reinforcement Learning - TRPO")
    p.add_argument("--num_workers", type=int, default=1,
                   help="How many parallel workers to use when collecting samples")
    p.add_argument("--env", type=str, required=True,
                   help="The MDP (build extensions: MountainCarGoal, GridGoalAny, "
                        "MountainCarLeft, FourRoomsGoal)")
    p.add_argument("--policy_init", type=str, default=None,
                   help="Path to the weights for custom policy initialization.")
    p.add_argument("--num_epochs", type=int, required=True, help="The number of training epochs")
    p.add_argument("--batch_size", type=int, required=True, help="The batch size")
    p.add_argument("--traj_len", type=int, required=True,
                   help="The maximum length of a trajectory")
    p.add_argument("--gamma", type=float, default=0.995, help="The discount factor")
    p.add_argument("--lambd", type=float, default=0.98, help="The GAE lambda")
    p.add_argument("--optimizer", type=str, default="adam",
                   help="The optimizer used for the critic, either adam or lbfgs")
    p.add_argument("--critic_lr", type=float, default=1e-2,
                   help="Learning rate for critic optimization")
    p.add_argument("--critic_reg", type=float, default=1e-3,
                   help="Regularization coefficient for critic optimization")
    p.add_argument("--critic_iters", type=int, default=5, help="Number of critic full updates")
    p.add_argument("--critic_batch_size", type=int, default=64,
                   help="Mini batch in case of adam optimizer for critic optimization")
    p.add_argument("--cg_iters", type=int, default=10, help="Conjugate gradient iterations")
    p.add_argument("--cg_damping", type=float, default=0.1,
                   help="Conjugate gradient damping factor")
    p.add_argument("--kl_thresh", type=float, required=True, help="KL threshold")
    p.add_argument("--seed", type=int, default=None, help="The random seed")
    p.add_argument("--tb_dir_name", type=str, default="goal_rl",
                   help="The tensorboard directory under which the directory of this experiment is put")
    p.add_argument("--results_dir", type=str, default=None,
                   help="(build extension) root of results/goal_rl; default: ./results/goal_rl")
    p.add_argument("--hidden_sizes", type=int, nargs="+", default=None, metavar="N",
                   help="(build extension) hidden layer widths of the policy instead of the "
                        "experiment spec's; default: the spec's")
    return p


def checkpoint_widths(state_dict):
    """Hidden layer widths a GaussianPolicy checkpoint holds, from its net.<i>.weight keys."""
    keys = sorted((k for k in state_dict if k.startswith("net.") and k.endswith(".weight")),
                  key=lambda k: int(k.split(".")[1]))
    return [int(state_dict[k].shape[0]) for k in keys]


def exp_specs():
    from ..envs import (AnyGoal, BoxGoal, BoxMazeContinuous, CustomRewardEnv, GridGoal,
                        GridWorldContinuous, MountainCarContinuous, ThresholdGoal)

    def grid_reward(make_reward):
        return dict(env_create=lambda: CustomRewardEnv(GridWorldContinuous(), make_reward()),
                    hidden_sizes=[300, 300], activation=nn.ReLU, log_std_init=-1.5)

    def grid(goal):
        return grid_reward(lambda: GridGoal(goal))

    # the MEPOL command line's MountainCar policy, so that its checkpoints load
    def mountain_car_reward(make_reward):
        return dict(env_create=lambda: CustomRewardEnv(MountainCarContinuous(), make_reward()),
                    hidden_sizes=[300, 300], activation=nn.ReLU, log_std_init=-0.5)

    mountain_car = mountain_car_reward(lambda: ThresholdGoal(0, 0.45))
    inf = float("inf")
    mujoco = dict(env_create=None, hidden_sizes=[400, 300], activation=nn.ReLU, log_std_init=-0.5)
    return {"GridGoal1": grid((5, 5)), "GridGoal2": grid((2, 5)), "GridGoal3": grid((5, 2)),
            "MountainCarGoal": mountain_car,
            "GridGoalAny": grid_reward(lambda: AnyGoal(GridGoal((5, 5)), GridGoal((2, 5)),
                                                       GridGoal((5, 2)))),
            "MountainCarLeft": mountain_car_reward(lambda: BoxGoal((-inf, -inf), (-1.1, inf))),
            "FourRoomsGoal": dict(
                env_create=lambda: CustomRewardEnv(BoxMazeContinuous.four_rooms(),
                                                   GridGoal((5, 5))),
                hidden_sizes=[300, 300], activation=nn.ReLU, log_std_init=-1.5),
            "AntEscape": dict(mujoco), "AntNavigate": dict(mujoco), "AntJump": dict(mujoco),
            "HumanoidUp": dict(mujoco)}


def create_critic(num_features, hidden_sizes=(64, 64), hidden_activation=nn.ReLU):
    """The reference's value function (goal_rl.py:187-208): an MLP with orthogonal weights."""
    layers, fan_in = [], num_features
    for width in hidden_sizes:
        layers.extend([nn.Linear(fan_in, width), hidden_activation()])
        fan_in = width
    layers.append(nn.Linear(fan_in, 1))
    vfunc = nn.Sequential(*layers)
    for module in vfunc:
        if isinstance(module, nn.Linear):
            nn.init.orthogonal_(module.weight)
    return vfunc


def main(argv=None):
    from ..algorithms.trpo import trpo
    from ..policy import GaussianPolicy

    args = build_parser().parse_args(argv)
    specs = exp_specs()
    spec = specs.get(args.env)
    if spec is None:
        print(f"Experiment name not found. Available ones are: {', '.join(specs)}.")
        return 1
    if spec["env_create"] is None:
        print(f"{args.env} needs MuJoCo (mujoco-py), which is outside this build's scope.")
        return 2
    hidden_sizes = args.hidden_sizes if args.hidden_sizes is not None else spec["hidden_sizes"]
    if any(w <= 0 for w in hidden_sizes):
        print("--hidden_sizes needs positive widths.")
        return 4
    if not torch.cuda.is_available():
        print("mepol_amd needs a ROCm GPU (MI355X); there is no CPU path.")
        return 3
    torch.set_default_dtype(torch.float64)
    device = torch.device("cuda")
    env = spec["env_create"]()
    policy = GaussianPolicy(num_features=env.num_features, hidden_sizes=hidden_sizes,
                            action_dim=env.action_space.shape[0], activation=spec["activation"],
                            log_std_init=spec["log_std_init"]).to(device)
    vfunc = create_critic(env.num_features).to(device)
    if args.policy_init is not None:
        kind = "MEPOLInit"
        checkpoint = torch.load(args.policy_init, map_location=device)
        own = policy.state_dict()
        if (set(checkpoint) != set(own)
                or any(tuple(checkpoint[k].shape) != tuple(v.shape) for k, v in own.items())):
            held = " ".join(str(w) for w in checkpoint_widths(checkpoint))
            print(f"--policy_init: the checkpoint holds hidden layers of widths {held}, the "
                  f"policy has {' '.join(str(w) for w in hidden_sizes)}; pass --hidden_sizes "
                  f"{held}.")
            return 4
        policy.load_state_dict(checkpoint)
    else:
        kind = "RandomInit"

    exp_name = f"env={args.env},init={kind}"
    if args.hidden_sizes is not None:
        exp_name += ",hidden=" + "x".join(str(w) for w in args.hidden_sizes)
    root = args.results_dir or os.path.join(os.getcwd(), "results", "goal_rl")
    out_path = os.path.join(root, args.tb_dir_name, exp_name + "__" +
                            datetime.now().strftime("%Y_%m_%d_%H_%M_%S") + "__" + str(os.getpid()))
    os.makedirs(out_path, exist_ok=True)
    with open(os.path.join(out_path, "log_info.txt"), "w") as f:
        f.write("Run info:\n")
        f.write("-" * 10 + "\n")
        for key, value in vars(args).items():
            if key in ("results_dir", "hidden_sizes") and value is None:
                continue  # absent: the file is the one the reference writes
            f.write(f"{key}={value}\n")
        f.write("-" * 10 + "\n")
        f.write(str(policy))
        f.write("-" * 10 + "\n")
        f.write(str(vfunc))
        f.write("\n")
        if args.seed is None:
            args.seed = int(np.random.randint(2 ** 16 - 1))
            f.write(f"Setting random seed {args.seed}\n")

    trpo(env_maker=spec["env_create"], env_name=args.env, num_epochs=args.num_epochs,
         batch_size=args.batch_size, traj_len=args.traj_len, gamma=args.gamma, lambd=args.lambd,
         vfunc=vfunc, policy=policy, optimizer=args.optimizer, critic_lr=args.critic_lr,
         critic_reg=args.critic_reg, critic_iters=args.critic_iters,
         critic_batch_size=args.critic_batch_size, cg_iters=args.cg_iters,
         cg_damping=args.cg_damping, kl_thresh=args.kl_thresh, num_workers=args.num_workers,
         out_path=out_path, seed=args.seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
