"""Per-step time of the one-launch rollouts on GridWorld (env 1) and on box mazes (env 2): what
data-driven walls cost on the serial tail of a step.

    python tools/maze_rollout_bench.py [--out profiles/maze_rollout_bench.json]
    python tools/maze_rollout_bench.py --gridworld_only     (also runs, copied, in an older tree)

Rows: MEPOL's GridWorld shape (20 trajectories x 1,200 steps) for [300, 300] (the two-layer kernel
in the form its plan picks) and [300, 300, 300] (the deep kernel), on GridWorld, on the default
GridWorld as a maze (7 walls) and on a 16-wall maze.  Each figure is the median over --reps
launches of the wall time between two device synchronisations, divided by the steps; the launch
includes the wrapper's per-call work (W2^T transpose, workspace, error-word read), the same on
every row.  --gridworld_only imports nothing the maze added, so a copy of this file in the tools/
of a checkout from before the maze times that tree's GridWorld kernels the same way."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sixteen_walls():
    from mepol_amd.envs import BoxMazeContinuous

    walls = [(-4.5 + 3.0 * (k % 4) - 0.4, -4.5 + 3.0 * (k % 4) + 0.4,
              -3.0 + 3.0 * (k // 4) - 0.4, -3.0 + 3.0 * (k // 4) + 0.4) for k in range(16)]
    return BoxMazeContinuous((-6.0, 6.0, -6.0, 6.0), walls, 0.2, ((-6.0, -6.0), (-4.0, -4.0)))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--num_traj", type=int, default=20)
    p.add_argument("--traj_len", type=int, default=1200)
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--gridworld_only", action="store_true")
    p.add_argument("--out", default=os.path.join(HERE, "profiles", "maze_rollout_bench.json"))
    args = p.parse_args(argv)
    sys.path.insert(0, HERE)
    import torch
    import torch.nn as nn

    from mepol_amd import ops
    from mepol_amd.envs import GridWorldContinuous
    from mepol_amd.policy import GaussianPolicy

    dev = torch.device("cuda")
    n, T = args.num_traj, args.traj_len
    envs = {"gridworld": (1, None)}
    if not args.gridworld_only:
        from mepol_amd.envs import BoxMazeContinuous

        envs["maze-gridworld-7-walls"] = (2, ops.maze_struct(BoxMazeContinuous.gridworld()))
        envs["maze-16-walls"] = (2, ops.maze_struct(sixteen_walls()))
    g = torch.Generator(device=dev).manual_seed(0)
    init = GridWorldContinuous().reset_batch_torch(n, dev, g)
    noise = torch.randn((T, n, 2), dtype=torch.float64, device=dev, generator=g)
    states = torch.empty((n, T + 1, 2), dtype=torch.float32, device=dev)
    actions = torch.empty((n, T, 2), dtype=torch.float32, device=dev)
    rows = {}
    for hidden in ([300, 300], [300, 300, 300]):
        torch.manual_seed(7)
        pol = GaussianPolicy(hidden, 2, 2, -1.5).to(dev)
        layers = [(m.weight.detach(), m.bias.detach()) for m in pol.net if isinstance(m, nn.Linear)]
        head = (pol.mean.weight.detach(), pol.mean.bias.detach(), pol.log_std.detach(), init, noise,
                states, actions)
        for name, (env_id, mz) in envs.items():
            kw = {} if mz is None else dict(maze=mz)

            def launch():
                if len(layers) == 2:
                    ops.rollout_mlp(env_id, *layers[0], *layers[1], *head, **kw)
                else:
                    ops.rollout_deep(env_id, layers, *head, **kw)

            ms = []
            for r in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                launch()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            row = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
                   "us_per_step": statistics.median(ms) * 1e3 / T,
                   "min_us_per_step": min(ms) * 1e3 / T, "samples": len(ms)}
            if len(layers) == 2:
                row["plan"] = (ops.rollout_mlp_plan(n, *hidden, 2) if env_id == 1
                               else ops.rollout_mlp_plan(n, *hidden, 2, env_id=env_id))
            rows[f"{'x'.join(map(str, hidden))}/{name}"] = row
            print(f"{'x'.join(map(str, hidden)):>12} {name:<24} {row['us_per_step']:.3f} us/step "
                  f"(min {row['min_us_per_step']:.3f})", flush=True)
    result = {"shape": {"num_traj": n, "traj_len": T},
              "library": "MEPOL_AMD_LIB" if os.environ.get("MEPOL_AMD_LIB") else "this tree",
              "run": {"reps": args.reps, "warmup": args.warmup},
              "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
