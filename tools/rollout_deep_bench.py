"""Rollout time per step of policies with three to six hidden layers on GridWorld 20 x 1200 and
MountainCar 20 x 400 (and 200 trajectories at [300, 300, 300]): the one-launch kernel
(csrc/rollout_deep.hip) against the replayed per-step graph (_RolloutGraph,
MEPOL_ROLLOUT_FUSED=0) and the eager per-step loop (MEPOL_ROLLOUT_GRAPH=0 as well).

    python tools/rollout_deep_bench.py                  every shape; one JSON line per shape
    python tools/rollout_deep_bench.py --sweep          GridWorld 20 x 1200 at growing weight
                                                        counts, for the crossover with the graph
    python tools/rollout_deep_bench.py --kernel-only    the kernel variant alone, 1 + REPS calls
                                                        per shape in the order of SHAPES, to be
                                                        run under rocprofv3 --kernel-trace --stats
    python tools/rollout_deep_bench.py --summarise DB   kernel mean per shape from that run's
                                                        rocprofv3 database (kernels view)

us per step = the time of one collect_particles_device call (initial states and noise drawn,
all T steps, the particle tensors returned) by device events, over T.  Every variant of a shape
is warmed up first (kernel code, workspaces, the graph capture); then the variants alternate,
REPS times each, in one process.  spread_us = max - min of a variant's repetitions.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 3
# (env, hidden sizes, trajectories, steps)
SHAPES = [(env, hid, nt, T)
          for env, T in (("GridWorld", 1200), ("MountainCar", 400))
          for hid, nt in (([300, 300, 300], 20), ([400, 300, 300], 20), ([512] * 6, 20),
                          ([300, 300, 300], 200))]
# between [400, 300, 300] (210k weight words per step) and [512] x 6 (1311k)
SWEEP = [("GridWorld", hid, 20, 1200)
         for hid in ([512] * 3, [384] * 6, [512] * 4, [448] * 6, [512] * 5)]
# (the kernel is timed at every shape, also those the eligibility rule keeps from it)
VARIANTS = {"kernel": {"MEPOL_ROLLOUT_FUSED": "1", "MEPOL_ROLLOUT_GRAPH": "1",
                       "MEPOL_ROLLOUT_DEEP_MAX_WORDS": str(1 << 30)},
            "graph": {"MEPOL_ROLLOUT_FUSED": "0", "MEPOL_ROLLOUT_GRAPH": "1"},
            "eager": {"MEPOL_ROLLOUT_FUSED": "0", "MEPOL_ROLLOUT_GRAPH": "0"}}


def weight_words(hid):
    """Words of W_2^T .. W_L^T, the weights the kernel reads per step and trajectory."""
    return sum(a * b for a, b in zip(hid[:-1], hid[1:]))


def run(variants, shapes):
    sys.path.insert(0, HERE)
    import torch

    from mepol_amd.algorithms import mepol as M
    from mepol_amd.experiments.mepol import exp_specs
    from mepol_amd.policy import GaussianPolicy

    for env_name, hid, nt, T in shapes:
        spec = exp_specs()[env_name]
        env = spec["env_create"]()
        torch.manual_seed(0)
        pol = GaussianPolicy(hid, 2, env.action_space.shape[0], spec["log_std_init"]).cuda()

        def once(variant):
            os.environ.update(VARIANTS[variant])
            g = torch.Generator(device="cuda").manual_seed(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = M.collect_particles_device(env, pol, nt, T, None, generator=g)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / T, out

        outs = {v: once(v)[1] for v in variants}  # warm-up of every variant of this shape
        row = {"env": env_name, "hidden": hid, "nt": nt, "T": T, "weight_words": weight_words(hid)}
        if "kernel" in outs and "eager" in outs:
            row["max_action_diff_vs_eager"] = (outs["kernel"][1] - outs["eager"][1]).abs().max().item()
        us = {v: [] for v in variants}
        for _ in range(REPS):
            for v in variants:
                us[v].append(once(v)[0])
        for v in variants:
            row[f"{v}_us_per_step"] = sorted(us[v])[len(us[v]) // 2]
            row[f"{v}_spread_us"] = max(us[v]) - min(us[v])
            row[f"{v}_samples_us"] = us[v]
        print(json.dumps(row), flush=True)
        M._ROLLOUT_GRAPHS.pop(pol, None)


def summarise(db):
    """The rollout_deep_kernel dispatches of a --kernel-only run, in dispatch order: 1 + REPS per
    shape, the first of each (the warm-up) dropped."""
    import sqlite3

    c = sqlite3.connect(db)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    name = "kernel_name" if "kernel_name" in cols else "name"
    rows = [(s, e - s) for n, s, e in c.execute(f"select {name}, start, end from kernels")
            if "rollout_deep_kernel" in n]
    durs = [d for _, d in sorted(rows)]
    if len(durs) != len(SHAPES) * (1 + REPS):
        sys.exit(f"{len(durs)} rollout_deep_kernel dispatches, expected {len(SHAPES) * (1 + REPS)}")
    for q, (env_name, hid, nt, T) in enumerate(SHAPES):
        d = durs[q * (1 + REPS) + 1:(q + 1) * (1 + REPS)]
        print(json.dumps({"env": env_name, "hidden": hid, "nt": nt, "T": T,
                          "kernel_mean_ms": sum(d) / len(d) / 1e6,
                          "kernel_mean_us_per_step": sum(d) / len(d) / 1e3 / T,
                          "kernel_ms": [x / 1e6 for x in d]}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kernel-only", action="store_true")
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--summarise", metavar="DB", default=None)
    a = p.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    run(["kernel"] if a.kernel_only else list(VARIANTS), SWEEP if a.sweep else SHAPES)


if __name__ == "__main__":
    sys.exit(main())
