"""Time of one Fisher-vector product (PolicyFisher.hvp) and of one whole trpo_step: the HIP
kernel path against the reference's method on the same GPU, i.e. the module's own double-backward
fallback forced by MEPOL_FVP_MIN_ROWS (the only correct alternative; GaussianPolicy's large-batch
paths are not twice differentiable).

    python tools/trpo_step_bench.py                 the whole sweep, one JSON line per row, then
                                                    a table and the floor these runs give
    python tools/trpo_step_bench.py --rows 500 2000 --policies gw

Policies: gw = 2 -> [300, 300] -> 2 (GridGoal), ant = 29 -> [400, 300] -> 8.  Rows: SWEEP_N.
Both paths run in this one process, alternating per repetition, after a warm-up of each.  An hvp
sample is a window of HVP_WINDOW products between two device events (ms per product); a
trpo_step sample is one step from the same initial parameters between two device events (the
step reads two scalars per backtracking trial on the host, so its time includes those round
trips).  Reported: median [min, max] over --reps samples.  "wins" = the kernel path's slowest
sample is faster than the fallback's fastest one; the floor is the smallest n from which it wins
the hvp for both policies at every larger n too.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_N = [500, 2000, 8000, 50000, 200000]
POLICIES = {"gw": dict(NF=2, HID=[300, 300], A=2), "ant": dict(NF=29, HID=[400, 300], A=8)}
HVP_WINDOW = 20
KL_THRESH, CG_ITERS, CG_DAMPING = 0.01, 10, 0.1
FORCE = {"kernels": "1", "fallback": str(10 ** 12)}  # MEPOL_FVP_MIN_ROWS of each path


def _case(pol, n):
    import torch

    from mepol_amd.policy import GaussianPolicy

    c = POLICIES[pol]
    dev = torch.device("cuda")
    torch.manual_seed(7)
    policy = GaussianPolicy(c["HID"], c["NF"], c["A"]).to(dev)
    g = torch.Generator(device=dev).manual_seed(8)
    kw = dict(dtype=torch.float64, device=dev, generator=g)
    states = torch.randn(n, c["NF"], **kw)
    noise = torch.randn(n, c["A"], **kw)
    with torch.no_grad():
        actions = policy.mean_action(states) + noise * torch.exp(policy.log_std)
    adv = noise[:, 0] - 0.5 * noise[:, -1] + 0.25 * noise[:, 0] * noise[:, -1]
    v = torch.randn(sum(p.numel() for p in policy.parameters()), **kw)
    return policy, states, actions, adv, v


def _timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def measure_row(pol, n, reps):
    import torch

    from mepol_amd.algorithms import trpo

    policy, states, actions, adv, v = _case(pol, n)
    theta0 = {k: t.clone() for k, t in policy.state_dict().items()}
    fishers = {}
    for path, floor in FORCE.items():
        os.environ["MEPOL_FVP_MIN_ROWS"] = floor
        fishers[path] = trpo.PolicyFisher(policy, states, CG_DAMPING)
        assert fishers[path].kernels == (path == "kernels")
    diff = (fishers["kernels"].hvp(v) - fishers["fallback"].hvp(v)).abs().max().item()
    scale = fishers["fallback"].hvp(v).abs().max().item()

    def hvp_window(path):
        def run():
            for _ in range(HVP_WINDOW):
                out = fishers[path].hvp(v)
            return out
        return run

    def step(path):
        def run():
            os.environ["MEPOL_FVP_MIN_ROWS"] = FORCE[path]
            policy.load_state_dict(theta0)
            return trpo.trpo_step(policy, states, actions, adv, KL_THRESH, CG_ITERS, CG_DAMPING)
        return run

    hvp_ms = {p: [] for p in FORCE}
    step_ms = {p: [] for p in FORCE}
    outcome = {}
    for path in FORCE:  # warm-up of every shape the timed windows use
        _timed(hvp_window(path))
        _timed(step(path))
    for _ in range(reps):
        for path in FORCE:
            hvp_ms[path].append(_timed(hvp_window(path))[0] / HVP_WINDOW)
        for path in FORCE:
            ms, outcome[path] = _timed(step(path))
            step_ms[path].append(ms)
    del fishers
    torch.cuda.empty_cache()
    return {"row": f"{pol}/{n}", "hvp_ms": hvp_ms, "step_ms": step_ms,
            "step_outcome": {p: [bool(o[0]), int(o[1])] for p, o in outcome.items()},
            "hvp_rel_diff": diff / scale}


def _cell(ms):
    s = sorted(ms)
    return f"{s[len(s) // 2]:9.3f} [{s[0]:.3f}, {s[-1]:.3f}]"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, nargs="*", default=SWEEP_N)
    p.add_argument("--policies", nargs="*", default=list(POLICIES), choices=list(POLICIES))
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    sys.path.insert(0, HERE)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("trpo_step_bench: no GPU; there is nothing to measure on a CPU")
    rows = []
    for pol in a.policies:
        for n in a.rows:
            r = measure_row(pol, n, a.reps)
            rows.append(r)
            print(json.dumps(r), flush=True)
    head = f"{'row':12s} {'what':5s} {'kernels ms':>30s} {'fallback ms':>30s} {'ratio':>6s}  wins"
    print(head)
    wins = {}
    for r in rows:
        for what in ("hvp", "step"):
            k, f = r[f"{what}_ms"]["kernels"], r[f"{what}_ms"]["fallback"]
            won = max(k) < min(f)
            if what == "hvp":
                wins[r["row"]] = won
            ratio = sorted(f)[len(f) // 2] / sorted(k)[len(k) // 2]
            print(f"{r['row']:12s} {what:5s} {_cell(k):>30s} {_cell(f):>30s} {ratio:6.2f}  "
                  f"{'yes' if won else 'no'}")
    floor = None
    for n in sorted(a.rows, reverse=True):
        if not all(wins.get(f"{pol}/{n}") for pol in a.policies):
            break
        floor = n
    print(f"floor from these runs: {floor}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
