"""Time mepol_critic_fit's launch alone (device events) at two step counts per shape; the slope
is the time per Adam step.  Prints one JSON list (the format of
profiles/r17/critic_fit/critic_kernel_bench.json).

    python tools/critic_kernel_bench.py [--reps 9] [--out FILE]

MEPOL_AMD_LIB selects the library under test, as everywhere.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = ((2, 64, 64, 64), (2, 64, 64, 16), (2, 16, 16, 64), (2, 16, 16, 16), (16, 64, 64, 64),
          (2, 32, 32, 32))
STEPS = (1875, 3750)


def measure(nf, h0, h1, B, n_steps, reps):
    from mepol_amd import ops
    from mepol_amd._lib import call, ptr

    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(nf + 17 * h0 + 257 * h1 + 4099 * B)
    f64 = dict(dtype=torch.float64, generator=g)
    N = 24000
    states, targets = torch.rand(N, nf, **f64).to(dev), torch.randn(N, **f64).to(dev)
    index = torch.randint(0, N, (n_steps * B,), generator=g).to(torch.int32).to(dev)
    shapes = [(h0, nf), (h0,), (h1, h0), (h1,), (1, h1), (1,)]
    start = [((torch.rand(s, **f64) * 2 - 1) / (s[-1] ** 0.5 if len(s) > 1 else 4.0)).to(dev)
             for s in shapes]
    p, m, v = ([torch.zeros_like(t) for t in start] for _ in range(3))
    scal = ops.adam_step_scalars(1e-2, (0.9, 0.999), 1, n_steps).to(dev)
    loss = torch.empty(n_steps, dtype=torch.float64, device=dev)
    arr = ctypes.c_void_p * 6
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(reps + 2):
        for t, s in zip(p, start):
            t.copy_(s)
        for t in m + v:
            t.zero_()
        e0.record()
        call("mepol_critic_fit", ptr(states), ptr(targets), N, ptr(index), n_steps, B, nf, h0, h1,
             arr(*[t.data_ptr() for t in p]), arr(*[t.data_ptr() for t in m]),
             arr(*[t.data_ptr() for t in v]), ptr(scal), 0.9, 0.999, 1e-8, ptr(loss),
             ops._stream())
        e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            ms.append(e0.elapsed_time(e1))
    assert bool(torch.isfinite(loss).all())
    return {"nf": nf, "h0": h0, "h1": h1, "B": B, "n_steps": n_steps,
            "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for shape in SHAPES:
        a, b = (measure(*shape, n, args.reps) for n in STEPS)
        slope = (b["median_ms"] - a["median_ms"]) / (b["n_steps"] - a["n_steps"]) * 1e3
        rows.append({"a": a, "b": b, "us_per_step_slope": slope,
                     "fixed_ms": a["median_ms"] - slope * 1e-3 * a["n_steps"]})
    text = json.dumps(rows, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps([{"shape": [r["a"][k] for k in ("nf", "h0", "h1", "B")],
                       "us_per_step": round(r["us_per_step_slope"], 3)} for r in rows]))


if __name__ == "__main__":
    main()
