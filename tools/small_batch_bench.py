"""Off-policy iteration time of batches under 16384 rows: this tree (HIP kernels and the graph
loop from policy.FUSED_MIN_ROWS rows) against another checkout, whose path for these batches is
nn.Linear on rocBLAS under autograd with one host round trip per iteration.

    python tools/small_batch_bench.py                   one pass over the sweep on this tree,
                                                        one JSON line per row
    python tools/small_batch_bench.py --compare DIR     DIR holds the other checkout's mepol_amd/
                                                        package; after one warm-up process per tree,
                                                        fresh child processes alternate between
                                                        the two trees (--reps each); a table and
                                                        the floor the runs give at the end
    python tools/small_batch_bench.py --loop-only       the MountainCar-script loop alone (--n
                                                        rows, default 8000; 2 -> [300, 300] -> 1,
                                                        k = 4), for rocprofv3 --kernel-trace --stats

Rows: N in SWEEP_N (20 trajectories of N / 20 steps) for 2 -> [300, 300] -> 1 at k = 4 and
29 -> [400, 300] -> 8 at k = 30, the deep policy 2 -> [300, 300, 300] -> 1 at N = 8000, and the
whole epoch of scripts/tae/mountain_car.sh (20 x 400 particles: rollout, k-NN, CSR, the loop of
up to 30 iterations with its KL test and backtracking, final entropy).

ms per accepted iteration = (t(24 iterations) - t(4 iterations)) / 20, both
off_policy_optimization calls timed by device events (every step accepted: kl_threshold 1e9),
so the per-epoch set-up and the final entropy pass cancel.  Both trees load this tree's library
(MEPOL_AMD_LIB).  MEPOL_FUSED_MIN_ROWS=1 is set for the children, so that every row of this tree
runs the new path whatever the committed floor is; the other tree does not read it.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_N = [500, 1000, 2000, 4000, 8000, 12000]
POLICIES = {"mc": dict(NF=2, HID=[300, 300], A=1, K=4),
            "c3": dict(NF=29, HID=[400, 300], A=8, K=30),
            "deep": dict(NF=2, HID=[300, 300, 300], A=1, K=4)}
ROWS = [("mc", n) for n in SWEEP_N] + [("c3", n) for n in SWEEP_N] + [("deep", 8000)]
NT = 20
BASE_ITERS, ITERS = 4, 20
SAMPLES = 3


def _loop_case(pol, n):
    import numpy as np
    import scipy.special
    import torch

    from mepol_amd.algorithms import mepol as M
    from mepol_amd.policy import GaussianPolicy

    c = POLICIES[pol]
    NF, HID, A, K, T = c["NF"], c["HID"], c["A"], c["K"], n // NT
    rng = np.random.default_rng(5)
    states = rng.standard_normal((NT, T + 1, NF)).astype(np.float32)
    actions = (0.5 * rng.standard_normal((NT, T, A))).astype(np.float32)
    dev = torch.device("cuda")
    st = torch.as_tensor(states, dtype=torch.float64, device=dev)
    ac = torch.as_tensor(actions, dtype=torch.float64, device=dev)
    rtl = torch.full((NT, 1), T, dtype=torch.int64, device=dev)
    nxt = torch.as_tensor(states[:, 1:].reshape(-1, NF), device=dev)
    torch.manual_seed(5)
    beh = GaussianPolicy(HID, NF, A).to(dev)
    tgt = GaussianPolicy(HID, NF, A).to(dev)
    last = GaussianPolicy(HID, NF, A).to(dev)
    opt = torch.optim.Adam(tgt.parameters(), lr=1e-5)
    st, ac, rl, _, D, I = M.make_particle_batch(st, ac, rtl, nxt, K)
    G = float(scipy.special.gamma(NF / 2 + 1))
    B = float(np.log(K) - scipy.special.digamma(K))

    def epoch(iters):
        tgt.load_state_dict(beh.state_dict())
        last.load_state_dict(beh.state_dict())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        res = M.off_policy_optimization(opt, beh, tgt, last, st, ac, NT, rl, D, I, K, G, B, NF,
                                        0.0, 1e9, iters, False, 2, 4, 1e-5)
        e1.record()
        e1.synchronize()
        assert res[1] == iters, res
        return e0.elapsed_time(e1), float(res[0])

    return epoch, tgt


def _loop_name(tgt):
    from mepol_amd.algorithms import device_loop

    it = device_loop._CACHE.get(tgt)
    return type(it).__name__ if it is not None else "eager"


def measure_row(pol, n):
    epoch, tgt = _loop_case(pol, n)
    epoch(BASE_ITERS)  # warm-up: kernel code, allocator pools, the graph capture
    per_iter = []
    for _ in range(SAMPLES):
        short, _ = epoch(BASE_ITERS)
        long_, H = epoch(BASE_ITERS + ITERS)
        per_iter.append((long_ - short) / ITERS)
    return {"row": f"{pol}/{n}", "loop": _loop_name(tgt), "samples_ms": per_iter, "H": H}


def measure_epoch(epochs=6):
    """scripts/tae/mountain_car.sh's epoch as algorithms.mepol.mepol() runs it, by wall clock
    around a device synchronisation (the epoch has host work); the first epoch is the warm-up."""
    import numpy as np
    import scipy.special
    import torch

    from mepol_amd.algorithms import mepol as M
    from mepol_amd.envs import ErgodicEnv, MountainCarContinuous
    from mepol_amd.policy import GaussianPolicy

    torch.set_default_dtype(torch.float64)
    torch.manual_seed(3)
    np.random.seed(3)
    env = ErgodicEnv(MountainCarContinuous())
    env.seed(3)
    dev = torch.device("cuda")
    nt, T, K, lr, eps = 20, 400, 4, 1e-4, 1e-15
    beh, tgt, last = (GaussianPolicy([300, 300], env.num_features, 1, -0.5).to(dev)
                      for _ in range(3))
    tgt.load_state_dict(beh.state_dict())
    opt = torch.optim.Adam(tgt.parameters(), lr=lr)
    ns = env.num_features
    G = float(scipy.special.gamma(ns / 2 + 1))
    B = float(np.log(K) - scipy.special.digamma(K))
    times, iters = [], []
    for _ in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last.load_state_dict(beh.state_dict())
        st, ac, rl, _, D, I = M.collect_particles_and_compute_knn(env, beh, nt, T, None, K, 1)
        res = M.off_policy_optimization(opt, beh, tgt, last, st, ac, nt, rl, D, I, K, G, B, ns,
                                        eps, 15.0, 30, True, 2, 10, lr)
        H = float(res[0])
        beh.load_state_dict(last.state_dict())
        tgt.load_state_dict(last.state_dict())
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
        iters.append(res[1])
    return {"row": "mountaincar-epoch", "loop": _loop_name(tgt), "samples_ms": times[1:],
            "off_iters": iters[1:], "H": H}


def measure(root, rows):
    sys.path.insert(0, root)
    for pol, n in rows:
        print(json.dumps(dict(measure_row(pol, n), root=root)), flush=True)
    print(json.dumps(dict(measure_epoch(), root=root)), flush=True)


def loop_only(n):
    sys.path.insert(0, HERE)
    epoch, tgt = _loop_case("mc", n)
    epoch(BASE_ITERS)
    epoch(BASE_ITERS + ITERS)
    print(json.dumps({"loop": _loop_name(tgt)}))


def _child(root, env, warm=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root]
    if warm:
        cmd += ["--rows", "1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit(r.returncode)
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def compare(other, reps):
    env = dict(os.environ, MEPOL_AMD_LIB=os.path.join(HERE, "mepol_amd", "libmepol_amd.so"),
               MEPOL_FUSED_MIN_ROWS="1")
    roots = (HERE, os.path.abspath(other))
    for root in roots:  # warm-up: code objects and the libraries' caches of both trees
        _child(root, env, warm=True)
    rows = {}
    for _ in range(reps):
        for root in roots:
            for r in _child(root, env):
                print(json.dumps(r), flush=True)
                e = rows.setdefault(r["row"], {}).setdefault(root, {"loop": r["loop"], "ms": []})
                e["ms"] += r["samples_ms"]
    print(f"{'row':20s} {'this tree':>34s} {'other tree':>34s}  faster")
    faster = {}
    for name, by in rows.items():
        a, b = by[roots[0]], by[roots[1]]
        faster[name] = max(a["ms"]) < min(b["ms"])  # the run ranges do not overlap
        cell = lambda e: (f"{sorted(e['ms'])[len(e['ms']) // 2]:8.3f} [{min(e['ms']):.3f}, "
                          f"{max(e['ms']):.3f}] {e['loop'][:9]}")
        print(f"{name:20s} {cell(a):>34s} {cell(b):>34s}  {'yes' if faster[name] else 'no'}")
    floor = None
    for n in sorted(SWEEP_N, reverse=True):  # the smallest N with every larger one faster too
        if not (faster.get(f"mc/{n}") and faster.get(f"c3/{n}")):
            break
        floor = n
    print(f"floor from these runs: {floor}")
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default=HERE)
    p.add_argument("--rows", type=int, default=len(ROWS), help="only the first ROWS rows")
    p.add_argument("--compare", metavar="DIR", default=None)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--loop-only", action="store_true")
    p.add_argument("--n", type=int, default=8000, help="rows of --loop-only")
    a = p.parse_args()
    if a.loop_only:
        return loop_only(a.n)
    if a.compare is None:
        return measure(a.root, ROWS[:a.rows])
    return compare(a.compare, a.reps)


if __name__ == "__main__":
    sys.exit(main())
