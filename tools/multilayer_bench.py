"""Off-policy iteration time of a three-hidden-layer policy, 29 -> [400, 300, 300] -> 8 at
N = 200k particles and k = 30: this tree's graph loop (algorithms/device_loop.py,
MultiLayerIteration) against another checkout's path for the same policy.

    python tools/multilayer_bench.py                      one measurement of this tree, one JSON line
    python tools/multilayer_bench.py --compare DIR        DIR holds the other checkout's mepol_amd/
                                                          package; fresh child processes alternate
                                                          between the two trees (--reps each)
    python tools/multilayer_bench.py --kernel OUT IN      mepol_hidden_backward alone at
                                                          (200k, OUT, IN), for a kernel trace

ms per accepted iteration = (t(A + ITERS iterations) - t(A iterations)) / ITERS with both
off_policy_optimization calls timed by device events (every step accepted: kl_threshold 1e9),
so the per-epoch set-up and the final entropy pass cancel.  The other tree loads this tree's
library (MEPOL_AMD_LIB): the kernels it uses are unchanged.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT, T, NF, A, K, HID = 400, 500, 29, 8, 30, [400, 300, 300]
BASE_ITERS, ITERS = 4, 20


def measure(root):
    sys.path.insert(0, root)
    import numpy as np
    import scipy.special
    import torch

    from mepol_amd.algorithms import device_loop
    from mepol_amd.algorithms import mepol as M
    from mepol_amd.policy import GaussianPolicy

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

    epoch(BASE_ITERS)  # warm-up: kernel code, allocator pools, the graph capture
    per_iter = []
    for _ in range(3):
        short, _ = epoch(BASE_ITERS)
        long_, H = epoch(BASE_ITERS + ITERS)
        per_iter.append((long_ - short) / ITERS)
    it = device_loop._CACHE.get(tgt)
    print(json.dumps({"root": root, "loop": type(it).__name__ if it is not None else "eager",
                      "ms_per_iteration": sorted(per_iter)[1], "samples_ms": per_iter,
                      "iters": ITERS, "H": H}))


def kernel_only(out_f, in_f, n=NT * T, calls=10):
    sys.path.insert(0, HERE)
    import torch

    from mepol_amd import ops

    g = torch.Generator(device="cuda").manual_seed(0)
    kw = dict(dtype=torch.float64, device="cuda", generator=g)
    dz, W = torch.randn(n, out_f, **kw), torch.randn(out_f, in_f, **kw)
    h = torch.relu(torch.randn(n, in_f, **kw))
    ws = ops.hidden_backward_workspace(n, in_f, dz.device)
    out = torch.empty((n, in_f), dtype=torch.float64, device="cuda")
    db = torch.empty(in_f, dtype=torch.float64, device="cuda")
    for _ in range(calls):
        ops.hidden_backward(dz, W, h, ws=ws, dz_out_buf=out, db_out=db)
    torch.cuda.synchronize()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default=HERE)
    p.add_argument("--compare", metavar="DIR", default=None)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--kernel", type=int, nargs=2, metavar=("OUT", "IN"), default=None)
    a = p.parse_args()
    if a.kernel:
        return kernel_only(*a.kernel)
    if a.compare is None:
        return measure(a.root)
    env = dict(os.environ, MEPOL_AMD_LIB=os.path.join(HERE, "mepol_amd", "libmepol_amd.so"))
    rows = []
    for _ in range(a.reps):
        for root in (HERE, os.path.abspath(a.compare)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root],
                               env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                return r.returncode
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[-1]), flush=True)
    for root in (HERE, os.path.abspath(a.compare)):
        ms = [r["ms_per_iteration"] for r in rows if r["root"] == root]
        loop = next(r["loop"] for r in rows if r["root"] == root)
        print(f"{loop:22s} {sum(ms) / len(ms):8.3f} ms / iteration  (runs: "
              + ", ".join(f"{m:.3f}" for m in ms) + f")  {root}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
