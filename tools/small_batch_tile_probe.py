"""us per policy_forward call by row tile and n (device events over 100 calls)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mepol_amd import ops
from mepol_amd.policy import GaussianPolicy

for nf, hid, a in ((2, [300, 300], 1), (29, [400, 300], 8)):
    torch.manual_seed(0)
    pol = GaussianPolicy(hid, nf, a).cuda()
    P = (pol.net[0].weight.detach(), pol.net[0].bias.detach(), pol.net[2].weight.detach(),
         pol.net[2].bias.detach(), pol.mean.weight.detach(), pol.mean.bias.detach(),
         pol.log_std.detach())
    for n in (500, 1000, 2000, 4000, 6000, 8000, 8160, 10000, 12000, 14000, 16320):
        s = torch.randn(n, nf, dtype=torch.float64, device="cuda")
        act = torch.randn(n, a, dtype=torch.float64, device="cuda")
        bufs = [torch.empty((n, hid[0]), dtype=torch.float64, device="cuda"),
                torch.empty((n, hid[1]), dtype=torch.float64, device="cuda"),
                torch.empty((n, a), dtype=torch.float64, device="cuda"),
                torch.empty(n, dtype=torch.float64, device="cuda")]
        row = []
        for t in (64, 32, 16):
            for _ in range(10):
                ops.policy_forward(s, *P, act, *bufs, row_tile=t)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                ops.policy_forward(s, *P, act, *bufs, row_tile=t)
            e1.record()
            e1.synchronize()
            row.append(e0.elapsed_time(e1) * 10)
        print(f"nf={nf} n={n:6d} auto={ops.policy_forward_plan(n, nf, hid[0], hid[1])['row_tile']:2d} "
              f"us/call tile64={row[0]:7.1f} tile32={row[1]:7.1f} tile16={row[2]:7.1f}", flush=True)
