"""us per gemm_nt call (bias + ReLU), variants 0 and 2, at the deep policy's small-batch shapes."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mepol_amd import ops

for n in (500, 2000, 4000, 8000, 12000, 16383):
    for k, m in ((300, 300), (64, 48)):
        A = torch.randn(n, k, dtype=torch.float64, device="cuda")
        B = torch.randn(m, k, dtype=torch.float64, device="cuda")
        b = torch.randn(m, dtype=torch.float64, device="cuda")
        out = torch.empty(n, m, dtype=torch.float64, device="cuda")
        row, res = [], []
        for v in (0, 2):
            for _ in range(10):
                ops.gemm_nt(A, B, bias=b, relu=True, out=out, variant=v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                ops.gemm_nt(A, B, bias=b, relu=True, out=out, variant=v)
            e1.record()
            e1.synchronize()
            row.append(e0.elapsed_time(e1) * 10)
            res.append(out.clone())
        print(f"n={n:6d} k={k} m={m} helper={ops.gemm_nt_variant(n, m)} us/call v0={row[0]:7.1f} "
              f"v2={row[1]:7.1f} same_bits={torch.equal(res[0], res[1])}", flush=True)
