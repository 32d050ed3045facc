"""tools/kloop_schedule.py on wgrad_kernel (no GPU: device code is only compiled): the pinned
ring_k_loop keeps its load lookahead in the compiled code."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location(
        "kloop_schedule", os.path.join(ROOT, "tools", "kloop_schedule.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wgrad_steady_state_keeps_its_lookahead():
    ks = _tool()
    kernels = ks.kernels(ks.compile_asm(os.path.join(ROOT, "mepol_amd", "csrc", "wgrad.hip"), []))
    sym = [s for s in kernels if "wgrad_kernel" in s and "reduce" not in s]
    assert len(sym) == 1, sorted(kernels)
    body, meta = kernels[sym[0]]
    assert int(meta["vgpr_count"]) <= 256 and int(meta["vgpr_spill_count"]) == 0, meta
    loops = [ks.summarize(body[a:b + 1]) for a, b, _, inner in ks.loops(body) if inner]
    steady = [r for r in loops if sum(n for c, n in r if c == "mfma") == 40]  # NS = 2 stages x 20
    assert len(steady) == 1, loops
    # stage by stage: the nine loads of the next stage, then 20 MFMAs whose waits leave at
    # least those nine loads outstanding
    seq = "".join("L" * n if c.startswith("global_load") else "M" * n if c == "mfma" else ""
                  for c, n in steady[0])
    assert seq == ("L" * 9 + "M" * 20) * 2, seq
    waits = [int(m.group(1)) for c, _ in steady[0] for m in [re.search(r"vmcnt\((\d+)\)", c)] if m]
    assert waits and min(waits) >= 9, waits
