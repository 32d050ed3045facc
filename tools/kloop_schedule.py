#!/usr/bin/env python3
"""Issue order of a kernel's innermost loops in the compiled gfx950 code.

    python tools/kloop_schedule.py mepol_amd/csrc/wgrad.hip wgrad_kernel
    python tools/kloop_schedule.py mepol_amd/csrc/gemm.hip dh1_layer1_bwd_kernel --all-loops

Compiles one source file to assembly with the Makefile's flags (device code only, no GPU
needed) and, for every kernel whose demangled name contains the given text, prints the VGPR,
AGPR and spill counts and a run-length summary, in program order, of the instructions that
decide the latency hiding of a K loop: global loads, LDS reads and writes, barriers, s_waitcnt
values and MFMA runs.  Every other instruction is left out.  It reports instruction order and
register counts and nothing else: what an order costs is measured on the GPU.

A loop is a backward branch to a label inside the kernel; an innermost loop holds no other.
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_flags(stem):
    """FLAGS and FLAGS_<stem> of the Makefile, variables expanded."""
    var = {}
    with open(os.path.join(ROOT, "Makefile")) as f:
        for line in f:
            m = re.match(r"^(\w+)\s*(\?=|:=|=)\s*(.*)$", line.rstrip("\n"))
            if m:
                var[m.group(1)] = m.group(3)

    def expand(s, depth=0):
        if depth > 8:
            return s
        return re.sub(r"\$\((\w+)\)", lambda m: expand(var.get(m.group(1), ""), depth + 1), s)

    hipcc = os.environ.get("HIPCC", expand(var.get("HIPCC", "hipcc")))
    flags = expand(var.get("FLAGS", "")).split() + expand(var.get("FLAGS_" + stem, "")).split()
    return hipcc, flags


def compile_asm(src, extra):
    stem = os.path.splitext(os.path.basename(src))[0]
    hipcc, flags = makefile_flags(stem)
    cmd = [hipcc] + flags + extra + ["-I" + os.path.join(ROOT, "include"), "--cuda-device-only",
                                     "-S", src, "-o", "-"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("compile failed: %s\n%s" % (" ".join(cmd), r.stderr))
    return r.stdout


def demangle(names):
    filt = os.path.join(os.path.dirname(makefile_flags("")[0]), "..", "llvm", "bin", "llvm-cxxfilt")
    for exe in (filt, "llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([exe] + names, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                               text=True)
        except OSError:
            continue
        out = r.stdout.split("\n")[:len(names)]
        if r.returncode == 0 and len(out) == len(names):
            return dict(zip(names, out))
    return {n: n for n in names}


def kernels(asm):
    """{symbol: (body lines, metadata dict)} for every kernel of the assembly."""
    lines = asm.split("\n")
    syms = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", x) for x in lines) if m]
    meta, cur = {}, None
    for x in lines:  # the amdhsa.kernels YAML: entries start at .agpr_count / end at .wavefront_size
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)\s*$", x)
        if not m:
            continue
        if x.lstrip().startswith("- .agpr_count") or cur is None:
            cur = {}
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "name" and m.group(2) in syms:
            meta[m.group(2)] = cur
    out = {}
    for s in syms:
        a = next((i for i, x in enumerate(lines) if x.startswith(s + ":")), None)
        if a is None:
            continue
        b = a
        while b < len(lines) and not lines[b].startswith(".Lfunc_end"):
            b += 1
        out[s] = (lines[a + 1:b], meta.get(s, {}))
    return out


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("global_load") or op.startswith("buffer_load") or op.startswith("flat_load"):
        return op
    if op.startswith("global_store") or op.startswith("buffer_store") or op.startswith("flat_store"):
        return op
    if op.startswith("scratch_"):
        return op
    if re.match(r"ds_(read|load)", op):
        return "lds_read(%s)" % op
    if re.match(r"ds_(write|store)", op):
        return "lds_write(%s)" % op
    if op == "s_barrier":
        return "s_barrier"
    if op == "s_waitcnt":
        return "s_waitcnt " + " ".join(ins.split()[1:])
    return None


def summarize(body):
    """Run-length list of the classified instructions of a range of lines."""
    runs = []
    for x in body:
        x = x.split(";")[0].strip()
        if not x or x.startswith(".") or x.endswith(":"):
            continue
        c = classify(x)
        if c is None:
            continue
        if runs and runs[-1][0] == c and not c.startswith("s_waitcnt"):
            runs[-1][1] += 1
        else:
            runs.append([c, 1])
    return runs


def loops(body):
    """(first line, last line, label) of every loop, innermost flagged."""
    label_at = {}
    for i, x in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", x)
        if m:
            label_at[m.group(1)] = i
    found = []
    for i, x in enumerate(body):
        m = re.match(r"\s*s_c?branch\S*\s+(\.LBB\d+_\d+)", x)
        if m and m.group(1) in label_at and label_at[m.group(1)] <= i:
            found.append((label_at[m.group(1)], i, m.group(1)))
    # one loop per header: the widest range of its back edges
    by_head = {}
    for a, b, lab in found:
        by_head[a] = (a, max(b, by_head.get(a, (a, b, lab))[1]), lab)
    res = sorted(by_head.values())
    inner = [not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in res) for l in res]
    return [(a, b, lab, f) for (a, b, lab), f in zip(res, inner)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("source", help="a .hip file of mepol_amd/csrc (or a copy of one)")
    ap.add_argument("kernel", help="text the demangled kernel name must contain")
    ap.add_argument("--all-loops", action="store_true", help="outer loops too")
    ap.add_argument("--min-mfma", type=int, default=1,
                    help="leave out loops with fewer MFMAs than this (default 1)")
    ap.add_argument("-X", dest="extra", action="append", default=[],
                    help="one more compiler flag (repeatable), e.g. -X=-DNAME=1")
    a = ap.parse_args()
    ks = kernels(compile_asm(a.source, a.extra))
    names = demangle(list(ks))
    hit = [s for s in ks if a.kernel in names[s]]
    if not hit:
        sys.exit("no kernel matches %r; kernels: %s" % (a.kernel, ", ".join(sorted(names.values()))))
    for s in hit:
        body, meta = ks[s]
        print("kernel %s" % names[s])
        print("  vgpr %s  agpr %s  vgpr_spill %s  sgpr_spill %s  scratch_bytes %s  lds_bytes %s" % (
            meta.get("vgpr_count", "?"), meta.get("agpr_count", "?"),
            meta.get("vgpr_spill_count", "?"), meta.get("sgpr_spill_count", "?"),
            meta.get("private_segment_fixed_size", "?"), meta.get("group_segment_fixed_size", "?")))
        for first, last, lab, inner in loops(body):
            if not (inner or a.all_loops):
                continue
            runs = summarize(body[first:last + 1])
            nm = sum(n for c, n in runs if c == "mfma")
            if nm < a.min_mfma:
                continue
            print("  %s loop %s (%d lines, %d mfma)" % ("innermost" if inner else "outer", lab,
                                                      last - first + 1, nm))
            for c, n in runs:
                print("    %s" % (c if c.startswith("s_waitcnt") or n == 1 and c == "s_barrier"
                                  else "%-3d x %s" % (n, c)))
        print()


if __name__ == "__main__":
    main()
