#!/usr/bin/env python3
"""Kernel time of the exact re-rank (`OriginalVectors.rerank_batch`) with f32, f16 and bf16 originals: 1M x 768 rows,
256 queries x 1024 uniformly random ids, everything resident on the device.  The times are those of the pair kernels
(`f32_pairs_kernel`, `half_pairs_kernel`) in a `rocprofv3 --kernel-trace --stats` run that this tool starts itself
(a fresh child process: the program goes right after `--`); the three stores are called in turn, warm, REPS times.

    python tools/time_rescore.py [--rows 1000000] [--dim 768] [--queries 256] [--ids 1024] [--reps 7] [--out FILE]

Pass condition printed at the end: a half kernel may be slower than the f32 kernel by at most the larger of 5 % and the
run-to-run spread ((max - min) / median over the repetitions, the largest of the three kernels')."""
import argparse
import csv
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("f32", "f16", "bf16")
WARMUP = 2


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--ids", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7, help="timed repetitions per store (at least 5)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


def child(a):
    """The profiled program: the three stores in turn, WARMUP + reps calls each."""
    sys.path.insert(0, ROOT)
    import torch

    import quantization_amd as qa

    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randn((a.rows, a.dim), device="cuda", generator=g)
    vp = qa.VectorParameters(a.dim, a.rows, qa.DistanceType.Dot, False)
    tensors = {"f32": data, "f16": data.to(torch.float16), "bf16": data.to(torch.bfloat16)}
    stores = {kind: qa.OriginalVectors.from_data(t, vp, borrow=True, dtype=kind) for kind, t in tensors.items()}
    queries = torch.randn((a.queries, a.dim), device="cuda", generator=g)
    ids = torch.randint(0, a.rows, (a.queries, a.ids), device="cuda", generator=g, dtype=torch.int32)
    oi = torch.empty((a.queries, a.k), dtype=torch.int32, device="cuda")
    osc = torch.empty((a.queries, a.k), device="cuda")
    for _ in range(WARMUP + a.reps):
        for kind in KINDS:
            stores[kind].rerank_batch(queries, ids, a.k, True, out_ids=oi, out_scores=osc)
            torch.cuda.synchronize()
    print("CHILD DONE")


def kind_of(kernel_name):
    """Which store a pair kernel of csrc/f32.hip serves, from its (demangled or mangled) name."""
    if "f32_pairs_kernel" in kernel_name:
        return "f32"
    m = re.search(r"half_pairs_kernel<\d+, *(\d+)", kernel_name) or re.search(r"half_pairs_kernelILi\d+ELi(\d+)E", kernel_name)
    if m:
        return {"1": "f16", "2": "bf16"}.get(m.group(1))
    return None


def main():
    a = parse_args()
    if a.child:
        return child(a)
    if a.reps < 5:
        sys.exit("--reps must be at least 5")
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "k", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows), "--dim", str(a.dim),
               "--queries", str(a.queries), "--ids", str(a.ids), "--k", str(a.k), "--reps", str(a.reps)]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if res.returncode != 0 or "CHILD DONE" not in res.stdout:
            sys.exit("the profiled run failed:\n" + (res.stdout + res.stderr)[-3000:])
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            sys.exit("rocprofv3 wrote no kernel trace")
        rows = [r for t in traces for r in csv.DictReader(open(t))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    times = {kind: [] for kind in KINDS}
    names = {}
    for r in rows:
        kind = kind_of(r["Kernel_Name"])
        if kind:
            times[kind].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            names[kind] = r["Kernel_Name"]
    esize = {"f32": 4, "f16": 2, "bf16": 2}
    pairs = a.queries * a.ids
    lines = [f"rerank_batch pair kernels, {a.rows} x {a.dim} rows, {a.queries} queries x {a.ids} random ids, device resident; "
             f"rocprofv3 --kernel-trace, {WARMUP} warm-up + {a.reps} timed dispatches per store, the stores called in turn"]
    med, spread = {}, {}
    for kind in KINDS:
        t = times[kind][WARMUP:]
        if len(t) != a.reps:
            sys.exit(f"{kind}: {len(times[kind])} dispatches in the trace, expected {WARMUP + a.reps} ({names.get(kind)})")
        med[kind] = statistics.median(t)
        spread[kind] = (max(t) - min(t)) / med[kind]
        gathered = pairs * a.dim * esize[kind]
        lines.append(f"{kind:5s} resident {a.rows * a.dim * esize[kind] / 1e9:6.3f} GB  median {med[kind]:9.1f} us  min {min(t):9.1f}  "
                     f"max {max(t):9.1f}  spread {100 * spread[kind]:4.1f} %  gathered {gathered / 1e6:7.1f} MB = "
                     f"{gathered / med[kind] / 1e6:6.3f} TB/s  all: {' '.join('%.1f' % x for x in t)}")
        lines.append(f"      kernel: {names[kind][:150]}")
    margin = max(0.05, max(spread.values()))
    ok = True
    for kind in ("f16", "bf16"):
        ratio = med[kind] / med["f32"]
        passed = ratio <= 1 + margin
        ok &= passed
        lines.append(f"{kind} / f32 = {ratio:.3f} ({'faster' if ratio < 1 else 'slower'} by {100 * abs(1 - ratio):.1f} %); allowed "
                     f"up to {1 + margin:.3f} (larger of 5 % and the spread {100 * max(spread.values()):.1f} %): "
                     f"{'PASS' if passed else 'FAIL'}")
    report = "\n".join(lines)
    print(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
