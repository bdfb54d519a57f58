#!/usr/bin/env python3
"""What a rotated scalar-u8 store costs, each call next to its yardstick, with HIP events around whole calls,
the median of `--reps` after a pre-warm (the method of tools/time_bin_rotated.py).

    python tools/time_u8_rotated.py [--rows 10000000] [--dim 768] [--reps 5] [--parent-lib PATH] [--out profiles/u8_rotated.txt]

    encode                 the rotated encode (min/max) of device data against the plain encode of the same data - by this
                           build and, with --parent-lib, by another build of the library (the parent commit's), which a
                           child process of this tool loads and times before this process touches the GPU
    encode, given interval the same with alpha_offset given: pass 2 alone (RotQuantizeSink in the rotation frame against quantize16_kernel)
    score_all, topk(30)    on the rotated store against the plain store: the kernels are the same, so a gap beyond the
                           run-to-run spread is a routing mistake to find
    encode_query           a host query against the rotated and the plain handle

Nothing here is a pass condition.  Fewer rows are taken when the device has less memory than the data and two stores need."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def measure(pairs, reps, prewarm_seconds):
    """[(name, [times of run], what, [times of base] or None)] for (name, run, base or None, what) pairs."""
    import torch

    from time_bin_two_bit import timed

    t_end = time.perf_counter() + prewarm_seconds
    while time.perf_counter() < t_end:
        for _, run, base, _ in pairs:
            run()
            if base:
                base()
        torch.cuda.synchronize()
    out = []
    for name, run, base, what in pairs:
        t, tb = [], []
        for _ in range(reps):
            t.append(timed(run))
            if base:
                tb.append(timed(base))
        out.append((name, t, what, tb or None))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prewarm-seconds", type=float, default=2.0)
    ap.add_argument("--parent-lib", default="", help="another build of libquantization_amd.so whose plain encode is the yardstick")
    ap.add_argument("--plain-encode-only", action="store_true", help="(the child of --parent-lib) print the plain encodes' medians")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "u8_rotated.txt"))
    a = ap.parse_args()
    parent = None
    if a.parent_lib:  # first, and finished before this process opens the GPU
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-encode-only", "--rows", str(a.rows), "--dim",
                              str(a.dim), "--reps", str(a.reps), "--prewarm-seconds", str(a.prewarm_seconds)],
                             env=dict(os.environ, QAMD_LIB_PATH=os.path.abspath(a.parent_lib)), capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit(f"the --parent-lib run failed:\n{res.stdout[-2000:]}{res.stderr[-2000:]}")
        parent = [float(v) for v in res.stdout.strip().splitlines()[-1].split()]  # rows, then (median, min, max) twice
    import torch

    import quantization_amd as qa

    E = qa.EncodedVectorsU8
    dim = a.dim
    free, _ = torch.cuda.mem_get_info()
    rows = min(a.rows, int(free * 0.6) // (dim * 4 + 4 * (dim + 4)))
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randn((rows, dim), device="cuda", generator=g, dtype=torch.float32)
    vp = qa.VectorParameters(dim, rows, qa.DistanceType.Dot, False)
    plain = E.encode(data, vp)
    ao_p = (float(plain.metadata["alpha"]), float(plain.metadata["offset"]))
    if a.plain_encode_only:
        res = measure([("encode", lambda: E.encode(data, vp), None, ""),
                       ("encode, given interval", lambda: E.encode(data, vp, alpha_offset=ao_p), None, "")], a.reps, a.prewarm_seconds)
        print(rows, *(f"{f(t):.5f}" for _, t, _, _ in res for f in (statistics.median, min, max)))
        return
    rot = E.encode(data, vp, rotated=True)
    ao_r = (float(rot.metadata["alpha"]), float(rot.metadata["offset"]))
    import numpy as np

    query = np.random.default_rng(2).standard_normal(dim).astype(np.float32)
    q_rot, q_plain = rot.encode_query(query), plain.encode_query(query)
    scores = torch.empty(rows, device="cuda")
    ids, top = torch.empty(30, dtype=torch.int32, device="cuda"), torch.empty(30, device="cuda")
    here = "the plain call of this build"
    pairs = [
        ("encode rotated", lambda: E.encode(data, vp, rotated=True), lambda: E.encode(data, vp), here),
        ("encode rotated, given interval", lambda: E.encode(data, vp, alpha_offset=ao_r, rotated=True),
         lambda: E.encode(data, vp, alpha_offset=ao_p), here),
        ("score_all", lambda: rot.score_all(q_rot, out=scores), lambda: plain.score_all(q_plain, out=scores), here),
        ("topk30", lambda: rot.topk(q_rot, 30, out_ids=ids, out_scores=top),
         lambda: plain.topk(q_plain, 30, out_ids=ids, out_scores=top), here),
        ("encode_query (host query)", lambda: rot.encode_query(query, q_rot), lambda: plain.encode_query(query, q_plain), here),
    ]
    gb = rows * dim * 4 / 1e9
    lines = [f"# {torch.cuda.get_device_name(0)}; {rows} x {dim} f32 from device memory ({gb:.1f} GB); HIP events around whole "
             f"calls, median (min-max) of {a.reps} after {a.prewarm_seconds} s of pre-warm, call and yardstick in turn\n"]

    def line_of(name, t, what, med_b, lo_b, hi_b):
        med = statistics.median(t)
        line = f"{name:<32} {med:9.4f} ms ({min(t):.4f}-{max(t):.4f})   {what}: {med_b:9.4f} ms ({lo_b:.4f}-{hi_b:.4f})   ratio {med / med_b:.2f}"
        if name.startswith("encode rotated"):
            line += f"   {gb / (med * 1e-3):6.0f} GB/s of f32 read against {gb / (med_b * 1e-3):6.0f} GB/s"
        return line + "\n"

    for i, (name, t, what, tb) in enumerate(measure(pairs, a.reps, a.prewarm_seconds)):
        lines.append(line_of(name, t, what, statistics.median(tb), min(tb), max(tb)))
        if parent and i < 2 and int(parent[0]) == rows:
            lines.append(line_of(name, t, f"the plain call of {a.parent_lib} (a process of its own)", *parent[1 + 3 * i:4 + 3 * i]))
    sys.stdout.writelines(lines)
    with open(a.out, "w") as f:
        f.writelines(lines)


if __name__ == "__main__":
    main()
