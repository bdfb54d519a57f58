#!/usr/bin/env python3
"""What a 4-bit scalar-u8 store costs and saves, each call next to its yardstick, with HIP events around
whole calls, the median of `--reps` after a pre-warm, call and yardstick in turn (the method of tools/time_u8_rotated.py).

    python tools/time_u8_four_bit.py [--rows 10000000] [--dim 768] [--reps 5] [--parent-lib PATH] [--out profiles/u8_four_bit.txt]

    encode                 the 4-bit encode (min/max) of device data, plain and rotated, against the 7-bit encode of the same
                           form by this build and, with --parent-lib, by another build of the library (the parent
                           commit's), which a child process of this tool loads and times before this process touches the GPU
    encode, given interval the same with alpha_offset given: pass 2 and the image alone
    score_all, topk(30)    the nibble scan (16 * ceil(dim / 32) + 4 bytes per row) against the 7-bit blocked scan of this
                           build's and of the parent's 7-bit store
    encode_query           a host query against the 4-bit and the 7-bit handle

The one condition: the 4-bit score_all and topk are not slower than this build's 7-bit ones; the last lines
say whether that held.  Fewer rows are taken when the device has less memory than the data and the stores need."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = ("encode", "encode, given interval", "score_all", "topk30", "encode_query (host query)")


def seven_bit_pairs(E, qa, data, vp, rotated, query, scores, ids, top):
    """The five timed calls on a 7-bit store of `data`, as (name, call) in CALLS' order."""
    store = E.encode(data, vp, rotated=rotated)
    ao = (float(store.metadata["alpha"]), float(store.metadata["offset"]))
    q = store.encode_query(query)
    return store, [lambda: E.encode(data, vp, rotated=rotated), lambda: E.encode(data, vp, alpha_offset=ao, rotated=rotated),
                   lambda: store.score_all(q, out=scores), lambda: store.topk(q, 30, out_ids=ids, out_scores=top),
                   lambda: store.encode_query(query, q)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prewarm-seconds", type=float, default=2.0)
    ap.add_argument("--parent-lib", default="", help="another build of libquantization_amd.so whose 7-bit calls are a yardstick")
    ap.add_argument("--seven-bit-only", action="store_true", help="(the child of --parent-lib) print the 7-bit calls' medians")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "u8_four_bit.txt"))
    a = ap.parse_args()
    parent = None
    if a.parent_lib:  # first, and finished before this process opens the GPU
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--seven-bit-only", "--rows", str(a.rows), "--dim",
                              str(a.dim), "--reps", str(a.reps), "--prewarm-seconds", str(a.prewarm_seconds)],
                             env=dict(os.environ, QAMD_LIB_PATH=os.path.abspath(a.parent_lib)), capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit(f"the --parent-lib run failed:\n{res.stdout[-2000:]}{res.stderr[-2000:]}")
        parent = [float(v) for v in res.stdout.strip().splitlines()[-1].split()]  # rows, then (median, min, max) per call and form
    import numpy as np
    import torch

    import quantization_amd as qa
    from time_u8_rotated import measure

    E = qa.EncodedVectorsU8
    dim = a.dim
    free, _ = torch.cuda.mem_get_info()
    # the data, one 7-bit store (bytes + image) and one 4-bit store at a time, and a store being encoded beside them
    rows = min(a.rows, int(free * 0.6) // (dim * 4 + 2 * 2 * (dim + 4) + 2 * (dim + dim // 2 + 8)))
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randn((rows, dim), device="cuda", generator=g, dtype=torch.float32)
    vp = qa.VectorParameters(dim, rows, qa.DistanceType.Dot, False)
    query = np.random.default_rng(2).standard_normal(dim).astype(np.float32)
    scores = torch.empty(rows, device="cuda")
    ids, top = torch.empty(30, dtype=torch.int32, device="cuda"), torch.empty(30, device="cuda")
    if a.seven_bit_only:
        out = [rows]
        for rotated in (False, True):
            store, calls = seven_bit_pairs(E, qa, data, vp, rotated, query, scores, ids, top)
            res = measure([(n, c, None, "") for n, c in zip(CALLS, calls)], a.reps, a.prewarm_seconds)
            out += [f"{f(t):.5f}" for _, t, _, _ in res for f in (statistics.median, min, max)]
            del store, calls
        print(*out)
        return
    gb = rows * dim * 4 / 1e9
    lines = [f"# {torch.cuda.get_device_name(0)}; {rows} x {dim} f32 from device memory ({gb:.1f} GB); HIP events around whole "
             f"calls, median (min-max) of {a.reps} after {a.prewarm_seconds} s of pre-warm, call and yardstick in turn\n"]
    held = []
    for fi, rotated in enumerate((False, True)):
        form = "rotated" if rotated else "plain"
        seven, base = seven_bit_pairs(E, qa, data, vp, rotated, query, scores, ids, top)
        four = E.encode(data, vp, rotated=rotated, bits=4)
        ao = (float(four.metadata["alpha"]), float(four.metadata["offset"]))
        q4 = four.encode_query(query)
        run = [lambda: E.encode(data, vp, rotated=rotated, bits=4), lambda: E.encode(data, vp, alpha_offset=ao, rotated=rotated, bits=4),
               lambda: four.score_all(q4, out=scores), lambda: four.topk(q4, 30, out_ids=ids, out_scores=top),
               lambda: four.encode_query(query, q4)]
        lines.append(f"# {form}: scan bytes per row {four.scan_bytes_per_row()} (4-bit) against {seven.scan_bytes_per_row()} by the "
                     f"7-bit store's report ({dim + 4 - 16 * (dim // 128)} in its blocked image); by bytes the scans' ratio would be "
                     f"{four.scan_bytes_per_row() / (dim + 4 - 16 * (dim // 128)):.2f}\n")
        here = "the 7-bit call of this build"
        res = measure([(f"{n}, 4-bit {form}", r, b, here) for n, r, b in zip(CALLS, run, base)], a.reps, a.prewarm_seconds)
        for i, (name, t, what, tb) in enumerate(res):
            med, med_b = statistics.median(t), statistics.median(tb)
            line = (f"{name:<44} {med:9.4f} ms ({min(t):.4f}-{max(t):.4f})   {what}: {med_b:9.4f} ms ({min(tb):.4f}-{max(tb):.4f})   "
                    f"ratio {med / med_b:.2f}")
            if i < 2:
                line += f"   {gb / (med * 1e-3):6.0f} GB/s of f32 read against {gb / (med_b * 1e-3):6.0f} GB/s"
            if i in (2, 3):
                line += f"   {rows * four.scan_bytes_per_row() / (med * 1e-3) / 1e9:6.0f} GB/s of image read"
                held.append((name, med <= med_b, med, med_b))
            lines.append(line + "\n")
            if parent and int(parent[0]) == rows:
                pm, plo, phi = parent[1 + 15 * fi + 3 * i:4 + 15 * fi + 3 * i]
                lines.append(f"{name:<44} {med:9.4f} ms ({min(t):.4f}-{max(t):.4f})   the 7-bit call of {a.parent_lib} (a process of "
                             f"its own): {pm:9.4f} ms ({plo:.4f}-{phi:.4f})   ratio {med / pm:.2f}\n")
        del seven, base, four, run, q4
    for name, ok, med, med_b in held:
        lines.append(f"# condition, {name}: {'held' if ok else 'NOT held'} ({med:.4f} ms against {med_b:.4f} ms)\n")
    sys.stdout.writelines(lines)
    with open(a.out, "w") as f:
        f.writelines(lines)


if __name__ == "__main__":
    main()
