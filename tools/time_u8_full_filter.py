"""topk_batch(30) of a full-range u8 store from the filter gate on: this tree's library (the filter form of
u8_full_batch_kernel) against the parent commit's (filter passes of u8_scan_multi_kernel), whole calls, device outputs.
Each arm runs in child processes of its own, alternated, every child under a time limit; device events, median of 15
after 5 warm calls.  The 7-bit store of the same shape is timed beside it in this tree's children, as context.
Usage: python tools/time_u8_full_filter.py PARENT_LIB [rows] [dim] >> profiles/u8_full_range_filter.txt
PARENT_LIB: libquantization_amd.so built from the parent commit."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5, 15, 16, 64, 128)


def child(rows, dim, seven_bit):
    import torch
    sys.path.insert(0, ROOT)
    import quantization_amd as qa
    x = torch.rand((rows, dim), device="cuda")
    vp = qa.VectorParameters(dim, rows, qa.DistanceType.Dot, False)
    stores = {"full": qa.EncodedVectorsU8.encode(x, vp, full_range=True)}
    if seven_bit:
        stores["7bit"] = qa.EncodedVectorsU8.encode(x, vp)
    del x
    ids = torch.empty(max(SIZES) * 30, dtype=torch.int32, device="cuda")
    sc = torch.empty(max(SIZES) * 30, dtype=torch.float32, device="cuda")
    res = {}
    for name, enc in stores.items():
        for nq in SIZES:
            b = enc.encode_query_batch(torch.rand((nq, dim), device="cuda"))
            ms = []
            for it in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                enc.topk_batch(b, 30, out_ids=ids[:nq * 30], out_scores=sc[:nq * 30])
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            res[f"{name}:{nq}"] = sorted(ms[5:])[7]
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_lib")
    ap.add_argument("rows", nargs="?", type=int, default=2000000)
    ap.add_argument("dim", nargs="?", type=int, default=768)
    ap.add_argument("--child", action="store_true", help="one arm, in this process (what the parent process starts)")
    args = ap.parse_args()
    if args.child:
        child(args.rows, args.dim, args.parent_lib == "-")
        sys.exit(0)
    runs = {"this": [], "parent": []}
    for rnd in range(2):
        for arm in ("this", "parent"):
            env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
            if arm == "parent":
                env["QAMD_LIB_PATH"] = os.path.abspath(args.parent_lib)
            p = subprocess.run([sys.executable, __file__, "--child", "-" if arm == "this" else "parent", str(args.rows), str(args.dim)],
                               capture_output=True, text=True, env=env, timeout=200)
            if p.returncode != 0:  # nothing more is started on the device
                sys.exit(f"{arm} child ended with {p.returncode}\n{p.stderr[-3000:]}")
            runs[arm].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:]))
    print(f"# topk_batch(30), {args.rows} x {args.dim} Dot store, device outputs, ms (two alternated child processes per arm)")
    for nq in SIZES:
        t, p = [r[f"full:{nq}"] for r in runs["this"]], [r[f"full:{nq}"] for r in runs["parent"]]
        s = [r[f"7bit:{nq}"] for r in runs["this"]]
        print(f"{nq:3d} queries: filter form {t[0]:.3f} {t[1]:.3f}   parent (scans) {p[0]:.3f} {p[1]:.3f}   7-bit store {s[0]:.3f} {s[1]:.3f}")
