"""score_batch of a full-range u8 store: u8_full_batch_kernel against passes of u8_scan_multi_kernel, the
A/B behind the route gate (u8_gemm_route.hpp full_batch_min).  Each arm runs in a child process of its own on the developer
library, alternated; QAMD_DEV_U8_FULL_MIN = 1000000 sends every batch to the scans.  Device events, median of 15 after 5.
Usage: python tools/time_u8_full_batch.py [rows] [dim] > profiles/u8_full_range_batch.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5, 8, 15, 16, 30, 32, 64)


def child(rows, dim):
    import torch
    sys.path.insert(0, ROOT)
    import quantization_amd as qa
    x = torch.rand((rows, dim), device="cuda")
    enc = qa.EncodedVectorsU8.encode(x, qa.VectorParameters(dim, rows, qa.DistanceType.Dot, False), full_range=True)
    del x
    out = torch.empty(max(SIZES) * rows, dtype=torch.float32, device="cuda")
    res = {}
    for nq in SIZES:
        b = enc.encode_query_batch(torch.rand((nq, dim), device="cuda"))
        ms = []
        for it in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            enc.score_batch(b, out=out[:nq * rows])
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res[nq] = sorted(ms[5:])[7]
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rows", nargs="?", type=int, default=2000000)
    ap.add_argument("dim", nargs="?", type=int, default=768)
    ap.add_argument("--child", action="store_true", help="one arm, in this process (what the parent starts)")
    args = ap.parse_args()
    rows, dim = args.rows, args.dim
    if args.child:
        child(rows, dim)
        sys.exit(0)
    runs = {"kernel": [], "scans": []}
    for rnd in range(2):
        for arm in ("kernel", "scans"):
            env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
            env["QAMD_LIB_PATH"] = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
            if arm == "scans":
                env["QAMD_DEV_U8_FULL_MIN"] = "1000000"
            p = subprocess.run([sys.executable, __file__, "--child", str(rows), str(dim)], capture_output=True, text=True, env=env, timeout=280)
            if p.returncode != 0:
                sys.exit(f"{arm} child ended with {p.returncode}\n{p.stderr[-3000:]}")
            runs[arm].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:]))
    print(f"# score_batch, {rows} x {dim} full-range Dot store, device output, ms (two alternated child processes per arm)")
    for nq in SIZES:
        k, s = [r[str(nq)] for r in runs["kernel"]], [r[str(nq)] for r in runs["scans"]]
        print(f"{nq:3d} queries: u8_full_batch_kernel {k[0]:.3f} {k[1]:.3f}   u8_scan_multi_kernel passes {s[0]:.3f} {s[1]:.3f}")
