#!/usr/bin/env python3
"""What 4- and 8-bit scalar queries cost against the binary scan: `score_all` to device memory and
`topk(30)` on one binary store (50M x 1024 bits by default; fewer rows when the device has less memory), with 1, 4 and 8
query bits, HIP events around every call, all from one process after a time-based pre-warm.

    python tools/time_bin_scalar_query.py [--rows 50000000] [--dim 1024] [--reps 15] [--prewarm-seconds 3] [--out FILE]

One JSON line per (call, bits): median / min / max ms, rows/s, the fraction of the 8 TB/s HBM floor (row bytes + the 4
score bytes `score_all` writes) and the ratio to the 1-bit time of the same run.  No ratio is a pass condition: the 1-bit
line is the yardstick and is to be held against the binary line under profiles/ (r04_bench_line_bin.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--prewarm-seconds", type=float, default=3.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bin_scalar_query.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import quantization_amd as qa

    vp0 = qa.VectorParameters(a.dim, 1, qa.DistanceType.Dot, False)
    nb = qa.EncodedVectorsBin.get_quantized_vector_size_from_params(vp0)
    free, _ = torch.cuda.mem_get_info()
    rows = min(a.rows, int(free * 0.6) // (nb + 4))
    g = torch.Generator(device="cuda").manual_seed(1)
    bits_rows = torch.randint(0, 256, (rows, nb), device="cuda", generator=g, dtype=torch.uint8)
    enc = qa.EncodedVectorsBin.from_storage(bits_rows, qa.VectorParameters(a.dim, rows, qa.DistanceType.Dot, False))
    del bits_rows
    query = np.random.default_rng(2).standard_normal(a.dim).astype(np.float32)
    queries = {bits: enc.encode_query(query, query_bits=bits) for bits in (1, 4, 8)}
    scores = torch.empty(rows, device="cuda")
    ids = torch.empty(30, dtype=torch.int32, device="cuda")
    top = torch.empty(30, device="cuda")
    calls = {"score_all": lambda q: enc.score_all(q, out=scores),
             "topk30": lambda q: enc.topk(q, 30, out_ids=ids, out_scores=top)}
    t_end = time.perf_counter() + a.prewarm_seconds  # clocks and caches settle on time, not on a call count
    while time.perf_counter() < t_end:
        for q in queries.values():
            for call in calls.values():
                call(q)
        torch.cuda.synchronize()
    recs = []
    for name, call in calls.items():
        times = {bits: [] for bits in queries}
        for _ in range(a.reps):  # the bit counts in turn, so that drift hits all three alike
            for bits, q in queries.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(q)
                e1.record()
                e1.synchronize()
                times[bits].append(e0.elapsed_time(e1))
        base = statistics.median(times[1])
        for bits, t in times.items():
            med = statistics.median(t)
            moved = rows * (nb + (4 if name == "score_all" else 0))
            recs.append({"call": name, "query_bits": bits, "rows": rows, "dim": a.dim, "row_bytes": nb, "reps": a.reps,
                         "ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                         "rows_per_s": round(rows / (med * 1e-3)), "hbm_floor_ms": round(moved / HBM_BYTES_PER_S * 1e3, 4),
                         "fraction_of_8TBs_floor": round(moved / HBM_BYTES_PER_S * 1e3 / med, 4),
                         "ratio_to_1_bit": round(med / base, 4), "timer": "HIP events, one process, one store",
                         "prewarm_seconds": a.prewarm_seconds, "device": torch.cuda.get_device_name(0)})
    with open(a.out, "w") as f:
        for r in recs:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
