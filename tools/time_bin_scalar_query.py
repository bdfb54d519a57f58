#!/usr/bin/env python3
"""What 4- and 8-bit scalar queries cost against the binary scan: `score_all` to device memory and
`topk(30)` on one binary store (50M x 1024 bits by default; fewer rows when the device has less memory), with 1, 4 and 8
query bits, HIP events around every call, all from one process after a time-based pre-warm.

    python tools/time_bin_scalar_query.py [--rows 50000000] [--dim 1024] [--reps 15] [--prewarm-seconds 3] [--out FILE]

One JSON line per (call, bits): median / min / max ms, rows/s, the fraction of the 8 TB/s HBM floor (row bytes + the 4
score bytes `score_all` writes) and the ratio to the 1-bit time of the same run.  No ratio is a pass condition: the 1-bit
line is the yardstick and is to be held against the binary line under profiles/ (r04_bench_line_bin.json).

    python tools/time_bin_scalar_query.py --batch [--rows 10000000,50000000] [--queries 8,32,64,256] [--reps 7] [--out FILE]

Batches of scalar queries (qamd_bin_encode_query_batch_scalar) against a LOOP of single-query calls over the same store:
`score_batch` against looped `score_all`, `topk_batch(30)` against looped `topk(30)`, 4 and 8 bits, and the binary batch
of the same size for context.  The loop runs the single-query kernels, which the batch route does not touch: it is the
baseline.  Per line: the kernel qamd_bin_batch_kernel names, median / min / max ms of batch and loop (HIP events, taken
in turn in one process after a pre-warm), and loop / batch.  The table goes to profiles/bin_scalar_batch.txt; the routing
thresholds of csrc/bin.hip (bin_scalar_mfma_min) are to be set from it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def timed(call):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def batch_main(a):
    import numpy as np
    import torch

    import quantization_amd as qa

    reps = a.reps or 7
    out_path = a.out or os.path.join(ROOT, "profiles", "bin_scalar_batch.txt")
    sizes = [int(x) for x in a.queries.split(",")]
    nb = qa.EncodedVectorsBin.get_quantized_vector_size_from_params(qa.VectorParameters(a.dim, 1, qa.DistanceType.Dot, False))
    head = (f"# {torch.cuda.get_device_name(0)}; dim {a.dim}; HIP events around each whole call, one process, batch and loop in turn, "
            f"{reps} repetitions after {a.prewarm_seconds} s of pre-warm per store; ms as median (min-max); seed 1 / 2\n"
            "# loop = n single-query calls (score_all to device memory / topk(30)) on the same handle: the baseline\n"
            f"{'rows':>9} {'call':>11} {'bits':>4} {'queries':>7}  {'kernel':<22} {'batch ms':>24} {'loop ms':>26} {'loop/batch':>10}\n")
    lines = [head]
    print(head, end="")
    for rows_want in [int(x) for x in (a.rows or "10000000,50000000").split(",")]:
        free, _ = torch.cuda.mem_get_info()
        rows = min(rows_want, int(free * 0.8) // (nb + 4 * max(sizes) + 4))
        g = torch.Generator(device="cuda").manual_seed(1)
        bits_rows = torch.randint(0, 256, (rows, nb), device="cuda", generator=g, dtype=torch.uint8)
        enc = qa.EncodedVectorsBin.from_storage(bits_rows, qa.VectorParameters(a.dim, rows, qa.DistanceType.Dot, False))
        del bits_rows
        queries = np.random.default_rng(2).standard_normal((max(sizes), a.dim)).astype(np.float32)
        one_scores = torch.empty(rows, device="cuda")
        one_ids, one_top = torch.empty(30, dtype=torch.int32, device="cuda"), torch.empty(30, device="cuda")
        singles = {bits: [enc.encode_query(q, query_bits=bits) for q in queries] for bits in (1, 4, 8)}
        t_end = time.perf_counter() + a.prewarm_seconds
        while time.perf_counter() < t_end:
            for bits in (1, 4, 8):
                enc.score_all(singles[bits][0], out=one_scores)
                enc.topk(singles[bits][0], 30, out_ids=one_ids, out_scores=one_top)
            torch.cuda.synchronize()
        for nq in sizes:
            scores = torch.empty(nq * rows, device="cuda")
            ids, top = torch.empty(nq * 30, dtype=torch.int32, device="cuda"), torch.empty(nq * 30, device="cuda")
            for bits in (4, 8, 1):
                batch = enc.encode_query_batch(queries[:nq], query_bits=bits)
                qs = singles[bits][:nq]
                pairs = {
                    "score_batch": (0, lambda: enc.score_batch(batch, out=scores),
                                    lambda: [enc.score_all(q, out=one_scores) for q in qs]),
                    "topk_batch30": (30, lambda: enc.topk_batch(batch, 30, out_ids=ids, out_scores=top),
                                     lambda: [enc.topk(q, 30, out_ids=one_ids, out_scores=one_top) for q in qs]),
                }
                for name, (k, run_batch, run_loop) in pairs.items():
                    run_batch()  # warm both forms at this shape
                    run_loop()
                    torch.cuda.synchronize()
                    tb, tl = [], []
                    for _ in range(reps):  # in turn, so that drift hits both alike
                        tb.append(timed(run_batch))
                        tl.append(timed(run_loop))
                    mb, ml = statistics.median(tb), statistics.median(tl)
                    line = (f"{rows:>9} {name:>11} {bits:>4} {nq:>7}  {enc.batch_kernel(batch, k):<22} "
                            f"{f'{mb:.3f} ({min(tb):.3f}-{max(tb):.3f})':>24} {f'{ml:.3f} ({min(tl):.3f}-{max(tl):.3f})':>26} "
                            f"{ml / mb:>10.2f}\n")
                    print(line, end="", flush=True)
                    lines.append(line)
                    with open(out_path, "w") as f:  # rewritten after every line: a cut-off run keeps what it measured
                        f.writelines(lines)
            del scores
        del enc, one_scores
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default=None, help="rows of the store (default 50000000; --batch: 10000000,50000000)")
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=None, help="timed repetitions (default 15; --batch: 7)")
    ap.add_argument("--prewarm-seconds", type=float, default=3.0)
    ap.add_argument("--batch", action="store_true", help="time batches of scalar queries against loops of single queries")
    ap.add_argument("--queries", default="8,32,64,256", help="--batch: the batch sizes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.batch:
        return batch_main(a)
    a.rows = int(a.rows or 50_000_000)
    a.reps = a.reps or 15
    a.out = a.out or os.path.join(ROOT, "profiles", "bin_scalar_query.jsonl")
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
