"""score_internal against the whole store, ms per call with device outputs, for u8 10M x 768, binary
50M x 1024, PQ 10M x 768 (m = 96) and PQ 12.5M x 1536 (m = 192).  Per store: score_internal_all(i) and topk_internal(i, 30);
beside them the same store's score_all / topk(30) with an encoded query; and the only alternative there was,
score_internal_ids(i, arange(n)) with the ids resident on the device.  Device events around 50 calls after a warm-up,
five rounds per figure: min / median / max, so that the spread of the repeated score_all timings is in the same output.

  python tools/time_internal.py [u8] [bin] [pq96] [pq192] [--query-only]

--query-only times score_all / topk alone (a library without the internal entry points: QAMD_LIB_PATH=<parent build>)."""
import sys as _sys
if "--help" in _sys.argv[1:] or "-h" in _sys.argv[1:]:
    print(__doc__)
    _sys.exit(0)
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import quantization_amd as qa

D = qa.DistanceType
dev = torch.device("cuda", 0)
REPS, ROUNDS = 50, 5
query_only = "--query-only" in _sys.argv[1:]
only = [a for a in _sys.argv[1:] if not a.startswith("-")]


def timed(fn, reps=REPS, rounds=ROUNDS):
    """ms per call: device events around `reps` calls, `rounds` times, after a quarter of a second of calls."""
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.25:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    ms.sort()
    return ms[0], ms[len(ms) // 2], ms[-1]


def report(store, name, fn, **kw):
    lo, med, hi = timed(fn, **kw)
    print(f"{store:24s} {name:34s} {med:9.4f} ms  (min {lo:.4f}, max {hi:.4f})", flush=True)
    return med


def run(store, enc, q, n):
    i = n // 2
    out = torch.empty(n, dtype=torch.float32, device=dev)
    ids = torch.empty(30, dtype=torch.int32, device=dev)
    sc = torch.empty(30, dtype=torch.float32, device=dev)
    base = report(store, "score_all(query)", lambda: enc.score_all(q, out=out))
    report(store, "topk(query, 30)", lambda: enc.topk(q, 30, out_ids=ids, out_scores=sc))
    if query_only:
        return
    got = report(store, "score_internal_all(i)", lambda: enc.score_internal_all(i, out=out))
    report(store, "topk_internal(i, 30)", lambda: enc.topk_internal(i, 30, out_ids=ids, out_scores=sc))
    all_ids = torch.arange(n, dtype=torch.int32, device=dev)
    pairs = report(store, "score_internal_ids(i, arange(n))", lambda: enc.score_internal_ids(i, all_ids, out=out), reps=10, rounds=3)
    print(f"{store:24s} score_internal_all / score_all = {got / base:.3f}; score_internal_ids / score_internal_all = "
          f"{pairs / got:.1f}", flush=True)


if not only or "u8" in only:
    n, dim = 10_000_000, 768
    data = torch.rand((n, dim), device=dev, dtype=torch.float32)  # encoded on the GPU, as bench.py builds its store
    enc = qa.EncodedVectorsU8.encode(data, qa.VectorParameters(dim, n, D.Dot, False))
    del data
    run("u8 10M x 768", enc, enc.encode_query(torch.rand(dim, device=dev)), n)
    del enc
if not only or "bin" in only:
    n, dim = 50_000_000, 1024
    rows = torch.randint(0, 256, (n, dim // 8), device=dev, dtype=torch.uint8)
    enc = qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(dim, n, D.Dot, False))
    del rows
    run("binary 50M x 1024", enc, enc.encode_query(torch.randn(dim, device=dev)), n)
    del enc
for tag, n, dim in (("pq96", 10_000_000, 768), ("pq192", 12_500_000, 1536)):
    if only and tag not in only:
        continue
    m = dim // 8
    rows = torch.randint(0, 256, (n, m), device=dev, dtype=torch.uint8)
    cen = np.random.default_rng(0).random((256, dim), dtype=np.float32)
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(dim, n, D.Dot, False), 8, cen)
    del rows
    run(f"PQ {n / 1e6:g}M x {dim} m={m}", enc, enc.encode_query(torch.rand(dim, device=dev)), n)
    del enc
