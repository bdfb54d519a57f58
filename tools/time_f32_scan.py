"""The whole-store exact scan of the original vectors, ms per call with device queries and outputs, at
10M x 768 and 1M x 768 rows kept as f32 and as bf16.  Per store: the baseline score_ids(q, arange(n)) with the ids
resident on the device (the unchanged list path, timed in the same run), score_all(q), topk(q, 30), and topk_batch(30)
at 1, 2, 4, 8 and 64 queries, reported per query.  Device events around 50 calls after a warm-up (a batch of Q queries:
max(3, 50 // Q) calls, so that a round still ranks at least 50 queries), five rounds per figure: min / median / max, so
that the spread of the baseline's own repeated rounds is in the same output.  score_all also reports the row bytes per
second it read.

  python tools/time_f32_scan.py [10M] [1M] [f32] [bf16] > profiles/f32_scan.txt"""
import sys as _sys
if "--help" in _sys.argv[1:] or "-h" in _sys.argv[1:]:
    print(__doc__)
    _sys.exit(0)
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import quantization_amd as qa

D = qa.DistanceType
dev = torch.device("cuda", 0)
REPS, ROUNDS = 50, 5
only = [a for a in _sys.argv[1:] if not a.startswith("-")]
sizes = [s for s in ("10M", "1M") if s in only] or ["10M", "1M"]
kinds = [k for k in ("f32", "bf16") if k in only] or ["f32", "bf16"]


def timed(fn, reps=REPS, rounds=ROUNDS):
    """ms per call: device events around `reps` calls, `rounds` times, after a quarter of a second of calls."""
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.25:
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


def report(store, name, fn, per=1, note="", **kw):
    lo, med, hi = (t / per for t in timed(fn, **kw))
    print(f"{store:18s} {name:34s} {med:9.4f} ms  (min {lo:.4f}, max {hi:.4f}){note(med) if note else ''}", flush=True)
    return lo, med, hi


for size in sizes:
    n, dim = (10_000_000 if size == "10M" else 1_000_000), 768
    for kind in kinds:
        store = f"{size} x {dim} {kind}"
        rows = torch.randn((n, dim), device=dev, dtype=torch.float32)
        if kind == "bf16":
            rows = rows.to(torch.bfloat16)
        orig = qa.OriginalVectors.from_data(rows, qa.VectorParameters(dim, n, D.Dot, False), borrow=True, dtype=kind)
        row_bytes = n * dim * rows.element_size()
        queries = torch.randn((64, dim), device=dev, dtype=torch.float32)
        q = queries[0].contiguous()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        all_ids = torch.arange(n, dtype=torch.int32, device=dev)
        tbs = lambda ms: f"  {row_bytes / ms / 1e9:.3f} TB/s of row bytes"
        b_lo, b_med, b_hi = report(store, "score_ids(q, arange(n))  [baseline]", lambda: orig.score_ids(q, all_ids, out=out), note=tbs)
        s_lo, s_med, s_hi = report(store, "score_all(q)", lambda: orig.score_all(q, out=out), note=tbs)
        print(f"{store:18s} baseline / score_all = {b_med / s_med:.2f}; the baseline's rounds spread {b_hi - b_lo:.4f} ms, "
              f"score_all is {b_med - s_med:.4f} ms faster: {'more' if b_med - s_med > b_hi - b_lo else 'NOT more'} than that spread "
              f"(slowest score_all round {s_hi:.4f}, fastest baseline round {b_lo:.4f})", flush=True)
        ids = torch.empty(30, dtype=torch.int32, device=dev)
        sc = torch.empty(30, dtype=torch.float32, device=dev)
        _, one, _ = report(store, "topk(q, 30)", lambda: orig.topk(q, 30, out_ids=ids, out_scores=sc))
        for nq in (1, 2, 4, 8, 64):
            qs = queries[:nq].contiguous()
            ids = torch.empty((nq, 30), dtype=torch.int32, device=dev)
            sc = torch.empty((nq, 30), dtype=torch.float32, device=dev)
            _, med, _ = report(store, f"topk_batch({nq} queries, 30) per query", lambda: orig.topk_batch(qs, 30, out_ids=ids, out_scores=sc),
                               per=nq, reps=max(3, REPS // nq))
            if nq == 8:
                print(f"{store:18s} topk_batch at 8 queries per query / topk = {med / one:.3f}", flush=True)
        del orig, rows, out, all_ids
        torch.cuda.empty_cache()
