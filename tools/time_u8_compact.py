"""A compact 4-bit u8 store against the 4-bit store that keeps its byte codes, rotated Dot rows of 768
dimensions: score_all, topk(30), the one-shot encode, 1M random pairs in 64 x 32-id bursts repeated, topk_batch of 8 and
64 queries, and the device bytes both stores own.  Device events around 20 calls after a warm-up, five rounds per figure:
median (min - max).  Every figure is one line of JSON on stdout as well.

  python tools/time_u8_compact.py [--rows N] [--plain-only] [scan] [encode] [pairs] [batch]

--plain-only times the plain 4-bit store in both columns and builds no compact one: for a library from before the flag
(QAMD_LIB_PATH), alternated with this one to see that the existing routes have not moved.

The byte counts need the developer library (QAMD_LIB_PATH=tools/lib/libquantization_amd_dev.so); without it they are
left out.  QAMD_DEV_STAGE_BYTES sets the compact builders' tile (and every other staging piece), which is how the tile
sizes of DESIGN 3.1z were compared: `encode` alone, once per value."""
import sys as _sys
if "--help" in _sys.argv[1:] or "-h" in _sys.argv[1:]:
    print(__doc__)
    _sys.exit(0)
import ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import quantization_amd as qa

D = qa.DistanceType
dev = torch.device("cuda", 0)
REPS, ROUNDS = 20, 5
args = _sys.argv[1:]
N = int(args[args.index("--rows") + 1]) if "--rows" in args else 10_000_000
only = [a for a in args if a in ("scan", "encode", "pairs", "batch")]
PLAIN_ONLY = "--plain-only" in args
DIM = 768


def timed(fn, reps=REPS):
    """ms per call: device events around `reps` calls, ROUNDS times, after a quarter of a second of calls."""
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.25:
        fn()
        torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def report(what, plain, comp):
    print(f"{what:34s} plain {plain[0]:9.4f} ms ({plain[1]:.4f} - {plain[2]:.4f})   compact {comp[0]:9.4f} ms "
          f"({comp[1]:.4f} - {comp[2]:.4f})   compact / plain {comp[0] / plain[0]:.3f}", flush=True)
    print(json.dumps({"what": what, "rows": N, "plain_ms": plain, "compact_ms": comp, "ratio": comp[0] / plain[0]}), flush=True)


def want(name):
    return not only or name in only


data = torch.randn((N, DIM), device=dev, dtype=torch.float32)
vp = qa.VectorParameters(DIM, N, D.Dot, False)
kw = {"rotated": True, "bits": 4}
if want("encode"):
    def enc_of(compact):
        def fn():
            qa.EncodedVectorsU8.encode(data, vp, **kw, **({"compact": True} if compact and not PLAIN_ONLY else {}))
        return fn
    report("one-shot encode", timed(enc_of(False), 3), timed(enc_of(True), 3))
plain = qa.EncodedVectorsU8.encode(data, vp, **kw)
comp = plain if PLAIN_ONLY else qa.EncodedVectorsU8.encode(data, vp, **kw, compact=True)
del data
L = qa.lib()
if hasattr(L, "qamd_dev_u8_store_bytes"):
    L.qamd_dev_u8_store_bytes.restype = C.c_uint64
    L.qamd_dev_u8_store_bytes.argtypes = [C.c_void_p]
    b = [int(L.qamd_dev_u8_store_bytes(h._h)) for h in (plain, comp)]
    print(f"device bytes owned: plain {b[0]}, compact {b[1]} ({b[0] / N:.1f} and {b[1] / N:.1f} per row)", flush=True)
    print(json.dumps({"what": "store_bytes", "rows": N, "plain": b[0], "compact": b[1]}), flush=True)
rng = np.random.default_rng(1)
queries = rng.normal(size=(64, DIM)).astype(np.float32)
if want("scan"):
    out = torch.empty(N, dtype=torch.float32, device=dev)
    ids, sc = torch.empty(30, dtype=torch.int32, device=dev), torch.empty(30, dtype=torch.float32, device=dev)
    qp, qc = plain.encode_query(queries[0]), comp.encode_query(queries[0])
    for _ in range(2):  # twice, alternated: the second pair shows what the first pair's spread is worth
        report("score_all", timed(lambda: plain.score_all(qp, out=out)), timed(lambda: comp.score_all(qc, out=out)))
        report("topk(30)", timed(lambda: plain.topk(qp, 30, out_ids=ids, out_scores=sc)),
               timed(lambda: comp.topk(qc, 30, out_ids=ids, out_scores=sc)))
if want("pairs"):
    n_lists, per = 64, 32
    reps = 1_000_000 // (n_lists * per)  # 1M pairs per figure: `reps` bursts of 64 lists x 32 ids
    lists = torch.arange(0, n_lists * per + 1, per, dtype=torch.int32, device=dev)
    pids = torch.from_numpy(rng.integers(0, N, size=(reps, n_lists * per)).astype(np.int32)).to(dev)
    rows = torch.from_numpy(rng.integers(0, N, size=n_lists).astype(np.int32)).to(dev)
    pout = torch.empty(n_lists * per, dtype=torch.float32, device=dev)
    bp, bc = plain.encode_query_batch(queries), comp.encode_query_batch(queries)

    def burst(h, b):
        def fn():
            for r in range(reps):
                h.score_ids_batch(b, lists, pids[r], out=pout)
        return fn

    def burst_internal(h):
        def fn():
            for r in range(reps):
                h.score_internal_ids_batch(rows, lists, pids[r], out=pout)
        return fn
    report("1M pairs, score_ids_batch", timed(burst(plain, bp), 2), timed(burst(comp, bc), 2))
    report("1M pairs, score_internal_ids_batch", timed(burst_internal(plain), 2), timed(burst_internal(comp), 2))
    one = torch.from_numpy(rng.integers(0, N, size=1_000_000).astype(np.int32)).to(dev)
    oout = torch.empty(1_000_000, dtype=torch.float32, device=dev)
    qp, qc = plain.encode_query(queries[0]), comp.encode_query(queries[0])
    report("1M pairs, one score_ids", timed(lambda: plain.score_ids(qp, one, out=oout)), timed(lambda: comp.score_ids(qc, one, out=oout)))
if want("batch"):
    for nq in (8, 64):
        bp, bc = plain.encode_query_batch(queries[:nq]), comp.encode_query_batch(queries[:nq])
        ids = torch.empty(nq * 30, dtype=torch.int32, device=dev)
        sc = torch.empty(nq * 30, dtype=torch.float32, device=dev)
        report(f"topk_batch({nq} queries, k=30)", timed(lambda: plain.topk_batch(bp, 30, out_ids=ids, out_scores=sc), 5),
               timed(lambda: comp.topk_batch(bc, 30, out_ids=ids, out_scores=sc), 5))
