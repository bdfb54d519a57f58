"""PQ topk_batch(30) of 64 queries, ms per query of the whole step with device outputs, with and without the packed four-query
filter pass (pq_scan_pack4_kernel): each shape runs in fresh children on the developer library, QAMD_PQ_PACK4=0 and default
alternating, three rounds - the spread of a route's three figures is the run-to-run noise to hold a difference against.
Shapes: 10M x 768 m = 96, 20M x 768 m = 48 (chunk 16), 8M x 1024 m = 128, and the rows of two LUT slices, which take the pass
slice by slice (pq_scan_pack4_kernel<SLICED>): 12.5M x 1536 m = 192, 8M x 2048 m = 256, 10M x 1280 m = 160, 8M x 1792 m = 224.
Optional arguments: the m values to run; --also LIB runs one more child per round on another build of the developer library
(the parent commit's, say).
The children print encode_query_batch's time too (the packed tables are built there); round 0 runs under QAMD_DEBUG_TOPK
(candidate counts, the filter that ran) and is slower for it on both routes: rounds 1 and 2 are the figures."""
import os, subprocess, sys, time
if "--help" in sys.argv[1:] or "-h" in sys.argv[1:]:
    print(__doc__)
    sys.exit(0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {96: (10_000_000, 768, 8), 48: (20_000_000, 768, 16), 128: (8_000_000, 1024, 8),
          192: (12_500_000, 1536, 8), 256: (8_000_000, 2048, 8), 160: (10_000_000, 1280, 8), 224: (8_000_000, 1792, 8)}

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import quantization_amd as qa
    n, dim, chunk = SHAPES[int(sys.argv[2])]
    dev = torch.device("cuda", 0)
    rows = torch.randint(0, 256, (n, dim // chunk), device=dev, dtype=torch.uint8)
    cen = np.random.default_rng(0).random((256, dim), dtype=np.float32)
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(dim, n, qa.DistanceType.Dot, False), chunk, cen)
    del rows
    queries = torch.rand(64, dim, device=dev)
    ids = torch.empty(64 * 30, dtype=torch.int32, device=dev)
    sc = torch.empty(64 * 30, dtype=torch.float32, device=dev)
    batch = enc.encode_query_batch(queries)
    for name, fn, reps in (("encode_query_batch", lambda: enc.encode_query_batch(queries, reuse=batch), 50),
                           ("topk_batch(30)", lambda: enc.topk_batch(batch, 30, out_ids=ids, out_scores=sc), 20)):
        t_warm = time.perf_counter()
        while time.perf_counter() - t_warm < 0.5:
            fn()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        print(f"{name} {(time.perf_counter() - t0) / reps / 64 * 1e3:.4f} ms per query", flush=True)
    sys.exit(0)

dev_lib = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
args = sys.argv[1:]
also = os.path.abspath(args.pop(args.index("--also") + 1)) if "--also" in args else None
for m in [int(a) for a in args if a != "--also"] or list(SHAPES):
    for rnd in range(3):
        for pack4, lib in [("0", dev_lib), ("1", dev_lib)] + ([("1", also)] if also else []):
            env = dict(os.environ, QAMD_LIB_PATH=lib, QAMD_PQ_PACK4=pack4)
            if rnd == 0:
                env["QAMD_DEBUG_TOPK"] = "1"
            res = subprocess.run([sys.executable, __file__, "--child", str(m)], capture_output=True, text=True, env=env, timeout=300)
            if res.returncode != 0:
                sys.exit(f"m={m} QAMD_PQ_PACK4={pack4}: child failed\n{res.stdout}{res.stderr[-2000:]}")
            dbg = [ln for ln in res.stderr.splitlines() if ln.startswith("[qamd fused_topk_batch]")][-1:]
            print(f"m={m} round {rnd} QAMD_PQ_PACK4={pack4}{' ' + os.path.relpath(lib, ROOT) if lib != dev_lib else ''}: " + "; ".join(res.stdout.strip().splitlines() + dbg), flush=True)
