"""OriginalVectors.topk_batch(30) of 16, 64, 256 and 1024 queries over 10M x 768 bf16 and f16 rows, ms per call and per query
with device outputs (device events, median of five after one warm-up call), with and without the matrix-core filter pass
(f32_mfma_filter_kernel): each element type runs in fresh children on the developer library, QAMD_F32_MFMA=0 and default in
turn.  The warm-up call runs first, so the one-off reduction for the store's magnitude is not in the figures; the child prints
the debug line of its last call (sample size, survivors per query, queries redone).
Optional arguments: rows and dim (default 10000000 768)."""
import os, statistics, subprocess, sys
if "--help" in sys.argv[1:] or "-h" in sys.argv[1:]:
    print(__doc__)
    sys.exit(0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    import torch
    import quantization_amd as qa
    kind, n, dim = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    dev = torch.device("cuda", 0)
    rows = torch.empty((n, dim), device=dev, dtype=torch.bfloat16 if kind == "bf16" else torch.float16)
    for r in range(0, n, 1 << 20):  # piece by piece: the f32 randoms of the whole store would not fit beside it
        piece = rows[r:r + (1 << 20)]
        piece.copy_(torch.rand(piece.shape, device=dev) - 0.5)
    ov = qa.OriginalVectors.from_data(rows, qa.VectorParameters(dim, n, qa.DistanceType.Dot, False), borrow=True, dtype=kind)
    for nq in (16, 64, 256, 1024):
        queries = torch.rand(nq, dim, device=dev) - 0.5
        ids = torch.empty(nq * 30, dtype=torch.int32, device=dev)
        sc = torch.empty(nq * 30, dtype=torch.float32, device=dev)
        times = []
        for rep in range(6):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ov.topk_batch(queries, 30, out_ids=ids, out_scores=sc)
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        ms = statistics.median(times[1:])
        print(f"{nq} queries: {ms:.3f} ms per call, {ms / nq:.4f} ms per query", flush=True)
    sys.exit(0)

dev_lib = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
n, dim = (sys.argv[1:3] + ["10000000", "768"][len(sys.argv[1:3]):])
for kind in ("bf16", "f16"):
    for switch in ("0", "1"):
        env = dict(os.environ, QAMD_LIB_PATH=dev_lib, QAMD_F32_MFMA=switch, QAMD_DEBUG_TOPK="1")
        res = subprocess.run([sys.executable, __file__, "--child", kind, n, dim], capture_output=True, text=True, env=env, timeout=600)
        if res.returncode != 0:
            sys.exit(f"{kind} QAMD_F32_MFMA={switch}: child failed\n{res.stdout}{res.stderr[-2000:]}")
        dbg = [ln for ln in res.stderr.splitlines() if ln.startswith("[qamd f32_topk_batch]")][-1:]
        for line in res.stdout.strip().splitlines() + dbg:
            print(f"{n} x {dim} {kind} QAMD_F32_MFMA={switch}: {line}", flush=True)
