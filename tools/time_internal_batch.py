"""Many stored rows against the whole store, ms per 8 rows with device rows and a device output:
score_internal_all_batch(8 rows) against 8 calls of score_internal_all, on u8 1M x 768 Dot, binary 4M x 1024 and PQ
1M x 768 (m = 96).  Device events around 20 calls after a warm-up, five rounds per figure: min / median / max.

  python tools/time_internal_batch.py [u8] [bin] [pq]"""
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
REPS, ROUNDS, R = 20, 5, 8
only = [a for a in _sys.argv[1:] if not a.startswith("-")]


def timed(fn):
    """ms per call: device events around REPS calls, ROUNDS times, after a quarter of a second of calls."""
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.25:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / REPS)
    ms.sort()
    return ms[0], ms[len(ms) // 2], ms[-1]


def run(store, enc, n):
    rows = np.random.default_rng(1).integers(0, n, size=R, dtype=np.uint32)
    drows = torch.from_numpy(rows.astype(np.int32)).to(dev)
    out = torch.empty(R * n, dtype=torch.float32, device=dev)
    per_row = [out[l * n:(l + 1) * n] for l in range(R)]

    def loop():
        for l in range(R):
            enc.score_internal_all(int(rows[l]), out=per_row[l])

    loop()
    torch.cuda.synchronize()
    want = out.clone()
    enc.score_internal_all_batch(drows, out=out)
    torch.cuda.synchronize()
    same = torch.equal(out.view(torch.int32), want.view(torch.int32))
    lo, loop_ms, hi = timed(loop)
    print(f"{store:22s} {R} x score_internal_all          {loop_ms:9.4f} ms  (min {lo:.4f}, max {hi:.4f})", flush=True)
    lo, batch_ms, hi = timed(lambda: enc.score_internal_all_batch(drows, out=out))
    print(f"{store:22s} score_internal_all_batch({R} rows) {batch_ms:9.4f} ms  (min {lo:.4f}, max {hi:.4f})", flush=True)
    print(f"{store:22s} batch / loop = {batch_ms / loop_ms:.3f}; bits equal: {same}", flush=True)


if not only or "u8" in only:
    n, dim = 1_000_000, 768
    data = torch.rand((n, dim), device=dev, dtype=torch.float32)
    enc = qa.EncodedVectorsU8.encode(data, qa.VectorParameters(dim, n, D.Dot, False))
    del data
    run("u8 1M x 768 Dot", enc, n)
    del enc
if not only or "bin" in only:
    n, dim = 4_000_000, 1024
    bits = torch.randint(0, 256, (n, dim // 8), device=dev, dtype=torch.uint8)
    enc = qa.EncodedVectorsBin.from_storage(bits, qa.VectorParameters(dim, n, D.Dot, False))
    del bits
    run("binary 4M x 1024", enc, n)
    del enc
if not only or "pq" in only:
    n, dim = 1_000_000, 768
    codes = torch.randint(0, 256, (n, dim // 8), device=dev, dtype=torch.uint8)
    cen = np.random.default_rng(0).random((256, dim), dtype=np.float32)
    enc = qa.EncodedVectorsPQ.from_storage(codes, qa.VectorParameters(dim, n, D.Dot, False), 8, cen)
    del codes
    run("PQ 1M x 768 m=96", enc, n)
    del enc
