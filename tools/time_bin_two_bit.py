#!/usr/bin/env python3
"""What the binary quantizer's two-bit rows cost: the statistics pass, the threshold encoder and the scans
of a two-bit store, each next to its yardstick, from one process with HIP events around whole calls, the median of
`--reps` after a pre-warm.

    python tools/time_bin_two_bit.py [--rows 10000000] [--dim 768] [--reps 5] [--out profiles/bin_two_bit.txt]

    find_stats             against rows x dim x 4 bytes at the on-box streaming-read ceiling (the probe bench.py --full
                           quotes: tools/probe, 16-byte nt loads over 4 GiB)
    encode, two bits       with given thresholds, against the one-bit encode of the same device data
    score_all, topk(30)    on the two-bit store, against a one-bit store of 2 x dim over the same bytes: the kernels are
                           the same, so a gap beyond the run-to-run spread is a routing mistake to find

    --scalar               instead: weighted 4- / 8-bit scalar queries against the two-bit store, each call
                           next to the unweighted scalar call on the one-bit store of 2 x dim over the same bytes -
                           encode_query and encode_query_batch (--queries, 64) produce the same output size there and the
                           weighted encoder reads lo / hi as well; score_all, topk(30), score_batch and topk_batch(30) are
                           the same kernels on the same bytes.  Default --out: profiles/bin_two_bit_scalar.txt

Nothing here is a pass condition.  Fewer rows are taken when the device has less memory than the f32 data needs."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def read_ceiling_gbps():
    """bench.py's streaming-read probe: 10 reads of 4 GiB after 3 warm ones."""
    import torch

    from quantization_amd import _lib

    P = C.CDLL(_lib.PROBE_PATH)
    P.qamd_probe_stream_read.restype = C.c_int
    P.qamd_probe_stream_read.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    probe = torch.zeros(4 << 30, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        if P.qamd_probe_stream_read(probe.data_ptr(), probe.numel(), scratch.data_ptr(), s):
            raise RuntimeError("probe launch failed")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        P.qamd_probe_stream_read(probe.data_ptr(), probe.numel(), scratch.data_ptr(), s)
    b.record()
    torch.cuda.synchronize()
    return probe.numel() * 10 / (a.elapsed_time(b) * 1e-3) / 1e9


def scalar_mode(a, rows):
    """Weighted scalar queries on a two-bit store against unweighted ones on the one-bit store of 2 x dim, same bytes."""
    import numpy as np
    import torch

    import quantization_amd as qa

    E, TWO = qa.EncodedVectorsBin, qa.BinaryEncoding.TwoBits
    dim, nq = a.dim, a.queries
    vp = qa.VectorParameters(dim, rows, qa.DistanceType.Dot, False)
    nb = E.get_quantized_vector_size_from_params(vp, encoding=TWO)
    g = torch.Generator(device="cuda").manual_seed(1)
    lo = hi = None
    same_bytes = torch.empty((rows, nb), dtype=torch.uint8, device="cuda")
    step = 1 << 20  # the f32 data a block at a time: only the rows stay
    for r0 in range(0, rows, step):
        block = torch.randn((min(step, rows - r0), dim), device="cuda", generator=g, dtype=torch.float32)
        if lo is None:
            lo, hi = E.thresholds_from_stats(*E.find_stats(block))
        part = E.encode(block, qa.VectorParameters(dim, block.shape[0], qa.DistanceType.Dot, False), encoding=TWO, thresholds=(lo, hi))
        part.storage_bytes(out=same_bytes[r0:r0 + block.shape[0]].view(-1))
        del part, block
    two = E.from_storage(same_bytes, vp, encoding=TWO, thresholds=(lo, hi))
    one_wide = E.from_storage(same_bytes, qa.VectorParameters(2 * dim, rows, qa.DistanceType.Dot, False))
    del same_bytes
    rng = np.random.default_rng(2)
    queries = torch.from_numpy(rng.standard_normal((nq, dim)).astype(np.float32)).cuda()
    h = torch.from_numpy(hi - lo).cuda()
    wide = torch.cat([queries * h, queries * h], dim=1).contiguous()  # (w | w): the same codes on the one-bit store
    scores = torch.empty(rows, device="cuda")
    ids, top = torch.empty(30, dtype=torch.int32, device="cuda"), torch.empty(30, device="cuda")
    bscores = torch.empty((nq, rows), device="cuda")
    bids, btop = torch.empty((nq, 30), dtype=torch.int32, device="cuda"), torch.empty((nq, 30), device="cuda")
    lines = [f"# {torch.cuda.get_device_name(0)}; {rows} x {dim} two-bit rows ({rows * nb / 1e9:.2f} GB) and the one-bit store of dim "
             f"{2 * dim} over the same bytes; weighted scalar queries (DESIGN 3.2f) against unweighted ones; batches of {nq}; HIP "
             f"events around whole calls, median (min-max) of {a.reps} after {a.prewarm_seconds} s of pre-warm, call and yardstick "
             f"in turn\n"]
    for bits in (4, 8):
        q_two = two.encode_query(queries[0], query_bits=bits, weighted=True)
        q_wide = one_wide.encode_query(wide[0], query_bits=bits)
        b_two = two.encode_query_batch(queries, query_bits=bits, weighted=True)
        b_wide = one_wide.encode_query_batch(wide, query_bits=bits)
        assert np.array_equal(q_two.encoded_vector, q_wide.encoded_vector), "the two stores must see the same planes"
        routes = (two.batch_kernel(b_two, 0), two.batch_kernel(b_two, 30), one_wide.batch_kernel(b_wide, 0), one_wide.batch_kernel(b_wide, 30))
        pairs = [
            ("encode_query", lambda: two.encode_query(queries[0], q_two, query_bits=bits, weighted=True),
             lambda: one_wide.encode_query(wide[0], q_wide, query_bits=bits)),
            ("encode_query_batch", lambda: two.encode_query_batch(queries, b_two, query_bits=bits, weighted=True),
             lambda: one_wide.encode_query_batch(wide, b_wide, query_bits=bits)),
            ("score_all", lambda: two.score_all(q_two, out=scores), lambda: one_wide.score_all(q_wide, out=scores)),
            ("topk30", lambda: two.topk(q_two, 30, out_ids=ids, out_scores=top),
             lambda: one_wide.topk(q_wide, 30, out_ids=ids, out_scores=top)),
            ("score_batch", lambda: two.score_batch(b_two, out=bscores), lambda: one_wide.score_batch(b_wide, out=bscores)),
            ("topk_batch30", lambda: two.topk_batch(b_two, 30, out_ids=bids, out_scores=btop),
             lambda: one_wide.topk_batch(b_wide, 30, out_ids=bids, out_scores=btop)),
        ]
        t_end = time.perf_counter() + a.prewarm_seconds
        while time.perf_counter() < t_end:
            for _, run, base in pairs:
                run()
                base()
            torch.cuda.synchronize()
        lines.append(f"# {bits}-bit queries; batch routes (two-bit score / topk, one-bit score / topk): {' '.join(routes)}\n")
        for name, run, base in pairs:
            t, tb = [], []
            for _ in range(a.reps):
                t.append(timed(run))
                tb.append(timed(base))
            med, mb = statistics.median(t), statistics.median(tb)
            line = (f"{bits}-bit {name:<19} two-bit, weighted {med:9.4f} ms ({min(t):.4f}-{max(t):.4f})   one-bit store of dim {2 * dim}, "
                    f"unweighted {mb:9.4f} ms ({min(tb):.4f}-{max(tb):.4f})   ratio {med / mb:.2f}")
            lines.append(line + "\n")
            print(line, flush=True)
            with open(a.out, "w") as f:  # rewritten after every line: a cut-off run keeps what it measured
                f.writelines(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prewarm-seconds", type=float, default=2.0)
    ap.add_argument("--scalar", action="store_true", help="time weighted scalar queries against the two-bit store")
    ap.add_argument("--queries", type=int, default=64, help="--scalar: queries per batch")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "bin_two_bit_scalar.txt" if a.scalar else "bin_two_bit.txt")
    import numpy as np
    import torch

    import quantization_amd as qa

    E, TWO = qa.EncodedVectorsBin, qa.BinaryEncoding.TwoBits
    dim = a.dim
    free, _ = torch.cuda.mem_get_info()
    rows = min(a.rows, int(free * 0.7) // (dim * 4 + dim))
    if a.scalar:
        return scalar_mode(a, rows)
    ceiling = read_ceiling_gbps()
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randn((rows, dim), device="cuda", generator=g, dtype=torch.float32)
    vp = qa.VectorParameters(dim, rows, qa.DistanceType.Dot, False)
    lo, hi = E.thresholds_from_stats(*E.find_stats(data))
    two = E.encode(data, vp, encoding=TWO, thresholds=(lo, hi))
    nb = E.get_quantized_vector_size_from_params(vp, encoding=TWO)
    same_bytes = torch.empty(rows * nb, dtype=torch.uint8, device="cuda")
    two.storage_bytes(out=same_bytes)
    one_wide = E.from_storage(same_bytes.view(rows, nb), qa.VectorParameters(2 * dim, rows, qa.DistanceType.Dot, False))
    del same_bytes
    query = np.random.default_rng(2).standard_normal(dim).astype(np.float32)
    q_two = two.encode_query(query)
    q_wide = one_wide.encode_query(np.where(np.unpackbits(q_two.encoded_vector, bitorder="little")[:2 * dim] != 0,
                                            np.float32(1), np.float32(-1)).astype(np.float32))
    scores = torch.empty(rows, device="cuda")
    ids, top = torch.empty(30, dtype=torch.int32, device="cuda"), torch.empty(30, device="cuda")
    pairs = [  # what is timed, its yardstick
        ("find_stats", lambda: E.find_stats(data), None),
        ("encode", lambda: E.encode(data, vp, encoding=TWO, thresholds=(lo, hi)), lambda: E.encode(data, vp)),
        ("score_all", lambda: two.score_all(q_two, out=scores), lambda: one_wide.score_all(q_wide, out=scores)),
        ("topk30", lambda: two.topk(q_two, 30, out_ids=ids, out_scores=top),
         lambda: one_wide.topk(q_wide, 30, out_ids=ids, out_scores=top)),
    ]
    t_end = time.perf_counter() + a.prewarm_seconds
    while time.perf_counter() < t_end:
        for _, run, base in pairs:
            run()
            if base:
                base()
        torch.cuda.synchronize()
    gb = rows * dim * 4 / 1e9
    lines = [f"# {torch.cuda.get_device_name(0)}; {rows} x {dim} f32 from device memory ({gb:.1f} GB); HIP events around whole calls, "
             f"median (min-max) of {a.reps} after {a.prewarm_seconds} s of pre-warm, call and yardstick in turn\n",
             f"# streaming-read ceiling of this device (tools/probe, as bench.py --full): {ceiling:.0f} GB/s\n"]
    for name, run, base in pairs:
        t, tb = [], []
        for _ in range(a.reps):
            t.append(timed(run))
            if base:
                tb.append(timed(base))
        med = statistics.median(t)
        line = f"{name:<11} two-bit {med:9.3f} ms ({min(t):.3f}-{max(t):.3f})"
        if name == "find_stats":
            floor = gb / ceiling * 1e3
            line += f"   {gb / (med * 1e-3):7.0f} GB/s read = {floor / med:.2f} of the read ceiling ({floor:.3f} ms)"
        else:
            mb = statistics.median(tb)
            what = "one-bit encode of the same data" if name == "encode" else f"one-bit store of dim {2 * dim}, same bytes"
            line += f"   {what}: {mb:9.3f} ms ({min(tb):.3f}-{max(tb):.3f})   two-bit / yardstick {med / mb:.2f}"
        lines.append(line + "\n")
        print(line, flush=True)
        with open(a.out, "w") as f:  # rewritten after every line: a cut-off run keeps what it measured
            f.writelines(lines)


if __name__ == "__main__":
    main()
