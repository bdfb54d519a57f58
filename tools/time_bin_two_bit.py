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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prewarm-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bin_two_bit.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import quantization_amd as qa

    E, TWO = qa.EncodedVectorsBin, qa.BinaryEncoding.TwoBits
    dim = a.dim
    free, _ = torch.cuda.mem_get_info()
    rows = min(a.rows, int(free * 0.7) // (dim * 4 + dim))
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
