#!/usr/bin/env python3
"""What the binary quantizer's rotated rows and block-rotated rows (3.2h) cost, each call next to its
yardstick, from one process with HIP events around whole calls, the median of `--reps` after a pre-warm (the method of
tools/time_bin_two_bit.py).

    python tools/time_bin_rotated.py [--rows 10000000] [--dim 768] [--reps 5] [--out profiles/bin_rotated.txt]

    encode                 rotated one-bit and rotated two-bit (given thresholds) encodes of device data, against the plain
                           one-bit encode of the same data (bin_encode_flat_kernel, the kernel the parent commit runs)
    encode_query           at dims 128 and `--dim`, 1 and 8 bits, rotated against plain one-bit handles
    score_all, topk(30)    on the rotated store, against a plain one-bit store of P dimensions over the same bytes: the
                           kernels are the same, so a gap beyond the run-to-run spread is a routing mistake to find
    blocks ...             when `--dim` is a multiple of 64: the same calls on the block-rotated encodings (rows of `--dim`
                           bits), each against two yardsticks in lines of their own - the padded ROTATED call and the plain
                           one-bit call (for the scans a plain store of `--dim` dimensions: the same kernels on as many bytes)

Nothing here is a pass condition.  Fewer rows are taken when the device has less memory than the f32 data needs."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_bin_two_bit import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prewarm-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bin_rotated.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import quantization_amd as qa

    E, B = qa.EncodedVectorsBin, qa.BinaryEncoding
    dim = a.dim
    p = 1 if dim <= 1 else 1 << (dim - 1).bit_length()  # P: the power of two at or above dim
    free, _ = torch.cuda.mem_get_info()
    rows = min(a.rows, int(free * 0.7) // (dim * 4 + p))
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randn((rows, dim), device="cuda", generator=g, dtype=torch.float32)
    vp = qa.VectorParameters(dim, rows, qa.DistanceType.Dot, False)
    rot = E.encode(data, vp, encoding=B.OneBitRotated)
    head = qa.VectorParameters(dim, min(rows, 1 << 20), qa.DistanceType.Dot, False)
    thr = E.encode(data[:head.count], head, encoding=B.TwoBitsRotated).thresholds  # thresholds of P entries for the timed encode
    nb = E.get_quantized_vector_size_from_params(vp, encoding=B.OneBitRotated)
    same_bytes = torch.empty(rows * nb, dtype=torch.uint8, device="cuda")
    rot.storage_bytes(out=same_bytes)
    wide = E.from_storage(same_bytes.view(rows, nb), qa.VectorParameters(p, rows, qa.DistanceType.Dot, False))
    del same_bytes
    query = np.random.default_rng(2).standard_normal(dim).astype(np.float32)
    q_rot = rot.encode_query(query)
    q_wide = wide.encode_query(np.where(np.unpackbits(q_rot.encoded_vector, bitorder="little")[:p] != 0,
                                        np.float32(1), np.float32(-1)).astype(np.float32))
    scores = torch.empty(rows, device="cuda")
    assert torch.equal(rot.score_all(q_rot, out=scores).clone(), wide.score_all(q_wide, out=scores))
    ids, top = torch.empty(30, dtype=torch.int32, device="cuda"), torch.empty(30, device="cuda")
    pairs = [  # what is timed, its yardstick, the yardstick's name
        ("encode one-bit rotated", lambda: E.encode(data, vp, encoding=B.OneBitRotated), lambda: E.encode(data, vp),
         "plain one-bit encode of the same data"),
        ("encode two-bit rotated", lambda: E.encode(data, vp, encoding=B.TwoBitsRotated, thresholds=thr), lambda: E.encode(data, vp),
         "plain one-bit encode of the same data"),
        ("score_all", lambda: rot.score_all(q_rot, out=scores), lambda: wide.score_all(q_wide, out=scores),
         f"one-bit store of dim {p}, same bytes"),
        ("topk30", lambda: rot.topk(q_rot, 30, out_ids=ids, out_scores=top), lambda: wide.topk(q_wide, 30, out_ids=ids, out_scores=top),
         f"one-bit store of dim {p}, same bytes"),
    ]
    if dim % 64 == 0:  # the block-rotated encodings beside the padded ones
        blk, plain = E.encode(data, vp, encoding=B.OneBitRotatedBlocks), E.encode(data, vp)
        thr_b = E.encode(data[:head.count], head, encoding=B.TwoBitsRotatedBlocks).thresholds  # dim entries
        q_blk, q_plain = blk.encode_query(query), plain.encode_query(query)
        for name, run, rot_base, plain_base, plain_what in (
                ("blocks encode one-bit", lambda: E.encode(data, vp, encoding=B.OneBitRotatedBlocks),
                 lambda: E.encode(data, vp, encoding=B.OneBitRotated), lambda: E.encode(data, vp), "plain one-bit encode"),
                ("blocks encode two-bit", lambda: E.encode(data, vp, encoding=B.TwoBitsRotatedBlocks, thresholds=thr_b),
                 lambda: E.encode(data, vp, encoding=B.TwoBitsRotated, thresholds=thr), lambda: E.encode(data, vp),
                 "plain one-bit encode"),
                ("blocks score_all", lambda: blk.score_all(q_blk, out=scores), lambda: rot.score_all(q_rot, out=scores),
                 lambda: plain.score_all(q_plain, out=scores), f"plain one-bit store of dim {dim}"),
                ("blocks topk30", lambda: blk.topk(q_blk, 30, out_ids=ids, out_scores=top),
                 lambda: rot.topk(q_rot, 30, out_ids=ids, out_scores=top),
                 lambda: plain.topk(q_plain, 30, out_ids=ids, out_scores=top), f"plain one-bit store of dim {dim}")):
            pairs.append((name, run, rot_base, f"the ROTATED call, rows of {p} bits"))
            pairs.append((name, run, plain_base, plain_what))
        for bits in (1, 8):
            qb, qr, qo = (h.encode_query(query, query_bits=bits) for h in (blk, rot, plain))
            run = (lambda qb=qb, bits=bits: blk.encode_query(query, qb, query_bits=bits))
            pairs.append((f"blocks encode_query dim {dim}, {bits} bit", run,
                          (lambda qr=qr, bits=bits: rot.encode_query(query, qr, query_bits=bits)), "ROTATED one-bit handle"))
            pairs.append((f"blocks encode_query dim {dim}, {bits} bit", run,
                          (lambda qo=qo, bits=bits: plain.encode_query(query, qo, query_bits=bits)), "plain one-bit handle"))
    small = {}
    for qd in sorted({128, dim}):
        x = torch.randn((4096, qd), device="cuda", generator=g, dtype=torch.float32)
        svp = qa.VectorParameters(qd, 4096, qa.DistanceType.Dot, False)
        small[qd] = (E.encode(x, svp, encoding=B.OneBitRotated), E.encode(x, svp), x[0].clone())
        for bits in (1, 8):
            r, o, qv = small[qd]
            qr, qo = r.encode_query(qv, query_bits=bits), o.encode_query(qv, query_bits=bits)
            pairs.append((f"encode_query dim {qd}, {bits} bit", (lambda r=r, qv=qv, qr=qr, bits=bits: r.encode_query(qv, qr, query_bits=bits)),
                          (lambda o=o, qv=qv, qo=qo, bits=bits: o.encode_query(qv, qo, query_bits=bits)), "plain one-bit handle"))
    t_end = time.perf_counter() + a.prewarm_seconds
    while time.perf_counter() < t_end:
        for _, run, base, _ in pairs:
            run()
            base()
        torch.cuda.synchronize()
    gb = rows * dim * 4 / 1e9
    lines = [f"# {torch.cuda.get_device_name(0)}; {rows} x {dim} f32 from device memory ({gb:.1f} GB), P = {p}; HIP events around "
             f"whole calls, median (min-max) of {a.reps} after {a.prewarm_seconds} s of pre-warm, call and yardstick in turn\n"]
    for name, run, base, what in pairs:
        t, tb = [], []
        for _ in range(a.reps):
            t.append(timed(run))
            tb.append(timed(base))
        med, mb = statistics.median(t), statistics.median(tb)
        line = f"{name:<28} {med:9.4f} ms ({min(t):.4f}-{max(t):.4f})   {what}: {mb:9.4f} ms ({min(tb):.4f}-{max(tb):.4f})   ratio {med / mb:.2f}"
        if " encode one" in " " + name or " encode two" in " " + name:
            line += f"   {gb / (med * 1e-3):6.0f} GB/s of f32 read against {gb / (mb * 1e-3):6.0f} GB/s"
        lines.append(line + "\n")
        print(line, flush=True)
        with open(a.out, "w") as f:  # rewritten after every line: a cut-off run keeps what it measured
            f.writelines(lines)


if __name__ == "__main__":
    main()
