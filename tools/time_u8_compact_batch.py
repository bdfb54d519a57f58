"""Batches of a compact 4-bit u8 store: score_batch and topk_batch(30) of 2 .. 1024 queries over 10M x 768
rotated Dot rows.  Up to 17 queries share passes of 8 over the nibble image (u8_scan_image_multi_kernel); from the gate on
the int8 matrix cores read the image (u8_compact_batch_kernel).

  python tools/time_u8_compact_batch.py [--rows N] [--nqs 2,8,18,64] [--parent-lib PATH] [--out profiles/u8_compact_mfma_batch.txt]

Every column is a child process of its own that builds the same seeded store and times the same calls:
  this      the developer library as built (passes of up to image_multi_width queries)
  QT 2      the same with QAMD_DEV_U8_COMPACT_QT=2, `QT 1` with 1: matrix-core passes of 32 and 16 queries instead of 64
  min 16    the same with QAMD_DEV_U8_COMPACT_MIN=16: the matrix cores from 16 queries on
  passes    the same with QAMD_DEV_U8_COMPACT_MIN=0: every batch on the image passes
  parent    --parent-lib, a library built from the parent commit; left out when not given
and `this` a second time at the end, so that the spread between two runs of one library is on the page.  The yardsticks
are the parent's column and n times this build's own single score_all / topk(30): never the new path itself.  `plain`
rows: topk_batch of the plain 4-bit store of the same data (byte codes on the matrix cores), a reference point.
Device events around REPS calls after a quarter of a second of warm-up, five rounds: median (min - max), in ms."""
import sys as _sys
if "--help" in _sys.argv[1:] or "-h" in _sys.argv[1:]:
    print(__doc__)
    _sys.exit(0)
import json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
args = sys.argv[1:]
opt = lambda name, dflt: args[args.index(name) + 1] if name in args else dflt
N, DIM, ROUNDS = int(opt("--rows", 10_000_000)), 768, 5
NQS = tuple(int(v) for v in opt("--nqs", "2,8,16,17,18,24,32,48,64,65,128,256,1024").split(","))


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import quantization_amd as qa

    dev = torch.device("cuda", 0)

    def timed(fn, reps):
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
        return [ms[len(ms) // 2], ms[0], ms[-1]]

    torch.manual_seed(7)
    data = torch.randn((N, DIM), device=dev, dtype=torch.float32)
    vp = qa.VectorParameters(DIM, N, qa.DistanceType.Dot, False)
    comp = qa.EncodedVectorsU8.encode(data, vp, rotated=True, bits=4, compact=True)
    plain = qa.EncodedVectorsU8.encode(data, vp, rotated=True, bits=4) if "--plain" in args else None
    del data
    top = max(NQS)
    queries = np.random.default_rng(1).normal(size=(top, DIM)).astype(np.float32)
    out = torch.empty(top * N, dtype=torch.float32, device=dev)
    ids, sc = torch.empty(top * 30, dtype=torch.int32, device=dev), torch.empty(top * 30, dtype=torch.float32, device=dev)
    q = comp.encode_query(queries[0])
    res = {"score 1": timed(lambda: comp.score_all(q, out=out[:N]), 20),
           "topk 1": timed(lambda: comp.topk(q, 30, out_ids=ids[:30], out_scores=sc[:30]), 20)}
    check = {}
    for nq in NQS:
        b = comp.encode_query_batch(queries[:nq])
        reps = max(2, 40 // nq)
        res[f"score {nq}"] = timed(lambda: comp.score_batch(b, out=out[:nq * N]), reps)
        res[f"topk {nq}"] = timed(lambda: comp.topk_batch(b, 30, out_ids=ids[:nq * 30], out_scores=sc[:nq * 30]), reps)
        # what the columns must agree on: the ids of every query and a checksum of the score bits
        check[str(nq)] = [int(ids[:nq * 30].to(torch.int64).sum()), int(sc[:nq * 30].view(torch.int32).to(torch.int64).sum()),
                          int(out[:nq * N].view(torch.int32).to(torch.int64).sum())]
        if plain is not None:
            pb = plain.encode_query_batch(queries[:nq])
            res[f"plain {nq}"] = timed(lambda: plain.topk_batch(pb, 30, out_ids=ids[:nq * 30], out_scores=sc[:nq * 30]), reps)
    print("RESULT " + json.dumps({"ms": res, "check": check}), flush=True)


def main():
    parent_lib, out_path = opt("--parent-lib", None), opt("--out", os.path.join(ROOT, "profiles", "u8_compact_mfma_batch.txt"))
    cols = [("this", DEV_LIB, {}), ("QT 2", DEV_LIB, {"QAMD_DEV_U8_COMPACT_QT": "2"}), ("QT 1", DEV_LIB, {"QAMD_DEV_U8_COMPACT_QT": "1"}),
            ("min 16", DEV_LIB, {"QAMD_DEV_U8_COMPACT_MIN": "16"}), ("passes", DEV_LIB, {"QAMD_DEV_U8_COMPACT_MIN": "0"})]
    if parent_lib:
        cols.append(("parent", os.path.abspath(parent_lib), {}))
    cols.append(("this again", DEV_LIB, {}))
    got = {}
    for name, lib, extra in cols:
        env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
        env.update(extra, QAMD_LIB_PATH=lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rows", str(N), "--nqs", ",".join(map(str, NQS))]
                           + (["--plain"] if name == "this" else []), env=env, capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.exit(f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")  # nothing more is started
        got[name] = json.loads(line[0][7:])
        print(name, json.dumps(got[name]), flush=True)
    names = [c[0] for c in cols]
    cell = lambda v: f"{v[0]:8.3f} ({v[1]:.3f} - {v[2]:.3f})"
    lines = [f"{N} x {DIM} rotated Dot rows, compact 4-bit store; ms per call, median (min - max) of {ROUNDS} rounds",
             "same results in every column: " + str(all(got[n]["check"] == got["this"]["check"] for n in names)), "",
             f"{'call':10s}" + "".join(f"{n:>28s}" for n in names) + f"{'n x single (this)':>20s}"]
    for what in ("score", "topk"):
        for nq in (1,) + NQS:
            key = f"{what} {nq}"
            lines.append(f"{key:10s}" + "".join(f"{cell(got[n]['ms'][key]):>28s}" for n in names)
                         + f"{nq * got['this']['ms'][what + ' 1'][0]:20.3f}")
    lines += [""] + [f"{'plain ' + str(nq):10s}{cell(got['this']['ms']['plain ' + str(nq)]):>28s}" for nq in NQS]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    child() if "--child" in args else main()
