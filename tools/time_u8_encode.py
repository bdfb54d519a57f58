"""The u8 encode of a device-resident 2M x 768 f32 store (min/max pass, quantize pass, packed image), ms per call:
device events around each of CALLS calls after a warm-up, ROUNDS rounds, min / median / max per round and over all
calls, so that a build's own run-to-run spread stands beside its figure.  --relu clips the data at zero first: half of
all values are then +0.0, every tile's minimum is a zero and every wave of minmax_stream_kernel takes the path that
reports its first zero.  Two builds are compared by running the tool once per library in one session:

  QAMD_LIB_PATH=/path/to/parent/libquantization_amd.so python tools/time_u8_encode.py
  python tools/time_u8_encode.py [--relu] [--rows N] [--dim D]        (profiles/u8_encode_shapes.txt)"""
import sys as _sys
if "--help" in _sys.argv[1:] or "-h" in _sys.argv[1:]:
    print(__doc__)
    _sys.exit(0)
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import quantization_amd as qa
from quantization_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--relu", action="store_true")
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(1)
data = torch.rand((args.rows, args.dim), device=dev, generator=g)
if args.relu:
    data = torch.clamp(data - 0.5, min=0.0)
vp = qa.VectorParameters(args.dim, args.rows, qa.DistanceType.Dot, False)


def one_call():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    enc = qa.EncodedVectorsU8.encode(data, vp)
    b.record()
    b.synchronize()
    del enc
    return a.elapsed_time(b)


for _ in range(5):
    one_call()
rounds = []
for _ in range(args.rounds):
    ms = sorted(one_call() for _ in range(args.calls))
    rounds.append({"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4)})
medians = sorted(r["median"] for r in rounds)
print(json.dumps({"tool": "time_u8_encode", "library": os.path.relpath(_lib.LIB_PATH), "rows": args.rows, "dim": args.dim,
                  "relu": args.relu, "calls_per_round": args.calls, "rounds": rounds,
                  "median_of_round_medians_ms": medians[len(medians) // 2],
                  "spread_of_round_medians_ms": [medians[0], medians[-1]]}))
