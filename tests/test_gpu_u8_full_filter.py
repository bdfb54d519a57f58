"""topk_batch of a full-range u8 store from the filter gate (32768 rows) on: the filter form of u8_full_batch_kernel
 against u8_full_range_model (int64 sums, the f32 epilogue), ranked by the total order on the score bits
with ties to the lower id.  Everything on raw bits."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import u8_full_range_model as wm

qa = pytest.importorskip("quantization_amd")
pytestmark = pytest.mark.gpu
f32, u32, D = np.float32, np.uint32, qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED = (0, 4, 14, 15, 30)  # query 0 and the last query of batches of 5, 15, 16 (a second pass of one query) and 31


def same(got, want, what=""):
    assert np.array_equal(np.ascontiguousarray(got, f32).view(u32), np.ascontiguousarray(want, f32).view(u32)), what


def ranked(sc, k, largest):
    key = np.ascontiguousarray(sc, f32).view(u32).astype(np.int64)
    key = np.where(key >> 31, 0x7FFFFFFF - (key & 0x7FFFFFFF), key + 0x80000000)
    order = np.lexsort((np.arange(sc.size), -key if largest else key))[:k]
    return order.astype(u32), sc[order]


@functools.lru_cache(maxsize=2)
def store(kind, dist, invert):
    """(store, 31 queries, model scores of the CHECKED ones) of "<dim>x<rows>": random rows, most codes above 127.  "ties:":
    every row from 40 on equals row 40.  "nonfinite:": six stored offsets are NaN, -NaN, +inf, -inf, +inf, -inf.  "edge:":
    codes 240..255 in rows and queries (stored offsets are the store's to choose: random), sums just under 2^29."""
    what, _, shape = kind.rpartition(":")
    dim, n = map(int, shape.split("x"))
    rng = np.random.default_rng(dim + n)
    if what == "edge":
        meta = wm.encode(np.zeros((1, dim), f32), int(dist), invert, f32(1) / f32(255), 0)[1]
        codes = np.frombuffer(rng.bytes(n * dim), np.uint8).reshape(n, dim) | np.uint8(0xF0)
        rows = np.concatenate([(rng.standard_normal(n).astype(f32) * f32(40)).view(np.uint8).reshape(n, 4), codes], axis=1)
        qs = (f32(255) - rng.integers(0, 16, (31, dim)).astype(f32)) / f32(255)
    else:
        x = rng.random((n, dim), dtype=f32) ** f32(0.4)
        x[0, 0], x[0, -1] = 0.0, 1.0
        if what == "ties":
            x[40:] = x[40]
        rows, meta = wm.encode(x, int(dist), invert, *wm.interval(x))
        qs = rng.random((31, dim), dtype=f32) ** f32(0.4)
    if what == "nonfinite":
        bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x7F800000, 0xFF800000], u32)
        rows[[7, 500, 16000, 16001, 32990, 32999], :4] = bits.view(np.uint8).reshape(6, 4)
    want = {}
    for j in CHECKED[:2 if what == "edge" else 5]:  # in row slices: the model widens the codes to int64
        qc, qoff = wm.encode_query(meta, qs[j])
        want[j] = np.concatenate([wm.scores(meta, rows[i:i + 4096], qc, qoff) for i in range(0, n, 4096)])
        assert what != "edge" or j or 2 ** 28.9 < max(wm.pair_sums(meta, rows[i:i + 4096], qc).max() for i in range(0, n, 4096)) < 2 ** 29
    md = {key: meta[key] for key in ("actual_dim", "alpha", "offset", "multiplier")}
    md.update(vector_parameters=qa.VectorParameters(dim, n, dist, invert), full_range=True)
    return qa.EncodedVectorsU8.from_storage(rows, md), qs, want


# 200: NKB 4, a padded last k-block; 768: NKB 12, 33000 = 515 * 64 + 40: a partial last tile; 1000: NKB 16; 2048: NKB 0, the
# fragment re-read per k-block.  k = 1024: pivot rank above 64, the exact per-query route.  nonfinite: pp_row_bound lets such
# rows reach the exact epilogue, where the total order places them.  ties: the tie sits at the pivot both ways, every list
# overflows and every query is redone exactly.  edge: the range edge of the integer pre-filter, every exact sum s near
# 247.5^2 * 8256 = 2^28.91, under 255^2 * 8256 = 536 846 400 < 2^29.  What meets in i32 there:
#   s = acc + 128 (sum c' + sum q') + 16384 ad:  |acc| <= 2^14 * 8256 < 2^27.1, |128 (..)| <= 2^15 * 8256 < 2^28.1,
#       16384 ad < 2^27.1: every partial sum is under 2^29.2, and s itself in [0, 2^29);
#   d = (s - B_q) - B_row:  |B_q| <= 2^29 (pp_bound clamps), so s - B_q is in (-2^29, 2^30); |B_row| <= 2^29, or exactly 2^30
#       on the permissive side for a non-finite offset, so d is in (-2^31 + 2^29, 2^31): inside an int because s < 2^29
#       strictly.  At ad = 8272 s can pass 2^29 and that last bound is gone: such rows stay on the scans.
@pytest.mark.parametrize("kind,sizes,ks", [(s, (5, 15, 16, 31), (30, 1024)) for s in ("200x33000", "768x33000", "1000x33000", "2048x32768")]
                         + [("nonfinite:768x33000", (5, 16), (30,)), ("ties:768x33000", (5, 16), (30,)), ("edge:8256x32768", (5,), (30,))])
@pytest.mark.parametrize("dist,invert", [(D.Dot, False), (D.Dot, True), (D.L2, False), (D.L2, True)])  # both LOW directions, both senses
def test_topk_batch(kind, sizes, ks, dist, invert):
    enc, qs, want = store(kind, dist, invert)
    for nq in sizes:
        b = enc.encode_query_batch(qs[:nq])
        for k, largest, j in [(k, lg, j) for k in ks for lg in (True, False) for j in (0, nq - 1)]:
            ids, sc = enc.topk_batch(b, k, largest=largest)
            wi, ws = ranked(want[j], k, largest)
            assert np.array_equal(ids[j], wi), (nq, k, largest, j)
            same(sc[j], ws, (nq, k, largest, j))


def child_main():
    L, info = qa.lib(), {}
    for name, kind, dist, sizes in (("random", "768x33000", D.Dot, (4, 5, 16)), ("ties", "ties:768x33000", D.Dot, (5, 16)),
                                    ("l1", "768x33000", D.L1, (5,))):
        enc, qs, want = store(kind, dist, False)
        for nq in sizes:
            ids, sc = enc.topk_batch(enc.encode_query_batch(qs[:nq]), 30)
            for j in (j for j in (0, nq - 1) if j in want):  # (the scans' side of the gate too: four queries, L1)
                wi, ws = ranked(want[j], 30, True)
                assert np.array_equal(ids[j], wi), (name, nq, j)
                same(sc[j], ws, (name, nq, j))
            info[f"{name}:{nq}"] = [int(fn(C.c_void_p(enc._h.value))) for fn in (L.qamd_dev_u8_last_full_filter, L.qamd_dev_u8_last_full_redone)]
    print("INFO " + json.dumps(info))


def test_which_kernel_ran():
    """[queries through the filter form, of those redone]: batches beyond one scan pass take the filter form and a random
    store has none redone; four queries and L1 stay on the scans; a store of ties has every query redone."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(QAMD_LIB_PATH=os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so"))
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_full_filter as T\nT.child_main()\n" % (ROOT, os.path.join(ROOT, "tests"))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "INFO " in res.stdout, f"exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert json.loads(res.stdout.split("INFO ")[1]) == {"random:4": [0, 0], "random:5": [5, 0], "random:16": [16, 0], "ties:5": [5, 5],
                                                        "ties:16": [16, 16], "l1:5": [0, 0]}
