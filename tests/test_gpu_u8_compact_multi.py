"""Batches of a compact 4-bit u8 store: up to 8 queries per pass over the nibble image (DESIGN.md 3.1z,
u8_scan_image_multi_kernel).  Raw bits against the oracle's scores of u8_four_bit_model's rows, and against the plain
4-bit store.  row_chunks 2 (rest group only), 3 (odd: the unread last query chunk), 16 (one ring group), 17, 34 (refill),
48 and 128; 2..17 queries: every NQ, an unused slot in each, a remainder of one, several groups.  The 32801-row stores are
the ones whose topk_batch takes the filtering pass (32768 rows and more): row_chunks 3 (the rest group alone), 17 (a ring
group and the rest) and 48 (three ring groups, no rest, fewer groups than the eight waves a block is split over)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import u8_four_bit_model as fm
from oracle import qoracle as qo
from util import assert_bits_equal, topk_want

pytestmark = pytest.mark.gpu
qa = pytest.importorskip("quantization_amd")
E, D, f32 = qa.EncodedVectorsU8, qa.DistanceType, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
NQS = (2, 3, 4, 5, 8, 9, 17)
# (dim, rotated, rows, metric, invert)
CASES = [(32, False, 1, D.Dot, False), (40, False, 65, D.L2, True), (256, False, 64, D.Dot, True), (272, False, 4099, D.L2, False),
         (544, False, 65, D.Dot, False), (768, True, 4099, D.Dot, False), (2048, False, 64, D.L2, True), (40, False, 32801, D.Dot, False),
         (272, False, 32801, D.L2, False), (768, True, 32801, D.Dot, False)]
IDS = [f"{d}{'r' if r else ''}x{n}-{m.name}{'-inv' if i else ''}" for d, r, n, m, i in CASES]
cases = pytest.mark.parametrize("case", CASES, ids=IDS)


@functools.lru_cache(maxsize=None)
def _case(dim, rotated, n, dist, invert):
    """Both handles and the oracle's scores of 17 queries and of 9 stored rows: built once, shared, never written to."""
    rng = np.random.default_rng(dim * 7 + n)
    x, qs = rng.normal(size=(n, dim)).astype(f32), rng.normal(size=(17, dim)).astype(f32)
    rows, meta = fm.encode(x, int(dist), invert, rotated)
    vp = qa.VectorParameters(dim, n, dist, invert)
    plain, comp = (E.encode(x, vp, rotated=rotated, bits=4, **kw) for kw in ({}, {"compact": True}))
    want = np.stack([qo.u8_score_all(meta, rows, *fm.encode_query(meta, q, rotated)) for q in qs])
    srows = np.array([0, n - 1] + [r % n for r in (37, 64, 63, 1, 100, 4098, 2)], np.uint32)
    m = min(n, 4099 if n <= 4099 else 70)  # (the oracle scores one pair per call)
    want_int = np.array([[qo.u8_score_internal(meta, rows, int(i), j) for j in range(m)] for i in srows], f32)
    for a in (x, qs, want, want_int):
        a.setflags(write=False)
    return {"x": x, "vp": vp, "qs": qs, "plain": plain, "comp": comp, "n": n, "want": want, "srows": srows, "want_int": want_int}


def _topk_same(got, want_scores, k, largest, what):
    for j, sc in enumerate(want_scores):
        ids, scores = topk_want(sc, k, largest)
        assert np.array_equal(np.asarray(got[0][j]), ids), f"{what}: ids of query {j}"
        assert_bits_equal(got[1][j], scores, f"{what}: scores of query {j}")


@cases
def test_score_batch(case):
    c = _case(*case)
    for nq in NQS:
        assert_bits_equal(c["comp"].score_batch(c["comp"].encode_query_batch(c["qs"][:nq])), c["want"][:nq], f"{nq} queries")
    assert_bits_equal(c["plain"].score_batch(c["plain"].encode_query_batch(c["qs"])), c["want"], "the plain store")


@cases
def test_topk_batch(case):
    c = _case(*case)
    for k in (30, 1024) if c["n"] >= 4099 else (30,):
        for nq in NQS:
            largest = bool((nq + k) % 2)
            got = c["comp"].topk_batch(c["comp"].encode_query_batch(c["qs"][:nq]), k, largest)
            _topk_same(got, c["want"][:nq], k, largest, f"{nq} queries, k {k}")
        want = c["plain"].topk_batch(c["plain"].encode_query_batch(c["qs"][:nq]), k, largest)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "the plain store"


@cases
def test_stored_rows_as_queries(case):
    c = _case(*case)
    comp, want, m = c["comp"], c["want_int"], c["want_int"].shape[1]
    for nq in (2, 3, 5, 8, 9):
        rows = c["srows"][:nq]
        assert_bits_equal(comp.score_internal_all_batch(rows, n_rows=m), want[:nq], f"{nq} rows")
        if m == c["n"]:
            _topk_same(comp.topk_internal_batch(rows, 30, nq % 2 == 0), want[:nq], 30, nq % 2 == 0, f"topk of {nq} rows")
    assert_bits_equal(c["plain"].score_internal_all_batch(c["srows"], n_rows=m), want, "the plain store")


def test_topk_batch_rescored():
    c = _case(768, True, 4099, D.Dot, False)
    orig = qa.OriginalVectors.from_data(c["x"], c["vp"])
    got, want = (h.topk_batch_rescored(h.encode_query_batch(c["qs"][:9]), orig, c["qs"][:9], 5, 50) for h in (c["comp"], c["plain"]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    for j in range(9):
        ids, sc = orig.rerank(c["qs"][j], topk_want(c["want"][j], 50)[0], 5)
        assert np.array_equal(got[0][j], ids) and np.array_equal(got[1][j].view(np.uint32), sc.view(np.uint32)), j


def child_main(one_cu):
    """On the developer library: which scan served each call.  A pass reports its queries, a single scan 1."""
    L = qa.lib()
    seen = lambda h, f: int(getattr(L, "qamd_dev_u8_last_scan_" + f)(h._h))  # (restype int is ctypes' default)
    last = lambda nq: 1 if nq % 8 == 1 else (nq % 8 or 8)  # groups of 8, then a smaller one, a remainder of one scanned singly
    for case in (CASES[3], CASES[7], CASES[8], CASES[9]):
        c = _case(*case)
        comp, plain, n = c["comp"], c["plain"], c["n"]
        split = 1
        while not one_cu and split < 8 and -(-n // 64) * split < 16 * int(L.qamd_dev_cu_count()):
            split *= 2
        for nq in NQS:
            b = comp.encode_query_batch(c["qs"][:nq])
            assert_bits_equal(comp.score_batch(b), c["want"][:nq], f"score_batch {nq}")
            assert [seen(comp, f) for f in ("queries", "packed", "split")] == [last(nq), 2, split], (case, nq)
            largest = bool(nq % 2)
            _topk_same(comp.topk_batch(b, 30, largest), c["want"][:nq], 30, largest, f"topk_batch {nq}")
            assert seen(comp, "queries") == (last(nq) if n >= 32768 else 1), (case, nq)  # small stores rank score arrays
        assert_bits_equal(comp.score_all(comp.encode_query(c["qs"][0])), c["want"][0], "score_all")
        assert seen(comp, "queries") == 1
        plain.score_all(plain.encode_query(c["qs"][0]))
        assert seen(plain, "packed") == 2
        plain.score_batch(plain.encode_query_batch(c["qs"][:2]))  # (rows of 17 and 48 chunks have the byte-code pass, of 3 not)
        assert seen(plain, "packed") == (0 if case[0] >= 9 * 16 else 2)  # a store with byte codes keeps their route
    print("DONE")


@pytest.mark.parametrize("one_cu", [False, True], ids=["as-built", "one-cu"])
def test_route_and_split(one_cu):
    if not os.path.exists(DEV_LIB):
        pytest.skip("no developer library")
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update({"QAMD_LIB_PATH": DEV_LIB}, **({"QAMD_DEV_CU_COUNT": "1"} if one_cu else {}))
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_compact_multi as T\nT.child_main(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), one_cu))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
