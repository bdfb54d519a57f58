"""Batches of a compact 4-bit u8 store from the gate on: u8_compact_batch_kernel, the int8 matrix cores straight from the
nibble image.  Raw bits against the oracle's scores of u8_four_bit_model's rows and against the plain 4-bit
store.  row_chunks 2 (one chunk of a four-chunk step), 3 (odd: zero high nibbles, an absent query chunk), 10 (a whole step
and one chunk), 48 (six whole steps) and 128 (the largest LDS image); 65 rows (a second, nearly empty block), 4099, and
32801 (the filter form); the gate, the gate + 1, 64, 65 and 70 queries (a second pass with a smaller QT, unused columns)."""
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
GATE = 18  # kCompactBatchMin (u8.hip)
NQS = (GATE, GATE + 1, 64, 65, 70)
# (dim, rotated, rows, metric, invert, kind)
CASES = [(32, False, 65, D.Dot, False, ""), (40, False, 4099, D.L2, True, ""), (160, False, 4099, D.Dot, True, ""),
         (768, True, 4099, D.Dot, False, ""), (2048, False, 65, D.L2, False, ""), (40, False, 32801, D.Dot, False, ""),
         (160, False, 32801, D.L2, False, ""), (768, True, 32801, D.Dot, False, "")]
HARD = [(160, False, 32801, D.Dot, False, "ties"), (2048, False, 32801, D.Dot, False, "all15"), (160, False, 32801, D.L2, False, "upsert")]
ident = lambda c: f"{c[0]}{'r' if c[1] else ''}x{c[2]}-{c[3].name}{'-inv' if c[4] else ''}{c[5]}"


@functools.lru_cache(maxsize=None)
def _case(dim, rotated, n, dist, invert, kind):
    """Both handles and the oracle's scores of 70 queries: built once, shared, never written to."""
    rng = np.random.default_rng(dim * 7 + n)
    x, qs = rng.normal(size=(n, dim)).astype(f32), rng.normal(size=(70, dim)).astype(f32)
    if kind == "ties":  # every second row identical: a tie group far larger than a candidate list
        x[::2] = x[0]
    if kind == "all15":  # every code 15 in the rows (but row 1, which spans the interval) and in query 0: the largest sum
        x[:], x[1], qs[0] = 1.0, 0.0, 1.0
    rows, meta = fm.encode(x, int(dist), invert, rotated)
    vp = qa.VectorParameters(dim, n, dist, invert)
    plain, comp = (E.encode(x, vp, rotated=rotated, bits=4, **kw) for kw in ({}, {"compact": True}))
    want = np.stack([qo.u8_score_all(meta, rows, *fm.encode_query(meta, q, rotated)) for q in qs[:GATE + 1 if kind == "all15" else 70]])
    for a in (x, qs, want):
        a.setflags(write=False)
    return {"x": x, "qs": qs, "plain": plain, "comp": comp, "n": n, "want": want, "meta": meta, "rows": rows}


def _topk_same(got, want_scores, k, largest, what):
    for j, sc in enumerate(want_scores):
        ids, scores = topk_want(sc, k, largest)
        assert np.array_equal(np.asarray(got[0][j]), ids), f"{what}: ids of query {j}"
        assert_bits_equal(got[1][j], scores, f"{what}: scores of query {j}")


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


def _batches(c, nqs, ks):
    comp, plain = c["comp"], c["plain"]
    for nq in nqs:
        b = comp.encode_query_batch(c["qs"][:nq])
        assert_bits_equal(comp.score_batch(b), c["want"][:nq], f"score_batch, {nq} queries")
        for k in ks:
            largest = bool((nq + k) % 2)
            got = comp.topk_batch(b, k, largest)
            _topk_same(got, c["want"][:nq], k, largest, f"{nq} queries, k {k}")
    pb = plain.encode_query_batch(c["qs"][:nq])
    assert_bits_equal(plain.score_batch(pb), c["want"][:nq], "the plain store")
    _same(got, plain.topk_batch(pb, k, largest), "the plain store's topk_batch")


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_batches(case):
    c = _case(*case)
    _batches(c, NQS, (30, 1024) if c["n"] >= 4099 else (30,))


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_stored_rows_as_queries(case):
    c = _case(*case)
    comp, plain, n = c["comp"], c["plain"], c["n"]
    m = min(n, 70)  # (the oracle scores one pair per call)
    for nq in (GATE, 70):
        rows = ((np.arange(nq, dtype=np.uint64) * 2654435761) % n).astype(np.uint32)
        want = np.array([[qo.u8_score_internal(c["meta"], c["rows"], int(i), j) for j in range(m)] for i in rows], f32)
        assert_bits_equal(comp.score_internal_all_batch(rows, n_rows=m), want, f"{nq} rows")
        assert_bits_equal(comp.score_internal_all_batch(rows), plain.score_internal_all_batch(rows), f"{nq} rows, the plain store")
        _same(comp.topk_internal_batch(rows, 30, nq % 2 == 0), plain.topk_internal_batch(rows, 30, nq % 2 == 0), f"topk of {nq} rows")


@pytest.mark.parametrize("case", HARD, ids=ident)
def test_hard_inputs(case):
    c = _case(*case)
    if case[5] != "upsert":
        return _batches(c, (GATE + 1,), (30,))
    # a store written after its first batch: the cached pivot sample is discarded, and both handles still agree
    comp, plain = (E.encode(c["x"], qa.VectorParameters(case[0], c["n"], case[3], case[4]), bits=4, **kw) for kw in ({"compact": True}, {}))
    new = np.random.default_rng(5).normal(size=(300, case[0])).astype(f32)
    for step in range(2):
        got, want = (h.topk_batch(h.encode_query_batch(c["qs"][:GATE]), 30, True) for h in (comp, plain))
        _same(got, want, f"topk_batch, step {step}")
        if step == 0:
            _topk_same(got, c["want"][:GATE], 30, True, "before the upsert")
            for h in (comp, plain):
                h.upsert(c["n"] - 100, new)
    assert_bits_equal(comp.score_batch(comp.encode_query_batch(c["qs"][:GATE])), plain.score_batch(plain.encode_query_batch(c["qs"][:GATE])), "after")


def child_main(off):
    """On the developer library: which kernel served each call."""
    L = qa.lib()
    served = lambda h: int(L.qamd_dev_u8_last_compact_batch(h._h))  # (restype int is ctypes' default)
    for case in (CASES[2], CASES[6]):
        c = _case(*case)
        comp = c["comp"]
        for nq in (17, GATE, 70):
            b = comp.encode_query_batch(c["qs"][:nq])
            assert_bits_equal(comp.score_batch(b), c["want"][:nq], f"score_batch {nq}")
            assert served(comp) == (0 if off or nq < GATE else nq), (case, nq, "score_batch")
            _topk_same(comp.topk_batch(b, 30, True), c["want"][:nq], 30, True, f"topk_batch {nq}")
            assert served(comp) == (0 if off or nq < GATE else nq), (case, nq, "topk_batch")
    print("DONE")


@pytest.mark.parametrize("off", [False, True], ids=["as-built", "switched-off"])
def test_route(off):
    if not os.path.exists(DEV_LIB):
        pytest.skip("no developer library")
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update({"QAMD_LIB_PATH": DEV_LIB}, **({"QAMD_DEV_U8_COMPACT_MIN": "0"} if off else {}))
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_compact_mfma as T\nT.child_main(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), off))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
