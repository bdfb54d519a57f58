"""Weighted 4- and 8-bit scalar queries against two-bit rows on the GPU, every comparison on raw f32 bits
and exact ids: the encoder against the per-dimension numpy oracle (two_bit_scalar_model.py), every scoring entry point,
the batch routes by name, refusals, save / load, and that nothing else changed.

A second oracle comes for free: a one-bit handle made by from_storage from the same row bytes with dim = 2 dim.  An
unweighted scalar query of the 2 dim values (w | w) against it has the same planes, so it must score the same on code the
one-bit suites already pin."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import two_bit_model as m
import two_bit_scalar_model as w
from util import assert_bits_equal, scalar_codes, scalar_scores, topk_want

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")

E = qa.EncodedVectorsBin
D = qa.DistanceType
S = qa.BitsStoreType
TWO = qa.BinaryEncoding.TwoBits
BITS = (4, 8)
METRICS = [(D.Dot, False), (D.Dot, True), (D.L2, False), (D.L1, True)]
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(_u(got).ravel() != _u(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} want {want.ravel()[bad[0]]!r}"


# ---------------------------------------------------------------------------------------------------------- encode
def _encode_thresholds(dim, seed):
    """Ordinary columns of unequal width, and where the row is long enough: lo == hi, (-inf, +inf), and one column a
    million times wider than the rest, which rules a."""
    rng = np.random.default_rng(seed)
    lo = rng.normal(size=dim).astype(f32)
    hi = (lo + (0.1 + rng.random(dim)).astype(f32)).astype(f32)
    lo[5::7] = hi[5::7]
    if dim > 2:
        lo[1], hi[1] = -np.inf, np.inf
        lo[2], hi[2] = f32(-3e6), f32(3e6)
    if dim > 70:
        lo[69], hi[69] = -np.inf, f32(0.0)  # h = +inf
    return lo, np.maximum(lo, hi)


def _encode_queries(dim, seed):
    rng = np.random.default_rng(seed)
    base = rng.normal(size=dim).astype(f32)
    qs = {"random": base, "zero": np.zeros(dim, f32), "plus": np.abs(base) + f32(0.1), "minus": -np.abs(base) - f32(0.1),
          "times 2^20": base * f32(2.0 ** 20), "minus zero": np.where(np.arange(dim) % 2 == 0, f32(-0.0), base).astype(f32)}
    for name, at in (("NaN first", 0), ("NaN last", dim - 1)):
        q = base.copy()
        q[at] = np.nan
        qs[name] = q
    q = base.copy()
    q[::3] = np.inf
    q[1::3] = -np.inf
    qs["infinities"] = q
    qs["all NaN"] = np.full(dim, np.nan, f32)
    q = base.copy()
    if dim > 2:
        q[2] = 0  # the wide column silent: the others spread over the codes
    qs["wide column silent"] = q
    q = base * f32(1e30)
    if dim > 2:
        q[2] = f32(-3e38)  # times the wide column's 6e6 the product overflows: w = -inf, code 0, and a comes from the rest
    qs["overflowing product"] = q
    return qs


@pytest.mark.parametrize("store", [S.U8, S.U128], ids=lambda s: s.name)
@pytest.mark.parametrize("dim", [1, 20, 33, 64, 100, 200, 1160])
def test_encode(dim, store):
    n = 3
    lo, hi = _encode_thresholds(dim, dim)
    x = np.random.default_rng(dim).normal(size=(n, dim)).astype(f32)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    enc = E.encode(x, vp, store=store, encoding=TWO, thresholds=(lo, hi))
    if dim == 100:  # the same handle rebuilt from its rows
        enc = E.from_storage(enc.storage_bytes(), vp, store, encoding=TWO, thresholds=(lo, hi))
    ref = E.from_storage(m.encode(x, lo, hi, int(store)), qa.VectorParameters(2 * dim, n, D.Dot, False), store)
    qs = _encode_queries(dim, dim + 1)
    block = np.stack(list(qs.values()))
    if dim > 2:
        a_plain = w.weighted_codes(qs["random"], lo, hi, 8)[1]
        assert w.weighted_codes(qs["times 2^20"], lo, hi, 8)[1] == a_plain * f32(2.0 ** 20)
        assert a_plain == abs(qs["random"][2]) * f32(6e6), "the wide column rules a"
    single = batch = None
    for bits in (8, 4, 8):
        batch = enc.encode_query_batch(block, batch, query_bits=bits, weighted=True)  # reused across bit counts
        assert batch.bits == bits
        for k, (name, q) in enumerate(qs.items()):
            codes, a = w.weighted_codes(q, lo, hi, bits)
            want = w.planes(codes, dim, bits, int(store))
            single = enc.encode_query(q, single, query_bits=bits, weighted=True)
            assert single.bits == bits
            _same(single.encoded_vector, want, f"{name}, {bits} bits: planes")
            _same(np.float32(single.max_abs), np.float32(a), f"{name}, {bits} bits: max_abs")
            _same(batch.encoded_vector(k), want, f"{name}, {bits} bits: query {k} of the batch")
            if k % 4 == 0:  # the one-bit handle of 2 dim takes (w | w) to the same planes
                ww = w.weights(q, lo, hi)
                _same(ref.encode_query(np.concatenate([ww, ww]), query_bits=bits).encoded_vector, want, f"{name}: (w | w)")
        if bits == 4:  # the objects move on to a binary query, weighted or not, and back
            rows = m.encode(block, lo, hi, int(store))
            single = enc.encode_query(block[0], single, query_bits=1, weighted=True)
            _same(single.encoded_vector, rows[0], "binary query through the weighted call")
            single = enc.encode_query(block[0], single)
            _same(single.encoded_vector, rows[0], "binary query")
            batch = enc.encode_query_batch(block, batch)
            assert batch.bits == 1
            _same(batch.encoded_vector(3), rows[3], "binary batch")


# -------------------------------------------------------------------------------------------------------- scoring
_stores = {}


def _store(dim, n, dist, invert, store, seed=0):
    """A two-bit store over columns of unequal scale; row 0 is at level 0 and row 1 at level 2 in every dimension."""
    key = (dim, n, dist, invert, store, seed)
    if key not in _stores:
        dkey = ("data", dim, n, seed)
        if dkey not in _stores:
            rng = np.random.default_rng(1000 * dim + n + seed)
            x = (rng.normal(size=(n, dim)) * rng.uniform(0.3, 1.5, size=dim)).astype(f32)
            x[0], x[1] = f32(-1e4), f32(1e4)
            lo, hi = m.thresholds(*m.stats(x[2:2002]))
            lv = m.levels(x, lo, hi).astype(np.int8)
            assert (lv[0] == 0).all() and (lv[1] == 2).all() and (hi > lo).all()
            _stores[dkey] = x, lo, hi, lv
        x, lo, hi, lv = _stores[dkey]
        enc = E.encode(x, qa.VectorParameters(dim, n, dist, invert), store=store, encoding=TWO, thresholds=(lo, hi))
        _stores[key] = x, lo, hi, lv, enc
    return _stores[key]


def _queries(x, lo, hi, nq, seed):
    """Noisy stored rows; query 1 has every w_i near +a and query 2 near -a: codes all L and all 0."""
    rng = np.random.default_rng(seed)
    n, dim = x.shape
    qs = (x[rng.integers(2, n, nq)] + 0.5 * rng.normal(size=(nq, dim))).astype(f32)
    if nq > 2:
        qs[1] = f32(1.0) / (hi - lo)
        qs[2] = -qs[1]
    return qs


SHAPES = [(20, 300, S.U8), (100, 5000, S.U128), (512, 4131, S.U128), (1160, 2000, S.U128)]


@pytest.mark.parametrize("dist,invert", METRICS, ids=lambda v: getattr(v, "name", str(v)))
@pytest.mark.parametrize("dim,n,store", SHAPES, ids=lambda v: getattr(v, "name", str(v)))
def test_every_entry_point(dim, n, store, dist, invert):
    x, lo, hi, lv, enc = _store(dim, n, dist, invert, store)
    ref = E.from_storage(enc.storage_bytes(), qa.VectorParameters(2 * dim, n, dist, invert), store)
    orig = qa.OriginalVectors.from_data(x, qa.VectorParameters(dim, n, dist, invert))
    queries = _queries(x, lo, hi, 3, dim)
    rng = np.random.default_rng(dim)
    ids = rng.integers(0, n, 37).astype(np.uint32)
    ids[:2] = 0, 1
    for bits in BITS:
        L = (1 << bits) - 1
        for qi, query in enumerate(queries):
            codes, _ = w.weighted_codes(query, lo, hi, bits)
            want = w.scores(lv, codes, dim, bits, dist, invert)
            if qi:  # the accumulator's two ends: X = 0 and X = code_bits * L
                assert (codes == (L if qi == 1 else 0)).all()
                ends = w.xor_from_levels(lv[:2], codes, bits)
                assert sorted(ends.tolist()) == [0, 2 * dim * L]
            q = enc.encode_query(query, query_bits=bits, weighted=True)
            got = enc.score_all(q)
            assert_bits_equal(got, want, f"score_all, {bits} bits, query {qi}")
            ww = w.weights(query, lo, hi)
            assert_bits_equal(ref.score_all(ref.encode_query(np.concatenate([ww, ww]), query_bits=bits)), want,
                              "the one-bit handle of 2 dim")
            assert_bits_equal(enc.score_ids(q, ids), want[ids], "score_ids")
            for i in (0, 1, n // 2, n - 1):
                assert_bits_equal([enc.score_point(q, i)], [want[i]], "score_point")
            for largest in (True, False):
                for k in (1, 10, 100):
                    wid, wsc = topk_want(want, k, largest)
                    gid, gsc = enc.topk(q, k, largest)
                    assert np.array_equal(gid, wid), ("topk ids", bits, qi, k, largest)
                    assert_bits_equal(gsc, wsc, "topk scores")
            cand, _ = enc.topk(q, 50, True)
            wid, wsc = orig.rerank(query, cand, 10, True)
            gid, gsc = enc.topk_rescored(q, orig, query, 10, 50, True)
            assert np.array_equal(gid, wid)
            assert_bits_equal(gsc, wsc, "topk_rescored")


def test_fused_topk_of_a_large_store():
    """32805 rows are past the single-launch top-k's plan at k = 200: the fused pipeline, and under its ties the classic one."""
    dim, n = 100, 32768 + 37
    x, lo, hi, lv, enc = _store(dim, n, D.Dot, False, S.U128)
    for bits in BITS:
        for qi, query in enumerate(_queries(x, lo, hi, 3, 5)):
            want = w.scores(lv, w.weighted_codes(query, lo, hi, bits)[0], dim, bits, D.Dot, False)
            q = enc.encode_query(query, query_bits=bits, weighted=True)
            for k, largest in ((30, True), (200, True), (200, False)):
                wid, wsc = topk_want(want, k, largest)
                gid, gsc = enc.topk(q, k, largest)
                assert np.array_equal(gid, wid), (bits, qi, k, largest)
                assert_bits_equal(gsc, wsc, "topk scores")


# -------------------------------------------------------------------------------------------------------- batches
def _want_batch(lv, queries, lo, hi, dim, bits, dist, invert):
    codes = np.stack([w.weighted_codes(q, lo, hi, bits)[0] for q in queries])
    return w.metric(w.xor_from_levels(lv, codes, bits), dim, bits, dist, invert)


@pytest.mark.parametrize("dim,kernel,dist,invert", [(100, "bin_gemm_rs_kernel", D.Dot, False), (512, "bin_gemm_rs_kernel", D.L2, False),
                                                    (2496, "bin_gemm_rs_kernel", D.Dot, True), (2560, "bin_scan_kernel", D.L1, True)],
                         ids=lambda v: getattr(v, "name", str(v)))
def test_score_batch(dim, kernel, dist, invert):
    """Rows of up to 4992 bits (dim 2496) take the int8 matrix cores from 5 queries on; 5120 bits go query by query."""
    n = 4096 + 35
    x, lo, hi, lv, enc = _store(dim, n, dist, invert, S.U128)
    queries = _queries(x, lo, hi, 70, dim + 1)
    for bits in BITS:
        want = _want_batch(lv, queries, lo, hi, dim, bits, dist, invert)
        for nq in (5, 33, 70):
            b = enc.encode_query_batch(queries[:nq], query_bits=bits, weighted=True)
            assert enc.batch_kernel(b, 0) == kernel
            assert_bits_equal(enc.score_batch(b), want[:nq], f"score_batch of {nq}, {bits} bits")
        q = enc.encode_query(queries[1], query_bits=bits, weighted=True)
        assert_bits_equal(enc.score_all(q), want[1], "the single query")


def _check_topk_batch(enc, b, queries, want, bits, k):
    for largest in (True, False):
        gid, gsc = enc.topk_batch(b, k, largest)
        for qi in range(len(queries)):
            wid, wsc = topk_want(want[qi], k, largest)
            assert np.array_equal(gid[qi], wid), ("topk_batch ids", bits, qi, largest)
            assert_bits_equal(gsc[qi], wsc, "topk_batch scores")
        for qi in (0, len(queries) - 1):
            sid, ssc = enc.topk(enc.encode_query(queries[qi], query_bits=bits, weighted=True), k, largest)
            assert np.array_equal(gid[qi], sid)
            assert_bits_equal(gsc[qi], ssc, "topk_batch against topk")


@pytest.mark.parametrize("dim,dist,invert", [(100, D.Dot, False), (512, D.L2, True)], ids=lambda v: getattr(v, "name", str(v)))
def test_topk_batch_on_the_matrix_cores(dim, dist, invert):
    n, k = 32768 + 37, 30
    x, lo, hi, lv, enc = _store(dim, n, dist, invert, S.U128)
    queries = _queries(x, lo, hi, 40, dim + 2)
    for bits in BITS:
        want = _want_batch(lv, queries, lo, hi, dim, bits, dist, invert)
        for nq in (12, 40):
            b = enc.encode_query_batch(queries[:nq], query_bits=bits, weighted=True)
            assert enc.batch_kernel(b, k) == "bin_gemm_rs_kernel"
            _check_topk_batch(enc, b, queries[:nq], want[:nq], bits, k)
        b = enc.encode_query_batch(queries[:11], query_bits=bits, weighted=True)  # one below the gate
        assert enc.batch_kernel(b, k) == "bin_topk_small_kernel"


TIE_DIM, TIE_N, TIE_K, TIE_Q, TIE_BITS = 100, 32768 + 37, 30, 12, 4


def _tie_case():
    """Rows drawn from 16 vectors, 60 % of them vector 0: the best 30 of a query near vector 0 are ~19 700 ties (queries
    0..5; queries 6..8 the same for the smallest scores), so its candidate lists overflow."""
    rng = np.random.default_rng(64)
    vectors = (rng.normal(size=(16, TIE_DIM)) * rng.uniform(0.3, 1.5, size=TIE_DIM)).astype(f32)
    which = np.where(rng.random(TIE_N) < 0.6, 0, rng.integers(1, 16, size=TIE_N))
    x = vectors[which]
    lo, hi = m.thresholds(*m.stats(rng.normal(size=(2000, TIE_DIM)) * 0.9))
    queries = (vectors[rng.integers(1, 16, TIE_Q)] + 0.3 * rng.normal(size=(TIE_Q, TIE_DIM))).astype(f32)
    queries[:6] = (vectors[0] + 0.1 * rng.normal(size=(6, TIE_DIM))).astype(f32)
    queries[6:9] = -queries[:3]
    return x, lo, hi, queries


def _tie_store(x, lo, hi):
    return E.encode(x, qa.VectorParameters(TIE_DIM, TIE_N, D.Dot, False), store=S.U128, encoding=TWO, thresholds=(lo, hi))


def tie_child(out_path):
    """Run by test_topk_batch_under_heavy_ties in a process of its own, on the developer library."""
    x, lo, hi, queries = _tie_case()
    enc = _tie_store(x, lo, hi)
    b = enc.encode_query_batch(queries, query_bits=TIE_BITS, weighted=True)
    R = {"kernel": np.frombuffer(enc.batch_kernel(b, TIE_K).encode(), dtype=np.uint8)}
    for largest in (True, False):
        R[f"ids{int(largest)}"], R[f"sc{int(largest)}"] = enc.topk_batch(b, TIE_K, largest)
    np.savez(out_path, **R)
    print("DONE")


def test_topk_batch_under_heavy_ties(tmp_path):
    """The matrix-core filter's candidate lists overflow and the queries are redone on the per-query path: the developer
    build's debug line says so, and the answers are the oracle's - the lowest row ids among the ties."""
    assert os.path.exists(DEV_LIB), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(QAMD_DEBUG_TOPK="1", QAMD_LIB_PATH=DEV_LIB)
    out = os.path.join(str(tmp_path), "ties.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_binary_two_bit_scalar_query as T\nT.tie_child(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"exit {res.returncode}\n{res.stderr[-4000:]}"
    R = np.load(out)
    assert R["kernel"].tobytes().decode() == "bin_gemm_rs_kernel"
    lines = [ln for ln in res.stderr.splitlines() if ln.startswith("[qamd bin topk_batch]")]
    assert len(lines) == 2, res.stderr[-4000:]
    for ln in lines:
        found = re.search(r"Q=12 r=\d+ candidates min/mean/max = \d+/\d+/\d+, filter (\w+), (\d+) queries redone, query bits 4$", ln)
        assert found, ln
        assert found.group(1) == "bin_gemm_rs_kernel" and int(found.group(2)) >= 1, ln
    x, lo, hi, queries = _tie_case()
    lv = m.levels(x, lo, hi).astype(np.int8)
    want = _want_batch(lv, queries, lo, hi, TIE_DIM, TIE_BITS, D.Dot, False)
    assert int((want[0] == want[0].max()).sum()) > 15000 and int((want[6] == want[6].min()).sum()) > 15000
    enc = _tie_store(x, lo, hi)
    b = enc.encode_query_batch(queries, query_bits=TIE_BITS, weighted=True)
    assert enc.batch_kernel(b, TIE_K) == "bin_gemm_rs_kernel"
    _check_topk_batch(enc, b, queries, want, TIE_BITS, TIE_K)  # the product library, against the oracle and topk
    for largest in (True, False):  # and the developer library's run gave the same
        gid, gsc = enc.topk_batch(b, TIE_K, largest)
        assert np.array_equal(R[f"ids{int(largest)}"], gid)
        assert_bits_equal(R[f"sc{int(largest)}"], gsc, "developer library")


def test_batches_below_the_gates_go_query_by_query():
    dim, n = 100, 5000
    x, lo, hi, lv, enc = _store(dim, n, D.Dot, False, S.U128)
    queries = _queries(x, lo, hi, 4, 9)
    for bits in BITS:
        want = _want_batch(lv, queries, lo, hi, dim, bits, D.Dot, False)
        b = enc.encode_query_batch(queries, query_bits=bits, weighted=True)
        assert enc.batch_kernel(b, 0) == "bin_scan_kernel" and enc.batch_kernel(b, 30) == "bin_topk_small_kernel"
        assert_bits_equal(enc.score_batch(b), want, "score_batch")
        _check_topk_batch(enc, b, queries, want, bits, 30)
    x, lo, hi, lv, enc = _store(20, 300, D.L2, False, S.U8)  # 8-byte rows never reach the matrix cores
    queries = _queries(x, lo, hi, 14, 10)
    for bits in BITS:
        want = _want_batch(lv, queries, lo, hi, 20, bits, D.L2, False)
        b = enc.encode_query_batch(queries, query_bits=bits, weighted=True)
        assert enc.batch_kernel(b, 0) == "bin_words_kernel" and enc.batch_kernel(b, 30) == "bin_words_kernel"
        assert_bits_equal(enc.score_batch(b), want, "score_batch on 8-byte rows")
        _check_topk_batch(enc, b, queries, want, bits, 30)


@pytest.mark.parametrize("dim,n,store", [(20, 300, S.U8), (100, 5000, S.U128), (1160, 2000, S.U128)],
                         ids=lambda v: getattr(v, "name", str(v)))
def test_score_ids_batch(dim, n, store):
    x, lo, hi, lv, enc = _store(dim, n, D.L2, False, store)
    rng = np.random.default_rng(dim)
    lengths = [0, 1, 300, 7, 0, 64, 129]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    ids = rng.integers(0, n, size=int(offs[-1])).astype(np.uint32)
    ids[2], ids[3], ids[4] = n - 1, 0, 1
    queries = _queries(x, lo, hi, len(lengths), dim + 3)
    for bits in BITS:
        want = _want_batch(lv, queries, lo, hi, dim, bits, D.L2, False)
        b = enc.encode_query_batch(queries, query_bits=bits, weighted=True)
        got = enc.score_ids_batch(b, offs, ids)
        for l in range(len(lengths)):
            sel = ids[offs[l]:offs[l + 1]]
            assert_bits_equal(got[offs[l]:offs[l + 1]], want[l][sel], f"list {l}, {bits} bits")


@pytest.mark.parametrize("n,nq,kernel", [(32768 + 37, 13, "bin_gemm_rs_kernel"), (5000, 3, "bin_topk_small_kernel")])
def test_topk_batch_rescored_is_rerank_of_topk_batch(n, nq, kernel):
    dim, k, cand = 100, 10, 60
    x, lo, hi, lv, enc = _store(dim, n, D.Dot, False, S.U128)
    orig = qa.OriginalVectors.from_data(x, qa.VectorParameters(dim, n, D.Dot, False))
    queries = _queries(x, lo, hi, nq, 21)
    for bits in BITS:
        b = enc.encode_query_batch(queries, query_bits=bits, weighted=True)
        assert enc.batch_kernel(b, cand) == kernel
        ids_c, _ = enc.topk_batch(b, cand)
        ids_r, sc_r = enc.topk_batch_rescored(b, orig, queries, k, cand)
        for qi in range(nq):
            wid, wsc = orig.rerank(queries[qi], ids_c[qi], k)
            assert np.array_equal(ids_r[qi], wid), (bits, qi)
            assert_bits_equal(sc_r[qi], wsc, "rescored scores")


# ------------------------------------------------------------------------------------------------ everything else
def test_on_one_bit_rows_weighted_is_unweighted():
    dim, n = 200, 500
    rng = np.random.default_rng(3)
    x = rng.normal(size=(n, dim)).astype(f32)
    enc = E.encode(x, qa.VectorParameters(dim, n, D.Dot, False))
    rows = enc.storage_bytes()
    queries = rng.normal(size=(6, dim)).astype(f32)
    queries[1, 0], queries[2, 5], queries[3] = np.nan, np.inf, 0
    q = b = None
    for bits in (1, 4, 8):
        for weighted in (True, False, True):  # one object moves between the two calls
            b = enc.encode_query_batch(queries, b, query_bits=bits, weighted=weighted)
            for qi, query in enumerate(queries):
                q = enc.encode_query(query, q, query_bits=bits, weighted=weighted)
                plain = enc.encode_query(query, query_bits=bits)
                _same(q.encoded_vector, plain.encoded_vector, f"query {qi}, {bits} bits")
                _same(np.float32(q.max_abs), np.float32(plain.max_abs), "max_abs")
                _same(b.encoded_vector(qi), plain.encoded_vector, "batch")
                if bits != 1:  # and what they were: the oracle of util.py
                    assert_bits_equal(enc.score_all(q), scalar_scores(rows, scalar_codes(query, bits)[0], dim, bits, D.Dot, False),
                                      "scores of a scalar query on one-bit rows")
            assert_bits_equal(enc.score_batch(b), np.stack([enc.score_all(enc.encode_query(qq, query_bits=bits)) for qq in queries]),
                              "score_batch")


def test_refusals():
    dim, n = 40, 10
    x = np.random.default_rng(1).normal(size=(n, dim)).astype(f32)
    lo, hi = np.full(dim, -0.5, f32), np.full(dim, 0.5, f32)
    enc = E.encode(x, qa.VectorParameters(dim, n, D.Dot, False), encoding=TWO, thresholds=(lo, hi))
    for bits in (0, 2, 3, 5, 7, 9, 16):
        with pytest.raises(qa.EncodingError):
            enc.encode_query(x[0], query_bits=bits, weighted=True)
        with pytest.raises(qa.EncodingError):
            enc.encode_query_batch(x[:3], query_bits=bits, weighted=True)
    for bad in (dim - 1, dim + 1):
        with pytest.raises(qa.EncodingError):
            enc.encode_query(np.zeros(bad, f32), query_bits=8, weighted=True)
        with pytest.raises(qa.EncodingError):
            enc.encode_query_batch(np.zeros((2, bad), f32), query_bits=4, weighted=True)
    for bits in BITS:  # the unweighted calls refuse a two-bit handle as before
        with pytest.raises(qa.EncodingError):
            enc.encode_query(x[0], query_bits=bits)
        with pytest.raises(qa.EncodingError):
            enc.encode_query_batch(x[:3], query_bits=bits)
    # code_bits * L must stay below 2^24: 32 896 dimensions at 8 bits, 559 240 at 4
    for bits, most in ((8, 32896), (4, 559240)):
        for dim, ok in ((most, True), (most + 1, False)):
            lo, hi = np.zeros(dim, f32), np.ones(dim, f32)
            big = E.encode(np.ones((1, dim), f32), qa.VectorParameters(dim, 1, D.Dot, False), encoding=TWO, thresholds=(lo, hi))
            query = np.full(dim, 0.25, f32)
            query[-1] = 1
            if not ok:
                with pytest.raises(qa.EncodingError):
                    big.encode_query(query, query_bits=bits, weighted=True)
                with pytest.raises(qa.EncodingError):
                    big.encode_query_batch(query[None, :], query_bits=bits, weighted=True)
                continue
            L = (1 << bits) - 1
            q = big.encode_query(query, query_bits=bits, weighted=True)
            codes, a = w.weighted_codes(query, lo, hi, bits)
            assert a == 1 and (2 * dim * L) < (1 << 24)
            assert_bits_equal(big.score_all(q), w.scores(m.levels(np.ones((1, dim), f32), lo, hi), codes, dim, bits, D.Dot, False),
                              f"the longest {bits}-bit query")
            b = big.encode_query_batch(query[None, :], query_bits=bits, weighted=True)
            _same(b.encoded_vector(0), q.encoded_vector, "batch")


def test_save_and_load(tmp_path):
    dim, n = 100, 5000
    x, lo, hi, lv, enc = _store(dim, n, D.L2, False, S.U128)
    enc.save(tmp_path / "two.bin", tmp_path / "two.json")
    back = E.load(tmp_path / "two.bin", tmp_path / "two.json", qa.VectorParameters(dim, n, D.Dot, False), S.U128)
    queries = _queries(x, lo, hi, 5, 33)
    for bits in BITS:
        b0 = enc.encode_query_batch(queries, query_bits=bits, weighted=True)
        b1 = back.encode_query_batch(queries, query_bits=bits, weighted=True)
        for qi, query in enumerate(queries):
            q0 = enc.encode_query(query, query_bits=bits, weighted=True)
            q1 = back.encode_query(query, query_bits=bits, weighted=True)
            _same(q1.encoded_vector, q0.encoded_vector, "planes after load")
            _same(np.float32(q1.max_abs), np.float32(q0.max_abs), "max_abs after load")
            _same(b1.encoded_vector(qi), b0.encoded_vector(qi), "batch after load")
        assert_bits_equal(back.score_all(q1), enc.score_all(q0), "scores after load")


def test_the_other_queries_are_what_they_were():
    """A handful of calls against the oracles; the existing suites are the real guard."""
    dim, n = 100, 5000
    x, lo, hi, lv, enc = _store(dim, n, D.Dot, False, S.U128)
    rows = m.encode(x, lo, hi, m.U128)
    queries = _queries(x, lo, hi, 6, 44)
    qrows = m.encode(queries, lo, hi, m.U128)
    want = np.stack([m.score_all(rows, r, dim, m.DOT, False) for r in qrows])
    assert_bits_equal(enc.score_all(enc.encode_query(queries[0])), want[0], "two-bit query")
    assert_bits_equal(enc.score_batch(enc.encode_query_batch(queries)), want, "two-bit batch")
    one = E.encode(x, qa.VectorParameters(dim, n, D.Dot, False), store=S.U128)
    orows = one.storage_bytes()
    for bits in BITS:
        wantb = np.stack([scalar_scores(orows, scalar_codes(q, bits)[0], dim, bits, D.Dot, False) for q in queries])
        assert_bits_equal(one.score_all(one.encode_query(queries[0], query_bits=bits)), wantb[0], "scalar query, one-bit rows")
        b = one.encode_query_batch(queries, query_bits=bits)
        assert one.batch_kernel(b, 0) == "bin_gemm_rs_kernel"
        assert_bits_equal(one.score_batch(b), wantb, "scalar batch, one-bit rows")
    sign = np.where(np.unpackbits(orows, axis=1, bitorder="little")[:, :dim] != 0, 1.0, -1.0)
    qsign = np.where(queries[0] > 0, 1.0, -1.0)
    assert_bits_equal(one.score_all(one.encode_query(queries[0])), (sign @ qsign).astype(f32), "binary query, one-bit rows")


# ---------------------------------------------------------------------------------------------------- handle reuse
def _reuse_stores():
    """A: one-bit, dim 100, U128.  B: two-bit, dim 100, U128 (200 bits to a row, no multiple of 64), also at 4100 rows,
    where a batch of 6 takes the matrix cores.  C: two-bit, dim 20, U8 (the tiny rows).  D: one-bit, dim 1160, U128."""
    rng = np.random.default_rng(2024)

    def make(dim, n, store, encoding):
        x = rng.normal(size=(n, dim)).astype(f32)
        return E.encode(x, qa.VectorParameters(dim, n, D.Dot, False), store=store, encoding=encoding)

    one = qa.BinaryEncoding.OneBit
    return {"A": make(100, 300, S.U128, one), "B": make(100, 300, S.U128, TWO), "C": make(20, 300, S.U8, TWO),
            "D": make(1160, 300, S.U128, one), "B4100": make(100, 4100, S.U128, TWO)}


REUSE_STEPS = [("D", 1, False), ("B", 8, True), ("A", 4, False), ("C", 4, True), ("B", 1, False), ("D", 8, False), ("A", 1, False)]


def test_one_handle_through_every_kind_of_query():
    """A query handle and a batch handle reused across stores, encodings, row lengths, bit counts and query counts give
    what fresh ones give: the bytes they hold, and every score and top-k as raw bits."""
    stores = _reuse_stores()
    rng = np.random.default_rng(7)
    q = None
    for name, bits, weighted in REUSE_STEPS:
        enc, what = stores[name], f"single, store {name}, {bits} bits"
        query = rng.normal(size=enc.vector_parameters.dim).astype(f32)
        q = enc.encode_query(query, q, query_bits=bits, weighted=weighted)
        fresh = enc.encode_query(query, query_bits=bits, weighted=weighted)
        assert q.bits == fresh.bits == bits
        _same(q.encoded_vector, fresh.encoded_vector, what + ": encoded_vector")
        _same(np.float32(q.max_abs), np.float32(fresh.max_abs), what + ": max_abs")
        _same(enc.score_all(q), enc.score_all(fresh), what + ": score_all")
        for got, want in zip(enc.topk(q, 10), enc.topk(fresh, 10)):
            _same(got, want, what + ": topk")

    def check_batch(enc, b, queries, bits, weighted, what):
        fresh = enc.encode_query_batch(queries, query_bits=bits, weighted=weighted)
        assert b.bits == fresh.bits == bits
        for qi in range(len(queries)):
            _same(b.encoded_vector(qi), fresh.encoded_vector(qi), f"{what}: encoded_vector({qi})")
        _same(enc.score_batch(b), enc.score_batch(fresh), what + ": score_batch")
        for got, want in zip(enc.topk_batch(b, 10), enc.topk_batch(fresh, 10)):
            _same(got, want, what + ": topk_batch")

    b = None
    for name, bits, weighted in REUSE_STEPS:
        enc = stores[name]
        queries = rng.normal(size=(6, enc.vector_parameters.dim)).astype(f32)
        b = enc.encode_query_batch(queries, b, query_bits=bits, weighted=weighted)
        check_batch(enc, b, queries, bits, weighted, f"batch of 6, store {name}, {bits} bits")
    enc = stores["B4100"]  # shrink and regrow on the matrix route: a stale code image or C tail would show
    for bits in (8, 4):
        for nq in (6, 2, 6):
            queries = rng.normal(size=(nq, 100)).astype(f32)
            b = enc.encode_query_batch(queries, b, query_bits=bits, weighted=True)
            assert enc.batch_kernel(b, 0) == ("bin_gemm_rs_kernel" if nq == 6 else "bin_scan_kernel")
            check_batch(enc, b, queries, bits, True, f"batch of {nq}, 4100 rows, {bits} bits")
