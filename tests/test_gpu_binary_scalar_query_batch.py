"""Batches of scalar (4- and 8-bit) queries against binary rows: qamd_bin_encode_query_batch_scalar and every call that
takes the batch, on the matrix-core route (bin_gemm_rs_kernel with the centred int8 codes) and on the per-query routes.

Expected values are util.scalar_codes / scalar_planes / scalar_scores - the per-dimension oracle of DESIGN.md 3.2d, which
knows nothing of bit planes or of the matrix form - and the single-query calls of the same store.  Every comparison is on
raw f32 bit patterns and exact ids.  EncodedVectorsBin.batch_kernel (qamd_bin_batch_kernel) names the route each case
takes, so the route is asserted, not assumed.

Two things the shapes bring with them: 64 dimensions in a U8 store are 8-byte rows, which have no 16-byte pieces and so no
matrix route - those cases are kept, compared with the same oracle, and asserted to take bin_words_kernel (the heavy-tie
case uses a U128 store for the same reason); and at 32 805 rows k = 1024 asks for more sample ranks than the matrix
top-k's pivot pass has (r > 64), so inside that route every query is handed to the per-query path - same answers.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import quantization_amd as qa
from util import assert_bits_equal, scalar_codes, scalar_metric, scalar_planes, scalar_scores, scalar_xor

pytestmark = pytest.mark.gpu

D = qa.DistanceType
U8, U128 = qa.BitsStoreType.U8, qa.BitsStoreType.U128
STORES = (U8, U128)
BITS = (4, 8)
METRICS = [(dist, inv) for dist in (D.Dot, D.L2) for inv in (False, True)]  # both signs of the epilogue, both ways round
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")

N_SCORE = 4096 + 35   # the last 64-row chunk is partial and its second 32-row half partly past the end
N_TOPK = 32768 + 37


# ------------------------------------------------------------------ data
def row_bytes(dim, kind):
    return qa.EncodedVectorsBin.get_quantized_vector_size_from_params(qa.VectorParameters(dim, 1, D.Dot, False), kind)


def pack_rows(bits01, dim, kind):
    """0/1 per dimension -> rows in the store's own row size, pad bits zero as the encoder leaves them."""
    rows = np.zeros((bits01.shape[0], row_bytes(dim, kind)), dtype=np.uint8)
    packed = np.packbits(bits01.astype(np.uint8), axis=1, bitorder="little")
    rows[:, :packed.shape[1]] = packed
    return rows


def row_bits(n, dim, seed):
    """Random bits; row 0 all ones, row 1 all zeros, and so the last row of the store."""
    bits01 = np.random.default_rng(seed).integers(0, 2, size=(n, dim), dtype=np.uint8)
    bits01[0] = 1
    bits01[1] = 0
    bits01[n - 1] = 1
    return bits01


def queries_of(nq, dim, seed):
    """Gaussian queries; query 0 all +a (every code L), query 1 all -a (every code 0), query 2 all zero (every code
    (L + 1) / 2): with the all-ones row the first two give the extreme accumulators +127 dim and -128 dim."""
    q = np.random.default_rng(seed).standard_normal((nq, dim)).astype(np.float32)
    q[0] = 2.5
    if nq > 1:
        q[1] = -2.5
    if nq > 2:
        q[2] = 0.0
    return q


def open_rows(rows, dim, dist=D.Dot, invert=False, kind=U8):
    return qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(dim, rows.shape[0], dist, invert), store=kind)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def oracle_x(bits01, queries, dim, bits):
    """int64 [n_queries, n]: X of every (query, row), from the per-dimension oracle, on the bits alone (row padding
    plays no part in it, so both store kinds share it)."""
    rows = pack_rows(bits01, dim, U128)
    return np.stack([scalar_xor(rows, scalar_codes(q, bits)[0], dim, bits) for q in queries])


def check_scores(enc, batch, queries, x, dim, bits, dist, inv, what, singles=True):
    got = enc.score_batch(batch)
    want = scalar_metric(x[:len(queries)], dim, bits, dist, inv)
    assert got.shape == want.shape
    assert_bits_equal(got, want, what + ": score_batch against the oracle")
    if singles:
        for qi, query in enumerate(queries):
            one = enc.score_all(enc.encode_query(query, query_bits=bits))
            assert_bits_equal(got[qi], one, f"{what}: query {qi} against score_all of the single query")


# ------------------------------------------------------------------ encode
ENCODE_DIMS = (1, 63, 64, 200, 1160)


def encode_queries(dim):
    rng = np.random.default_rng(900 + dim)
    q = rng.standard_normal((9, dim)).astype(np.float32)
    q[0] = 0.0                 # all zero: a = 0, every code (L + 1) / 2
    q[1] = 3.0                 # all +a
    q[2] = -3.0                # all -a
    q[3, 0] = np.nan           # NaN counts as 0.0f and does not enter a
    q[4, 0] = np.inf           # +-inf do not enter a; codes L and 0
    q[4, dim // 2] = -np.inf
    q[5] *= np.float32(2.0 ** -10)  # max |q| of these two differ by 2^20: a is per query, never per batch
    q[6] = q[5] * np.float32(2.0 ** 20)
    q[7, dim - 1] = np.nan
    q[8, :] = -0.0
    return q


@pytest.mark.parametrize("kind", STORES, ids=lambda k: k.name)
@pytest.mark.parametrize("dim", ENCODE_DIMS)
def test_encode_matches_the_single_query_and_the_oracle(dim, kind):
    enc = open_rows(pack_rows(row_bits(8, dim, dim), dim, kind), dim, kind=kind)
    queries = encode_queries(dim)
    nb = row_bytes(dim, kind)
    for bits in BITS:
        batch = enc.encode_query_batch(queries, query_bits=bits)
        assert batch.bits == bits and batch.n_queries == len(queries)
        for qi, query in enumerate(queries):
            got = batch.encoded_vector(qi)
            single = enc.encode_query(query, query_bits=bits)
            want = scalar_planes(scalar_codes(query, bits)[0], bits, nb)
            assert got.shape == (bits, nb)
            assert np.array_equal(got, single.encoded_vector), f"dim {dim} bits {bits} query {qi}: batch != encode_query"
            assert np.array_equal(got, want), f"dim {dim} bits {bits} query {qi}: batch != oracle planes"


def test_a_batch_is_reused_across_bit_counts():
    dim = 200
    enc = open_rows(pack_rows(row_bits(8, dim, 1), dim, U8), dim)
    nb = row_bytes(dim, U8)
    batch = None
    for bits, nq in ((8, 9), (1, 4), (4, 7), (8, 2)):
        queries = encode_queries(dim)[:nq]
        got = enc.encode_query_batch(queries, reuse=batch, query_bits=bits)
        assert batch is None or got is batch
        batch = got
        assert batch.bits == bits and batch.n_queries == nq
        for qi, query in enumerate(queries):
            if bits == 1:
                want = enc.encode_query(query).encoded_vector
            else:
                want = scalar_planes(scalar_codes(query, bits)[0], bits, nb)
            assert np.array_equal(batch.encoded_vector(qi), want), (bits, qi)
        # and the batch scores as what it now holds
        x = oracle_x(row_bits(8, dim, 1), queries, dim, bits) if bits != 1 else None
        got_sc = enc.score_batch(batch)
        for qi, query in enumerate(queries):
            if bits == 1:
                want_sc = enc.score_all(enc.encode_query(query))
            else:
                want_sc = scalar_metric(x[qi], dim, bits, D.Dot, False)
            assert_bits_equal(got_sc[qi], want_sc, f"reused batch at {bits} bits, query {qi}")


# ------------------------------------------------------------------ score_batch on the matrix cores
# 64: one K-block (U128 store; the U8 store's 8-byte rows stay off the matrix cores); 200: pad bits inside a K-block;
# 1024: exactly one 8-block register pass; 1160: a second pass with nk < 8
MATRIX_DIMS = (64, 200, 1024, 1160)
BATCHES = (5, 33, 65)  # one partly filled tile; a partly filled second tile; the two-fragment tile, last tile partial


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("dim", MATRIX_DIMS)
def test_score_batch_on_the_matrix_cores(dim, bits):
    n = N_SCORE
    bits01 = cached(("score bits", dim), lambda: row_bits(n, dim, 4000 + dim))
    queries = cached(("score queries", dim), lambda: queries_of(max(BATCHES), dim, 5000 + dim))
    x = oracle_x(bits01, queries, dim, bits)
    assert x[0, 0] == 0 and x[1, 0] == dim * ((1 << bits) - 1)  # the all-ones row against all-L and all-0 codes
    for kind in STORES:
        rows = pack_rows(bits01, dim, kind)
        for dist, inv in METRICS:
            enc = open_rows(rows, dim, dist, inv, kind)
            for nq in BATCHES:
                batch = enc.encode_query_batch(queries[:nq], query_bits=bits)
                # (64 dims in a U8 store are 8-byte rows: no 16-byte pieces, so no matrix route - scanned dword by dword)
                assert enc.batch_kernel(batch, 0) == ("bin_gemm_rs_kernel" if rows.shape[1] % 16 == 0 else "bin_words_kernel")
                what = f"{n}x{dim} {kind.name} {dist.name} invert={inv} bits {bits}, {nq} queries"
                # the single queries once per store and metric (the 65-query batch covers the others' queries)
                check_scores(enc, batch, queries[:nq], x, dim, bits, dist, inv, what, singles=nq == max(BATCHES))


# ------------------------------------------------------------------ score_batch off the matrix cores
# (n, dim, store, kernel): under the row gate; under 64 dims (8-byte rows are scanned dword by dword, 16-byte rows piece
# by piece); a query tile that does not fit LDS (bin_mfma_frags == 0: more than 39 K-blocks)
FALLBACKS = [
    (100, 200, U8, "bin_scan_kernel"),
    (N_SCORE, 40, U128, "bin_scan_kernel"),
    (N_SCORE, 40, U8, "bin_words_kernel"),
    (N_SCORE, 5200, U8, "bin_scan_kernel"),
]


@pytest.mark.parametrize("n,dim,kind,kernel", FALLBACKS, ids=[f"{f[0]}x{f[1]}-{f[2].name}" for f in FALLBACKS])
def test_score_batch_falls_back_query_by_query(n, dim, kind, kernel):
    bits01 = row_bits(n, dim, n + dim)
    rows = pack_rows(bits01, dim, kind)
    queries = queries_of(7, dim, 6000 + dim)
    for bits in BITS:
        x = oracle_x(bits01, queries, dim, bits)
        for dist, inv in METRICS:
            enc = open_rows(rows, dim, dist, inv, kind)
            batch = enc.encode_query_batch(queries, query_bits=bits)
            assert enc.batch_kernel(batch, 0) == kernel
            check_scores(enc, batch, queries, x, dim, bits, dist, inv, f"{n}x{dim} {kind.name} {dist.name} invert={inv} bits {bits}")


# ------------------------------------------------------------------ topk_batch
def check_topk_batch(enc, batch, queries, bits01, dim, bits, dist, inv, k, largest, what):
    """Ids and scores equal topk of each single scalar query; the scores equal the oracle's at those ids."""
    ids, sc = enc.topk_batch(batch, k, largest=largest)
    assert ids.shape == (len(queries), k)
    for qi, query in enumerate(queries):
        one_ids, one_sc = enc.topk(enc.encode_query(query, query_bits=bits), k, largest=largest)
        assert np.array_equal(ids[qi], one_ids), f"{what} k={k} largest={largest} query {qi}: ids differ from topk"
        assert_bits_equal(sc[qi], one_sc, f"{what} k={k} largest={largest} query {qi}: scores against topk")
        at = pack_rows(bits01[ids[qi]], dim, U128)
        want = scalar_scores(at, scalar_codes(query, bits)[0], dim, bits, dist, inv)
        assert_bits_equal(sc[qi], want, f"{what} k={k} largest={largest} query {qi}: scores against the oracle")
    return ids, sc


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("kind", STORES, ids=lambda k: k.name)
@pytest.mark.parametrize("dim", (200, 1024))
def test_topk_batch_on_the_matrix_cores(dim, kind, bits):
    n = N_TOPK
    bits01 = cached(("topk bits", dim), lambda: row_bits(n, dim, 7000 + dim))
    queries = cached(("topk queries", dim), lambda: queries_of(70, dim, 8000 + dim))
    rows = pack_rows(bits01, dim, kind)
    # the metric: Dot at 4 bits, inverted L2 at 8 (multiplier +4), and the other sign on the other store kind
    dist, inv = (D.Dot, kind == U128) if bits == 4 else (D.L2, kind == U8)
    enc = open_rows(rows, dim, dist, inv, kind)
    for nq in (12, 70):
        batch = enc.encode_query_batch(queries[:nq], query_bits=bits)
        for k in (1, 30, 1024):
            assert enc.batch_kernel(batch, k) == "bin_gemm_rs_kernel"
            for largest in (True, False):
                check_topk_batch(enc, batch, queries[:nq], bits01, dim, bits, dist, inv, k, largest,
                                 f"{n}x{dim} {kind.name} {dist.name} invert={inv} bits {bits}, {nq} queries")


def test_topk_batch_of_64_copies_of_one_query():
    """Near-duplicate queries: a passing row appends to every query's list at once."""
    n, dim, bits = N_TOPK, 200, 8
    bits01 = cached(("topk bits", dim), lambda: row_bits(n, dim, 7000 + dim))
    enc = open_rows(pack_rows(bits01, dim, U8), dim)
    queries = np.repeat(queries_of(4, dim, 11)[3:4], 64, axis=0)
    batch = enc.encode_query_batch(queries, query_bits=bits)
    assert enc.batch_kernel(batch, 30) == "bin_gemm_rs_kernel"
    ids, sc = check_topk_batch(enc, batch, queries, bits01, dim, bits, D.Dot, False, 30, True, "64 copies")
    assert np.array_equal(ids, np.repeat(ids[:1], 64, axis=0)) and np.array_equal(sc.view(np.uint32), np.repeat(sc[:1], 64, axis=0).view(np.uint32))


def test_topk_batch_falls_back_query_by_query():
    n, dim = 5000, 200
    bits01 = row_bits(n, dim, 5)
    queries = queries_of(3, dim, 6)
    for kind in STORES:
        enc = open_rows(pack_rows(bits01, dim, kind), dim, D.L2, False, kind)
        for bits in BITS:
            batch = enc.encode_query_batch(queries, query_bits=bits)
            for k in (1, 30, 100):
                assert not enc.batch_kernel(batch, k).startswith("bin_gemm")
                for largest in (True, False):
                    check_topk_batch(enc, batch, queries, bits01, dim, bits, D.L2, False, k, largest, f"{n}x{dim} {kind.name} bits {bits}")


# ---- heavy ties: the redo path, proven by the developer build's debug line (a U128 store: 64 dims are one 16-byte piece
# there; the U8 store's 8-byte rows never reach the matrix cores)
TIE_DIM, TIE_BITS, TIE_Q, TIE_K = 64, 4, 12, 30


def tie_case():
    """Rows drawn from 16 patterns, 60% of them pattern 0; queries 0..5 agree in sign with pattern 0 (their best rows are
    ~19 700 ties: the candidate lists overflow), queries 6..8 with its complement (the same for the smallest scores)."""
    rng = np.random.default_rng(64)
    patterns = rng.integers(0, 2, size=(16, TIE_DIM), dtype=np.uint8)
    which = np.where(rng.random(N_TOPK) < 0.6, 0, rng.integers(1, 16, size=N_TOPK))
    bits01 = patterns[which]
    queries = rng.standard_normal((TIE_Q, TIE_DIM)).astype(np.float32)
    sign = patterns[0].astype(np.float32) * 2 - 1
    queries[:6] = np.abs(queries[:6]) * sign
    queries[6:9] = -np.abs(queries[6:9]) * sign
    return bits01, queries


def tie_child(out_path):
    bits01, queries = tie_case()
    enc = open_rows(pack_rows(bits01, TIE_DIM, U128), TIE_DIM, kind=U128)
    batch = enc.encode_query_batch(queries, query_bits=TIE_BITS)
    R = {"kernel": np.frombuffer(enc.batch_kernel(batch, TIE_K).encode(), dtype=np.uint8)}
    for largest in (True, False):
        print(f"STEP largest={largest}", file=sys.stderr, flush=True)
        ids, sc = enc.topk_batch(batch, TIE_K, largest=largest)
        R[f"ids{int(largest)}"], R[f"sc{int(largest)}"] = ids, sc
    print("STEP end", file=sys.stderr, flush=True)
    np.savez(out_path, **R)
    print("DONE")


def test_topk_batch_under_heavy_ties_redoes_queries(tmp_path):
    assert os.path.exists(DEV_LIB), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(QAMD_DEBUG_TOPK="1", QAMD_LIB_PATH=DEV_LIB)
    out = os.path.join(str(tmp_path), "ties.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_binary_scalar_query_batch as T\nT.tie_child(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"exit {res.returncode}\n{res.stderr[-4000:]}"
    R = np.load(out)
    assert R["kernel"].tobytes().decode() == "bin_gemm_rs_kernel"
    lines = [ln for ln in res.stderr.splitlines() if ln.startswith("[qamd bin topk_batch]")]
    assert len(lines) == 2, res.stderr[-4000:]
    for ln in lines:
        m = re.search(r"Q=12 r=\d+ candidates min/mean/max = \d+/\d+/\d+, filter (\w+), (\d+) queries redone, query bits 4$", ln)
        assert m, ln
        assert m.group(1) == "bin_gemm_rs_kernel" and int(m.group(2)) >= 1, ln
    # the answers: those of the single queries (this process, the product library) and of the oracle
    bits01, queries = tie_case()
    enc = open_rows(pack_rows(bits01, TIE_DIM, U128), TIE_DIM, kind=U128)
    rows128 = pack_rows(bits01, TIE_DIM, U128)
    for largest in (True, False):
        ids, sc = R[f"ids{int(largest)}"], R[f"sc{int(largest)}"]
        for qi, query in enumerate(queries):
            one_ids, one_sc = enc.topk(enc.encode_query(query, query_bits=TIE_BITS), TIE_K, largest=largest)
            assert np.array_equal(ids[qi], one_ids), f"largest={largest} query {qi}: ids"
            assert_bits_equal(sc[qi], one_sc, f"largest={largest} query {qi}: scores")
            want = scalar_scores(rows128[ids[qi]], scalar_codes(query, TIE_BITS)[0], TIE_DIM, TIE_BITS, D.Dot, False)
            assert_bits_equal(sc[qi], want, f"largest={largest} query {qi}: scores against the oracle")
    # and the product library gives the same through the same route
    batch = enc.encode_query_batch(queries, query_bits=TIE_BITS)
    assert enc.batch_kernel(batch, TIE_K) == "bin_gemm_rs_kernel"
    for largest in (True, False):
        ids, sc = enc.topk_batch(batch, TIE_K, largest=largest)
        assert np.array_equal(ids, R[f"ids{int(largest)}"]) and np.array_equal(sc.view(np.uint32), R[f"sc{int(largest)}"].view(np.uint32))


# ------------------------------------------------------------------ score_ids_batch
@pytest.mark.parametrize("dim,kind", [(200, U8), (40, U8), (1160, U128)], ids=lambda v: getattr(v, "name", str(v)))
def test_score_ids_batch(dim, kind):
    n = 1500
    bits01 = row_bits(n, dim, 30 + dim)
    enc = open_rows(pack_rows(bits01, dim, kind), dim, D.L2, True, kind)
    rng = np.random.default_rng(dim)
    lengths = [0, 1, 300, 7, 0, 64, 129]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    ids = rng.integers(0, n, size=int(offs[-1])).astype(np.uint32)
    ids[2], ids[3] = ids[1], n - 1       # repeated ids, the last row
    ids[offs[3]] = n - 1
    ids[offs[6]:offs[6] + 4] = ids[offs[6]]
    queries = queries_of(len(lengths), dim, 40 + dim)
    for bits in BITS:
        batch = enc.encode_query_batch(queries, query_bits=bits)
        got = enc.score_ids_batch(batch, offs, ids)
        for l, query in enumerate(queries):
            single = enc.encode_query(query, query_bits=bits)
            sel = ids[offs[l]:offs[l + 1]]
            want = np.array([enc.score_point(single, int(i)) for i in sel], dtype=np.float32)
            assert_bits_equal(got[offs[l]:offs[l + 1]], want, f"dim {dim} {kind.name} bits {bits}, list {l}")
            oracle = scalar_scores(pack_rows(bits01[sel], dim, U128), scalar_codes(query, bits)[0], dim, bits, D.L2, True)
            assert_bits_equal(want, oracle, f"dim {dim} {kind.name} bits {bits}, list {l}: score_point against the oracle")


# ------------------------------------------------------------------ topk_batch_rescored
@pytest.mark.parametrize("n,nq", [(N_TOPK, 13), (5000, 3)], ids=["matrix", "per-query"])
def test_topk_batch_rescored_is_rerank_of_topk_batch(n, nq):
    dim, k, cand = 200, 10, 100
    rng = np.random.default_rng(n)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    enc = qa.EncodedVectorsBin.encode(data, vp)
    orig = qa.OriginalVectors.from_data(data, vp)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    for bits in BITS:
        batch = enc.encode_query_batch(queries, query_bits=bits)
        assert enc.batch_kernel(batch, cand).startswith("bin_gemm_rs_kernel") == (n == N_TOPK)
        ids_c, _ = enc.topk_batch(batch, cand)
        ids_r, sc_r = enc.topk_batch_rescored(batch, orig, queries, k, cand)
        for qi in range(nq):
            want_ids, want_sc = orig.rerank(queries[qi], ids_c[qi], k)
            assert np.array_equal(ids_r[qi], want_ids), f"bits {bits} query {qi}: rescored ids"
            assert_bits_equal(sc_r[qi], want_sc, f"bits {bits} query {qi}: rescored scores")


# ------------------------------------------------------------------ unchanged behaviour
def test_binary_batches_are_what_they_were():
    dim, n = 1024, N_TOPK
    bits01 = cached(("topk bits", dim), lambda: row_bits(n, dim, 7000 + dim))
    enc = open_rows(pack_rows(bits01, dim, U8), dim)
    queries = queries_of(16, dim, 3)
    old = qa._base.EncodedVectorsBase.encode_query_batch(enc, queries)  # the call as it was: qamd_bin_encode_query_batch
    new = enc.encode_query_batch(queries, query_bits=1)
    assert old.bits == 1 and new.bits == 1
    for qi, query in enumerate(queries):
        want = enc.encode_query(query).encoded_vector
        assert np.array_equal(new.encoded_vector(qi), want) and np.array_equal(old.encoded_vector(qi), want), qi
    assert_bits_equal(enc.score_batch(new), enc.score_batch(old), "binary batch through the new signature")
    # a 1024-bit store: 16 binary queries filter on the FP4 matrix cores, 16 scalar queries on the int8 ones
    assert enc.batch_kernel(new, 30) == "bin_gemm_rs4_kernel" and enc.batch_kernel(new, 0) == "bin_gemm_rs_kernel"
    for bits in BITS:
        scalar = enc.encode_query_batch(queries, query_bits=bits)
        assert enc.batch_kernel(scalar, 30) == "bin_gemm_rs_kernel" and enc.batch_kernel(scalar, 0) == "bin_gemm_rs_kernel"
    many = enc.encode_query_batch(queries_of(400, dim, 4))
    assert enc.batch_kernel(many, 30) in ("bin_gemm_rs4_kernel", "bin_gemm_qs4_kernel")
    # per-query routes of binary batches
    small = open_rows(pack_rows(bits01[:3000], dim, U8), dim)
    assert small.batch_kernel(small.encode_query_batch(queries), 0) == "bin_scan_multi_kernel"
    assert small.batch_kernel(small.encode_query_batch(queries), 10) == "bin_topk_small_kernel"
    other = open_rows(pack_rows(row_bits(8, 200, 1), 200, U8), 200)
    with pytest.raises(qa.EncodingError):
        other.batch_kernel(new, 0)
