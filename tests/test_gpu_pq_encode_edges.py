"""The PQ encoder side of csrc/pq.hip at its edges: assignment on ties and special values, every way in, the chunk loop's
slicing, and the query tables on special values - against the oracle (oracle/qoracle.c), byte for byte / bit for bit.

Routes follow from shapes (cs_fast_shape in pq.hip): dim % chunk == 0 and chunk in {1, 2, 4, 8, 16, 32} take
`pq_encode_cs_kernel<chunk>` (two centroids per packed-f32 instruction, the pair table through the scalar cache, software-
pipelined one step ahead); everything else takes `pq_encode_kernel` (centroids in LDS).  Both claim the reference's walk:
index order, strict '<', a sequential uncontracted f32 sum, f32::MAX start.  The inputs come from tests/util.py and are
proven to be decided by exactly those properties in tests/test_pq_encode_model.py (no GPU needed there).

NaN rule for tables and scores: where the oracle has a NaN any NaN is accepted (an x86 NaN and a GPU default NaN differ in
the sign bit); everywhere else the bits must match, the sign of zero included.  A query batch has no table read-back, so
`encode_query_batch` is checked through `score_batch` against single queries, and the transposed table ([code][chunk],
written separately from the row-major one) through the whole-store scans that read it."""
import numpy as np
import pytest

import util
from util import assert_bits_equal_nan, describe_code_mismatches, pq_near_tie_table, pq_special_case

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
torch = pytest.importorskip("torch")
D = qa.DistanceType

CS_SHAPES = util.PQ_EDGE_CS_SHAPES            # (chunk, dim): pq_encode_cs_kernel<chunk>
GENERIC_SHAPES = util.PQ_EDGE_GENERIC_SHAPES  # pq_encode_kernel; (40, 33): chunk > dim
ROW_COUNTS = util.PQ_EDGE_ROW_COUNTS          # none a multiple of the 256-row workgroup


def cs_fast_shape(dim, chunk):
    return dim % chunk == 0 and chunk in (1, 2, 4, 8, 16, 32)


def _ties(chunk, dim, n=max(ROW_COUNTS)):
    """The shape's largest near-tie table (or its first n rows)."""
    data, cen, _cases = util.pq_edge_tie_tables(chunk, dim)[-1]
    return data[:n], cen


_oracle_codes = {}


def _want(qo, key, data, chunk, cen):
    """qo.pq_encode, computed once per input and shared by the tests that need it."""
    if key not in _oracle_codes:
        _oracle_codes[key] = qo.pq_encode(data, chunk, cen)
        _oracle_codes[key].setflags(write=False)
    return _oracle_codes[key]


def _encode(data, dim, chunk, cen, **kw):
    n = int(data.shape[0])
    return qa.EncodedVectorsPQ.encode(data, qa.VectorParameters(dim, n, D.L2, False), chunk, centroids=cen, **kw)


def _assert_codes(got, want, data, cen, chunk):
    got = np.asarray(got)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        raise AssertionError(describe_code_mismatches(got, want, data, cen, chunk))


# ------------------------------------------------------------------ (a) every instantiation on ties and special values
@pytest.mark.parametrize("chunk,dim", CS_SHAPES + GENERIC_SHAPES)
def test_encode_near_ties_every_instantiation(qo, chunk, dim):
    """Rows between two centroids at (nearly) equal f32 distance, at both halves of a centroid pair, across pairs and
    pipeline steps, at 0 / 1 and 254 / 255: the code is decided by the sum order, by contraction or by the strict '<'.
    Three tables per shape (257, 1000 and 2051 rows), each leading with another of the three kinds."""
    assert cs_fast_shape(dim, chunk) == ((chunk, dim) in CS_SHAPES)
    for v, (data, cen, _cases) in enumerate(util.pq_edge_tie_tables(chunk, dim)):
        assert data.shape[0] == ROW_COUNTS[v]
        want = _want(qo, ("ties", chunk, dim, v), data, chunk, cen)
        _assert_codes(_encode(data, dim, chunk, cen).storage_bytes(), want, data, cen, chunk)


@pytest.mark.parametrize("chunk,dim", CS_SHAPES + GENERIC_SHAPES)
def test_encode_special_values_every_instantiation(qo, chunk, dim):
    """NaN in a row / in centroids, infinities, differences that overflow, subnormals (kept, not flushed), -0.0: the
    codes are the oracle's, which test_pq_encode_model.py pins literally."""
    rows, cen, literal = pq_special_case(dim, chunk)
    n = 1000
    data = np.ascontiguousarray(rows[np.arange(n) % rows.shape[0]])
    want = _want(qo, ("special", chunk, dim), data, chunk, cen)
    assert np.array_equal(want[:rows.shape[0]], literal)
    enc = _encode(data, dim, chunk, cen)
    _assert_codes(enc.storage_bytes(), want, data, cen, chunk)


# ------------------------------------------------------------------ (b) ways in
@pytest.mark.parametrize("chunk,dim", [(8, 64), (2, 16), (7, 100)])
def test_encode_ways_in_give_the_same_bytes(qo, chunk, dim):
    """Host array, a torch CUDA tensor read in place, and encode_stream with ragged batches (1, 255, 256, 257, the rest;
    host and device batches)."""
    data, cen = _ties(chunk, dim)
    n = data.shape[0]
    want = _want(qo, ("ties", chunk, dim, 2), data, chunk, cen)
    vp = qa.VectorParameters(dim, n, D.L2, False)
    dev = torch.from_numpy(data).cuda()
    _assert_codes(_encode(dev, dim, chunk, cen).storage_bytes(), want, data, cen, chunk)
    cuts = np.cumsum([0, 1, 255, 256, 257])
    bounds = list(zip(cuts, list(cuts[1:]) + [n]))
    assert bounds[-1] == (769, n) and n > 769
    for src in (data, dev):
        batches = lambda src=src: iter([src[a:b] for a, b in bounds])
        st = qa.EncodedVectorsPQ.encode_stream(batches, vp, chunk, centroids=cen)
        _assert_codes(st.storage_bytes(), want, data, cen, chunk)


# ------------------------------------------------------------------ (c) the chunk loop's slices
def _slicing(n, m):
    """launch_assign's arithmetic (pq.hip): (gx, want, slices, per)."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    want = 4 * cu
    gx = (n + 255) // 256
    slices = 1
    if gx < want:
        slices = min(m, (want + gx - 1) // gx)
    per = (m + slices - 1) // slices
    slices = (m + per - 1) // per
    return gx, want, slices, per


def _mixed(qo, chunk, dim, n, seed):
    """Random rows around the near-tie table's centroids with its near-tie rows mixed in (every 1/400th row, the
    first and the last)."""
    ties, cen, _cases = pq_near_tie_table(dim, chunk, 700, seed=chunk * 1000 + dim)
    rng = np.random.default_rng(seed)
    data = ties[rng.integers(0, ties.shape[0], n)] + rng.standard_normal((n, dim), dtype=np.float32) * np.float32(0.3)
    at = np.unique(np.concatenate([np.arange(0, n, max(1, n // 400)), [n - 1]]))
    data[at] = ties[np.arange(at.size) % ties.shape[0]]
    data = np.ascontiguousarray(data, dtype=np.float32)
    return data, cen, qo.pq_encode(data, chunk, cen)


@pytest.mark.parametrize("chunk,dim,n,kind", [(1, 131, 257, "per1"), (3, 392, 257, "per1"),
                                              (1, 131, 2001, "per2_last1"), (3, 392, 2001, "per2_last1"),
                                              (2, 6, 262_145, "one_slice"), (3, 7, 262_145, "one_slice")])
def test_encode_chunk_loop_slices(qo, chunk, dim, n, kind):
    """launch_assign splits the chunk loop over blockIdx.y when there are few row blocks: one chunk per slice, two per
    slice with a ragged last slice of one (c_end = min(m, ...)), and one slice looping over all chunks.  chunk 1 / 2:
    pq_encode_cs_kernel, chunk 3: pq_encode_kernel (its LDS table is reloaded per chunk of the loop)."""
    m = qo.pq_chunks(dim, chunk)
    gx, want, slices, per = _slicing(n, m)
    if kind == "per1":
        assert per == 1 and slices == m
    elif kind == "per2_last1":
        assert per == 2 and slices == (m + 1) // 2 and m - (slices - 1) * per == 1
    else:
        assert gx >= want and slices == 1 and per == m > 1
    data, cen, codes = _mixed(qo, chunk, dim, n, seed=n + dim)
    enc = _encode(data, dim, chunk, cen)
    _assert_codes(enc.storage_bytes(), codes, data, cen, chunk)


# ------------------------------------------------------------------ (d) count <= 256 from device-resident data
@pytest.mark.parametrize("n,chunk,dim", [(256, 4, 32), (100, 7, 100), (1, 2, 6)])
def test_encode_small_count_device_resident(qo, n, chunk, dim):
    """count <= 256: the centroids are the vectors themselves, zero-filled (encoded_vectors_pq.rs:290-297); device-
    resident data are copied out for that (the copy_out branch of qamd_pq_encode)."""
    data = _ties(chunk, dim)[0][:n]
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    host = qa.EncodedVectorsPQ.encode(data, vp, chunk)
    dev = qa.EncodedVectorsPQ.encode(torch.from_numpy(data).cuda(), vp, chunk)
    cen = qo.pq_centroids_small(data)
    want = qo.pq_encode(data, chunk, cen)
    for enc in (host, dev):
        util.assert_bits_equal(enc.centroids, cen, "centroids")
        _assert_codes(enc.storage_bytes(), want, data, cen, chunk)


# ------------------------------------------------------------------ (e) query tables
SPECIAL_CODES = (2, 3, 4, 5, 6)                         # NaN, +inf, -inf, 3e38, -3e38 (util.PQ_SPECIAL_CENTROIDS)
FINITE_CODES = np.array([0, 1, 7, 8, 9, 10, 11] + list(range(12, 256)), dtype=np.uint8)
METRICS = [(D.Dot, False), (D.Dot, True), (D.L1, False), (D.L1, True), (D.L2, False), (D.L2, True)]


def _special_queries(dim, seed):
    """Six queries: plain values; zeros of both signs and subnormals; +-3e38; infinities; one NaN; a mix of all."""
    rng = np.random.default_rng(seed)
    base = (rng.random((6, dim), dtype=np.float32) * 4 - 2).astype(np.float32)
    pools = [None, [0.0, -0.0, 1e-40, -1e-40, 2e-20], [3e38, -3e38, 1.0], [np.inf, -np.inf, 0.5], [np.nan],
             [0.0, -0.0, 1e-40, 3e38, -3e38, np.inf, -np.inf, np.nan, 1000.25]]
    for q, pool in enumerate(pools):
        if pool is None:
            continue
        k = 1 if q == 4 else max(1, dim // 3)
        at = rng.choice(dim, size=k, replace=False)
        base[q, at] = np.array(pool, dtype=np.float32)[rng.integers(0, len(pool), k)]
    return base


@pytest.mark.parametrize("dim,chunk", [(16, 1), (31, 2), (10, 3), (50, 20), (64, 8)])
def test_query_tables_on_special_values(qo, dim, chunk):
    """pq_lut_kernel: q.lut against qo.pq_encode_query for Dot / L1 / L2, with and without invert (-0.0 under invert,
    NaN and infinite entries), shapes with a ragged last chunk."""
    _rows, cen, _ = pq_special_case(dim, chunk)
    m = qo.pq_chunks(dim, chunk)
    rows = np.zeros((8, m), dtype=np.uint8)
    queries = _special_queries(dim, seed=dim)
    signs = set()
    for dist, invert in METRICS:
        enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(dim, 8, dist, invert), chunk, cen)
        for q in queries:
            want = qo.pq_encode_query(q, chunk, cen, int(dist), invert)
            assert_bits_equal_nan(enc.encode_query(q).lut, want, f"lut {dist} invert={invert}")
            signs |= set(util.bits(want[want == 0]).tolist())
            nan_chunks = np.flatnonzero(np.isnan(np.pad(q, (0, m * chunk - dim)).reshape(m, chunk)).any(axis=1))
            assert np.isnan(want.reshape(m, 256)[nan_chunks]).all(), "a NaN query entry makes its chunk's whole table NaN"
    assert signs == {0x00000000, 0x80000000}, "the tables hold zeros of both signs"


def _special_store_rows(n, m, seed, special=SPECIAL_CODES):
    """Codes of mostly finite centroids; 30 % of the rows carry one special code, 10 % two."""
    rng = np.random.default_rng(seed)
    rows = FINITE_CODES[rng.integers(0, FINITE_CODES.size, (n, m))]
    kind = rng.random(n)
    for r in np.flatnonzero(kind < 0.4):
        for c in rng.choice(m, size=2 if kind[r] < 0.1 else 1, replace=False):
            rows[r, c] = special[rng.integers(0, len(special))]
    return np.ascontiguousarray(rows)


@pytest.mark.parametrize("m,dim,chunk,n,kernel", [(16, 31, 2, 4100, "pq_scan_skew_kernel"),
                                                  (96, 96, 1, 4097, "pq_scan_skew_kernel"),
                                                  (192, 383, 2, 4111, "pq_scan_skew_kernel<SLICED>")])
def test_transposed_table_through_the_scans(qo, m, dim, chunk, n, kernel):
    """pq_lut_kernel / pq_lut_batch_kernel write the transposed table [code][chunk] separately; stores of >= 4096 rows
    scan it (skewed: m = 16 two rows per ring row, m = 96 whole rows, m = 192 two slices).  score_all equals the oracle's
    score_point_sse order under the NaN rule, score_ids (row-major table) gives the same, score_batch equals single
    queries.  No top-k here: the order of NaN scores is not specified."""
    assert qo.pq_chunks(dim, chunk) == m
    _rows, cen, _ = pq_special_case(dim, chunk)
    rows = _special_store_rows(n, m, seed=m)
    queries = _special_queries(dim, seed=m)[[0, 1, 3, 4, 5]]
    ids = np.concatenate([[0, n - 1], np.random.default_rng(m).integers(0, n, 200)]).astype(np.uint32)
    for dist, invert in ((D.Dot, True), (D.L2, False), (D.L1, True)):
        enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(dim, n, dist, invert), chunk, cen)
        assert enc.scan_kernel()[0] == kernel
        batch = enc.score_batch(enc.encode_query_batch(queries))
        some_finite = some_nan = some_inf = False
        for qi, q in enumerate(queries):
            lut = qo.pq_encode_query(q, chunk, cen, int(dist), invert)
            want = qo.pq_score_all(rows, lut, order=qo.ORDER_SSE)
            eq = enc.encode_query(q)
            got = enc.score_all(eq)
            assert_bits_equal_nan(got, want, f"score_all m={m} {dist} invert={invert} query {qi}")
            assert_bits_equal_nan(enc.score_ids(eq, ids), want[ids], "score_ids")
            assert_bits_equal_nan(batch[qi], got, f"score_batch row {qi} against the single query")
            assert_bits_equal_nan(batch[qi], want, f"score_batch row {qi}")
            some_finite |= bool(np.isfinite(want).any())
            some_nan |= bool(np.isnan(want).any())
            some_inf |= bool(np.isinf(want).any())
        assert some_finite and some_nan and some_inf


@pytest.mark.parametrize("invert", [False, True])
def test_topk_with_infinite_scores_and_no_nan(qo, invert):
    """One top-k case on scores with +inf, -inf and tables with -0.0 entries but no NaN: a positive query, rows with at
    most one infinite centroid, never both signs in one row."""
    m, dim, chunk, n = 16, 32, 2, 4100
    _rows, cen, _ = pq_special_case(dim, chunk)
    rows = _special_store_rows(n, m, seed=5, special=(3,))
    minus = np.flatnonzero((rows != 3).all(axis=1))[::7]
    rows[minus, minus % m] = 4
    query = (np.random.default_rng(5).random(dim, dtype=np.float32) + np.float32(0.5)).astype(np.float32)
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(dim, n, D.Dot, invert), chunk, cen)
    lut = qo.pq_encode_query(query, chunk, cen, int(D.Dot), invert)
    want = qo.pq_score_all(rows, lut, order=qo.ORDER_SSE)
    assert not np.isnan(want).any() and np.isposinf(want).sum() > 30 and np.isneginf(want).sum() > 30
    assert (util.bits(lut) == 0x80000000).any() == invert
    eq = enc.encode_query(query)
    util.assert_bits_equal(enc.score_all(eq), want, "score_all")
    for largest in (True, False):
        ids, sc = enc.topk(eq, 30, largest=largest)
        want_ids, want_sc = util.topk_want(want, 30, largest)
        util.assert_bits_equal(sc, want_sc, f"top-k scores largest={largest}")
        assert np.array_equal(ids, want_ids), f"top-k ids largest={largest}"


# ------------------------------------------------------------------ (f) score_internal on special centroids
@pytest.mark.parametrize("dim,chunk", [(10, 3), (16, 1), (40, 2)])
def test_score_internal_on_special_centroids(qo, dim, chunk):
    """pq_internal_kernel (single call) and pq_internal_pairs_kernel (score_internal_ids burst) decode both rows to
    centroids that carry NaN, infinities, +-3e38, subnormals and -0.0."""
    _rows, cen, _ = pq_special_case(dim, chunk)
    m = qo.pq_chunks(dim, chunk)
    n = 300
    rng = np.random.default_rng(dim)
    rows = _special_store_rows(n, m, seed=dim)
    rows[:20] = rng.integers(0, 12, (20, m), dtype=np.uint8)  # rows of special centroids only
    rows[20] = 9                                              # -0.0 everywhere
    rows[21] = 0
    ids = np.concatenate([[20, 21, 0, n - 1], rng.integers(0, n, 120)]).astype(np.uint32)
    for dist, invert in METRICS:
        enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(dim, n, dist, invert), chunk, cen)
        for i in (0, 20, 21, 150):
            want = np.array([qo.pq_score_internal(rows, dim, chunk, cen, int(dist), invert, i, int(j)) for j in ids],
                            dtype=np.float32)
            assert_bits_equal_nan(enc.score_internal_ids(i, ids), want, f"score_internal_ids {dist} invert={invert} i={i}")
            for k in (0, 1, 2, 7, 50):
                assert_bits_equal_nan([enc.score_internal(i, int(ids[k]))], [want[k]], f"score_internal {i}, {ids[k]}")
