"""NaN and infinite scores on every top-k route: one ordering, one NaN and tie rule.

Every route sorts candidates by (topk_ordered_bits(score) << 32 | row id), a total order on the f32 bit pattern:
ascending -NaN < -inf < negative finite < -0 < +0 < positive finite < +inf < +NaN, reversed for `largest`, equal bit
patterns to the lower id; a returned score is the row's own bits.  tests/util.py topk_total_order is that rule on the
host (tests/test_topk_order_model.py checks it without a GPU).

How an expected list is formed: a case takes score_all for the query, checks it against the oracle with
assert_bits_equal_nan (an x86 NaN and the GPU's default NaN differ in the sign bit), and then builds the expected list
from the GPU's OWN score_all bits through the model.  Ids must match exactly, scores bit for bit, in both directions.

How special scores are planted: exactly one special operand per row, only the NaN patterns 0x7FC00000 / 0xFFC00000 as
inputs.  u8: rows and metadata of an ordinary oracle encode of random data, `vector_offset` of chosen rows overwritten,
adopted with from_storage.  PQ: from_storage with chunk 1; codes 250 .. 255 of chunk 0 map to the centroid values +inf,
-inf, +NaN, -NaN, 3e38, -3e38, query[0] = 1 and ordinary rows draw chunk-0 codes below 250.  Special rows sit at row 0,
row n - 1, the middle, on both sides of a 64-row and of a 4096-row boundary and in adjacent groups of one pattern (ties
that must go to the lower id).  Profiles: "few" (2 - 3 rows of each kind), "flood" (more than 8192 rows of +inf and more
than 8192 of -inf plus a few NaN: the best tie group exceeds the 8192 candidate slots - the overflow and exact-redo path
with an infinite pivot) and "all_nan" (every score is the same NaN, the order is by id alone: PQ with query[0] = NaN;
u8 with a NaN `offset` in the store's metadata, which makes every Dot query offset sum * alpha * offset a NaN (L1, whose
query offset is 0: a NaN `multiplier`) - a NaN inside a u8 query cannot do it, the encoder turns it into a code and
computes the offset from the codes).

Which kernel serves a u8 batch is decided by u8_gemm_route(); there is no introspection call for it on a handle, so the
shapes of those cases live in tests/util.py and tests/test_topk_order_model.py asserts, through the route header on the
host, that at 256 CUs each reaches the kernel it is named after.  PQ stores assert scan_kernel()."""
import functools

import numpy as np
import pytest

from util import (SPECIAL_U8_FAMILIES, SPECIAL_U8_GEMM_SHAPE, SPECIAL_U8_SHORT_ROW_BATCHES, assert_bits_equal_nan, bits,
                  topk_total_order)

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
torch = pytest.importorskip("torch")

D = qa.DistanceType
PAD = 0xFFFFFFFF
P_NAN, N_NAN, P_INF, N_INF = 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000
U8_KINDS = [P_NAN, N_NAN, P_INF, N_INF]               # vector_offset bit patterns, by kind index
PQ_CODES = [252, 253, 250, 251, 254, 255]             # chunk-0 codes of the same kinds, then +3e38 and -3e38
PQ_VALUES = {250: np.inf, 251: -np.inf, 254: 3e38, 255: -3e38}  # 252 / 253: the two NaN patterns, set by bits
FLOOD = 8200                                          # rows per infinite group of the flood profile: more than kTopkCandCap
BIG = 2 ** 20 + 7


def f32_bits(pattern: int) -> np.float32:
    return np.array([pattern], dtype=np.uint32).view(np.float32)[0]


def planted(n: int, profile: str, kinds: int):
    """[(kind index, rows)]: kind 0 +NaN, 1 -NaN, 2 +inf, 3 -inf, 4 / 5 (PQ only) +-3e38."""
    assert n >= 4200
    mid = n // 2
    if profile == "few":
        slots = [[0, 64, 4096],            # +NaN: the first row, the first rows behind a 64- and a 4096-row boundary
                 [63, 4095, n - 1],        # -NaN: the last rows before those boundaries, the last row
                 [65, 66, mid],            # +inf: an adjacent pair
                 [mid + 1, mid + 2, 4097],  # -inf: an adjacent pair next to the +inf row
                 [61, 62, 4094],
                 [67, 68, 4098]]
        return [(kind, np.array(rows)) for kind, rows in enumerate(slots[:kinds])]
    assert profile == "flood" and mid > 100 + FLOOD + 64 and mid + FLOOD < n - 1
    return [(0, np.array([0, 64])), (1, np.array([63, n - 1])),
            (2, np.arange(100, 100 + FLOOD)), (3, np.arange(mid, mid + FLOOD))]


def assert_same_list(got_ids, got_sc, want_ids, want_sc, what):
    got_ids, want_ids = np.asarray(got_ids, dtype=np.uint32).ravel(), np.asarray(want_ids, dtype=np.uint32).ravel()
    g, w = bits(got_sc).ravel(), bits(want_sc).ravel()
    assert got_ids.shape == want_ids.shape and g.shape == w.shape, what
    bad = np.flatnonzero((got_ids != want_ids) | (g != w))
    if bad.size:
        p = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {w.size} entries differ, first at position {p}: got id {got_ids[p]} "
                             f"score {g[p]:#010x}, want id {want_ids[p]} score {w[p]:#010x}")


class Failures:
    """Collects the mismatches of one case, so that a failing case names every direction / k / query that failed."""

    def __init__(self):
        self.msgs = []

    def same(self, got_ids, got_sc, want_ids, want_sc, what):
        try:
            assert_same_list(got_ids, got_sc, want_ids, want_sc, what)
        except AssertionError as e:
            self.msgs.append(str(e))

    def check(self):
        assert not self.msgs, f"{len(self.msgs)} lists differ:\n" + "\n".join(self.msgs[:12])


# ===================================================================================================== u8 stores
@functools.lru_cache(maxsize=None)
def u8_base(qo, n, dim, dist, invert):
    """(rows, Meta) of an ordinary oracle encode of random data."""
    data = np.random.default_rng(n * 7 + dim).random((n, dim), dtype=np.float32)
    return qo.u8_encode(data, int(dist), invert)


def u8_store(qo, n, dim, dist, invert, profile, multiplier=None):
    """(handle, rows, Meta): the base store with `vector_offset` of the planted rows overwritten (all_nan: the plain
    rows under a NaN metadata offset).  `multiplier`: put in place of the encode's (0 and inf are what sends a batch to u8_gemm_kernel)."""
    rows, meta0 = u8_base(qo, n, dim, dist, invert)
    rows = rows.copy()
    meta = type(meta0).from_buffer_copy(meta0)
    if multiplier is not None:
        meta.multiplier = multiplier
    if profile == "all_nan" and dist == D.L1:
        meta.multiplier = float("nan")  # an L1 query offset is 0: the NaN comes in through multiplier * sum
    elif profile == "all_nan":
        meta.offset = float("nan")  # 0x7FC00000
    else:
        off = rows[:, :4].view(np.uint32).reshape(-1)
        for kind, at in planted(n, profile, 4):
            off[at] = U8_KINDS[kind]
    md = {"actual_dim": meta.actual_dim, "alpha": meta.alpha, "offset": meta.offset, "multiplier": meta.multiplier,
          "vector_parameters": qa.VectorParameters(dim, n, dist, invert)}
    return qa.EncodedVectorsU8.from_storage(rows, md), rows, meta


def u8_queries(dim, nq, profile, seed=1):
    return np.random.default_rng(seed * 1000 + dim + nq + len(profile)).random((nq, dim), dtype=np.float32)


def u8_scores(qo, enc, rows, meta, query, q_enc, sample=None):
    """score_all of the GPU, checked against the oracle: every row, or (wide rows, where the oracle takes seconds per
    query) the rows `sample`, which hold every planted row."""
    got = enc.score_all(q_enc)
    codes, qoff = qo.u8_encode_query(meta, query)
    order = qo.ORDER_AVX2 if meta.actual_dim <= 1040 else qo.ORDER_SIMPLE
    if sample is None:
        want = qo.u8_score_all(meta, rows, codes, qoff, order=order)
        assert_bits_equal_nan(got, want, "score_all vs oracle")
    else:
        sub = type(meta).from_buffer_copy(meta)
        sub.count = sample.size
        want = qo.u8_score_all(sub, np.ascontiguousarray(rows[sample]), codes, qoff, order=order)
        assert_bits_equal_nan(got[sample], want, "score_all vs oracle on the sampled rows")
    return got


def check_planted_scores(scores, n, profile):
    """The planted rows carry what was planted: the profile is what the docstring says (not an all-NaN store, say)."""
    if profile == "all_nan":
        assert np.all(bits(scores) == bits(scores)[0]) and np.isnan(scores[0]), "every score is the same NaN"
        return
    b = bits(scores)
    for kind, at in planted(n, profile, 4):
        assert np.all(b[at] == U8_KINDS[kind]), f"planted kind {kind}: {b[at][:4]}"
    assert np.isfinite(scores).sum() == n - sum(at.size for _, at in planted(n, profile, 4))


U8_SMALL = (20_000, 64)


@pytest.mark.parametrize("profile", ["few", "flood", "all_nan"])
@pytest.mark.parametrize("query_on", ["device", "host"])
def test_u8_single_query_small_store(qo, profile, query_on):
    """20 000 rows, dim 64.  k = 1, 30, 64: the single-launch small-store kernel (n <= 2M, k <= 64) - u8_topk_small_kernel
    for a query encoded from device memory, u8_topk_small_fused_kernel for a host query (its encoding is deferred into
    the top-k launch; a fresh query object per call, since the first consumer encodes it).  k = 200, 1024: the classic
    path, score array + radix select (n < 32768)."""
    n, dim = U8_SMALL
    enc, rows, meta = u8_store(qo, n, dim, D.Dot, False, profile)
    query = u8_queries(dim, 1, profile)[0]

    def encoded():
        return enc.encode_query(torch.from_numpy(query).cuda() if query_on == "device" else query)

    scores = u8_scores(qo, enc, rows, meta, query, encoded())
    check_planted_scores(scores, n, profile)
    f = Failures()
    for largest in (True, False):
        for k in (1, 30, 64, 200, 1024):
            ids, sc = enc.topk(encoded(), k, largest=largest)
            f.same(ids, sc, *topk_total_order(scores, k, largest), f"k={k} largest={largest}")
    f.check()


@pytest.mark.parametrize("profile", ["few", "flood", "all_nan"])
def test_u8_single_query_large_store(qo, profile):
    """2^20 + 7 rows, dim 32.  k = 1024: fused_topk - pivot from a sample, the scan in FILTER mode (topk_offer: key
    compare), one sort of the candidates; the flood profile overflows the candidate slots and is redone exactly.
    k = 30: with n <= 2M still the single-launch kernel, here with many workgroups (last-arriver merge)."""
    n, dim = BIG, 32
    enc, rows, meta = u8_store(qo, n, dim, D.Dot, False, profile)
    query = u8_queries(dim, 1, profile)[0]
    q = enc.encode_query(query)
    scores = u8_scores(qo, enc, rows, meta, query, q)
    check_planted_scores(scores, n, profile)
    f = Failures()
    for largest in (True, False):
        for k in (30, 1024):
            ids, sc = enc.topk(q, k, largest=largest)
            f.same(ids, sc, *topk_total_order(scores, k, largest), f"k={k} largest={largest}")
    f.check()


def check_u8_batch(qo, enc, rows, meta, queries, ks, n, profile, sample=None):
    """Every query of the batch, both directions, every k: topk_batch == the model on the query's own score_all bits
    == the single-query topk."""
    batch = enc.encode_query_batch(queries)
    lists = {(k, largest): enc.topk_batch(batch, k, largest=largest) for k in ks for largest in (True, False)}
    f = Failures()
    q = None
    for qi in range(queries.shape[0]):
        q = enc.encode_query(queries[qi], reuse=q)
        scores = u8_scores(qo, enc, rows, meta, queries[qi], q, sample if qi else None)  # query 0: every row
        if qi == 0 and meta.multiplier not in (0.0, np.inf):
            check_planted_scores(scores, n, profile)
        for (k, largest), (ids, sc) in lists.items():
            want = topk_total_order(scores, k, largest)
            f.same(ids[qi], sc[qi], *want, f"topk_batch query {qi} k={k} largest={largest}")
            f.same(*enc.topk(q, k, largest=largest), *want, f"topk query {qi} k={k} largest={largest}")
    f.check()


def oracle_sample(n, profile):
    """Every planted row and every 16th of the others (the oracle's share of a wide store)."""
    at = [np.arange(0, n, 16)] + ([rows for _, rows in planted(n, profile, 4)] if profile != "all_nan" else [])
    return np.unique(np.concatenate(at))


U8_FAMILIES = SPECIAL_U8_FAMILIES  # (family, rows, dim, queries): tests/util.py, checked there against u8_gemm_route()


@pytest.mark.parametrize("profile,dist", [("few", D.Dot), ("few", D.L2), ("flood", D.Dot), ("all_nan", D.Dot)])
@pytest.mark.parametrize("family,n,dim,nq", U8_FAMILIES, ids=[f[0] for f in U8_FAMILIES])
def test_u8_batch_matrix_core_families(qo, family, n, dim, nq, profile, dist):
    """topk_batch on the matrix cores (fused: n >= 32768), one case per kernel family; k = 30 (batch_emit_wave_kernel)
    and 200 (batch_emit_kernel).  Dot has a positive multiplier, L2 a negative one: with `largest` both directions of
    the integer pre-filter (LOW) run.  A +NaN row is the best row of every `largest` query, a -NaN row of every
    smallest-first query; in the flood profile the pivot of a `largest` query is +inf, more rows tie with it than a
    query has candidate slots, and the call must fall back to the exact single-query path."""
    enc, rows, meta = u8_store(qo, n, dim, dist, False, profile)
    sample = oracle_sample(n, profile) if dim >= 256 else None
    check_u8_batch(qo, enc, rows, meta, u8_queries(dim, nq, profile), (30, 200), n, profile, sample)


@pytest.mark.parametrize("multiplier", [0.0, np.inf])
@pytest.mark.parametrize("profile", ["few", "flood"])
def test_u8_batch_gemm_kernel_degenerate_multiplier(qo, profile, multiplier):
    """u8_gemm_kernel: the filter pass of a store whose multiplier is 0 (constant data: alpha = 0) or infinite - no
    integer pre-filter exists for those.  multiplier 0: a score is q_offset + vector_offset, ordinary rows tie in large
    groups.  multiplier inf: inf * s is +inf, or NaN for s = 0 (the zero-code rows 10 .. 19 here), whatever the
    offsets - a NaN score that no offset announces."""
    n, dim, nq = SPECIAL_U8_GEMM_SHAPE
    enc, rows, meta = u8_store(qo, n, dim, D.Dot, False, profile, multiplier=multiplier)
    if multiplier == np.inf:
        rows = rows.copy()
        rows[10:20, 4:] = 0
        md = {"actual_dim": meta.actual_dim, "alpha": meta.alpha, "offset": meta.offset, "multiplier": meta.multiplier,
              "vector_parameters": qa.VectorParameters(dim, n, D.Dot, False)}
        enc = qa.EncodedVectorsU8.from_storage(rows, md)
    check_u8_batch(qo, enc, rows, meta, u8_queries(dim, nq, profile), (30, 200), n, profile)


def pivot_sample_row(j: int, n: int) -> int:
    """Store row of sample row j (gather_rows_kernel: the golden-ratio scatter of csrc/batch_common.hpp)."""
    return ((((j * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF) >> 32) * n) >> 32


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("multiplier", [None, 0.0], ids=["rs", "gemm"])
def test_u8_batch_losing_side_nan_rows_do_not_fill_a_short_list(qo, multiplier, largest):
    """A list with fewer than k rows at least as good as the pivot must go to the exact path, however many NaN rows of
    the LOSING side of the order the store holds (-NaN for `largest`, +NaN for smallest-first: they rank behind every
    other row and are no candidates).  33 000 rows, k = 200, pivot rank 64 of 2048 sampled rows: the first 64 sample
    rows (one per thread of batch_pivot_kernel) get offsets far beyond every other score, so the pivot is the worst of
    them and exactly 64 rows reach it; 300 other rows are losing-side NaNs.  A filter that let those through would
    count 364 candidates, skip the fallback and return 64 rows followed by NaNs.  With the encode's multiplier the
    batch runs u8_gemm_rs_kernel (pre-filter), with multiplier 0 u8_gemm_kernel."""
    n, dim, nq = SPECIAL_U8_GEMM_SHAPE
    k = 200
    rows, meta0 = u8_base(qo, n, dim, D.Dot, False)
    rows = rows.copy()
    meta = type(meta0).from_buffer_copy(meta0)
    if multiplier is not None:
        meta.multiplier = multiplier
    chosen = np.array([pivot_sample_row(j, n) for j in range(64)])
    assert np.unique(chosen).size == 64
    off = rows[:, :4].view(np.float32).reshape(-1)
    off[chosen] = (1e6 + 1000.0 * np.arange(64)).astype(np.float32) * (1 if largest else -1)
    losing = np.setdiff1d(np.arange(20_000, 20_400), chosen)[:300]
    rows[:, :4].view(np.uint32).reshape(-1)[losing] = N_NAN if largest else P_NAN
    md = {"actual_dim": meta.actual_dim, "alpha": meta.alpha, "offset": meta.offset, "multiplier": meta.multiplier,
          "vector_parameters": qa.VectorParameters(dim, n, D.Dot, False)}
    enc = qa.EncodedVectorsU8.from_storage(rows, md)
    queries = u8_queries(dim, nq, "few")
    batch = enc.encode_query_batch(queries)
    ids, sc = enc.topk_batch(batch, k, largest=largest)
    f = Failures()
    for qi in range(nq):
        q = enc.encode_query(queries[qi])
        scores = u8_scores(qo, enc, rows, meta, queries[qi], q)
        want = topk_total_order(scores, k, largest)
        assert np.array_equal(np.sort(want[0][:64]), np.sort(chosen)) and not np.isnan(want[1]).any()
        f.same(ids[qi], sc[qi], *want, f"topk_batch query {qi}")
        f.same(*enc.topk(q, k, largest=largest), *want, f"topk query {qi}")
    f.check()


@pytest.mark.parametrize("profile", ["few", "flood", "all_nan"])
@pytest.mark.parametrize("n,dim,nq", SPECIAL_U8_SHORT_ROW_BATCHES)
def test_u8_batch_of_two_and_four_queries(qo, profile, n, dim, nq):
    """2 and 4 queries on 2^20 + 7 rows, dim 32, k = 30 and 1024.  Up to 2M rows, and on rows shorter than 144 code
    bytes at any size, such a batch takes the matrix cores (rs, the 32-query tile); see
    test_u8_batch_vector_alu_multi_scan for the vector-ALU pass."""
    enc, rows, meta = u8_store(qo, n, dim, D.Dot, False, profile)
    check_u8_batch(qo, enc, rows, meta, u8_queries(dim, nq, profile), (30, 1024), n, profile)


@pytest.mark.parametrize("profile", ["few", "flood", "all_nan"])
@pytest.mark.parametrize("nq", [2, 4])
def test_u8_batch_vector_alu_multi_scan(qo, profile, nq):
    """u8_topk_batch_scans: above 2M rows (qamd_u8_topk_batch: n > 2 << 20) two queries, and L1 with any count, take
    ONE filtering pass of u8_scan_multi_kernel per group of queries and fused_topk_batch (topk_offer: key compare) -
    on rows of at least 144 code bytes (multi_width: 9 chunks of 16; shorter rows go to the matrix cores, see
    test_u8_batch_of_two_and_four_queries).  2^21 + 7 rows of dim 144 is the smallest store that reaches it: two Dot
    queries, four L1 queries."""
    n, dim = 2 ** 21 + 7, 144
    dist = D.Dot if nq == 2 else D.L1
    enc, rows, meta = u8_store(qo, n, dim, dist, False, profile)
    check_u8_batch(qo, enc, rows, meta, u8_queries(dim, nq, profile), (30, 1024), n, profile)


# ===================================================================================================== PQ stores
@functools.lru_cache(maxsize=None)
def pq_base(n, m):
    """(rows u8 [n, m] with chunk-0 codes below 250, centroids [256, m]: random, 250 .. 255 of chunk 0 special)."""
    rng = np.random.default_rng(n * 3 + m)
    cen = (rng.random((256, m), dtype=np.float32) - 0.5).astype(np.float32)
    for code, value in PQ_VALUES.items():
        cen[code, 0] = value
    cen.view(np.uint32)[252, 0] = P_NAN
    cen.view(np.uint32)[253, 0] = N_NAN
    rows = rng.integers(0, 256, size=(n, m), dtype=np.uint8)
    rows[:, 0] = rng.integers(0, 250, size=n, dtype=np.uint8)
    return rows, cen


def pq_store(n, m, dist, invert, profile):
    rows, cen = pq_base(n, m)
    rows = rows.copy()
    if profile != "all_nan":
        for kind, at in planted(n, profile, 6):
            rows[at, 0] = PQ_CODES[kind]
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(m, n, dist, invert), 1, cen)
    return enc, rows, cen


def pq_queries(m, nq, profile):
    q = (np.random.default_rng(m + nq).random((nq, m), dtype=np.float32) - 0.5).astype(np.float32)
    q[:, 0] = f32_bits(P_NAN) if profile == "all_nan" else 1.0
    return q


def pq_scores(qo, enc, rows, cen, dist, invert, query, q_enc, n, profile):
    got = enc.score_all(q_enc)
    lut = qo.pq_encode_query(query, 1, cen, int(dist), invert)
    assert_bits_equal_nan(got, qo.pq_score_all(rows, lut, order=qo.ORDER_SSE), "score_all vs oracle")
    if profile == "all_nan":
        assert np.all(bits(got) == bits(got)[0]) and np.isnan(got[0]), "every score is the same NaN"
    else:
        # the planted rows are special: +-inf and NaN rows are not finite (L2: +inf and NaN only), +-3e38 rows are huge
        for kind, at in planted(n, profile, 6):
            if kind < 4:
                assert not np.isfinite(got[at]).any(), kind
                assert np.isnan(got[at]).all() == (kind < 2), kind
    return got


PQ_METRICS = [(D.Dot, False), (D.Dot, True)]
# 6000 rows cannot hold the flood profile's two groups of 8200: it runs on 20 000 rows, which take the same routes
PQ_SMALL_CASES = [(16, 6000, "few"), (16, 6000, "all_nan"), (16, 20_000, "flood"),
                  (96, 6000, "few"), (96, 6000, "all_nan"), (96, 20_000, "flood")]


def check_pq_single(qo, m, n, profile, dist, invert, ks):
    enc, rows, cen = pq_store(n, m, dist, invert, profile)
    assert enc.scan_kernel() == ("pq_scan_skew_kernel", 1)
    query = pq_queries(m, 1, profile)[0]
    q = enc.encode_query(query)
    scores = pq_scores(qo, enc, rows, cen, dist, invert, query, q, n, profile)
    f = Failures()
    for largest in (True, False):
        for k in ks:
            ids, sc = enc.topk(q, k, largest=largest)
            f.same(ids, sc, *topk_total_order(scores, k, largest), f"k={k} largest={largest}")
    f.check()


@pytest.mark.parametrize("dist,invert", PQ_METRICS)
@pytest.mark.parametrize("m,n,profile", PQ_SMALL_CASES)
def test_pq_single_query_small_store(qo, m, n, profile, dist, invert):
    """6000 (flood: 20 000) rows, m = 16 and 96 codes per row, whole-store scan pq_scan_skew_kernel.  k = 1, 30, 64:
    pq_topk_small_kernel (single launch); k = 200: the classic path (n < 32768)."""
    check_pq_single(qo, m, n, profile, dist, invert, (1, 30, 64, 200))


@pytest.mark.parametrize("m,n,profile", [(16, 6000, "few"), (96, 20_000, "flood"), (16, BIG, "few")])
def test_pq_l2(qo, m, n, profile):
    """L2: (1 - c)^2 is +inf for both infinite centroids and for +-3e38 (the square overflows), NaN for the NaN ones -
    only +inf and NaN scores exist, and far more rows tie at +inf."""
    check_pq_single(qo, m, n, profile, D.L2, False, (30, 200, 1024))


@pytest.mark.parametrize("dist,invert", PQ_METRICS)
@pytest.mark.parametrize("profile", ["few", "flood", "all_nan"])
@pytest.mark.parametrize("m", [16, 96])
def test_pq_large_store_single_and_batch(qo, m, profile, dist, invert):
    """2^20 + 7 rows.  Single query: k = 30 the single-launch kernel (n <= 2M), k = 1024 fused_topk (filtering
    pq_scan_skew_kernel).  topk_batch of 5 queries at k = 10 (pq_topk_small per query) and k = 1024 (on 256 CUs the
    side-by-side filter pass, SkewBatch: topk_offer_shard per query; else per-query pipelines): every query against the
    model and against its single-query topk."""
    n = BIG
    enc, rows, cen = pq_store(n, m, dist, invert, profile)
    assert enc.scan_kernel() == ("pq_scan_skew_kernel", 1)
    queries = pq_queries(m, 5, profile)
    batch = enc.encode_query_batch(queries)
    lists = {(k, largest): enc.topk_batch(batch, k, largest=largest) for k in (10, 1024) for largest in (True, False)}
    f = Failures()
    for qi in range(5):
        q = enc.encode_query(queries[qi])
        scores = pq_scores(qo, enc, rows, cen, dist, invert, queries[qi], q, n, profile)
        for (k, largest), (ids, sc) in lists.items():
            want = topk_total_order(scores, k, largest)
            f.same(ids[qi], sc[qi], *want, f"topk_batch query {qi} k={k} largest={largest}")
            f.same(*enc.topk(q, k, largest=largest), *want, f"topk query {qi} k={k} largest={largest}")
        if qi == 0:
            for largest in (True, False):
                f.same(*enc.topk(q, 30, largest=largest), *topk_total_order(scores, 30, largest), f"topk k=30 {largest}")
    f.check()


# ===================================================================================================== rescoring
R_N, R_DIM, R_CAND, R_K = 5000, 32, 256, 30


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def rescore_data(kind):
    """(clean f32 rows for the quantized store, original rows with one inf or NaN coordinate in the planted rows).
    Half of the planted rows are the largest rows of the clean data and half the smallest, so that the quantized top
    candidates of either direction hold some of them.  bf16: every value has its low 16 bits clear (exact in bf16)."""
    rng = np.random.default_rng(41)
    clean = rng.random((R_N, R_DIM), dtype=np.float32)
    special = []
    for kind_i, at in planted(R_N, "few", 4):
        clean[at[::2]] = 0.98 + 0.01 * rng.random((at[::2].size, R_DIM), dtype=np.float32)
        clean[at[1::2]] = 0.01 * rng.random((at[1::2].size, R_DIM), dtype=np.float32)
        special += [(int(r), U8_KINDS[kind_i]) for r in at]
    orig = clean.copy()
    if kind == "bf16":
        orig.view(np.uint32)[...] &= 0xFFFF0000
    for j, (r, pattern) in enumerate(special):
        orig.view(np.uint32)[r, (3 * j) % R_DIM] = pattern  # one special coordinate per planted row
    return clean, orig, np.array([r for r, _ in special])


def rescore_query():
    return (np.random.default_rng(43).random(R_DIM, dtype=np.float32) + 0.25).astype(np.float32)  # positive: inf stays inf


def make_orig(kind, orig, vp):
    if kind == "bf16":
        return qa.OriginalVectors.from_data((orig.view(np.uint32) >> 16).astype(np.uint16), vp, dtype="bf16")
    return qa.OriginalVectors.from_data(orig, vp)


def exact_scores(qo, dist, invert, q, data, ids):
    q = np.ascontiguousarray(q, dtype=np.float32)
    fn, dim, base, qp = qo.lib().qo_metric_f32, data.shape[1], data.ctypes.data, q.ctypes.data
    out = np.array([fn(int(dist), qp, base + int(i) * dim * 4, dim) for i in ids], dtype=np.float32)
    return -out if invert else out


def model_rerank(ids, scores, k, largest):
    """The best k of the id list by (key of the score, id): topk_total_order over the list taken in ascending id order, so
    that its tie rule (lower position) is the contract's (lower id)."""
    ids = np.asarray(ids, dtype=np.uint32).ravel()
    order = np.argsort(ids, kind="stable")
    pos, sc = topk_total_order(np.asarray(scores, dtype=np.float32)[order], k, largest)
    out = np.full(k, PAD, dtype=np.uint32)
    out[pos != PAD] = ids[order][pos[pos != PAD]]
    return out, sc


@pytest.mark.parametrize("kind,dist,invert", [("f32", D.Dot, False), ("f32", D.Dot, True), ("f32", D.L2, False),
                                              ("bf16", D.Dot, False)])
def test_rerank_and_rerank_batch(qo, kind, dist, invert):
    """qamd_f32_rerank / _rerank_batch (rerank_kernel: the candidates' exact scores sorted by the key) over 256 ids
    that hold every planted row: rows with one +-inf or +-NaN coordinate, so exact scores are +-inf and NaN of both
    signs.  Host id lists, and a device list with one id >= count, whose NaN score is ranked by the rule like any."""
    _clean, orig_rows, special = rescore_data(kind)
    vp = qa.VectorParameters(R_DIM, R_N, dist, invert)
    orig = make_orig(kind, orig_rows, vp)
    rng = np.random.default_rng(47)
    queries = np.stack([rescore_query(), rescore_query()[::-1].copy()])
    others = np.setdiff1d(rng.permutation(R_N)[: R_CAND], special)[: R_CAND - special.size]
    ids = rng.permutation(np.concatenate([special, others]).astype(np.uint32))
    assert ids.size == R_CAND
    f = Failures()
    for q in queries:
        scores = orig.score_ids(q, ids)
        assert_bits_equal_nan(scores, exact_scores(qo, dist, invert, q, orig_rows, ids), "score_ids vs oracle")
        assert not np.isfinite(scores[np.isin(ids, special)]).any()
        for largest in (True, False):
            f.same(*orig.rerank(q, ids, R_K, largest=largest), *model_rerank(ids, scores, R_K, largest), f"rerank {largest}")
    two = np.stack([ids, ids[::-1]])
    for largest in (True, False):
        got_ids, got_sc = orig.rerank_batch(queries, two, R_K, largest=largest)
        for qi in range(2):
            scores = orig.score_ids(queries[qi], two[qi])
            f.same(got_ids[qi], got_sc[qi], *model_rerank(two[qi], scores, R_K, largest), f"rerank_batch {qi} {largest}")
    # a device list with an id past the end: it takes part with the NaN that score_ids gives it
    bad = ids.copy()
    bad[5] = R_N + 17
    out = torch.empty(bad.size, device="cuda")
    orig.score_ids(torch.from_numpy(queries[0]).cuda(), dev_u32(bad), out=out)
    torch.cuda.synchronize()
    scores = out.cpu().numpy()
    assert np.isnan(scores[5])
    for largest in (True, False):
        oi = torch.empty(R_K, dtype=torch.int32, device="cuda")
        os_ = torch.empty(R_K, device="cuda")
        orig.rerank(torch.from_numpy(queries[0]).cuda(), dev_u32(bad), R_K, largest=largest, out_ids=oi, out_scores=os_)
        torch.cuda.synchronize()
        want = model_rerank(bad, scores, R_K, largest)
        f.same(oi.cpu().numpy().view(np.uint32), os_.cpu().numpy(), *want, f"device list with an id past the end {largest}")
        where = np.flatnonzero(want[0] == R_N + 17)
        if bits(scores)[5] >> 31 == (0 if largest else 1):
            assert where.size == 1, "a NaN on the best side of the order is in the list"
    f.check()


@pytest.mark.parametrize("kind,dist,invert", [("f32", D.Dot, False), ("f32", D.L2, False), ("bf16", D.Dot, False)])
@pytest.mark.parametrize("which", ["u8", "pq"])
def test_topk_rescored_and_batch(qo, which, kind, dist, invert):
    """*_topk_rescored / *_topk_batch_rescored (candidates = 256, k = 30): the quantized store holds clean data, the
    originals the rows with one infinite or NaN coordinate.  Expected: the model's rerank of the ids that the quantized
    topk(candidates) returns, which in turn equal the model on the quantized score_all."""
    clean, orig_rows, special = rescore_data(kind)
    vp = qa.VectorParameters(R_DIM, R_N, dist, invert)
    orig = make_orig(kind, orig_rows, vp)
    if which == "u8":
        enc = qa.EncodedVectorsU8.encode(clean, vp)
    else:
        enc = qa.EncodedVectorsPQ.encode(clean, vp, 2, centroids=np.ascontiguousarray(clean[:256]))
    queries = np.stack([rescore_query(), rescore_query()[::-1].copy(), rescore_query() * 2])
    batch = enc.encode_query_batch(queries)
    f = Failures()
    for largest in (True, False):
        got_b = enc.topk_batch_rescored(batch, orig, queries, R_K, R_CAND, largest=largest)
        seen = 0
        for qi, query in enumerate(queries):
            q = enc.encode_query(query)
            cand, cand_sc = enc.topk(q, R_CAND, largest=largest)
            f.same(cand, cand_sc, *topk_total_order(enc.score_all(q), R_CAND, largest), f"quantized topk {qi} {largest}")
            exact = orig.score_ids(query, cand)
            assert_bits_equal_nan(exact, exact_scores(qo, dist, invert, query, orig_rows, cand), "score_ids vs oracle")
            seen += int(np.isin(cand, special).sum())
            want = model_rerank(cand, exact, R_K, largest)
            f.same(*enc.topk_rescored(q, orig, query, R_K, R_CAND, largest=largest), *want, f"topk_rescored {qi} {largest}")
            f.same(got_b[0][qi], got_b[1][qi], *want, f"topk_batch_rescored {qi} {largest}")
        assert seen >= 3, "the candidates hold planted rows"
    f.check()


# ===================================================================================================== sharded handles
def shard_planted(n, shards=3):
    """few + rows on both sides of every shard boundary ((g * n) / shards) and inside every shard."""
    extra = []
    for g in range(1, shards):
        b = (g * n) // shards
        extra += [(0, [b]), (1, [b - 1]), (2, [b + 1]), (3, [b - 2])]
    return planted(n, "few", 4) + [(kind, np.array(at)) for kind, at in extra]


@pytest.mark.parametrize("store", ["u8", "pq"])
def test_sharded_topk_and_topk_batch(qo, store):
    """ShardedVectorsU8 / ShardedVectorsPQ.from_storage on [0, 0, 0]: per-shard top-k, peer copy, merge_topk_kernel
    (global id = shard base + local id).  Planted rows sit in every shard and on both sides of both shard boundaries.
    topk at k = 30 and 200, topk_batch of 3 queries: the model on the single handle's score_all bits, and the single
    handle's own lists."""
    n = 40_000
    if store == "u8":
        dim = 64
        rows, meta0 = u8_base(qo, n, dim, D.Dot, False)
        rows = rows.copy()
        off = rows[:, :4].view(np.uint32).reshape(-1)
        for kind, at in shard_planted(n):
            off[at] = U8_KINDS[kind]
        md = {"actual_dim": meta0.actual_dim, "alpha": meta0.alpha, "offset": meta0.offset, "multiplier": meta0.multiplier,
              "vector_parameters": qa.VectorParameters(dim, n, D.Dot, False)}
        one = qa.EncodedVectorsU8.from_storage(rows, md)
        sh = qa.ShardedVectorsU8.from_storage(rows, md, [0, 0, 0])
        queries = u8_queries(dim, 3, "few")
    else:
        dim = 16
        rows, cen = pq_base(n, dim)
        rows = rows.copy()
        for kind, at in shard_planted(n):
            rows[at, 0] = PQ_CODES[kind]
        vp = qa.VectorParameters(dim, n, D.Dot, False)
        one = qa.EncodedVectorsPQ.from_storage(rows, vp, 1, cen)
        sh = qa.ShardedVectorsPQ.from_storage(rows, vp, 1, cen, [0, 0, 0])
        queries = pq_queries(dim, 3, "few")
    f = Failures()
    sb = sh.encode_query_batch(queries)
    for largest in (True, False):
        for k in (30, 200):
            b_ids, b_sc = sh.topk_batch(sb, k, largest=largest)
            for qi, query in enumerate(queries):
                q1 = one.encode_query(query)
                scores = one.score_all(q1)
                assert np.array_equal(bits(sh.score_all(sh.encode_query(query))), bits(scores)), "sharded score_all"
                want = topk_total_order(scores, k, largest)
                f.same(*sh.topk(sh.encode_query(query), k, largest=largest), *want, f"sharded topk {qi} k={k} {largest}")
                f.same(b_ids[qi], b_sc[qi], *want, f"sharded topk_batch {qi} k={k} {largest}")
                f.same(*one.topk(q1, k, largest=largest), *want, f"single handle {qi} k={k} {largest}")
    f.check()


@pytest.mark.parametrize("largest", [True, False])
def test_topk_merge_on_hand_made_lists(largest):
    """qamd_topk_merge directly: 3 shards x 2 queries x k = 8 lists in device memory, made by the model from score
    vectors that hold every special pattern (two NaN payloads, +-0, a repeated value); one shard is shorter than k, so
    its lists end in padding (id 0xFFFFFFFF, score -inf / +inf), which must not take part."""
    import ctypes as C

    from quantization_amd import _lib

    specials = np.array([0x7FC00000, 0xFF800000, 0x00000000, 0x3F800000, 0xFFC00000, 0x7F7FFFFF, 0x80000001, 0x7FC00001,
                         0x80000000, 0x3F800000, 0xFF7FFFFF, 0x7F800000, 0x00000001, 0xFFC00001], dtype=np.uint32)
    rng = np.random.default_rng(53)
    bounds = [0, 20, 25, 60]
    k, nq, world = 8, 2, 3
    all_scores = rng.standard_normal((nq, bounds[-1])).astype(np.float32)
    for qi in range(nq):
        all_scores.view(np.uint32)[qi, rng.choice(bounds[-1], 2 * specials.size, replace=False)] = np.tile(specials, 2)
    ids = np.zeros((world, nq, k), dtype=np.uint32)
    sc = np.zeros((world, nq, k), dtype=np.float32)
    for g in range(world):
        for qi in range(nq):
            ids[g, qi], sc[g, qi] = topk_total_order(all_scores[qi, bounds[g]:bounds[g + 1]], k, largest)
    assert (ids[1] == PAD).any()
    d_ids, d_sc = dev_u32(ids), torch.from_numpy(sc.view(np.int32)).cuda()
    out_ids = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    out_sc = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    bases = (C.c_uint64 * world)(*bounds[:-1])
    st = _lib.lib().qamd_topk_merge(C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_sc.data_ptr()), nq * k, bases, world, nq, k,
                                    int(largest), C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_sc.data_ptr()),
                                    _lib.MEM_DEVICE, None)
    assert st == _lib.OK, _lib.lib().qamd_last_error()
    torch.cuda.synchronize()
    got_ids = out_ids.cpu().numpy().view(np.uint32)
    got_sc = out_sc.cpu().numpy().view(np.float32)
    f = Failures()
    for qi in range(nq):
        f.same(got_ids[qi], got_sc[qi], *topk_total_order(all_scores[qi], k, largest), f"query {qi}")
    f.check()
