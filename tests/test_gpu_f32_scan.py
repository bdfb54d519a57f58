"""The whole-store exact scan of the original vectors: OriginalVectors.score_all / topk / topk_batch, i.e. the null-id-list
forms of qamd_f32_score_ids / qamd_f32_rerank / qamd_f32_rerank_batch (f32_scan.hip).

Every comparison is on raw bits (util.assert_bits_equal), against two independent references: the oracle's restatement
of DistanceType::distance (qo_metric_f32, looped over the rows; for f16 / bf16 stores on the exactly widened rows) and
the list path score_ids(q, arange(n)), which is another kernel.  Expected top-k lists are util.topk_total_order of the
oracle's scores.

Special values: +-0, subnormals, values near max / dim, and rows holding +inf, -inf, +NaN and -NaN.  An x86 NaN and the
GPU's default NaN differ in the sign bit, so no score here is a NaN that an operation GENERATES: a special row holds
exactly one inf or NaN (patterns 0x7FC00000 / 0xFFC00000), in the column where every query of this file is 1.0, and
the NaN a score ends as is that operand, propagated.  Under L2 the operand passes a subtraction, which may flip a NaN's
sign (nan_sign_of_the_device): those two scores per query take their bits from the list path.

Launch arithmetic: a wave takes 64 consecutive rows, a workgroup 256, and the grid is ceil(n / 256) workgroups - no
workgroup loops over tiles, so there is no row count "past a full grid's round" to add to 1 .. 1000.
The score workspace cap of a batch (512 MiB) is not reachable at test size: 8 queries shrink to 4 only past 16.7M rows.
The batch tests therefore cover the group forms 8, 4, 2, 1 and their remainders, not the shrinking."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from util import assert_bits_equal, topk_total_order

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
torch = pytest.importorskip("torch")
from oracle import qoracle as qo  # noqa: E402
from quantization_amd import _lib  # noqa: E402
from quantization_amd.encoded_vectors import check, in_buf, out_buf, stream_ptr  # noqa: E402

D = qa.DistanceType
PAD = 0xFFFFFFFF
METRICS = [(D.Dot, False), (D.Dot, True), (D.L1, False), (D.L1, True), (D.L2, False), (D.L2, True)]
P_NAN, N_NAN = 0x7FC00000, 0xFFC00000
F32_DIMS = [1, 3, 4, 31, 32, 33, 36, 64, 65, 768, 4099]
HALF_DIMS = [1, 2, 3, 8, 63, 64, 65, 66, 72, 769]
ROW_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1000]
QUERY_COUNTS = [1, 2, 3, 5, 8, 9, 17]


# ------------------------------------------------------------------------------------------------ data
def to_store(f32, kind):
    """f32 values as the store's numpy form: f32, float16 (round to nearest even) or bf16 bit patterns in uint16."""
    f32 = np.ascontiguousarray(f32, dtype=np.float32)
    if kind == "f32":
        return f32.copy()
    if kind == "f16":
        with np.errstate(over="ignore"):
            return f32.astype(np.float16)
    u = f32.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(stored, kind):
    if kind == "f32":
        return stored
    if kind == "f16":
        return stored.astype(np.float32)
    return (stored.astype(np.uint32) << 16).view(np.float32)


def from_f32_bits(pattern, kind):
    """The store's element whose exact widening has the f32 bit pattern `pattern` (upper 16 bits only for bf16; for f16
    the patterns used here: +-0, +-inf, the two NaNs)."""
    if kind == "f32":
        return np.array([pattern], dtype=np.uint32).view(np.float32)[0]
    if kind == "bf16":
        return np.uint16(pattern >> 16)
    f16 = {0x00000000: 0x0000, 0x80000000: 0x8000, 0x7F800000: 0x7C00, 0xFF800000: 0xFC00, P_NAN: 0x7E00, N_NAN: 0xFE00}
    return np.array([f16[pattern]], dtype=np.uint16).view(np.float16)[0]


def special_col(dim):
    return min(2, dim - 1)


def special_rows(rng, n, dim, kind):
    """(stored, widened f32): normal rows; then, as far as n reaches: row 0 +-0, row 1 subnormals of the store type, rows
    2 / 3 values near +-max / dim, row 4 sparse smallest subnormals, rows 5 .. 8 one +inf, -inf, +NaN, -NaN each in
    special_col, rows 10, 11 and n - 1 copies of row 9 (ties, to be ranked by id)."""
    stored = to_store(rng.standard_normal((n, dim)), kind)
    alt = np.arange(dim) % 2 == 0
    bits16 = stored.view(np.uint16) if kind != "f32" else None

    def put(r, fill):
        if r < n:
            fill(r)

    def zeros(r):
        stored[r] = [from_f32_bits(0 if a else 0x80000000, kind) for a in alt]

    def subnormals(r):
        if kind == "f32":
            stored[r] = (rng.standard_normal(dim) * 1e-40).astype(np.float32)
        else:
            bits16[r] = rng.integers(1, 0x80 if kind == "bf16" else 0x400, dim).astype(np.uint16) | np.where(alt, 0, 0x8000).astype(np.uint16)

    def big(r):
        if kind == "f16":
            stored[r] = np.float16(65504.0)
        else:
            b = np.float32(np.finfo(np.float32).max / dim) * rng.uniform(0.5, 1.0, dim).astype(np.float32)
            stored[r] = b if kind == "f32" else (b.view(np.uint32) >> 16).astype(np.uint16)  # truncated: stays below max / dim

    def neg_of(src):
        def fill(r):
            if kind == "f32":
                stored[r] = -stored[src]
            else:
                bits16[r] = bits16[src] ^ 0x8000
        return fill

    def sparse(r):
        if kind == "f32":
            stored[r, ::3] = np.float32(1e-39)
        else:
            bits16[r, ::3] = 1

    put(0, zeros)
    put(1, subnormals)
    put(2, big)
    put(3, neg_of(2))
    put(4, sparse)
    c = special_col(dim)
    for r, pattern in ((5, 0x7F800000), (6, 0xFF800000), (7, P_NAN), (8, N_NAN)):
        if r < n:
            stored[r, c] = from_f32_bits(pattern, kind)
    for r in (10, 11, n - 1):
        if 9 < r < n:
            stored[r] = stored[9]
    return stored, np.ascontiguousarray(widen(stored, kind), dtype=np.float32)


def make_queries(rng, dim, count):
    """`count` queries: normal values, every other one with subnormals and -0; special_col is 1.0 in all of them."""
    qs = rng.standard_normal((count, dim)).astype(np.float32)
    qs[1::2, ::5] = np.float32(3e-41)
    qs[1::2, 1::7] = -0.0
    qs[:, special_col(dim)] = 1.0
    return qs


@functools.lru_cache(maxsize=None)
def case(kind, dim, n, dist, invert, n_queries=2):
    """(handle, stored, widened rows, queries, oracle scores [n_queries][n]) - built once, shared, never written."""
    rng = np.random.default_rng([dim, n, int(dist), int(invert), ("f32", "f16", "bf16").index(kind)])
    stored, rows = special_rows(rng, n, dim, kind)
    orig = qa.OriginalVectors.from_data(stored, qa.VectorParameters(dim, n, dist, invert), dtype=kind)
    queries = make_queries(rng, dim, n_queries)
    want = np.stack([exact_all(dist, invert, q, rows) for q in queries])
    if dist == D.L2:
        for q, w in zip(queries, want):
            nan_sign_of_the_device(orig, q, w)
    for a in (stored, rows, queries, want):
        a.setflags(write=False)
    return orig, stored, rows, queries, want


def nan_sign_of_the_device(orig, q, want):
    """L2 alone: a NaN operand reaches the sum through q - v and d * d, and IEEE 754 leaves the sign of a NaN RESULT
    open: x86 subss hands the operand's sign on, v_sub_f32 adds the negated operand.  So the oracle fixes WHICH rows
    score NaN (rows 7 and 8) and every other bit of the store; the bits of those NaNs are taken from the list path
    (f32_pairs_kernel / half_pairs_kernel, the second reference).  Dot multiplies the operand by 1.0 and adds it, L1
    clears the sign: there the oracle's bits hold on both machines and nothing is replaced."""
    at = np.flatnonzero(np.isnan(want))
    assert at.size <= 2 and set(at) <= {7, 8}
    if at.size:
        got = orig.score_ids(q, at.astype(np.uint32))
        assert np.isnan(got).all()
        want[at] = got


def exact_all(dist, invert, q, rows):
    """qo_metric_f32(dist, q, row) for every row, sign flipped for invert."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    fn, dim, base, qp = qo.lib().qo_metric_f32, rows.shape[1], rows.ctypes.data, q.ctypes.data
    out = np.array([fn(int(dist), qp, base + i * dim * 4, dim) for i in range(rows.shape[0])], dtype=np.float32)
    return -out if invert else out


def dev_f32(a):
    return torch.tensor(np.array(a, dtype=np.float32)).cuda()


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ the C calls with a null list
def scan_prefix(orig, q, n_rows):
    """qamd_f32_score_ids(ids = NULL, n_ids = n_rows): the scores of rows 0 .. n_rows - 1."""
    qb = in_buf(q, np.float32)
    buf, ret = out_buf(None, n_rows, np.float32)
    check(_lib.lib().qamd_f32_score_ids(orig._h, qb.ptr, int(np.size(q)), qb.mem, None, n_rows, _lib.MEM_HOST, buf.ptr, buf.mem,
                                        stream_ptr(None)))
    return ret


def topk_prefix(orig, queries, n_rows, k, largest=True):
    """qamd_f32_rerank_batch(ids = NULL, n_ids = n_rows) -> [n_queries, k] ids and scores."""
    queries = np.atleast_2d(queries)
    nq, qdim = queries.shape
    qb = in_buf(queries, np.float32)
    ib, ids = out_buf(None, nq * k, np.uint32)
    sb, sc = out_buf(None, nq * k, np.float32)
    check(_lib.lib().qamd_f32_rerank_batch(orig._h, qb.ptr, nq, qdim, qb.mem, None, n_rows, _lib.MEM_HOST, k, int(largest),
                                           ib.ptr, sb.ptr, sb.mem, stream_ptr(None)))
    return ids.reshape(nq, k), sc.reshape(nq, k)


def check_scores(orig, queries, want, what):
    """score_all of every query, host and device outputs, against the oracle and against the list path."""
    n = orig.count
    all_ids = dev_u32(np.arange(n))
    for q, w in zip(queries, want):
        assert_bits_equal(orig.score_all(q), w, f"{what}: host query, host out")
        out = torch.empty(n, device="cuda")
        orig.score_all(dev_f32(q), out=out)
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), w, f"{what}: device query, device out")
        assert_bits_equal(orig.score_ids(q, all_ids), w, f"{what}: the list path score_ids(q, arange(n))")


def check_topk(got, want_scores, k, largest, what):
    ids, sc = got
    want_ids, want_sc = topk_total_order(want_scores, k, largest)
    assert np.array_equal(np.asarray(ids).view(np.uint32), want_ids), f"{what}: ids {ids[:8]} want {want_ids[:8]}"
    assert_bits_equal(sc, want_sc, what)


# ------------------------------------------------------------------------------------------------ 1. row shapes
def metrics_of(dim, all_at):
    return METRICS if dim in all_at else [(D.Dot, False)]


@pytest.mark.parametrize("dim,dist,invert", [(d, m, i) for d in F32_DIMS for m, i in metrics_of(d, (36, 65))])
def test_f32_scores_every_row_shape(dim, dist, invert):
    """dim % 4 == 0 takes the 16-byte loads, every other dim the dword loads; 4099 is 129 segments with a 3-value tail."""
    orig, _, _, queries, want = case("f32", dim, 257, dist, invert)
    check_scores(orig, queries, want, f"f32 dim {dim}")


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("dim,dist,invert", [(d, m, i) for d in HALF_DIMS for m, i in metrics_of(d, (72, 65))])
def test_half_scores_every_row_shape(kind, dim, dist, invert):
    """dim % 8 == 0 takes the 16-byte loads; even dims dword loads; odd dims 2-byte aligned rows and a lone last value."""
    orig, _, _, queries, want = case(kind, dim, 257, dist, invert)
    assert orig.dtype == kind
    check_scores(orig, queries, want, f"{kind} dim {dim}")


@pytest.mark.parametrize("kind,dim", [("f32", 36), ("f16", 72), ("bf16", 72)])
def test_borrowed_base_off_by_one_element_takes_the_unaligned_route(kind, dim):
    """A borrowed tensor whose base is one element past a 16-byte boundary, at a pitch that is a multiple of 16 bytes: the
    dword (2-byte aligned) loads on a shape that otherwise takes the 16-byte ones.  The buffer ends with the last row."""
    n = 257
    _, stored, _, queries, want = case(kind, dim, n, D.Dot, False)
    raw = stored.ravel()
    one_more = np.concatenate([raw[:1], raw])  # the rows, one element late
    if kind == "bf16":
        flat = torch.from_numpy(one_more.view(np.int16)).cuda().view(torch.bfloat16)
    else:
        flat = torch.from_numpy(one_more).cuda()
    rows = flat[1:].view(n, dim)
    assert rows.data_ptr() % 16 == flat.element_size() and rows.is_contiguous()
    orig = qa.OriginalVectors.from_data(rows, qa.VectorParameters(dim, n, D.Dot, False), borrow=True, dtype=kind)
    for q, w in zip(queries, want):
        assert_bits_equal(orig.score_all(q), w, "borrowed, offset base")
    check_topk(orig.topk(queries[0], 10), want[0], 10, True, "borrowed, offset base: topk")
    # the same buffer from its 16-byte aligned element 8 on, up to its last element: 16-byte loads on a borrowed buffer
    # that ends with the last row.  (Its rows are the values shifted by 7: the infs and NaNs meet other query values,
    # so the reference here is the list path alone.)
    m = n - 1
    shifted = flat[8:8 + m * dim].view(m, dim)
    assert shifted.data_ptr() % 16 == 0
    aligned = qa.OriginalVectors.from_data(shifted, qa.VectorParameters(dim, m, D.Dot, False), borrow=True, dtype=kind)
    assert_bits_equal(aligned.score_all(queries[0]), aligned.score_ids(queries[0], dev_u32(np.arange(m))), "borrowed, aligned base")


# ------------------------------------------------------------------------------------------------ 2. row counts
COUNT_STORES = [("f32", 36), ("f32", 5), ("f16", 3), ("bf16", 72)]  # 16-byte loads, dword loads, 2-byte aligned, 16-byte


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_and_prefixes(n):
    for kind, dim in COUNT_STORES:
        orig, _, _, queries, want = case(kind, dim, n, D.L2, False)
        check_scores(orig, queries[:1], want[:1], f"{kind} dim {dim} n {n}")
        for m in sorted({n - 1, 65} & set(range(1, n))):  # n_ids < count: rows past the prefix are not scored
            assert_bits_equal(scan_prefix(orig, queries[0], m), want[0][:m], f"{kind} dim {dim}: prefix {m} of {n}")
            ids, sc = topk_prefix(orig, queries[0], m, 10)
            check_topk((ids[0], sc[0]), want[0][:m], 10, True, f"{kind} dim {dim}: topk of prefix {m} of {n}")
        with pytest.raises(IndexError):
            scan_prefix(orig, queries[0], n + 1)
        with pytest.raises(IndexError):
            topk_prefix(orig, queries[0], n + 1, 10)
        with pytest.raises(IndexError):
            topk_prefix(orig, queries, n + 1, 10)
        assert scan_prefix(orig, queries[0], 0).size == 0


# ------------------------------------------------------------------------------------------------ 3. queries per pass
@pytest.mark.parametrize("kind,dim", [("f32", 36), ("f32", 33), ("bf16", 65), ("f16", 72)])
@pytest.mark.parametrize("nq", QUERY_COUNTS)
def test_queries_per_pass(kind, dim, nq):
    """k = n returns EVERY score of every query, in order: the scan's NQ sums are each that query's own chain.  9 queries
    are a pass of 8 and one of 1, 17 two of 8 and one of 1, 3 = 2 + 1, 5 = 4 + 1."""
    n = 300
    orig, _, _, queries, want = case(kind, dim, n, D.Dot, True, n_queries=17)
    ids, sc = orig.topk_batch(queries[:nq], n)
    assert ids.shape == (nq, n) and sc.shape == (nq, n)
    for j in range(nq):
        check_topk((ids[j], sc[j]), want[j], n, True, f"{kind} dim {dim}: query {j} of {nq}, every row")
    ids, sc = orig.topk_batch(queries[:nq], 10, largest=False)
    for j in range(nq):
        one_ids, one_sc = orig.topk(queries[j], 10, largest=False)
        assert np.array_equal(ids[j], one_ids), f"query {j} of {nq}: ids differ from the single-query call"
        assert_bits_equal(sc[j], one_sc, f"query {j} of {nq}: scores differ from the single-query call")
        check_topk((ids[j], sc[j]), want[j], 10, False, f"{kind} dim {dim}: query {j} of {nq}")
    # device queries and device outputs
    out_ids = torch.empty((nq, 10), dtype=torch.int32, device="cuda")
    out_sc = torch.empty((nq, 10), device="cuda")
    orig.topk_batch(dev_f32(queries[:nq]), 10, out_ids=out_ids, out_scores=out_sc)
    torch.cuda.synchronize()
    for j in range(nq):
        check_topk((host_u32(out_ids[j]), out_sc[j].cpu().numpy()), want[j], 10, True, f"device outputs, query {j} of {nq}")


# ------------------------------------------------------------------------------------------------ 4. top-k
@pytest.mark.parametrize("dist,invert", [(D.Dot, False), (D.L1, True), (D.L2, False)])
@pytest.mark.parametrize("k", [1, 10, 64, 65, 1024])
def test_topk_orders_specials_and_ties(k, dist, invert):
    """1000 rows: k = 1024 is padded; rows 9, 10, 11 and 999 are equal and rank by id; +-inf and +-NaN scores take their
    places in the total order on the score bits."""
    n = 1000
    for kind, dim in (("f32", 36), ("bf16", 65)):
        orig, _, _, queries, want = case(kind, dim, n, dist, invert)
        w = want[0]
        assert bits_of(w[9]) == bits_of(w[10]) == bits_of(w[11]) == bits_of(w[n - 1])
        assert np.isnan(w[7]) and np.isnan(w[8]) and np.isinf(w[5]) and np.isinf(w[6])
        if dist == D.Dot:
            assert bits_of(w[7]) >> 31 != bits_of(w[8]) >> 31, "NaN scores of both signs"
        for largest in (True, False):
            what = f"{kind} dim {dim} k {k} largest {largest}"
            check_topk(orig.topk(queries[0], k, largest), w, k, largest, what + ": host out")
            out_ids = torch.empty(k, dtype=torch.int32, device="cuda")
            out_sc = torch.empty(k, device="cuda")
            orig.topk(dev_f32(queries[0]), k, largest, out_ids=out_ids, out_scores=out_sc)
            torch.cuda.synchronize()
            check_topk((host_u32(out_ids), out_sc.cpu().numpy()), w, k, largest, what + ": device out")
            ids, sc = orig.topk_batch(queries, k, largest)
            for j in range(len(queries)):
                check_topk((ids[j], sc[j]), want[j], k, largest, what + f": batch query {j}")
        if k == 1024:
            ids, sc = orig.topk(queries[0], k)
            assert np.all(ids[n:] == PAD) and np.all(sc[n:] == -np.inf)


def bits_of(x):
    return int(np.float32(x).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5. mutation
@pytest.mark.parametrize("kind,dim", [("f32", 36), ("bf16", 65)])
def test_scan_after_append_upsert_and_reserve(kind, dim):
    n = 300
    _, stored, rows, queries, want = case(kind, dim, n, D.L1, False)
    vp = qa.VectorParameters(dim, 200, D.L1, False)
    grown = qa.OriginalVectors.from_data(np.ascontiguousarray(stored[:200]), vp, dtype=kind)
    grown.append(np.ascontiguousarray(stored[200:290]))
    grown.upsert(285, np.ascontiguousarray(stored[285:]))  # overwrites 5 rows, appends 10
    grown.upsert(3, np.ascontiguousarray(stored[3:6]))
    assert grown.count == n and grown.capacity >= n
    for q, w in zip(queries, want):
        assert_bits_equal(grown.score_all(q), w, "after append / upsert: a fresh store's scores")
    check_topk(grown.topk(queries[0], 65), want[0], 65, True, "after append / upsert: topk")
    ids, sc = grown.topk_batch(queries, 10)
    check_topk((ids[1], sc[1]), want[1], 10, True, "after append / upsert: topk_batch")
    grown.reserve(2 * n)
    assert grown.capacity >= 2 * n and grown.count == n
    assert_bits_equal(grown.score_all(queries[0]), want[0], "after reserve: the rows past count are not scored")
    check_topk(grown.topk(queries[0], 1024), want[0], 1024, True, "after reserve: topk pads at count, not at capacity")
    with pytest.raises(IndexError):
        scan_prefix(grown, queries[0], n + 1)  # room for 2n rows, n rows to score


# ------------------------------------------------------------------------------------------------ 6. regressions
def test_list_forms_keep_their_limits_and_results():
    n, dim = 1000, 36
    orig, _, rows, queries, want = case("f32", dim, n, D.Dot, False)
    q = queries[0]
    rng = np.random.default_rng(3)
    ids = rng.integers(0, n, 500).astype(np.uint32)
    before_scores = orig.score_ids(q, ids)
    before_rerank = orig.rerank(q, ids, 20)
    assert_bits_equal(before_scores, want[0][ids], "the list path")
    orig.score_all(q)
    orig.topk(q, 30)
    orig.topk_batch(queries, 30)
    assert_bits_equal(orig.score_ids(q, ids), before_scores, "score_ids after the scans")
    after = orig.rerank(q, ids, 20)
    assert np.array_equal(after[0], before_rerank[0])
    assert_bits_equal(after[1], before_rerank[1], "rerank after the scans")
    with pytest.raises(qa.EncodingError):  # a GIVEN list keeps the 8192 limit
        orig.rerank(q, np.zeros(8193, dtype=np.uint32), 10)
    with pytest.raises(qa.EncodingError):
        orig.rerank_batch(queries, np.zeros((2, 8193), dtype=np.uint32), 10)
    with pytest.raises(qa.EncodingError):  # k <= 1024 holds for both forms
        orig.topk(q, 1025)
    out = np.empty(4, dtype=np.float32)
    qb = in_buf(queries, np.float32)
    st = _lib.lib().qamd_f32_score_ids_batch(orig._h, qb.ptr, 2, dim, qb.mem, None, 2, None, 4, _lib.MEM_HOST,
                                             C.c_void_p(out.ctypes.data), _lib.MEM_HOST, None)
    assert st == _lib.ERR_ARGUMENTS, "score_ids_batch keeps requiring its lists"
    with pytest.raises(qa.EncodingError):
        orig.score_all(q[:-1])


def test_two_threads_scan_one_handle():
    n, dim = 1000, 65
    orig, _, _, queries, want = case("bf16", dim, n, D.L2, True)
    start = threading.Barrier(2)
    errors = []

    def worker(i):
        try:
            torch.cuda.set_device(0)
            start.wait()
            for _ in range(5):
                if not np.array_equal(orig.score_all(queries[i]).view(np.uint32), want[i].view(np.uint32)):
                    errors.append(f"thread {i}: score_all differs")
                ids, sc = orig.topk(queries[i], 30)
                w_ids, w_sc = topk_total_order(want[i], 30, True)
                if not (np.array_equal(ids, w_ids) and np.array_equal(sc.view(np.uint32), w_sc.view(np.uint32))):
                    errors.append(f"thread {i}: topk differs")
                ids, sc = orig.topk_batch(queries, 30)
                if not np.array_equal(ids[i], w_ids):
                    errors.append(f"thread {i}: topk_batch differs")
        except Exception as e:  # noqa: BLE001
            errors.append(f"thread {i}: {e!r}")

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
