"""score_internal against the whole store: score_internal_all / topk_internal of the three quantizers.

Every score is compared as a raw bit pattern with BOTH yardsticks: the oracle's *_score_internal(i, j) looped over j, and
score_internal_ids(i, arange(n)) on the same handle (the random-access pair kernels).  Top-k is checked against
util.topk_total_order on those scores, both directions.  Stores are adopted from seeded random codes (from_storage), rows i
= 0, n // 2 and n - 1.  The shapes are the smallest that reach each route: u8 rows of 1, 7 (ragged), 8 (the shortest with a
packed image), 48 and 129 chunks (generic scan, classic top-k) and lane mode 1; binary rows of 1 .. 129 bytes, one and two
bits; PQ rows of 1 .. 160 chunks (row-per-lane form, one slice, the largest slice, sliced on the 128-byte pitch, sliced on
the planar image); stores of 1, 65 / 100 and 4099 / 4133 rows (below and above every whole-store gate, no multiple of a
tile); k on both sides of the single-launch limit (64) and up to 1000 / 1024.
"""
import ctypes as C

import numpy as np
import pytest

from util import (U8_ALPHA, assert_bits_equal, bin_random_rows, bits, store_rows, topk_total_order, wide_dot_pair_2096)

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
from oracle import qoracle as qo  # noqa: E402
from quantization_amd import _lib  # noqa: E402

D = qa.DistanceType
SETTINGS = [(d, inv) for d in (D.Dot, D.L2, D.L1) for inv in (False, True)]
SETTING_IDS = [f"{d.name}{'-inv' if inv else ''}" for d, inv in SETTINGS]


def rows_of(n):
    return sorted({0, n // 2, n - 1})


def check_store(enc, n, oracle_scores, ks, what, rows=None):
    """score_internal_all(i) against both yardsticks and topk_internal(i, k) for every k, both directions."""
    ids_all = np.arange(n, dtype=np.uint32)
    for i in (rows_of(n) if rows is None else rows):
        want = oracle_scores(i)
        pairs = enc.score_internal_ids(i, ids_all)
        assert_bits_equal(pairs, want, f"{what} n={n} i={i}: score_internal_ids against the oracle")
        got = enc.score_internal_all(i)
        assert got.shape == (n,)
        assert_bits_equal(got, want, f"{what} n={n} i={i}: score_internal_all against the oracle")
        assert_bits_equal(got, pairs, f"{what} n={n} i={i}: score_internal_all against score_internal_ids")
        for k in ks:
            for largest in (True, False):
                ids, sc = enc.topk_internal(i, k, largest)
                wi, ws = topk_total_order(want, k, largest)
                tag = f"{what} n={n} i={i} k={k} largest={largest}"
                assert np.array_equal(ids, wi), f"{tag}: ids {ids[:8]} want {wi[:8]}"
                assert_bits_equal(sc, ws, f"{tag}: scores")


# ---------------------------------------------------------------------------------------------------------------- u8
U8_OFFSET = 0.25  # a store offset other than 0: score_internal's `diff` = actual_dim * offset^2 is in every score


def u8_meta(dim, n, dist, invert):
    """(from_storage metadata, oracle Meta) as the reference's encoder writes them at alpha 1 / 127, offset 0.25."""
    _, meta = qo.u8_encode_with(np.zeros((1, dim), dtype=np.float32), int(dist), bool(invert), float(U8_ALPHA), U8_OFFSET)
    meta.count = n
    md = {"actual_dim": int(meta.actual_dim), "alpha": np.float32(meta.alpha), "offset": np.float32(meta.offset),
          "multiplier": np.float32(meta.multiplier),
          "vector_parameters": qa.VectorParameters(dim, n, qa.DistanceType(int(dist)), bool(invert))}
    return md, meta


def u8_open(rows, dim, dist, invert):
    md, meta = u8_meta(dim, rows.shape[0], dist, invert)
    return qa.EncodedVectorsU8.from_storage(rows, md), meta


def u8_oracle(meta, rows, order=qo.ORDER_SIMPLE):
    n = rows.shape[0]
    return lambda i: np.array([qo.u8_score_internal(meta, rows, i, j, order) for j in range(n)], dtype=np.float32)


U8_KS = (1, 64, 65, 1000)


@pytest.mark.parametrize("dist,invert", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("dim", [16, 100, 128, 768, 2064])
def test_u8_every_route(dim, dist, invert):
    for n in (1, 65, 4099):
        rows, _ = store_rows(dim, n, seed=3)
        enc, meta = u8_open(rows, dim, dist, invert)
        check_store(enc, n, u8_oracle(meta, rows), U8_KS, f"u8 dim={dim} {dist.name} invert={invert}")


@pytest.mark.parametrize("dist", [D.Dot, D.L2], ids=["Dot", "L2"])
def test_u8_lane_mode_1(dist):
    """dim 1536 with rows of all-127 codes mixed in, so that pair sums pass 2^24 (127 * 127 * 1536 = 24.8M): lane mode 1
    against the oracle's AVX2 order, mode 0 against the exact sum rounded once.  (Below actual_dim 2096 the two orders
    cannot differ - each f32 half sum of the lane order stays exact - so the case where they do is the next test.)"""
    dim = 1536
    for n in (65, 4099):
        rows, _ = store_rows(dim, n, seed=5)
        full = sorted({0, n // 2, n - 1, 7, 8, 30})
        rows[full, 4:] = 127
        rows[8, 4] = 126  # an odd pair sum above 2^24: not an f32
        enc, meta = u8_open(rows, dim, dist, False)
        assert max(int(rows[a, 4:].astype(np.int64) @ rows[b, 4:].astype(np.int64)) for a in full for b in (7, 8)) > 2 ** 24
        check_store(enc, n, u8_oracle(meta, rows), (1, 64, 65), f"u8 lane mode 0 {dist.name}")
        enc.set_lane_mode(1)
        check_store(enc, n, u8_oracle(meta, rows, qo.ORDER_AVX2), (1, 64, 65, 1000), f"u8 lane mode 1 {dist.name}")


def test_u8_lane_modes_differ_at_2096():
    """The first row length at which the lane order can differ from the exact sum, on util.wide_dot_pair_2096: the two
    modes of one store give different bits for that pair, each its oracle order's."""
    dim, n = 2096, 65
    q, v = wide_dot_pair_2096()
    rows, _ = store_rows(dim, n, seed=9)
    rows[0, 4:], rows[n // 2, 4:], rows[n - 1, 4:] = q, v, v
    enc, meta = u8_open(rows, dim, D.Dot, False)
    simple, lanes = u8_oracle(meta, rows), u8_oracle(meta, rows, qo.ORDER_AVX2)
    assert bits(simple(0))[n // 2] != bits(lanes(0))[n // 2]
    check_store(enc, n, simple, (1, 64), "u8 2096 lane mode 0")
    enc.set_lane_mode(1)
    check_store(enc, n, lanes, (1, 64), "u8 2096 lane mode 1")


@pytest.mark.parametrize("dist", [D.Dot, D.L2], ids=["Dot", "L2"])
@pytest.mark.parametrize("dim", [128, 2064], ids=["fused", "classic"])
def test_u8_special_scores(dim, dist):
    """+inf, -inf and NaN planted in a few rows' stored offsets: the scores carry them and every route ranks them by the
    one total order of DESIGN 3.5 (+NaN outermost for `largest`, -NaN for smallest-first), both directions."""
    n = 4099
    rows, _ = store_rows(dim, n, seed=11)
    planted = {5: 0x7F800000, 77: 0xFF800000, 900: 0x7FC00000, 901: 0xFFC00001, 2050: 0x7F800000, 4098: 0x7FC00123}
    for r, u in planted.items():
        rows[r, :4] = np.array([u], dtype=np.uint32).view(np.uint8)
    enc, meta = u8_open(rows, dim, dist, False)
    oracle = u8_oracle(meta, rows)
    want = oracle(n // 2)
    assert np.isnan(want[[900, 901, 4098]]).all() and np.isinf(want[[5, 77, 2050]]).all()
    check_store(enc, n, oracle, U8_KS, f"u8 special offsets dim={dim} {dist.name}", rows=[n // 2])


# ------------------------------------------------------------------------------------------------------------ binary
def bin_open(rows, dim, dist, invert, two):
    vp = qa.VectorParameters(dim, rows.shape[0], dist, invert)
    if not two:
        return qa.EncodedVectorsBin.from_storage(rows, vp)
    lo, hi = np.full(dim, -0.5, dtype=np.float32), np.full(dim, 0.5, dtype=np.float32)
    return qa.EncodedVectorsBin.from_storage(rows, vp, encoding=qa.BinaryEncoding.TwoBits, thresholds=(lo, hi))


@pytest.mark.parametrize("dist,invert", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("two", [False, True], ids=["one-bit", "two-bit"])
@pytest.mark.parametrize("dim", [8, 128, 1024, 1032])
def test_binary_every_route(dim, two, dist, invert):
    """A two-bit row is scored as a one-bit row of 2 dim bits: that is the oracle's row.  Binary scores
    take few values, so the fused route's candidate list overflows and the exact path has to answer (k = 200)."""
    code_bits = 2 * dim if two else dim
    for n in (1, 65, 4099):
        rows = bin_random_rows(n, code_bits, seed=dim + n)
        enc = bin_open(rows, dim, dist, invert, two)
        oracle = lambda i: np.array([qo.bin_score_internal(rows, code_bits, int(dist), invert, i, j) for j in range(n)],
                                    dtype=np.float32)
        check_store(enc, n, oracle, (1, 64, 200), f"binary dim={dim} two={two} {dist.name} invert={invert}")


# ---------------------------------------------------------------------------------------------------------------- PQ
PQ_MS = [1, 3, 16, 17, 96, 100, 144, 150, 160]
PQ_KS = (1, 64, 65, 1024)


def pq_dim(m, chunk):
    return 8 * m - 3 if chunk == "ragged" else m * chunk


def pq_store(m, chunk, n, dist, invert, seed, centroids=None):
    dim, cs = pq_dim(m, chunk), (8 if chunk == "ragged" else chunk)
    rng = np.random.default_rng(1000 * m + 10 * n + seed)
    cen = rng.standard_normal((256, dim)).astype(np.float32) if centroids is None else centroids(dim)
    rows = rng.integers(0, 256, size=(n, m), dtype=np.uint8)
    assert qo.pq_chunks(dim, cs) == m
    return rows, cen, dim, cs


def pq_open(rows, cen, dim, cs, dist, invert):
    return qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(dim, rows.shape[0], dist, invert), cs, cen)


def pq_oracle(rows, cen, dim, cs, dist, invert):
    n = rows.shape[0]
    return lambda i: np.array([qo.pq_score_internal(rows, dim, cs, cen, int(dist), invert, i, j) for j in range(n)],
                              dtype=np.float32)


def pq_cases():
    """Every m with every metric setting; chunk size 8, 1 and the ragged dim = 8 m - 3 rotate so that each m meets each."""
    chunks = (8, 1, "ragged")
    return [(m, chunks[(a + b) % 3], d, inv) for a, m in enumerate(PQ_MS) for b, (d, inv) in enumerate(SETTINGS)]


@pytest.mark.parametrize("m,chunk,dist,invert", pq_cases(),
                         ids=[f"m{m}-cs{c}-{d.name}{'-inv' if inv else ''}" for m, c, d, inv in pq_cases()])
def test_pq_every_route(m, chunk, dist, invert):
    for n in (1, 100, 4133):
        rows, cen, dim, cs = pq_store(m, chunk, n, dist, invert, seed=1)
        enc = pq_open(rows, cen, dim, cs, dist, invert)
        check_store(enc, n, pq_oracle(rows, cen, dim, cs, dist, invert), PQ_KS,
                    f"pq m={m} chunk={chunk} {dist.name} invert={invert}")


@pytest.mark.parametrize("dist", [D.Dot, D.L2, D.L1], ids=["Dot", "L2", "L1"])
@pytest.mark.parametrize("m", [3, 100, 150])
def test_pq_zero_centroids_inverted_score_minus_zero(m, dist):
    """All chunk metrics are +0: the sum is +0 and `invert` negates it once, after the sum -> 0x80000000 for every row, as
    score_internal gives (a table negated entry by entry would sum -0 + -0 ... from +0 to +0)."""
    for n in (100, 4133):
        rows, cen, dim, cs = pq_store(m, 8, n, dist, True, seed=2, centroids=lambda dim: np.zeros((256, dim), dtype=np.float32))
        enc = pq_open(rows, cen, dim, cs, dist, True)
        for i in rows_of(n):
            got = enc.score_internal_all(i)
            assert np.all(bits(got) == 0x80000000), f"m={m} n={n} i={i}: {bits(got)[:4]}"
            assert_bits_equal(got, enc.score_internal_ids(i, np.arange(n, dtype=np.uint32)), "against score_internal_ids")
            assert bits(qo.pq_score_internal(rows, dim, cs, cen, int(dist), True, i, 0)) == 0x80000000
        ids, sc = enc.topk_internal(n // 2, 65, True)
        assert np.array_equal(ids, np.arange(65)) and np.all(bits(sc) == 0x80000000)  # all tie: the lowest ids


@pytest.mark.parametrize("n", [100, 4133])
def test_pq_rows_of_equal_codes_tie_to_the_lower_id(n):
    m, cs = 96, 8
    rows, cen, dim, cs = pq_store(m, cs, n, D.L2, True, seed=3)
    i = n // 2
    twins = [3, i, n - 2]
    rows[twins] = rows[i]
    enc = pq_open(rows, cen, dim, cs, D.L2, True)
    oracle = pq_oracle(rows, cen, dim, cs, D.L2, True)
    want = oracle(i)
    assert len({int(b) for b in bits(want[twins])}) == 1
    for k in (1, 3, 64, 65):
        ids, _ = enc.topk_internal(i, k, True)  # inverted L2: the row's own copies are the best rows
        assert list(ids[:min(k, 3)]) == twins[:min(k, 3)], (k, ids[:3])
    check_store(enc, n, oracle, (1, 3, 64, 65), "pq equal rows", rows=[i])


# ------------------------------------------------------------------------------------------------------ store changes
def test_scores_follow_append_and_upsert():
    """After append and upsert on a built store of each kind score_internal_all covers the new count and sees the new
    codes; after an overwrite of row i itself the scores follow.  The oracle reads the rows the store exports."""
    rng = np.random.default_rng(17)
    dim, n0 = 128, 1000
    data = rng.random((n0 + 40, dim), dtype=np.float32)
    cen = rng.standard_normal((256, dim)).astype(np.float32)
    vp = qa.VectorParameters(dim, n0, D.Dot, False)
    u8 = qa.EncodedVectorsU8.encode(data[:n0], vp)
    pq = qa.EncodedVectorsPQ.encode(data[:n0], vp, 8, centroids=cen)
    bn = qa.EncodedVectorsBin.encode(data[:n0] - 0.5, vp)

    def oracles(n):
        ur = u8.storage_bytes()
        md = u8.metadata
        meta = qo.Meta(int(md["actual_dim"]), float(md["alpha"]), float(md["offset"]), float(md["multiplier"]), dim, n,
                       int(D.Dot), 0)
        pr, br = pq.storage_bytes(), bn.storage_bytes()
        return {"u8": (u8, u8_oracle(meta, ur)), "pq": (pq, pq_oracle(pr, cen, dim, 8, D.Dot, False)),
                "bin": (bn, lambda i: np.array([qo.bin_score_internal(br, dim, int(D.Dot), False, i, j) for j in range(n)],
                                               dtype=np.float32))}

    i = 500
    before = {k: e.score_internal_all(i) for k, (e, _) in oracles(n0).items()}
    for e, shift in ((u8, 0.0), (pq, 0.0), (bn, 0.5)):
        e.upsert(998, data[n0 + 37:n0 + 40] - shift)  # the last two rows and one more
        e.append(data[n0:n0 + 37] - shift)
    n = n0 + 38
    for kind, (e, oracle) in oracles(n).items():
        assert e.count == n
        check_store(e, n, oracle, (1, 65), f"{kind} after append / upsert", rows=[i, n - 1])
        assert_bits_equal(e.score_internal_all(i)[:998], before[kind][:998], f"{kind}: untouched rows")
    for e, shift in ((u8, 0.0), (pq, 0.0), (bn, 0.5)):
        e.upsert(i, data[7:8][:, ::-1].copy() - shift)  # row i itself
    for kind, (e, oracle) in oracles(n).items():
        check_store(e, n, oracle, (1, 65), f"{kind} after overwriting row i", rows=[i])
        assert not np.array_equal(bits(e.score_internal_all(i)[:998]), bits(before[kind][:998])), kind


# ----------------------------------------------------------------------------------------------------------- refusals
def small_stores():
    u8_rows, _ = store_rows(32, 10, seed=1)
    u8, _ = u8_open(u8_rows, 32, D.Dot, False)
    rows, cen, dim, cs = pq_store(4, 8, 10, D.Dot, False, seed=4)
    return [u8, pq_open(rows, cen, dim, cs, D.Dot, False), bin_open(bin_random_rows(10, 64, seed=1), 64, D.Dot, False, False)]


def test_refusals():
    L = _lib.lib()
    out = np.zeros(16, dtype=np.float32)
    ids = np.zeros(1025, dtype=np.uint32)
    sc = np.zeros(1025, dtype=np.float32)
    o, ip, sp = out.ctypes.data, ids.ctypes.data, sc.ctypes.data
    for enc in small_stores():
        all_, topk = enc._fn("score_internal_all"), enc._fn("topk_internal")
        assert all_(enc._h, 10, o, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS  # i == count
        assert b"out of range" in L.qamd_last_error()
        assert topk(enc._h, 10, 3, 1, ip, sp, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS
        assert topk(enc._h, 0, 1025, 1, ip, sp, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS  # k > 1024
        assert all_(enc._h, 0, None, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS  # null outputs
        assert topk(enc._h, 0, 3, 1, None, sp, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS
        assert topk(enc._h, 0, 3, 1, ip, None, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS
        assert topk(enc._h, 0, 0, 1, None, None, _lib.MEM_HOST, None) == _lib.OK  # k == 0: nothing is asked for
        assert all_(enc._h, 9, o, _lib.MEM_HOST, None) == _lib.OK and topk(enc._h, 9, 3, 1, ip, sp, _lib.MEM_HOST, None) == _lib.OK


def test_pq_without_centroids_is_refused():
    """The one PQ handle that has no centroids: a store of dimension 0 (256 x 0 values)."""
    L = _lib.lib()
    vp = qa.VectorParameters(0, 3, D.Dot, False).to_c()
    cen = np.zeros(4, dtype=np.float32)
    rows = np.zeros(4, dtype=np.uint8)
    h = C.c_void_p()
    assert L.qamd_pq_from_rows(rows.ctypes.data, _lib.MEM_HOST, C.byref(vp), 8, cen.ctypes.data, None, C.byref(h)) == _lib.OK
    try:
        out = np.zeros(4, dtype=np.float32)
        ids = np.zeros(4, dtype=np.uint32)
        assert L.qamd_pq_score_internal_all(h, 0, out.ctypes.data, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS
        assert b"centroids" in L.qamd_last_error()
        assert L.qamd_pq_topk_internal(h, 0, 2, 1, ids.ctypes.data, out.ctypes.data, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS
    finally:
        L.qamd_pq_free(h)


def test_empty_stores_are_ok():
    L = _lib.lib()
    ids = np.zeros(3, dtype=np.uint32)
    sc = np.zeros(3, dtype=np.float32)
    u8, _ = u8_open(np.zeros((0, 36), dtype=np.uint8), 32, D.Dot, False)
    cen = np.zeros((256, 32), dtype=np.float32)
    stores = [u8, pq_open(np.zeros((0, 4), dtype=np.uint8), cen, 32, 8, D.Dot, False),
              bin_open(np.zeros((0, 8), dtype=np.uint8), 64, D.Dot, False, False)]
    for enc in stores:
        assert enc._fn("score_internal_all")(enc._h, 0, None, _lib.MEM_HOST, None) == _lib.OK
        assert enc._fn("topk_internal")(enc._h, 0, 3, 1, ids.ctypes.data, sc.ctypes.data, _lib.MEM_HOST, None) == _lib.OK
        assert np.all(ids == 0xFFFFFFFF) and np.all(np.isneginf(sc))  # the padding of a short list
        assert L.qamd_last_error() is not None


# --------------------------------------------------------------------------------- the query scans are unchanged
def test_query_scans_are_unchanged_after_internal_calls():
    """score_all / topk with an encoded query still equal the oracle bit for bit in a process that has run the internal
    forms of the same kernels: the EPI_POINT instantiations, the binary scans and the PQ query scans are what they were."""
    rng = np.random.default_rng(23)
    n, dim = 4099, 768
    # u8: the packed image's blocked scan
    rows, query = store_rows(dim, n, seed=2)
    enc, meta = u8_open(rows, dim, D.Dot, False)
    enc.score_internal_all(7), enc.topk_internal(7, 65)
    codes, qoff = qo.u8_encode_query(meta, query)
    want = qo.u8_score_all(meta, rows, codes, qoff)
    q = enc.encode_query(query)
    assert_bits_equal(enc.score_all(q), want, "u8 score_all")
    for k in (30, 65):
        ids, sc = enc.topk(q, k)
        wi, ws = topk_total_order(want, k)
        assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), f"u8 topk k={k}"
    # binary
    brows = bin_random_rows(n, 1024, seed=3)
    benc = bin_open(brows, 1024, D.Dot, False, False)
    benc.score_internal_all(7), benc.topk_internal(7, 200)
    bq = np.where(rng.random(1024) < 0.5, -1.0, 1.0).astype(np.float32)
    want = qo.bin_score_all(brows, qo.bin_encode(bq[None, :])[0], 1024, qo.DOT, False)
    bqe = benc.encode_query(bq)
    assert_bits_equal(benc.score_all(bqe), want, "binary score_all")
    ids, sc = benc.topk(bqe, 30)
    wi, ws = topk_total_order(want, 30)
    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), "binary topk"
    # PQ
    prows, cen, pdim, cs = pq_store(96, 8, 4133, D.Dot, False, seed=5)
    penc = pq_open(prows, cen, pdim, cs, D.Dot, False)
    penc.score_internal_all(7), penc.topk_internal(7, 65)
    pquery = rng.standard_normal(pdim).astype(np.float32)
    want = qo.pq_score_all(prows, qo.pq_encode_query(pquery, cs, cen, qo.DOT, False), order=qo.ORDER_SSE)
    pq = penc.encode_query(pquery)
    assert_bits_equal(penc.score_all(pq), want, "pq score_all")
    for k in (30, 65):
        ids, sc = penc.topk(pq, k)
        wi, ws = topk_total_order(want, k)
        assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), f"pq topk k={k}"


def test_device_outputs():
    """Device outputs: score_internal_all only enqueues on the caller's stream, topk_internal synchronises it."""
    torch = pytest.importorskip("torch")
    n = 4099
    rows, _ = store_rows(128, n, seed=4)
    u8, _ = u8_open(rows, 128, D.L2, True)
    prows, cen, pdim, cs = pq_store(150, 8, n, D.L2, False, seed=6)
    stores = [u8, pq_open(prows, cen, pdim, cs, D.L2, False), bin_open(bin_random_rows(n, 128, seed=5), 128, D.L1, False, False)]
    for enc in stores:
        want = enc.score_internal_all(n - 1)
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        enc.score_internal_all(n - 1, out=out)
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), want, "device output")
        oi = torch.empty(65, dtype=torch.int32, device="cuda")
        os_ = torch.empty(65, dtype=torch.float32, device="cuda")
        enc.topk_internal(n - 1, 65, False, out_ids=oi, out_scores=os_)
        wi, ws = topk_total_order(want, 65, False)
        assert np.array_equal(oi.cpu().numpy().view(np.uint32), wi)
        assert_bits_equal(os_.cpu().numpy(), ws, "device top-k scores")
