"""Many stored rows against the whole store: the null-list form of *_score_internal_ids_batch and
*_score_internal_ids, score_internal_all_batch and topk_internal_batch of the three quantizers.

Every score is compared as a raw bit pattern with three yardsticks: the oracle's *_score_internal(i, j) looped over j,
score_internal_ids(i, arange(n)) on the same handle (the random-access pair kernels), and score_internal_all(i).  The
references of a store are computed once per distinct row and shared by every list length.  Shapes are the smallest that
reach each route: u8 rows of 8 pieces (no multi form), 13 (ragged), 48 (4-wide; L1: 8-wide), 112 and 128 (2-wide), 129 (no
multi form) and lane mode 1; binary rows of 4 .. 65 pieces; PQ rows below and above the quad kernel and on the planar
image; row counts that leave partial tiles and waves whose later tiles are past the end; list lengths with an unused slot
in a pass, a remainder of one and several groups, duplicates and the last row included.
"""
import ctypes as C

import numpy as np
import pytest

from util import (U8_ALPHA, assert_bits_equal, bin_open_rows, bin_random_rows, bits, store_rows, topk_total_order,
                  wide_dot_pair_2096)

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
from oracle import qoracle as qo  # noqa: E402
from quantization_amd import _lib  # noqa: E402

D = qa.DistanceType
SETTINGS = [(d, inv) for d in (D.Dot, D.L2, D.L1) for inv in (False, True)]
SETTING_IDS = [f"{d.name}{'-inv' if inv else ''}" for d, inv in SETTINGS]
SENTINEL = np.float32(-12345.5)


def master_rows(n, length=17):
    """The rows of every list of a store: rows[:len].  The last row first, a duplicate from length 4 on."""
    rows = np.random.default_rng(1000 + n).integers(0, n, size=length, dtype=np.uint32)
    rows[0] = n - 1
    rows[3] = rows[1]
    return rows


def prefixes(n):
    return sorted({p for p in (1, 64, n - 1, n) if 1 <= p <= n})


def references(enc, n, oracle, rows, what):
    """{i: scores} for the distinct rows, the three yardsticks agreeing on each."""
    ids_all = np.arange(n, dtype=np.uint32)
    refs = {}
    for i in sorted({int(r) for r in rows}):
        want = oracle(i)
        assert_bits_equal(enc.score_internal_ids(i, ids_all), want, f"{what} n={n} i={i}: score_internal_ids against the oracle")
        assert_bits_equal(enc.score_internal_all(i), want, f"{what} n={n} i={i}: score_internal_all against the oracle")
        refs[i] = want
    return refs


def check_batch(enc, n, oracle, what, lens, master=None):
    master = master_rows(n) if master is None else master
    refs = references(enc, n, oracle, master[:max(lens)], what)
    for ln in lens:
        rows = master[:ln]
        got = enc.score_internal_all_batch(rows)
        assert got.shape == (ln, n)
        for l, i in enumerate(rows):
            assert_bits_equal(got[l], refs[int(i)], f"{what} n={n} len={ln} l={l} row={i}")
    rows = master[:min(5, max(lens))]
    for p in prefixes(n):
        got = enc.score_internal_all_batch(rows, n_rows=p)
        assert got.shape == (len(rows), p)
        for l, i in enumerate(rows):
            assert_bits_equal(got[l], refs[int(i)][:p], f"{what} n={n} prefix={p} l={l} row={i}")
        i = int(rows[-1])  # the single-row null list: score_internal_all's scan over a prefix
        one = enc.score_internal_ids(i, None, n_rows=p)
        assert one.shape == (p,)
        assert_bits_equal(one, refs[i][:p], f"{what} n={n} prefix={p}: score_internal_ids(i, None)")
    return refs


# ---------------------------------------------------------------------------------------------------------------- u8
U8_OFFSET = 0.25  # a store offset other than 0: score_internal's `diff` = actual_dim * offset^2 is in every score
U8_LENS = (1, 2, 3, 4, 5, 8, 9, 17)
U8_COUNTS = (1, 63, 65, 1025, 4099)


def u8_open(rows, dim, dist, invert):
    _, meta = qo.u8_encode_with(np.zeros((1, dim), dtype=np.float32), int(dist), bool(invert), float(U8_ALPHA), U8_OFFSET)
    meta.count = rows.shape[0]
    md = {"actual_dim": int(meta.actual_dim), "alpha": np.float32(meta.alpha), "offset": np.float32(meta.offset),
          "multiplier": np.float32(meta.multiplier),
          "vector_parameters": qa.VectorParameters(dim, rows.shape[0], qa.DistanceType(int(dist)), bool(invert))}
    return qa.EncodedVectorsU8.from_storage(rows, md), meta


def u8_oracle(meta, rows, order=qo.ORDER_SIMPLE):
    n = rows.shape[0]
    return lambda i: np.array([qo.u8_score_internal(meta, rows, i, j, order) for j in range(n)], dtype=np.float32)


@pytest.mark.parametrize("dist,invert", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("dim", [128, 208, 768, 1792, 2048, 2064])
def test_u8_every_route(dim, dist, invert):
    for n in U8_COUNTS:
        rows, _ = store_rows(dim, n, seed=3)
        enc, meta = u8_open(rows, dim, dist, invert)
        check_batch(enc, n, u8_oracle(meta, rows), f"u8 dim={dim} {dist.name} invert={invert}", U8_LENS)


def test_u8_lane_mode_1_at_2096():
    """Lane mode 1 on a Dot store takes the lane-order kernel row by row: on util.wide_dot_pair_2096 the two modes give
    different bits, each its oracle order's, through the batch as through the single-row calls."""
    dim, n = 2096, 65
    q, v = wide_dot_pair_2096()
    rows, _ = store_rows(dim, n, seed=9)
    rows[0, 4:], rows[n // 2, 4:], rows[n - 1, 4:] = q, v, v
    enc, meta = u8_open(rows, dim, D.Dot, False)
    master = np.array([0, n // 2, n - 1, 0, 5], dtype=np.uint32)
    simple = check_batch(enc, n, u8_oracle(meta, rows), "u8 2096 lane mode 0", (2, 5), master)
    enc.set_lane_mode(1)
    lanes = check_batch(enc, n, u8_oracle(meta, rows, qo.ORDER_AVX2), "u8 2096 lane mode 1", (2, 5), master)
    assert bits(simple[0])[n // 2] != bits(lanes[0])[n // 2]


@pytest.mark.parametrize("dist", [D.Dot, D.L1], ids=["Dot", "L1"])
def test_u8_lane_mode_1_below_2096(dist):
    """Mode 1 at a row size that has a multi form in mode 0 (dim 768): Dot goes row by row, L1 has no lane order."""
    dim, n = 768, 1025
    rows, _ = store_rows(dim, n, seed=5)
    enc, meta = u8_open(rows, dim, dist, False)
    enc.set_lane_mode(1)
    check_batch(enc, n, u8_oracle(meta, rows, qo.ORDER_AVX2 if dist == D.Dot else qo.ORDER_SIMPLE), f"u8 mode 1 {dist.name}", (3, 9))


# ------------------------------------------------------------------------------------------------------------ binary
BIN_LENS = (1, 2, 3, 5, 8, 9)
BIN_COUNTS = (1, 65, 4099)
U8S, U128S = qa.BitsStoreType.U8, qa.BitsStoreType.U128


def bin_oracle(rows, code_bits, dist, invert, store=0):
    n = rows.shape[0]
    return lambda i: np.array([qo.bin_score_internal(rows, code_bits, int(dist), invert, i, j, int(store)) for j in range(n)],
                              dtype=np.float32)


def bin_open(rows, dim, dist, invert, two, store):
    if not two:
        return bin_open_rows(rows, dim, dist, invert, int(store))
    lo, hi = np.full(dim, -0.5, dtype=np.float32), np.full(dim, 0.5, dtype=np.float32)
    return qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(dim, rows.shape[0], dist, invert), store=store,
                                             encoding=qa.BinaryEncoding.TwoBits, thresholds=(lo, hi))


BIN_SHAPES = [(512, False, U128S), (512, True, U128S), (1024, False, U128S), (1152, False, U128S), (2048, False, U8S),
              (4096, False, U128S), (8192, False, U128S), (8320, False, U128S), (1000, False, U8S), (1000, True, U8S)]


@pytest.mark.parametrize("dim,two,store", BIN_SHAPES, ids=[f"{d}{'-two' if t else ''}-{s.name}" for d, t, s in BIN_SHAPES])
def test_binary_every_route(dim, two, store):
    """A two-bit row is scored as a one-bit row of 2 dim bits: that is the oracle's row.  Rows of 4 (per
    row), 8, 9, 16, 32, 64 (4-wide only) and 65 (per row) pieces; dim 1000 on the u8 store type."""
    code_bits = 2 * dim if two else dim
    for k, (dist, invert) in enumerate(SETTINGS):
        for n in BIN_COUNTS if k == (dim // 8) % len(SETTINGS) else (65,):  # every setting at 65 rows, one at every count
            rows = bin_random_rows(n, code_bits, seed=dim + n, kind=int(store))
            enc = bin_open(rows, dim, dist, invert, two, store)
            check_batch(enc, n, bin_oracle(rows, code_bits, dist, invert, store),
                        f"binary dim={dim} two={two} {store.name} {dist.name} invert={invert}", BIN_LENS)


@pytest.mark.parametrize("encoding", [qa.BinaryEncoding.OneBitRotated, qa.BinaryEncoding.TwoBitsRotated], ids=["one", "two"])
def test_binary_rotated_store(encoding):
    """A rotated store is served as a plain store of P dimensions: the oracle reads the rows it exports."""
    dim, n, p = 600, 1030, 1024
    x = np.random.default_rng(3).standard_normal((n, dim)).astype(np.float32)
    enc = qa.EncodedVectorsBin.encode(x, qa.VectorParameters(dim, n, D.L2, True), encoding=encoding)
    rows = enc.storage_bytes()
    code_bits = 2 * p if encoding.two_bits else p
    check_batch(enc, n, bin_oracle(rows, code_bits, D.L2, True), f"binary {encoding.name}", BIN_LENS)


# ---------------------------------------------------------------------------------------------------------------- PQ
def pq_store(m, n, seed, zero=False):
    dim, cs = 8 * m, 8
    rng = np.random.default_rng(1000 * m + 10 * n + seed)
    cen = np.zeros((256, dim), dtype=np.float32) if zero else rng.standard_normal((256, dim)).astype(np.float32)
    return rng.integers(0, 256, size=(n, m), dtype=np.uint8), cen, dim, cs


def pq_open(rows, cen, dim, cs, dist, invert):
    return qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(dim, rows.shape[0], dist, invert), cs, cen)


def pq_oracle(rows, cen, dim, cs, dist, invert):
    n = rows.shape[0]
    return lambda i: np.array([qo.pq_score_internal(rows, dim, cs, cen, int(dist), invert, i, j) for j in range(n)], dtype=np.float32)


@pytest.mark.parametrize("n", [1000, 5000])
@pytest.mark.parametrize("m", [12, 16, 96, 160])
def test_pq_every_route(m, n):
    """m = 12 (row-per-lane form), 16 and 96 (quad kernel, one slice), 160 (planar image); 1000 and 5000 rows lie either
    side of the quad kernel's 4096.  33 rows: more than one LUT group at m = 160 (25 LUTs in 4 MiB)."""
    dist, invert = SETTINGS[(m + n // 1000) % len(SETTINGS)]
    rows, cen, dim, cs = pq_store(m, n, seed=1)
    enc = pq_open(rows, cen, dim, cs, dist, invert)
    master = master_rows(n, 33)
    master[4:] = master[4 + np.arange(29) % 3]  # 33 rows, 6 distinct: the oracle loop stays short
    check_batch(enc, n, pq_oracle(rows, cen, dim, cs, dist, invert), f"pq m={m} {dist.name} invert={invert}", (1, 3, 33), master)


@pytest.mark.parametrize("n", [1000, 5000])
def test_pq_zero_centroids_inverted_score_minus_zero(n):
    """All chunk metrics are +0: the sum is +0 and `invert` negates it once, after the sum -> 0x80000000 for every pair."""
    rows, cen, dim, cs = pq_store(96, n, seed=2, zero=True)
    enc = pq_open(rows, cen, dim, cs, D.L2, True)
    got = enc.score_internal_all_batch(np.array([0, n - 1, 7], dtype=np.uint32))
    assert got.shape == (3, n) and np.all(bits(got) == 0x80000000)
    assert bits(qo.pq_score_internal(rows, dim, cs, cen, int(D.L2), True, 7, 0)) == 0x80000000


def test_pq_without_centroids_is_refused():
    L = _lib.lib()
    vp = qa.VectorParameters(0, 3, D.Dot, False).to_c()
    cen = np.zeros(4, dtype=np.float32)
    rows = np.zeros(4, dtype=np.uint8)
    h = C.c_void_p()
    assert L.qamd_pq_from_rows(rows.ctypes.data, _lib.MEM_HOST, C.byref(vp), 8, cen.ctypes.data, None, C.byref(h)) == _lib.OK
    try:
        out = np.full(8, SENTINEL, dtype=np.float32)
        r = np.zeros(2, dtype=np.uint32)
        assert L.qamd_pq_score_internal_ids_batch(h, r.ctypes.data, None, 2, None, 3, _lib.MEM_HOST, out.ctypes.data,
                                                  _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS
        assert b"centroids" in L.qamd_last_error()
        assert L.qamd_pq_score_internal_ids(h, 0, None, 3, _lib.MEM_HOST, out.ctypes.data, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS
        assert b"centroids" in L.qamd_last_error()
        assert np.all(out == SENTINEL)
    finally:
        L.qamd_pq_free(h)


# ------------------------------------------------------------------------------------------------- all three quantizers
def three_stores(n=1025):
    """One store of each kind with a multi form, and the scores of every row of a short list."""
    rows, _ = store_rows(768, n, seed=4)
    u8, _ = u8_open(rows, 768, D.L2, True)
    prows, cen, pdim, cs = pq_store(16, n, seed=6)
    return [("u8", u8), ("pq", pq_open(prows, cen, pdim, cs, D.L2, False)),
            ("bin", bin_open_rows(bin_random_rows(n, 1024, seed=5, kind=1), 1024, D.L1, False, 1))]


def raw_batch(enc, rows, offsets, ids, n_ids, lists_mem, out, out_mem, n_lists=None):
    ptr = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    n_lists = (0 if rows is None else len(rows)) if n_lists is None else n_lists
    return enc._fn("score_internal_ids_batch")(enc._h, ptr(rows), ptr(offsets), n_lists, ptr(ids), n_ids, lists_mem, ptr(out),
                                               out_mem, None)


def test_refusals_write_nothing():
    L = _lib.lib()
    n = 1025
    for kind, enc in three_stores(n):
        out = np.full(3 * (n + 1), SENTINEL, dtype=np.float32)
        rows = np.array([0, 5, n - 1], dtype=np.uint32)
        offsets = np.array([0, 1, 2, 3], dtype=np.uint32)
        H = _lib.MEM_HOST
        assert raw_batch(enc, rows, None, None, n + 1, H, out, H) == _lib.ERR_OUT_OF_RANGE, kind  # n_ids > count
        assert raw_batch(enc, rows, offsets, None, 3, H, out, H) == _lib.ERR_ARGUMENTS, kind  # the caller forgot the ids
        assert b"list_offsets" in L.qamd_last_error()
        assert raw_batch(enc, None, None, None, 3, H, out, H, n_lists=3) == _lib.ERR_ARGUMENTS, kind  # NULL rows
        assert raw_batch(enc, rows, None, None, 3, H, None, H) == _lib.ERR_ARGUMENTS, kind  # NULL out
        bad = np.array([0, n, 5], dtype=np.uint32)
        assert raw_batch(enc, bad, None, None, n, H, out, H) == _lib.ERR_OUT_OF_RANGE, kind  # a host row >= count
        assert raw_batch(enc, rows, None, None, 0, H, out, H) == _lib.OK, kind  # n_ids == 0
        assert raw_batch(enc, rows, None, None, n, H, out, H, n_lists=0) == _lib.OK, kind  # n_lists == 0
        one = enc._fn("score_internal_ids")
        assert one(enc._h, 0, None, n + 1, H, out.ctypes.data, H, None) == _lib.ERR_OUT_OF_RANGE, kind
        assert one(enc._h, n, None, 3, H, out.ctypes.data, H, None) == _lib.ERR_OUT_OF_RANGE, kind
        assert one(enc._h, 0, None, 0, H, out.ctypes.data, H, None) == _lib.OK, kind
        assert one(enc._h, 0, None, 3, H, None, H, None) == _lib.ERR_ARGUMENTS, kind
        assert np.all(out == SENTINEL), kind
        # a given list behaves as before: NULL ids with offsets was and is refused, a real burst still works
        ids = np.array([1, 2, 3], dtype=np.uint32)
        assert raw_batch(enc, rows, offsets, ids, 3, H, out, H) == _lib.OK, kind
        want = [enc.score_internal(int(r), int(j)) for r, j in zip(rows, ids)]
        assert_bits_equal(out[:3], np.array(want, dtype=np.float32), f"{kind}: list form")


def test_device_rows_and_outputs():
    """Device rows need a device output and only enqueue; a device row >= count turns its own list into NaN and leaves
    its neighbours bit-exact; host rows with a device output and the host output agree."""
    torch = pytest.importorskip("torch")
    n = 1025
    for kind, enc in three_stores(n):
        rows = np.array([3, n - 1, 3, 77, 500, 9, 1024, 0, 12], dtype=np.uint32)
        want = enc.score_internal_all_batch(rows)  # host rows, host output
        for l, i in enumerate(rows):
            assert_bits_equal(want[l], enc.score_internal_all(int(i)), f"{kind} l={l}")
        out = torch.full((len(rows) * n,), float(SENTINEL), dtype=torch.float32, device="cuda")
        enc.score_internal_all_batch(rows, out=out)  # host rows, device output
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy().reshape(len(rows), n), want, f"{kind}: host rows, device output")
        drows = torch.from_numpy(rows.astype(np.int32)).cuda()
        out.fill_(float(SENTINEL))
        enc.score_internal_all_batch(drows, out=out)  # device rows, device output
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy().reshape(len(rows), n), want, f"{kind}: device rows")
        host = np.full(len(rows) * n, SENTINEL, dtype=np.float32)
        assert raw_batch(enc, drows, None, None, n, _lib.MEM_DEVICE, host, _lib.MEM_HOST, n_lists=len(rows)) == _lib.ERR_ARGUMENTS
        assert np.all(host == SENTINEL), kind
        # rows that cannot be validated: lists 1 and 5 (one in a pass of several rows, one more), a prefix
        bad = rows.copy()
        bad[1], bad[5] = n, 0xFFFFFFFF
        dbad = torch.from_numpy(bad.view(np.int32).copy()).cuda()
        p = n - 1
        out.fill_(float(SENTINEL))
        enc.score_internal_all_batch(dbad, n_rows=p, out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[len(rows) * p:] == SENTINEL), kind
        got = got[:len(rows) * p].reshape(len(rows), p)
        for l in range(len(rows)):
            if l in (1, 5):
                assert np.isnan(got[l]).all(), f"{kind}: list {l} of a row out of range"
            else:
                assert_bits_equal(got[l], want[l][:p], f"{kind}: list {l} beside a row out of range")
        # the single-row null list with a device output
        one = torch.empty(p, dtype=torch.float32, device="cuda")
        enc.score_internal_ids(77, None, out=one, n_rows=p)
        torch.cuda.synchronize()
        assert_bits_equal(one.cpu().numpy(), want[3][:p], f"{kind}: single-row null list, device output")


def test_scores_follow_append_and_upsert():
    """After append and upsert on a built store of each kind the batch covers the new count and sees the new codes."""
    rng = np.random.default_rng(17)
    dim, n0 = 128, 1000
    data = rng.random((n0 + 40, dim), dtype=np.float32)
    cen = rng.standard_normal((256, dim)).astype(np.float32)
    vp = qa.VectorParameters(dim, n0, D.Dot, False)
    stores = {"u8": (qa.EncodedVectorsU8.encode(data[:n0], vp), 0.0), "pq": (qa.EncodedVectorsPQ.encode(data[:n0], vp, 8, centroids=cen), 0.0),
              "bin": (qa.EncodedVectorsBin.encode(data[:n0] - 0.5, vp), 0.5)}
    rows = np.array([500, 999, 3, 998, 500], dtype=np.uint32)
    before = {k: e.score_internal_all_batch(rows) for k, (e, _) in stores.items()}
    n = n0 + 38
    for kind, (e, shift) in stores.items():
        assert before[kind].shape == (5, n0)
        e.upsert(998, data[n0 + 37:n0 + 40] - shift)  # the last two rows and one more
        e.append(data[n0:n0 + 37] - shift)
        assert e.count == n
        now = np.array([500, n - 1, 3, 998, 1000], dtype=np.uint32)
        got = e.score_internal_all_batch(now)
        assert got.shape == (5, n)
        for l, i in enumerate(now):
            assert_bits_equal(got[l], e.score_internal_ids(int(i), np.arange(n, dtype=np.uint32)), f"{kind} after append / upsert, row {i}")
        assert_bits_equal(got[0][:998], before[kind][0][:998], f"{kind}: untouched rows")
        assert not np.array_equal(bits(got[3][:998]), bits(before[kind][3][:998])), kind  # row 998 was overwritten


def test_query_scans_are_unchanged_after_batch_calls():
    """score_all / topk with an encoded query still equal the oracle bit for bit in a process that has run the batch
    forms: the EPI_POINT instantiations of the multi-query scan included (score_batch)."""
    rng = np.random.default_rng(23)
    n, dim = 4099, 768
    some = np.array([7, 0, n - 1, 7, 100], dtype=np.uint32)
    rows, query = store_rows(dim, n, seed=2)
    _, meta = qo.u8_encode_with(np.zeros((1, dim), dtype=np.float32), int(D.Dot), False, float(U8_ALPHA), 0.0)
    meta.count = n
    md = {"actual_dim": int(meta.actual_dim), "alpha": np.float32(meta.alpha), "offset": np.float32(meta.offset),
          "multiplier": np.float32(meta.multiplier), "vector_parameters": qa.VectorParameters(dim, n, D.Dot, False)}
    enc = qa.EncodedVectorsU8.from_storage(rows, md)
    enc.score_internal_all_batch(some)
    codes, qoff = qo.u8_encode_query(meta, query)
    want = qo.u8_score_all(meta, rows, codes, qoff)
    q = enc.encode_query(query)
    assert_bits_equal(enc.score_all(q), want, "u8 score_all")
    batch = enc.encode_query_batch(np.stack([query] * 3))
    sb = enc.score_batch(batch)
    for j in range(3):
        assert_bits_equal(sb[j], want, f"u8 score_batch query {j}")
    ids, sc = enc.topk(q, 65)
    wi, ws = topk_total_order(want, 65)
    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), "u8 topk"
    # binary
    brows = bin_random_rows(n, 1024, seed=3)
    benc = bin_open_rows(brows, 1024, D.Dot, False)
    benc.score_internal_all_batch(some)
    bq = np.where(rng.random(1024) < 0.5, -1.0, 1.0).astype(np.float32)
    want = qo.bin_score_all(brows, qo.bin_encode(bq[None, :])[0], 1024, qo.DOT, False)
    bqe = benc.encode_query(bq)
    assert_bits_equal(benc.score_all(bqe), want, "binary score_all")
    bb = benc.score_batch(benc.encode_query_batch(np.stack([bq] * 8)))
    assert_bits_equal(bb[7], want, "binary score_batch")
    ids, sc = benc.topk(bqe, 30)
    wi, ws = topk_total_order(want, 30)
    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), "binary topk"
    # PQ
    prows, cen, pdim, cs = pq_store(96, 4133, seed=5)
    penc = pq_open(prows, cen, pdim, cs, D.Dot, False)
    penc.score_internal_all_batch(some)
    pquery = rng.standard_normal(pdim).astype(np.float32)
    want = qo.pq_score_all(prows, qo.pq_encode_query(pquery, cs, cen, qo.DOT, False), order=qo.ORDER_SSE)
    pq = penc.encode_query(pquery)
    assert_bits_equal(penc.score_all(pq), want, "pq score_all")
    ids, sc = penc.topk(pq, 65)
    wi, ws = topk_total_order(want, 65)
    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), "pq topk"


# ------------------------------------------------------------------------------------------------- topk_internal_batch
TOPK_KS = (1, 10, 65, 1024)


def check_topk(enc, rows, what, ks=TOPK_KS):
    pytest.importorskip("torch")
    for k in ks:
        for largest in (True, False):
            ids, sc = enc.topk_internal_batch(rows, k, largest)
            assert ids.shape == (len(rows), k) and sc.shape == (len(rows), k)
            for l, i in enumerate(rows):
                wi, ws = enc.topk_internal(int(i), k, largest)
                tag = f"{what} l={l} row={i} k={k} largest={largest}"
                assert np.array_equal(ids[l], wi), f"{tag}: ids {ids[l][:8]} want {wi[:8]}"
                assert_bits_equal(sc[l], ws, f"{tag}: scores")


def test_topk_internal_batch_equals_topk_internal():
    n = 4099
    rows = np.array([5, n - 1, 5, 0, 2048], dtype=np.uint32)
    for kind, enc in three_stores(n):
        check_topk(enc, rows, kind)


def test_topk_internal_batch_ties_and_padding():
    """A binary store of 64-bit rows, many of them equal: scores tie heavily and go to the lower id.  A store of 40 rows
    with k up to 1024: the padding of a short list."""
    torch = pytest.importorskip("torch")
    n = 4099
    brows = bin_random_rows(n, 64, seed=8)
    brows[::3] = brows[0]
    enc = bin_open_rows(brows, 64, D.Dot, False)
    check_topk(enc, np.array([0, 3, 1, n - 1], dtype=np.uint32), "binary ties")
    ids, _ = enc.topk_internal_batch(np.array([3], dtype=np.uint32), 10)
    assert np.array_equal(ids[0], np.arange(0, 30, 3))  # the equal rows are the best, lowest ids first
    small, _ = u8_open(store_rows(128, 40, seed=1)[0], 128, D.Dot, False)
    check_topk(small, np.array([39, 0, 7], dtype=np.uint32), "u8 k > count", ks=(10, 65, 1024))
    ids, sc = small.topk_internal_batch(np.array([7], dtype=np.uint32), 65)
    assert np.all(ids[0, 40:] == 0xFFFFFFFF) and np.all(np.isneginf(sc[0, 40:]))
    # device outputs
    oi = torch.empty((3, 10), dtype=torch.int32, device="cuda")
    os_ = torch.empty((3, 10), dtype=torch.float32, device="cuda")
    rows = np.array([1, n - 1, 3], dtype=np.uint32)
    enc.topk_internal_batch(rows, 10, False, out_ids=oi, out_scores=os_)
    torch.cuda.synchronize()
    wi, ws = enc.topk_internal_batch(rows, 10, False)
    assert np.array_equal(oi.cpu().numpy().view(np.uint32), wi)
    assert_bits_equal(os_.cpu().numpy(), ws, "device top-k scores")
