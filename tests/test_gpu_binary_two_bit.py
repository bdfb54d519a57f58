"""Two-bit binary rows on the GPU, every comparison on raw bits: the statistics pass, the threshold
encoder for rows, queries and batches, the streaming encoder, every scoring entry point and batch route, save / load.

Two oracles: the numpy model (two_bit_model.py), and a one-bit handle made by qamd_bin_from_rows from the same bytes with
dim = 2 dim - the row sizes coincide, so every score must equal on code the one-bit tests already pin."""
import ctypes as C
import os

import numpy as np
import pytest

import two_bit_model as m
from util import assert_bits_equal, topk_want

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

E = qa.EncodedVectorsBin
D = qa.DistanceType
S = qa.BitsStoreType
TWO = qa.BinaryEncoding.TwoBits
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(_u(got).ravel() != _u(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} want {want.ravel()[bad[0]]!r}"


# ------------------------------------------------------------------------------------------------------ statistics
def _stat_data(n, dim, seed):
    """Ordinary columns, and among them: NaN and +-inf entries, an all-NaN column, a constant column, +-1e30, denormals."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, dim)) * rng.uniform(0.3, 1.5, size=dim) + rng.normal(size=dim)).astype(np.float32)
    if n == 0:
        return x
    kinds = ["specials", "all_nan", "constant", "huge", "denormal"]
    for c in range(dim):
        kind = kinds[c % 7] if c % 7 < len(kinds) else "ordinary"
        if dim == 1:
            kind = kinds[seed % len(kinds)]
        if kind == "specials":
            x[rng.random(n) < 0.2, c] = np.nan
            x[rng.random(n) < 0.1, c] = np.inf
            x[rng.random(n) < 0.1, c] = -np.inf
        elif kind == "all_nan":
            x[:, c] = np.nan
        elif kind == "constant":
            x[:, c] = np.float32(0.1)
        elif kind == "huge":
            x[:, c] = np.where(rng.random(n) < 0.5, np.float32(1e30), np.float32(-1e30))
        elif kind == "denormal":
            x[:, c] = (rng.integers(-9, 10, size=n) * np.float32(1e-45)).astype(np.float32)
    return x


COUNTS = [0, 1, 4095, 4096, 4097, 2 * 4096 + 37]
STAT_DIMS = [1, 3, 4, 65, 100, 768]


@pytest.mark.parametrize("dim", STAT_DIMS)
def test_statistics_and_thresholds(dim):
    import torch
    for k, n in enumerate(COUNTS):
        x = _stat_data(n, dim, 10 + k)
        want = m.stats(x)
        got = E.find_stats(x)
        for g, w, what in zip(got, want, ("n", "sum", "sumsq")):
            _same(g, w, f"host {what} {n}x{dim}")
        if n:
            dev = torch.from_numpy(x).cuda()
            for g, w, what in zip(E.find_stats(dev), want, ("n", "sum", "sumsq")):
                _same(g, w, f"device {what} {n}x{dim}")
            flat = torch.zeros(n * dim + 1, dtype=torch.float32, device="cuda")
            flat[1:] = dev.reshape(-1)
            off = flat[1:].view(n, dim)  # one float past a 16-byte boundary
            assert off.data_ptr() % 16 == 4
            for g, w, what in zip(E.find_stats(off), want, ("n", "sum", "sumsq")):
                _same(g, w, f"unaligned device {what} {n}x{dim}")
        wlo, whi = m.thresholds(*want)
        enc = E.encode(x, qa.VectorParameters(dim, n, D.Dot, False), encoding=TWO)
        assert enc.encoding == TWO
        lo, hi = enc.thresholds
        _same(lo, wlo, f"lo {n}x{dim}")
        _same(hi, whi, f"hi {n}x{dim}")
        _same(enc.storage_bytes(), m.encode(x, wlo, whi, m.U8), f"rows {n}x{dim}")


# ------------------------------------------------------------------------------------------------------------ rows
def _thresholds(dim, seed):
    rng = np.random.default_rng(seed)
    lo = rng.normal(size=dim).astype(np.float32)
    hi = (lo + rng.random(dim).astype(np.float32)).astype(np.float32)
    lo[::5] = 0.0  # +-0 sit exactly on a threshold
    hi[::7] = lo[::7]  # lo == hi is allowed: level 1 is then unreachable
    if dim > 3:
        lo[3], hi[3] = -0.0, 0.0
    return lo, np.maximum(lo, hi)


def _row_data(n, dim, lo, hi, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, dim)).astype(np.float32)
    inf = np.float32(np.inf)
    special = [lo, hi, np.nextafter(lo, -inf), np.nextafter(lo, inf), np.nextafter(hi, -inf), np.nextafter(hi, inf),
               np.zeros(dim, np.float32), -np.zeros(dim, np.float32), np.full(dim, np.nan, np.float32),
               np.full(dim, inf), np.full(dim, -inf)]
    for r, row in enumerate(special):
        x[r] = row
    pick = rng.integers(0, len(special), size=(n, dim))
    mask = rng.random((n, dim)) < 0.3
    mask[:len(special)] = False
    allv = np.stack(special)  # [kinds, dim]
    x[mask] = allv[pick, np.arange(dim)[None, :].repeat(n, 0)][mask]
    return x


ROW_DIMS = [1, 20, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 768, 1024, 2049]


@pytest.mark.parametrize("store", [S.U8, S.U128])
@pytest.mark.parametrize("dim", ROW_DIMS)
def test_rows(dim, store):
    n = 70
    lo, hi = _thresholds(dim, dim)
    x = _row_data(n, dim, lo, hi, dim + 1)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    enc = E.encode(x, vp, store=store, encoding=TWO, thresholds=(lo, hi))
    glo, ghi = enc.thresholds
    _same(glo, lo, "the caller's lo")
    _same(ghi, hi, "the caller's hi")
    want = m.encode(x, lo, hi, int(store))
    assert want.shape[1] == E.get_quantized_vector_size_from_params(vp, store, TWO)
    got = enc.storage_bytes()
    _same(got, want, f"rows dim {dim}")
    bits = np.unpackbits(got, axis=1, bitorder="little")
    assert not bits[:, 2 * dim:].any(), "pad bits"
    lv = m.levels(x, lo, hi)  # NaN and -inf are level 0, +inf level 2
    assert (lv[8] == 0).all() and (lv[10] == 0).all() and (lv[9] == 2).all()
    assert np.array_equal(bits[:, :dim] + bits[:, dim:2 * dim], lv)
    _same(enc.storage_rows(3, 11), want[3:14], "ranged export")
    import torch
    dev = E.encode(torch.from_numpy(x).cuda(), vp, store=store, encoding=TWO, thresholds=(lo, hi))
    _same(dev.storage_bytes(), want, f"rows from device data, dim {dim}")


# ------------------------------------------------------------------------------------------------------- streaming
def _stream(x, vp, observe, push, thresholds=None, store=S.U8):
    """begin_enc, observe batches of the given sizes, push batches of the given sizes, finish."""
    L = _lib.lib()
    c = vp.to_c()
    e = C.c_void_p()
    lo = hi = None
    if thresholds is not None:
        lo, hi = (C.c_void_p(t.ctypes.data) for t in thresholds)
    assert L.qamd_bin_encoder_begin_enc(C.byref(c), int(store), int(TWO), lo, hi, C.cast(None, _lib.STOP_FN), None, None,
                                        C.byref(e)) == _lib.OK
    try:
        for fn, sizes in ((L.qamd_bin_encoder_observe, observe), (L.qamd_bin_encoder_push, push)):
            r = 0
            for sz in sizes:
                part = np.ascontiguousarray(x[r:r + sz])
                st = fn(e, C.c_void_p(part.ctypes.data), part.shape[0], _lib.MEM_HOST)
                assert st == _lib.OK, (fn.__name__, r, sz, st, L.qamd_last_error())
                r += part.shape[0]
        out = C.c_void_p()
        h, e = e, None
        assert L.qamd_bin_encoder_finish(h, C.byref(out)) == _lib.OK
    finally:
        if e is not None:
            L.qamd_bin_encoder_abort(e)
    return E(out, vp, store, 0)


def _cuts(n, sizes):
    """Batch sizes that cut [0, n) after `sizes` rows each, cycling, until n rows are covered."""
    out, r, i = [], 0, 0
    while r < n:
        sz = min(sizes[i % len(sizes)], n - r)
        out.append(sz)
        r += sz
        i += 1
    return out


@pytest.fixture(scope="module")
def stream_case():
    n, dim = 2 * 4096 + 37, 20
    x = _stat_data(n, dim, 77)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    one_shot = E.encode(x, vp, encoding=TWO)
    return x, vp, one_shot.thresholds, one_shot.storage_bytes()


@pytest.mark.parametrize("observe,push", [
    ([1, 4094, 2, 1 << 20], [1 << 20]),       # blocks cut at rows 1, 4095 and 4097; everything pushed at once
    ([4095], [4097]),
    ([4097], [4095]),
    ([1 << 20], [1]),                          # one row per push
    ([1], [1 << 20]),                          # one row per observe: the open block is carried 4095 times
])
def test_streaming_is_the_one_shot_encode(stream_case, observe, push):
    x, vp, (wlo, whi), wrows = stream_case
    enc = _stream(x, vp, _cuts(vp.count, observe), _cuts(vp.count, push))
    lo, hi = enc.thresholds
    _same(lo, wlo, "lo")
    _same(hi, whi, "hi")
    _same(enc.storage_bytes(), wrows, "rows")
    _same(lo, m.thresholds(*m.stats(x))[0], "lo against the model")


def test_streaming_through_the_mirror_and_misuse(stream_case):
    x, vp, (wlo, whi), wrows = stream_case
    enc = E.encode_stream(lambda: (x[i:i + 3000] for i in range(0, vp.count, 3000)), vp, encoding=TWO)
    _same(enc.thresholds[0], wlo, "lo")
    _same(enc.storage_bytes(), wrows, "rows")
    given = E.encode_stream(lambda: (x[i:i + 5000] for i in range(0, vp.count, 5000)), vp, encoding=TWO, thresholds=(wlo, whi))
    _same(given.storage_bytes(), wrows, "rows with given thresholds")
    L = _lib.lib()
    c = vp.to_c()
    nul = C.cast(None, _lib.STOP_FN)
    part = np.ascontiguousarray(x[:100])
    p = C.c_void_p(part.ctypes.data)
    e = C.c_void_p()
    assert L.qamd_bin_encoder_begin_enc(C.byref(c), 0, int(TWO), None, None, nul, None, None, C.byref(e)) == _lib.OK
    assert L.qamd_bin_encoder_observe(e, p, 100, _lib.MEM_HOST) == _lib.OK
    assert L.qamd_bin_encoder_push(e, p, 100, _lib.MEM_HOST) == _lib.ERR_ARGUMENTS  # too few rows were observed
    L.qamd_bin_encoder_abort(e)
    small = qa.VectorParameters(vp.dim, 100, D.Dot, False).to_c()
    e = C.c_void_p()
    assert L.qamd_bin_encoder_begin_enc(C.byref(small), 0, int(TWO), None, None, nul, None, None, C.byref(e)) == _lib.OK
    assert L.qamd_bin_encoder_observe(e, p, 100, _lib.MEM_HOST) == _lib.OK
    assert L.qamd_bin_encoder_push(e, p, 50, _lib.MEM_HOST) == _lib.OK
    assert L.qamd_bin_encoder_observe(e, p, 1, _lib.MEM_HOST) == _lib.ERR_ARGUMENTS  # observe after a push
    L.qamd_bin_encoder_abort(e)
    for enc_kind, lo, hi in ((0, None, None), (int(TWO), C.c_void_p(wlo.ctypes.data), C.c_void_p(whi.ctypes.data))):
        e = C.c_void_p()  # nothing to learn: observe is accepted and does nothing, before or after a push
        assert L.qamd_bin_encoder_begin_enc(C.byref(small), 0, enc_kind, lo, hi, nul, None, None, C.byref(e)) == _lib.OK
        assert L.qamd_bin_encoder_observe(e, p, 100, _lib.MEM_HOST) == _lib.OK
        assert L.qamd_bin_encoder_push(e, p, 100, _lib.MEM_HOST) == _lib.OK
        assert L.qamd_bin_encoder_observe(e, p, 100, _lib.MEM_HOST) == _lib.OK
        out = C.c_void_p()
        assert L.qamd_bin_encoder_finish(e, C.byref(out)) == _lib.OK
        h = E(out, qa.VectorParameters(vp.dim, 100, D.Dot, False), S.U8, 0)
        if enc_kind:
            _same(h.storage_bytes(), wrows[:100], "rows")


# --------------------------------------------------------------------------------------------------------- queries
@pytest.mark.parametrize("store", [S.U8, S.U128])
@pytest.mark.parametrize("dim", [1, 20, 33, 64, 100, 768, 2049])
def test_queries(dim, store):
    n = 40
    lo, hi = _thresholds(dim, 3 * dim)
    x = _row_data(n, dim, lo, hi, 5 * dim)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    enc = E.encode(x, vp, store=store, encoding=TWO, thresholds=(lo, hi))
    rows = m.encode(x, lo, hi, int(store))
    batch = enc.encode_query_batch(x)
    reuse = None
    for r in (0, 1, 8, 9, 17, n - 1):
        reuse = q = enc.encode_query(x[r], reuse)
        _same(q.encoded_vector, rows[r], f"query {r}")
        _same(batch.encoded_vector(r), rows[r], f"batch query {r}")
        want = m.score_all(rows, rows[r], dim, m.DOT, False)
        assert_bits_equal(enc.score_all(q), want, "score_all")
        internal = np.array([enc.score_internal(r, j) for j in range(n)], dtype=np.float32)
        assert_bits_equal(internal, want, "the query of row r's vector scores as score_internal(r, .)")
    for bits in (4, 8):  # scalar queries against two-bit rows are refused
        with pytest.raises(qa.EncodingError):
            enc.encode_query(x[0], query_bits=bits)
        with pytest.raises(qa.EncodingError):
            enc.encode_query_batch(x[:3], query_bits=bits)
    with pytest.raises(qa.EncodingError):
        enc.encode_query(np.zeros(dim + 1, dtype=np.float32))


# --------------------------------------------------------------------------------------------------------- scoring
def _pair(dim, n, dist, invert, store, seed):
    """A two-bit store, its model rows, and the one-bit U128 / U8 handle over the same bytes with dim = 2 dim."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, dim)) * rng.uniform(0.3, 1.5, size=dim)).astype(np.float32)
    lo, hi = m.thresholds(*m.stats(x[:2000]))
    vp = qa.VectorParameters(dim, n, dist, invert)
    enc = E.encode(x, vp, store=store, encoding=TWO, thresholds=(lo, hi))
    rows = m.encode(x, lo, hi, int(store))
    ref = E.from_storage(rows, qa.VectorParameters(2 * dim, n, dist, invert), store)
    return x, lo, hi, enc, rows, ref


def _as_floats(row, bits):
    """A one-bit query's f32 form whose sign bits are `row`."""
    b = np.unpackbits(row, bitorder="little")[:bits]
    return np.where(b != 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32)


SHAPES = [  # dim, rows, store: what the shape reaches
    (8, 300, S.U8),         # 2-byte rows at the 4-byte device stride
    (20, 300, S.U8),        # 8-byte rows: dword kernels
    (100, 5000, S.U128),    # 32-byte rows: the scan, the single-launch top-k
    (512, 4200, S.U128),    # 128-byte rows: the multi-query scan, the int8 matrix cores
    (4100, 260, S.U128),    # 65 pieces: longer than the 16-byte-piece kernels take
]


@pytest.mark.parametrize("dim,n,store", SHAPES)
@pytest.mark.parametrize("dist,invert", [(D.Dot, False), (D.Dot, True), (D.L2, False), (D.L1, True)])
def test_every_entry_point(dim, n, store, dist, invert):
    x, lo, hi, enc, rows, ref = _pair(dim, n, dist, invert, store, dim)
    rng = np.random.default_rng(dim + 1)
    queries = (x[rng.integers(0, n, 14)] + 0.5 * rng.normal(size=(14, dim))).astype(np.float32)
    qrows = m.encode(queries, lo, hi, int(store))
    q = enc.encode_query(queries[0])
    rq = ref.encode_query(_as_floats(qrows[0], 2 * dim))
    want = m.score_all(rows, qrows[0], dim, int(dist), invert)
    assert_bits_equal(enc.score_all(q), want, "score_all against the model")
    assert_bits_equal(ref.score_all(rq), want, "the one-bit handle of 2 dim against the model")
    ids = rng.integers(0, n, 37).astype(np.uint32)
    assert_bits_equal(enc.score_ids(q, ids), want[ids], "score_ids")
    for i in (0, n // 2, n - 1):
        assert_bits_equal([enc.score_point(q, i)], [want[i]], "score_point")
        j = int(ids[i % 37])
        wi = m.score_all(rows[j:j + 1], rows[i], dim, int(dist), invert)
        assert_bits_equal([enc.score_internal(i, j)], wi, "score_internal")
        assert_bits_equal([enc.score_internal(i, j)], [ref.score_internal(i, j)], "score_internal against one bit")
    assert_bits_equal(enc.score_internal_ids(5, ids), m.score_all(rows[ids], rows[5], dim, int(dist), invert), "score_internal_ids")
    offs = np.array([0, 5, 5, 20, 37], dtype=np.uint32)
    lrows = np.array([3, 0, n - 1, 7], dtype=np.uint32)
    assert_bits_equal(enc.score_internal_ids_batch(lrows, offs, ids), ref.score_internal_ids_batch(lrows, offs, ids),
                      "score_internal_ids_batch")
    for largest in (True, False):
        for k in (1, 10):
            wid, wsc = topk_want(want, k, largest)
            gid, gsc = enc.topk(q, k, largest)
            assert np.array_equal(gid, wid), ("topk ids", k, largest)
            assert_bits_equal(gsc, wsc, "topk scores")
    orig = qa.OriginalVectors.from_data(x, qa.VectorParameters(dim, n, dist, invert))  # originals keep dim, not 2 dim
    cand, _ = enc.topk(q, 50, True)
    wid, wsc = orig.rerank(queries[0], cand, 10, True)
    gid, gsc = enc.topk_rescored(q, orig, queries[0], 10, 50, True)
    assert np.array_equal(gid, wid)
    assert_bits_equal(gsc, wsc, "topk_rescored")
    # batches of 2 .. 8 and of 12 and more
    for nq in (2, 3, 8, 14):
        b = enc.encode_query_batch(queries[:nq])
        rb = ref.encode_query_batch(np.stack([_as_floats(r, 2 * dim) for r in qrows[:nq]]))
        assert enc.batch_kernel(b, 0) == ref.batch_kernel(rb, 0) and enc.batch_kernel(b, 10) == ref.batch_kernel(rb, 10)
        wantb = np.stack([m.score_all(rows, qrows[i], dim, int(dist), invert) for i in range(nq)])
        assert_bits_equal(enc.score_batch(b), wantb, f"score_batch of {nq}")
        gid, gsc = enc.topk_batch(b, 10, True)
        for i in range(nq):
            wid, wsc = topk_want(wantb[i], 10, True)
            assert np.array_equal(gid[i], wid), ("topk_batch ids", nq, i)
            assert_bits_equal(gsc[i], wsc, "topk_batch scores")
        boffs = np.array([0, 17, 37] + [37] * (nq - 2), dtype=np.uint32)
        wl = np.concatenate([wantb[0][ids[:17]], wantb[1][ids[17:]]])
        assert_bits_equal(enc.score_ids_batch(b, boffs, ids), wl, "score_ids_batch")


def _topk_batch_case(dim, n, nq, store=S.U128, k=10, seed=1):
    x, lo, hi, enc, rows, ref = _pair(dim, n, D.Dot, False, store, seed)
    rng = np.random.default_rng(seed + 1)
    queries = (x[rng.integers(0, n, nq)] + 0.5 * rng.normal(size=(nq, dim))).astype(np.float32)
    qrows = m.encode(queries, lo, hi, int(store))
    b = enc.encode_query_batch(queries)
    rb = ref.encode_query_batch(np.stack([_as_floats(r, 2 * dim) for r in qrows]))
    names = enc.batch_kernel(b, 0), enc.batch_kernel(b, k)
    assert names == (ref.batch_kernel(rb, 0), ref.batch_kernel(rb, k)), "a two-bit store routes as the one-bit store of 2 dim"
    for largest in (True, False):
        gid, gsc = enc.topk_batch(b, k, largest)
        rid, rsc = ref.topk_batch(rb, k, largest)
        assert np.array_equal(gid, rid)
        assert_bits_equal(gsc, rsc, "topk_batch against the one-bit handle")
        for i in (0, nq // 2, nq - 1):
            want = m.score_all(rows, qrows[i], dim, m.DOT, False)
            wid, wsc = topk_want(want, k, largest)
            assert np.array_equal(gid[i], wid), (names, i, largest)
            assert_bits_equal(gsc[i], wsc, "topk_batch against the model")
    return enc, b, rows, qrows, names


def test_fused_and_matrix_topk_at_dim_64():
    """32768 rows of dim 64 (16-byte rows): the fused single-query top-k and, from 12 queries, the int8 matrix-core filter."""
    n = 32768
    enc, b, rows, qrows, names = _topk_batch_case(64, n, 12)
    assert names[1] == "bin_gemm_rs_kernel"
    q = enc.encode_query(np.zeros(64, dtype=np.float32))
    want = m.score_all(rows, m.encode(np.zeros((1, 64), np.float32), *enc.thresholds, m.U128)[0], 64, m.DOT, False)
    for k in (30, 200):  # the single-launch top-k takes k <= 64; beyond, the fused pipeline
        wid, wsc = topk_want(want, k, True)
        gid, gsc = enc.topk(q, k, True)
        assert np.array_equal(gid, wid)
        assert_bits_equal(gsc, wsc, "topk")


@pytest.mark.parametrize("dim,nq,kernel", [(d, q, "bin_gemm_rs4_kernel") for d in (256, 384, 512, 768) for q in (5, 130)]
                         + [(768, 800, "bin_gemm_qs4_kernel")])
def test_fp4_forms(dim, nq, kernel):
    """Rows of 512, 768, 1024 and 1536 bits: the row-streaming FP4 filter while the batch's nibble image fits LDS in at
    most four passes (192 queries per pass at 1536 bits), the query-streaming one beyond."""
    enc, b, rows, qrows, names = _topk_batch_case(dim, 32768, nq, seed=dim + nq)
    assert names[1] == kernel, names


@pytest.mark.parametrize("dim,inside", [(2496, True), (2560, False)])
def test_matrix_gate(dim, inside):
    """4992-bit rows are the longest the matrix cores take; 5120-bit rows go to the scans."""
    n = 4200
    x, lo, hi, enc, rows, ref = _pair(dim, n, D.Dot, False, S.U128, dim)
    b = enc.encode_query_batch(x[:12])
    name = enc.batch_kernel(b, 0)
    assert (name == "bin_gemm_rs_kernel") == inside, name
    want = np.stack([m.score_all(rows, rows[i], dim, m.DOT, False) for i in range(12)])
    assert_bits_equal(enc.score_batch(b), want, "score_batch")


@pytest.fixture(scope="module")
def routes_taken():
    """Kernel names qamd_bin_batch_kernel gives for two-bit batches that were then scored: (kernel of score_batch, kernel
    of topk_batch(10)) per case, every result bit-equal to the one-bit handle of 2 dim over the same bytes."""
    taken = set()
    cases = [(20, 300, S.U8, 14), (100, 5000, S.U128, 3), (512, 4200, S.U128, 3), (512, 4200, S.U128, 14),
             (256, 32768, S.U128, 5), (768, 32768, S.U128, 800)]
    for dim, n, store, nq in cases:
        x, lo, hi, enc, rows, ref = _pair(dim, n, D.Dot, False, store, dim + nq)
        queries = x[:nq] if nq <= n else np.tile(x, (nq // n + 1, 1))[:nq]
        qrows = m.encode(queries, lo, hi, int(store))
        b = enc.encode_query_batch(queries)
        rb = ref.encode_query_batch(np.stack([_as_floats(r, 2 * dim) for r in qrows]))
        assert_bits_equal(enc.score_batch(b), ref.score_batch(rb), "score_batch")
        gid, gsc = enc.topk_batch(b, 10, True)
        rid, rsc = ref.topk_batch(rb, 10, True)
        assert np.array_equal(gid, rid)
        assert_bits_equal(gsc, rsc, "topk_batch")
        taken.update((enc.batch_kernel(b, 0), enc.batch_kernel(b, 10)))
    return taken


def test_every_batch_kernel_was_taken(routes_taken):
    """Every kernel name qamd_bin_batch_kernel can return is taken by a two-bit batch.  bin_words_kernel has no batch form:
    a batch of 12 or more queries reaches it only query by query, on rows that are not whole 16-byte pieces or longer than
    64 of them (here: 14 queries on 8-byte rows)."""
    names = {"bin_gemm_rs_kernel", "bin_gemm_rs4_kernel", "bin_gemm_qs4_kernel", "bin_scan_multi_kernel", "bin_scan_kernel",
             "bin_words_kernel", "bin_topk_small_kernel"}
    assert names - routes_taken == set(), f"batch kernels no two-bit batch took: {sorted(names - routes_taken)}"


# --------------------------------------------------------------------------------------------------- save and load
def test_save_and_load(tmp_path):
    dim, n = 100, 300
    x, lo, hi, enc, rows, ref = _pair(dim, n, D.L2, True, S.U128, 9)
    enc.save(tmp_path / "two.bin", tmp_path / "two.json")
    vp = qa.VectorParameters(dim, n, D.Dot, False)  # the file rules the metric
    back = E.load(tmp_path / "two.bin", tmp_path / "two.json", vp, S.U128)
    assert back.encoding == TWO and back.vector_parameters.distance_type == D.L2 and back.vector_parameters.invert
    _same(back.thresholds[0], lo, "lo")
    _same(back.thresholds[1], hi, "hi")
    _same(back.storage_bytes(), rows, "rows")
    assert (tmp_path / "two.bin").read_bytes() == rows.tobytes()
    q, bq = enc.encode_query(x[7]), back.encode_query(x[7])
    _same(bq.encoded_vector, q.encoded_vector, "query")
    assert_bits_equal(back.score_all(bq), enc.score_all(q), "scores")
    assert back.metadata["encoding"] == TWO and "encoding" not in ref.metadata
    # a one-bit save beside it is the committed fixture's format, byte for byte
    fixture = open(os.path.join(ROOT, "tests", "golden", "meta_bin.json"), "rb").read()
    import json
    fv = json.loads(fixture)["vector_parameters"]
    fvp = qa.VectorParameters(fv["dim"], 5, D[fv["distance_type"]], bool(fv["invert"]))
    one = E.encode(np.ones((5, fv["dim"]), dtype=np.float32), fvp)
    one.save(tmp_path / "one.bin", tmp_path / "one.json")
    saved = (tmp_path / "one.json").read_bytes()
    assert saved == fixture.replace(f'"count":{fv["count"]}'.encode(), b'"count":5')
    assert E.load(tmp_path / "one.bin", tmp_path / "one.json", fvp).encoding == qa.BinaryEncoding.OneBit
