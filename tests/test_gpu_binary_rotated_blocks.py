"""Block-rotated binary rows on the GPU, every comparison on raw bits against the numpy model
(rotated_blocks_model.py composed with the models of the plain encodings): the rows, the thresholds, the query codes, and
the scores of every route by the plain store's rule on the model's bytes.

The dims are the smallest at which each path of the two rotation kernels can go wrong: every K = ceil(dim / 256) of the
wave-per-row form, idle lanes in the last chunk, each stage at which the network may stop, and the workgroup-per-row form
with a chunk count that is no multiple of the workgroup."""
import json

import numpy as np
import pytest

import rotated_blocks_model as bm
import rotated_model as rm
import two_bit_model as m
import two_bit_scalar_model as sm
from util import assert_bits_equal, scalar_codes, scalar_planes, scalar_scores, topk_want

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")

E = qa.EncodedVectorsBin
D = qa.DistanceType
S = qa.BitsStoreType
B = qa.BinaryEncoding
ONE_B, TWO_B = B.OneBitRotatedBlocks, B.TwoBitsRotatedBlocks
f32 = np.float32

# dim: blocks, what it exercises
ROW_DIMS = [
    64,     # B = dim: the ROTATED rows
    192,    # 3 x 64: idle lanes in the only chunk, stop after lane stage 8
    320,    # 5 x 64: K = 2, half-empty last chunk
    384,    # 3 x 128: stop after lane stage 16
    768,    # 3 x 256: K = 3, no chunk stage
    832,    # 13 x 64: K = 4, whose chunk stages 1 and 2 are present but not taken
    1280,   # 5 x 256: K = 5
    1536,   # 3 x 512: K = 6, one chunk stage
    1792,   # 7 x 256: K = 7
    1984,   # 31 x 64: K = 8, idle lanes, no chunk stage taken
    2048,   # B = dim: the ROTATED rows
    2112,   # 33 x 64: workgroup per row, 528 chunks
    3072,   # 3 x 1024: workgroup per row, stages in LDS
    12288,  # 3 x 4096: workgroup per row
    16384,  # B = dim: the ROTATED rows, workgroup per row
]


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(_u(got).ravel() != _u(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} want {want.ravel()[bad[0]]!r}"


def _data(n, dim, seed):
    """Columns of unequal scale and a mean; planted: an all-zero row, rows with a NaN, +inf, -inf, a row of subnormals."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, dim)) * rng.uniform(0.3, 1.5, size=dim) + 0.2 * rng.normal(size=dim)).astype(f32)
    if n >= 8:
        x[0] = 0.0
        x[1, rng.integers(dim)] = np.nan
        x[2, rng.integers(dim)] = np.inf
        x[3, rng.integers(dim)] = -np.inf
        x[4] = (rng.integers(-9, 10, size=dim) * f32(1e-45)).astype(f32)
        x[5, ::3] = -0.0
    return x


def _dist(dim):
    return [D.Dot, D.L1, D.L2][(dim // 64) % 3], bool((dim // 64) % 2)


def _model_rows(x, enc, store, thresholds=None):
    """(rows u8, thresholds or None) of the model: a plain store of dim dimensions over y."""
    y = bm.rotate(x)
    dim = y.shape[1]
    if enc == ONE_B:
        return rm.one_bit_rows(y, m.row_bytes(dim, int(store))), None
    lo, hi = thresholds if thresholds is not None else m.thresholds(*m.stats(y), 0.43)
    return m.encode(y, lo, hi, int(store)), (lo, hi)


def _query_rows(queries, enc, thr, store, nb):
    yq = bm.rotate(queries)
    if enc == ONE_B:
        return rm.one_bit_rows(yq, nb)
    return m.encode(yq, thr[0], thr[1], int(store))


def _metric(xor, code_bits, dist, invert):
    xor = np.asarray(xor).astype(f32)
    zeros = (f32(code_bits) - xor).astype(f32)
    return ((zeros - xor) if (dist == D.Dot) != bool(invert) else (xor - zeros)).astype(f32)


def _check_store(h, enc, want, thr, dim, store):
    assert h.encoding == enc
    assert h.code_bits == (2 * dim if enc == TWO_B else dim)
    assert want.shape[1] == E.get_quantized_vector_size_from_params(h.vector_parameters, store, enc)
    if thr is None:
        assert h.thresholds is None
    else:
        lo, hi = h.thresholds
        assert lo.size == dim and hi.size == dim
        _same(lo, thr[0], "lo")
        _same(hi, thr[1], "hi")
    _same(h.storage_bytes(), want, "rows")


# ------------------------------------------------------------------------------------------------ rows and routes
@pytest.mark.parametrize("enc", [ONE_B, TWO_B])
@pytest.mark.parametrize("store", [S.U8, S.U128])
@pytest.mark.parametrize("dim", ROW_DIMS)
def test_rows_and_routes(dim, store, enc):
    import torch
    n = 200
    dist, invert = _dist(dim)
    x = _data(n, dim, dim)
    vp = qa.VectorParameters(dim, n, dist, invert)
    want, thr = _model_rows(x, enc, store)
    blk = E.encode(x, vp, store=store, encoding=enc)
    _check_store(blk, enc, want, thr, dim, store)
    if enc == ONE_B:
        assert not want[0].any(), "an all-zero row has no bit set"
    assert not np.unpackbits(blk.storage_bytes(), axis=1, bitorder="little")[:, blk.code_bits:].any(), "pad bits"
    # the plain store's size: a row keeps dim (or 2 dim) bits
    assert want.shape[1] == E.get_quantized_vector_size_from_params(vp, store, B.TwoBits if enc == TWO_B else B.OneBit)
    # device data: aligned (16-byte loads) and one float past a 16-byte boundary (guarded dword loads)
    flat = torch.zeros(n * dim + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(x).cuda().reshape(-1)
    off = flat[1:].view(n, dim)
    assert off.data_ptr() % 16 == 4
    for src in (torch.from_numpy(x).cuda(), off):
        _same(E.encode(src, vp, store=store, encoding=enc, thresholds=thr).storage_bytes(), want, "rows from device data")
    if dim & (dim - 1) == 0:  # B = dim: byte-identical to the ROTATED encodings, only the reported value differs
        rot = E.encode(x, vp, store=store, encoding=B.OneBitRotated if enc == ONE_B else B.TwoBitsRotated)
        assert rot.encoding != blk.encoding and rot.code_bits == blk.code_bits
        _same(blk.storage_bytes(), rot.storage_bytes(), "rows against a ROTATED handle")
        if thr is not None:
            _same(blk.thresholds[0], rot.thresholds[0], "lo against a ROTATED handle")
            _same(blk.thresholds[1], rot.thresholds[1], "hi against a ROTATED handle")
        _same(blk.encode_query(x[7]).encoded_vector, rot.encode_query(x[7]).encoded_vector, "query against a ROTATED handle")

    rng = np.random.default_rng(dim + 5)
    queries = (x[[7, 9, 11, 13, 15]] + 0.5 * rng.normal(size=(5, dim))).astype(f32)
    qrows = _query_rows(queries, enc, thr, store, want.shape[1])
    model = np.stack([_metric(m.xor_count(want, r), blk.code_bits, dist, invert) for r in qrows])
    q = blk.encode_query(queries[0])
    _same(q.encoded_vector, qrows[0], "query bits against the model")
    assert_bits_equal(blk.score_all(q), model[0], "score_all")
    assert_bits_equal(blk.score_internal_all(9), _metric(m.xor_count(want, want[9]), blk.code_bits, dist, invert),
                      "score_internal_all")
    batch = blk.encode_query_batch(queries)
    for i in range(5):
        _same(batch.encoded_vector(i), qrows[i], f"batch query {i}")
    assert_bits_equal(blk.score_batch(batch), model, "score_batch")
    for largest in (True, False):
        for k in (1, 10):
            ids, sc = blk.topk(q, k, largest)
            wid, wsc = topk_want(model[0], k, largest)
            assert np.array_equal(ids, wid), ("topk ids", k, largest)
            assert_bits_equal(sc, wsc, "topk scores")
            bids, bsc = blk.topk_batch(batch, k, largest)
            for i in range(5):
                wid, wsc = topk_want(model[i], k, largest)
                assert np.array_equal(np.asarray(bids).reshape(5, k)[i], wid), ("topk_batch ids", i, k, largest)
                assert_bits_equal(np.asarray(bsc).reshape(5, k)[i], wsc, "topk_batch scores")
    with pytest.raises(qa.EncodingError):
        blk.encode_query(np.zeros(dim + 64, dtype=f32))
    with pytest.raises(qa.EncodingError):
        blk.encode_query_batch(np.zeros((2, dim + 64), dtype=f32))


@pytest.mark.parametrize("dim", [192, 2112])
def test_thresholds_learnt_across_a_statistics_block_edge(dim):
    n = 4097
    x = _data(n, dim, 4097 + dim)
    want, thr = _model_rows(x, TWO_B, S.U8)
    blk = E.encode(x, qa.VectorParameters(dim, n, D.Dot, False), encoding=TWO_B)
    _check_store(blk, TWO_B, want, thr, dim, S.U8)


# --------------------------------------------------------------------------------------------------------- queries
def _scalar_want(enc, yq, thr, dim, bits, store, rows, dist, invert):
    """(planes u8 [bits, nb], max_abs, scores f32 [n]) of the models for one rotated query yq [dim]."""
    if enc == ONE_B:
        codes, a = scalar_codes(yq, bits)
        return scalar_planes(codes, bits, rows.shape[1]), a, scalar_scores(rows, codes, dim, bits, dist, invert)
    codes, a = sm.weighted_codes(yq, thr[0], thr[1], bits)
    planes = sm.planes(codes, dim, bits, int(store))
    return planes, a, sm.metric(sm.xor_from_planes(rows, planes), dim, bits, int(dist), invert)


@pytest.mark.parametrize("enc", [ONE_B, TWO_B])
@pytest.mark.parametrize("dim", [192, 768, 1536, 3072])
def test_queries(dim, enc):
    n, store = 64, S.U8
    dist, invert = _dist(dim + 64)
    x = _data(n, dim, dim + 11)
    vp = qa.VectorParameters(dim, n, dist, invert)
    rows, thr = _model_rows(x, enc, store)
    blk = E.encode(x, vp, store=store, encoding=enc)
    rng = np.random.default_rng(dim)
    queries = (x[rng.integers(0, n, size=33)] + 0.5 * rng.normal(size=(33, dim))).astype(f32)
    queries[1, dim // 2] = np.nan
    queries[2, 0] = np.inf
    yqs = bm.rotate(queries)
    weighted = enc == TWO_B
    # one bit per query dimension: single and batches of 3 and 33
    qrows = _query_rows(queries, enc, thr, store, rows.shape[1])
    want1 = np.stack([_metric(m.xor_count(rows, r), blk.code_bits, dist, invert) for r in qrows])
    for nq in (3, 33):
        b = blk.encode_query_batch(queries[:nq])
        assert b.bits == 1
        for i in range(nq):
            _same(b.encoded_vector(i), qrows[i], f"batch of {nq}, query {i}")
        assert_bits_equal(blk.score_batch(b), want1[:nq], f"score_batch of {nq}")
    _same(blk.encode_query(queries[4]).encoded_vector, qrows[4], "single query")
    # 4 and 8 bits: unweighted on one-bit rows, weighted on two-bit rows
    n_model = 5  # (the plane oracle sets one bit at a time)
    for bits in (4, 8):
        wants = [_scalar_want(enc, yqs[i], thr, dim, bits, store, rows, dist, invert) for i in range(n_model)]
        for i in (0, 1, 2):
            q = blk.encode_query(queries[i], query_bits=bits, weighted=weighted)
            assert q.bits == bits
            _same(q.encoded_vector, wants[i][0], f"{bits}-bit planes, query {i}")
            _same(q.max_abs, wants[i][1], "max_abs")
            assert_bits_equal(blk.score_all(q), wants[i][2], f"{bits}-bit score_all, query {i}")
        for nq in (3, 33):
            b = blk.encode_query_batch(queries[:nq], query_bits=bits, weighted=weighted)
            assert b.bits == bits
            got = blk.score_batch(b)
            for i in range(min(nq, n_model)):
                _same(b.encoded_vector(i), wants[i][0], f"{bits}-bit batch of {nq}, query {i}")
                assert_bits_equal(got[i], wants[i][2], f"{bits}-bit score_batch of {nq}, query {i}")
        if enc == ONE_B:  # on one-bit rows the weighted call is the unweighted one
            _same(blk.encode_query(queries[0], query_bits=bits, weighted=True).encoded_vector, wants[0][0], "weighted = unweighted")
        else:  # the existing refusal keeps its shape
            with pytest.raises(qa.EncodingError):
                blk.encode_query(queries[0], query_bits=bits)
            with pytest.raises(qa.EncodingError):
                blk.encode_query_batch(queries[:3], query_bits=bits)
        with pytest.raises(qa.EncodingError):
            blk.encode_query(np.zeros(dim + 64, dtype=f32), query_bits=bits, weighted=weighted)


# ------------------------------------------------------------------------------------- streaming, upsert, save / load
@pytest.mark.parametrize("enc", [ONE_B, TWO_B])
def test_streaming_with_uneven_batches(enc):
    n, dim = 4098, 320
    x = _data(n, dim, 31)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    one_shot = E.encode(x, vp, encoding=enc)

    def batches():
        r = 0
        for sz in (1, 4095, 2):
            yield x[r:r + sz]
            r += sz
    streamed = E.encode_stream(batches, vp, encoding=enc)
    assert streamed.encoding == enc and streamed.code_bits == one_shot.code_bits
    _same(streamed.storage_bytes(), one_shot.storage_bytes(), "streamed rows")
    if enc == TWO_B:
        for g, w in zip(streamed.thresholds, one_shot.thresholds):
            _same(g, w, "streamed thresholds")
    want, thr = _model_rows(x, enc, S.U8)
    _check_store(streamed, enc, want, thr, dim, S.U8)


@pytest.mark.parametrize("enc", [ONE_B, TWO_B])
@pytest.mark.parametrize("dim", [192, 768, 2112])
def test_upsert_and_append(dim, enc):
    x = _data(50, dim, dim + 3)
    h = E.encode(x[:30], qa.VectorParameters(dim, 30, D.Dot, False), encoding=enc)
    thr = h.thresholds
    h.reserve(64)
    h.append(x[30:40])
    h.upsert(5, x[40:50])
    now = np.concatenate([x[:5], x[40:50], x[15:40]])
    fresh = E.encode(now, qa.VectorParameters(dim, 40, D.Dot, False), encoding=enc, thresholds=thr)
    _same(h.storage_bytes(), fresh.storage_bytes(), "rows after append and upsert")
    want, _ = _model_rows(now, enc, S.U8, thr)
    _same(h.storage_bytes(), want, "rows after append and upsert, against the model")


@pytest.mark.parametrize("store", [S.U8, S.U128])
@pytest.mark.parametrize("enc", [ONE_B, TWO_B])
def test_save_load_round_trip(tmp_path, enc, store):
    n, dim = 40, 192
    x = _data(n, dim, 8)
    vp = qa.VectorParameters(dim, n, D.L2, True)
    blk = E.encode(x, vp, store=store, encoding=enc)
    data, meta = tmp_path / "rows.bin", tmp_path / "meta.json"
    blk.save(data, meta)
    js = json.load(open(meta))
    assert js["encoding"] == ("OneBitRotatedBlocks" if enc == ONE_B else "TwoBitsRotatedBlocks")
    if enc == TWO_B:
        assert len(js["thresholds"]["lo"]) == dim and len(js["thresholds"]["hi"]) == dim
    else:
        assert "thresholds" not in js
    back = E.load(data, meta, qa.VectorParameters(dim, n, D.Dot, False), store=store)
    assert back.encoding == enc and back.code_bits == blk.code_bits
    _same(back.storage_bytes(), blk.storage_bytes(), "rows")
    if enc == TWO_B:
        for g, w in zip(back.thresholds, blk.thresholds):
            _same(g, w, "thresholds")
    qf = x[9]
    _same(back.encode_query(qf).encoded_vector, blk.encode_query(qf).encoded_vector, "query after load")
    assert_bits_equal(back.score_all(back.encode_query(qf)), blk.score_all(blk.encode_query(qf)), "scores after load")


@pytest.mark.parametrize("enc", [ONE_B, TWO_B])
def test_topk_rescored_against_originals_of_dim(enc):
    n, dim = 500, 192
    x = _data(n, dim, 12)
    x[:8] = np.random.default_rng(1).normal(size=(8, dim)).astype(f32)  # the originals hold no specials
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    blk = E.encode(x, vp, encoding=enc)
    orig = qa.OriginalVectors.from_data(x, vp)
    qf = (x[77] + 0.1).astype(f32)
    q = blk.encode_query(qf)
    cand, _ = blk.topk(q, 50, True)
    wid, wsc = orig.rerank(qf, cand, 10, True)
    gid, gsc = blk.topk_rescored(q, orig, qf, 10, 50, True)
    assert np.array_equal(gid, wid)
    assert_bits_equal(gsc, wsc, "topk_rescored")


# ------------------------------------------------------------------------------------------------ unchanged handles
def test_plain_and_rotated_handles_are_unchanged_beside_block_ones():
    n, dim = 40, 192
    x = _data(n, dim, 5)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    E.encode(x, vp, encoding=ONE_B), E.encode(x, vp, encoding=TWO_B)
    one = E.encode(x, vp)
    assert one.encoding == B.OneBit and one.code_bits == dim and one.thresholds is None
    bits = np.zeros((n, m.row_bytes(dim, 0) * 8), dtype=np.uint8)
    bits[:, :dim] = x > 0
    _same(one.storage_bytes(), np.packbits(bits, axis=1, bitorder="little"), "one-bit rows")
    two = E.encode(x, vp, encoding=B.TwoBits)
    lo, hi = m.thresholds(*m.stats(x), 0.43)
    assert two.encoding == B.TwoBits and two.code_bits == 2 * dim
    _same(two.thresholds[0], lo, "two-bit lo")
    _same(two.thresholds[1], hi, "two-bit hi")
    _same(two.storage_bytes(), m.encode(x, lo, hi, m.U8), "two-bit rows")
    y = rm.rotate(x)  # P = 256 values
    rot1 = E.encode(x, vp, encoding=B.OneBitRotated)
    assert rot1.encoding == B.OneBitRotated and rot1.code_bits == 256
    _same(rot1.storage_bytes(), rm.one_bit_rows(y, m.row_bytes(256, 0)), "rotated one-bit rows")
    rot2 = E.encode(x, vp, encoding=B.TwoBitsRotated)
    rlo, rhi = m.thresholds(*m.stats(y), 0.43)
    assert rot2.encoding == B.TwoBitsRotated and rot2.code_bits == 512 and rot2.thresholds[0].size == 256
    _same(rot2.thresholds[0], rlo, "rotated lo")
    _same(rot2.thresholds[1], rhi, "rotated hi")
    _same(rot2.storage_bytes(), m.encode(y, rlo, rhi, m.U8), "rotated two-bit rows")
