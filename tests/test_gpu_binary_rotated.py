"""Rotated binary rows on the GPU, every comparison on raw bits.

Two oracles: the numpy model (rotated_model.py, composed with the models of the plain encodings), and a PLAIN store made
by from_storage from the same bytes with dim = P - one-bit for a rotated one-bit handle, two-bit with the same thresholds
for a rotated two-bit one.  Every scoring route of the rotated store must equal that store's: same kernels, same routes."""
import json

import numpy as np
import pytest

import rotated_model as rm
import two_bit_model as m
import two_bit_scalar_model as sm
from util import assert_bits_equal, scalar_codes, scalar_planes, scalar_scores

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

E = qa.EncodedVectorsBin
D = qa.DistanceType
S = qa.BitsStoreType
B = qa.BinaryEncoding
ONE_R, TWO_R = B.OneBitRotated, B.TwoBitsRotated
f32 = np.float32

# 2048 is the widest row the wave-per-row kernel takes (kRotWaveMax): 2049 pads to 4096 and takes the workgroup-per-row one.
# A source row shorter than P: 257 and 300 (P = 512, two chunks per lane, dword and 16-byte loads) and 5000 (P = 8192,
# the workgroup-per-row kernel).
ROW_DIMS = [1, 2, 3, 63, 64, 65, 100, 128, 129, 257, 300, 1024, 1025, 2047, 2048, 2049, 5000, 16384]


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
    return [D.Dot, D.L1, D.L2][dim % 3], bool(dim % 2)


def _model_rows(x, enc, store, thresholds=None):
    """(rows u8, thresholds or None, P) of the model."""
    y = rm.rotate(x)
    p = y.shape[1]
    if enc == ONE_R:
        return rm.one_bit_rows(y, m.row_bytes(p, int(store))), None, p
    lo, hi = thresholds if thresholds is not None else m.thresholds(*m.stats(y), 0.43)
    return m.encode(y, lo, hi, int(store)), (lo, hi), p


def _plain(rows, p, n, dist, invert, store, thr):
    vp = qa.VectorParameters(p, n, dist, invert)
    if thr is None:
        return E.from_storage(rows, vp, store=store)
    return E.from_storage(rows, vp, store=store, encoding=B.TwoBits, thresholds=thr)


def _floats_of_bits(row, p):
    """+-1 floats whose one-bit encoding is the first p bits of `row`."""
    return np.where(np.unpackbits(row, bitorder="little")[:p] == 1, f32(1.0), f32(-1.0)).astype(f32)


def _metric(xor, code_bits, dist, invert):
    xor = np.asarray(xor).astype(f32)
    zeros = (f32(code_bits) - xor).astype(f32)
    return ((zeros - xor) if (dist == D.Dot) != bool(invert) else (xor - zeros)).astype(f32)


def _check_store(enc_h, enc, want, thr, p, store):
    assert enc_h.encoding == enc
    assert enc_h.code_bits == (2 * p if enc == TWO_R else p)
    assert want.shape[1] == E.get_quantized_vector_size_from_params(enc_h.vector_parameters, store, enc)
    if thr is None:
        assert enc_h.thresholds is None
    else:
        lo, hi = enc_h.thresholds
        assert lo.size == p and hi.size == p
        _same(lo, thr[0], "lo")
        _same(hi, thr[1], "hi")
    _same(enc_h.storage_bytes(), want, "rows")


# ------------------------------------------------------------------------------------------------ rows and routes
@pytest.mark.parametrize("enc", [ONE_R, TWO_R])
@pytest.mark.parametrize("store", [S.U8, S.U128])
@pytest.mark.parametrize("dim", ROW_DIMS)
def test_rows_and_routes(dim, store, enc):
    import torch
    n = 40
    dist, invert = _dist(dim)
    x = _data(n, dim, dim)
    vp = qa.VectorParameters(dim, n, dist, invert)
    want, thr, p = _model_rows(x, enc, store)
    rot = E.encode(x, vp, store=store, encoding=enc)
    _check_store(rot, enc, want, thr, p, store)
    if enc == ONE_R:
        assert not want[0].any(), "an all-zero row has no bit set"
    assert not np.unpackbits(rot.storage_bytes(), axis=1, bitorder="little")[:, rot.code_bits:].any(), "pad bits"
    # device data: aligned (16-byte loads where dim % 4 == 0) and one float past a 16-byte boundary (dword loads)
    flat = torch.zeros(n * dim + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(x).cuda().reshape(-1)
    off = flat[1:].view(n, dim)
    assert off.data_ptr() % 16 == 4
    for src in (torch.from_numpy(x).cuda(), off):
        _same(E.encode(src, vp, store=store, encoding=enc, thresholds=thr).storage_bytes(), want, "rows from device data")

    plain = _plain(want, p, n, dist, invert, store, thr)
    assert plain.encoding == (B.TwoBits if enc == TWO_R else B.OneBit) and plain.code_bits == rot.code_bits
    rng = np.random.default_rng(dim + 5)
    qf = (x[7] + 0.5 * rng.normal(size=dim)).astype(f32)
    yq = rm.rotate(qf)
    q = rot.encode_query(qf)
    if enc == ONE_R:
        qrow = rm.one_bit_rows(yq, want.shape[1])[0]
        pq = plain.encode_query(_floats_of_bits(qrow, p))
    else:
        qrow = m.encode(yq, thr[0], thr[1], int(store))[0]
        pq = plain.encode_query(yq[0])
    _same(q.encoded_vector, qrow, "query bits against the model")
    _same(pq.encoded_vector, qrow, "the plain store takes the same query bytes")
    scores = rot.score_all(q)
    assert_bits_equal(scores, _metric(m.xor_count(want, qrow), rot.code_bits, dist, invert), "score_all against the model")
    assert_bits_equal(scores, plain.score_all(pq), "score_all against the plain store")
    assert_bits_equal(rot.score_internal_all(9), plain.score_internal_all(9), "score_internal_all")
    for largest in (True, False):
        for k in (1, 10):
            for got, ref in ((rot.topk(q, k, largest), plain.topk(pq, k, largest)),
                             (rot.topk_internal(9, k, largest), plain.topk_internal(9, k, largest))):
                assert np.array_equal(got[0], ref[0]), ("ids", k, largest)
                assert_bits_equal(got[1], ref[1], "top-k scores")
    with pytest.raises(qa.EncodingError):
        rot.encode_query(np.zeros(dim + 1, dtype=f32))
    with pytest.raises(qa.EncodingError):
        rot.encode_query_batch(np.zeros((2, dim + 1), dtype=f32))


@pytest.mark.parametrize("enc", [ONE_R, TWO_R])
def test_statistics_cross_a_block(enc):
    n, dim = 4097, 100
    x = _data(n, dim, 4097)
    want, thr, p = _model_rows(x, enc, S.U8)
    rot = E.encode(x, qa.VectorParameters(dim, n, D.Dot, False), encoding=enc)
    _check_store(rot, enc, want, thr, p, S.U8)


# --------------------------------------------------------------------------------------------------------- queries
def _scalar_want(enc, yq, thr, p, bits, store, rows, dist, invert):
    """(planes u8 [bits, nb], max_abs, scores f32 [n]) of the models for one rotated query yq [P]."""
    if enc == ONE_R:
        codes, a = scalar_codes(yq, bits)
        return scalar_planes(codes, bits, rows.shape[1]), a, scalar_scores(rows, codes, p, bits, dist, invert)
    codes, a = sm.weighted_codes(yq, thr[0], thr[1], bits)
    planes = sm.planes(codes, p, bits, int(store))
    return planes, a, sm.metric(sm.xor_from_planes(rows, planes), p, bits, int(dist), invert)


@pytest.mark.parametrize("enc", [ONE_R, TWO_R])
@pytest.mark.parametrize("dim", [3, 100, 1024, 2049, 16384])
def test_queries(dim, enc):
    n, store = 40, S.U8
    dist, invert = _dist(dim + 1)
    x = _data(n, dim, dim + 11)
    vp = qa.VectorParameters(dim, n, dist, invert)
    rows, thr, p = _model_rows(x, enc, store)
    rot = E.encode(x, vp, store=store, encoding=enc)
    rng = np.random.default_rng(dim)
    queries = (x[rng.integers(0, n, size=33)] + 0.5 * rng.normal(size=(33, dim))).astype(f32)
    queries[1, dim // 2] = np.nan
    queries[2, 0] = np.inf
    yqs = rm.rotate(queries)
    weighted = enc == TWO_R
    # one bit per query dimension: single and batches of 3 and 33
    if enc == ONE_R:
        qrows = rm.one_bit_rows(yqs, rows.shape[1])
    else:
        qrows = m.encode(yqs, thr[0], thr[1], int(store))
    want1 = np.stack([_metric(m.xor_count(rows, r), rot.code_bits, dist, invert) for r in qrows])
    for nq in (3, 33):
        b = rot.encode_query_batch(queries[:nq])
        assert b.bits == 1
        for i in range(nq):
            _same(b.encoded_vector(i), qrows[i], f"batch of {nq}, query {i}")
        assert_bits_equal(rot.score_batch(b), want1[:nq], f"score_batch of {nq}")
    _same(rot.encode_query(queries[4]).encoded_vector, qrows[4], "single query")
    # 4 and 8 bits: unweighted on rotated one-bit rows, weighted on rotated two-bit rows
    n_model = 33 if p <= 1024 else 3  # (the plane oracle sets one bit at a time)
    for bits in (4, 8):
        wants = [_scalar_want(enc, yqs[i], thr, p, bits, store, rows, dist, invert) for i in range(n_model)]
        for i in (0, 1, 2):
            q = rot.encode_query(queries[i], query_bits=bits, weighted=weighted)
            assert q.bits == bits
            _same(q.encoded_vector, wants[i][0], f"{bits}-bit planes, query {i}")
            _same(q.max_abs, wants[i][1], "max_abs")
            assert_bits_equal(rot.score_all(q), wants[i][2], f"{bits}-bit score_all, query {i}")
        for nq in (3, 33):
            b = rot.encode_query_batch(queries[:nq], query_bits=bits, weighted=weighted)
            assert b.bits == bits
            got = rot.score_batch(b)
            for i in range(min(nq, n_model)):
                _same(b.encoded_vector(i), wants[i][0], f"{bits}-bit batch of {nq}, query {i}")
                assert_bits_equal(got[i], wants[i][2], f"{bits}-bit score_batch of {nq}, query {i}")
        if enc == ONE_R:  # on one-bit rows the weighted call is the unweighted one
            _same(rot.encode_query(queries[0], query_bits=bits, weighted=True).encoded_vector, wants[0][0], "weighted = unweighted")
        else:  # the existing refusal keeps its shape
            with pytest.raises(qa.EncodingError):
                rot.encode_query(queries[0], query_bits=bits)
            with pytest.raises(qa.EncodingError):
                rot.encode_query_batch(queries[:3], query_bits=bits)
        with pytest.raises(qa.EncodingError):
            rot.encode_query(np.zeros(dim + 1, dtype=f32), query_bits=bits, weighted=weighted)


# ------------------------------------------------------------------------------------- streaming, upsert, save / load
@pytest.mark.parametrize("enc", [ONE_R, TWO_R])
def test_streaming_with_uneven_batches(enc):
    n, dim = 4098, 100
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
    if enc == TWO_R:
        for g, w in zip(streamed.thresholds, one_shot.thresholds):
            _same(g, w, "streamed thresholds")
    want, thr, p = _model_rows(x, enc, S.U8)
    _check_store(streamed, enc, want, thr, p, S.U8)


@pytest.mark.parametrize("enc", [ONE_R, TWO_R])
@pytest.mark.parametrize("dim", [100, 1024, 2049])
def test_upsert_and_append(dim, enc):
    x = _data(50, dim, dim + 3)
    enc_h = E.encode(x[:30], qa.VectorParameters(dim, 30, D.Dot, False), encoding=enc)
    thr = enc_h.thresholds
    enc_h.append(x[30:40])
    enc_h.upsert(5, x[40:50])
    now = np.concatenate([x[:5], x[40:50], x[15:40]])
    fresh = E.encode(now, qa.VectorParameters(dim, 40, D.Dot, False), encoding=enc, thresholds=thr)
    _same(enc_h.storage_bytes(), fresh.storage_bytes(), "rows after append and upsert")
    want, _, _ = _model_rows(now, enc, S.U8, thr)
    _same(enc_h.storage_bytes(), want, "rows after append and upsert, against the model")


@pytest.mark.parametrize("store", [S.U8, S.U128])
@pytest.mark.parametrize("enc", [ONE_R, TWO_R])
def test_save_load_round_trip(tmp_path, enc, store):
    n, dim = 40, 100
    dist, invert = D.L2, True
    x = _data(n, dim, 8)
    vp = qa.VectorParameters(dim, n, dist, invert)
    rot = E.encode(x, vp, store=store, encoding=enc)
    data, meta = tmp_path / "rows.bin", tmp_path / "meta.json"
    rot.save(data, meta)
    js = json.load(open(meta))
    assert js["encoding"] == ("OneBitRotated" if enc == ONE_R else "TwoBitsRotated")
    if enc == TWO_R:
        assert len(js["thresholds"]["lo"]) == 128 and len(js["thresholds"]["hi"]) == 128
    back = E.load(data, meta, qa.VectorParameters(dim, n, D.Dot, False), store=store)
    assert back.encoding == enc and back.code_bits == rot.code_bits
    _same(back.storage_bytes(), rot.storage_bytes(), "rows")
    if enc == TWO_R:
        for g, w in zip(back.thresholds, rot.thresholds):
            _same(g, w, "thresholds")
    qf = x[3]
    assert_bits_equal(back.score_all(back.encode_query(qf)), rot.score_all(rot.encode_query(qf)), "scores after load")


@pytest.mark.parametrize("enc", [ONE_R, TWO_R])
def test_topk_rescored_against_originals_of_dim(enc):
    n, dim = 500, 100
    x = _data(n, dim, 12)
    x[:8] = np.random.default_rng(1).normal(size=(8, dim)).astype(f32)  # the originals hold no specials
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    rot = E.encode(x, vp, encoding=enc)
    orig = qa.OriginalVectors.from_data(x, vp)  # originals keep dim, not P
    qf = (x[77] + 0.1).astype(f32)
    q = rot.encode_query(qf)
    cand, _ = rot.topk(q, 50, True)
    wid, wsc = orig.rerank(qf, cand, 10, True)
    gid, gsc = rot.topk_rescored(q, orig, qf, 10, 50, True)
    assert np.array_equal(gid, wid)
    assert_bits_equal(gsc, wsc, "topk_rescored")


# ------------------------------------------------------------------------------------------------ unchanged handles
def test_plain_handles_are_unchanged_beside_rotated_ones():
    n, dim = 40, 100
    x = _data(n, dim, 5)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    E.encode(x, vp, encoding=ONE_R), E.encode(x, vp, encoding=TWO_R)
    one = E.encode(x, vp)
    assert one.encoding == B.OneBit and one.code_bits == dim and one.thresholds is None
    bits = np.zeros((n, m.row_bytes(dim, 0) * 8), dtype=np.uint8)
    bits[:, :dim] = x > 0
    rows1 = np.packbits(bits, axis=1, bitorder="little")
    _same(one.storage_bytes(), rows1, "one-bit rows")
    qf = x[7]
    assert_bits_equal(one.score_all(one.encode_query(qf)), scalar_scores(rows1, (qf > 0).astype(np.uint32), dim, 1, D.Dot, False),
                      "one-bit scores")
    two = E.encode(x, vp, encoding=B.TwoBits)
    lo, hi = m.thresholds(*m.stats(x), 0.43)
    assert two.encoding == B.TwoBits and two.code_bits == 2 * dim
    _same(two.thresholds[0], lo, "two-bit lo")
    _same(two.thresholds[1], hi, "two-bit hi")
    rows2 = m.encode(x, lo, hi, m.U8)
    _same(two.storage_bytes(), rows2, "two-bit rows")
    assert_bits_equal(two.score_all(two.encode_query(qf)), m.score_all(rows2, m.encode(qf, lo, hi, m.U8)[0], dim, m.DOT, False),
                      "two-bit scores")
