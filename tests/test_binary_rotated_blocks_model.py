"""Block-rotated binary rows without a GPU: the numpy model's transform against a float64 block-diagonal
Hadamard product on inputs where f32 is exact, its equality with the padded rotation at power-of-two dims, IEEE specials
that stay inside their block, the recall the block rotation buys at equal bytes on 3.2g's recipe, the refusals that are
made before a device is needed, and the public surface."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import rotated_blocks_model as bm
import rotated_model as rm
import two_bit_model as m
import two_bit_scalar_model as sm

import quantization_amd as qa
from quantization_amd import _lib

E = qa.EncodedVectorsBin
D = qa.DistanceType
S = qa.BitsStoreType
B = qa.BinaryEncoding
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------- transform
def _hadamard(p):
    h = np.ones((1, 1), dtype=np.float64)
    while h.shape[0] < p:
        h = np.block([[h, h], [h, -h]])
    return h


def test_block_sizes():
    assert [bm.block(d) for d in (64, 192, 320, 384, 768, 960, 1280, 1536, 1792, 2048, 2112, 3072, 12288, 16384)] == \
        [64, 64, 64, 128, 256, 64, 256, 512, 256, 2048, 64, 1024, 4096, 16384]
    for enc in (B.OneBitRotatedBlocks, B.TwoBitsRotatedBlocks):
        assert [enc.encoder_dim(d) for d in (0, 64, 192, 768, 1536, 16384)] == [0, 64, 192, 768, 1536, 16384]
    assert B.OneBitRotated.encoder_dim(768) == 1024  # the padded rotation is as it was


@pytest.mark.parametrize("dim", [64, 192, 320, 768, 1536])
def test_butterflies_are_the_block_diagonal_hadamard_product_where_f32_is_exact(dim):
    b = bm.block(dim)
    rng = np.random.default_rng(dim)
    x = rng.integers(-1000, 1001, size=(5, dim)).astype(f32)  # |sums| <= 512 * 1000 < 2^24: every f32 step is exact
    signs = 1.0 - 2.0 * rm.sign_bits(dim).astype(np.float64)
    want = (x.astype(np.float64) * signs) @ np.kron(np.eye(dim // b), _hadamard(b)).T
    got = bm.rotate(x)
    assert got.dtype == f32 and got.shape == (5, dim)
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("dim", [64, 256, 1024])
def test_a_power_of_two_dim_is_the_padded_rotation(dim):
    rng = np.random.default_rng(dim + 1)
    x = (rng.normal(size=(7, dim)) * rng.uniform(0.3, 1.5, size=dim)).astype(f32)
    x[1, 3], x[2, 5], x[3] = np.nan, np.inf, f32(1e-45)
    assert bm.block(dim) == dim
    assert np.array_equal(bm.rotate(x).view(np.uint32), rm.rotate(x).view(np.uint32))


def test_specials_stay_inside_their_block():
    dim = 192  # three blocks of 64
    x = np.ones((3, dim), dtype=f32)
    x[0, 70] = np.nan
    x[1, 130] = np.inf
    x[2, 5], x[2, 9] = np.inf, np.inf
    y = bm.rotate(x)
    assert np.isnan(y[0, 64:128]).all() and np.isfinite(y[0, :64]).all() and np.isfinite(y[0, 128:]).all()
    assert np.isinf(y[1, 128:]).all() and np.isfinite(y[1, :128]).all()
    assert np.isnan(y[2, :64]).any() and np.isfinite(y[2, 64:]).all()  # two infinities meet as inf - inf in block 0 alone
    sub = np.zeros((1, 64), dtype=f32)
    sub[0, :2] = f32(1e-45)  # the smallest subnormal: kept, not flushed
    assert np.any(bm.rotate(sub) != 0)
    zero = bm.rotate(np.zeros((1, dim), dtype=f32))
    assert not (zero > 0).any() and (zero == 0).all()  # an all-zero row has no bit set


# ------------------------------------------------------------------------------------------------------------- recall
def _scalar_planes_xor(rows_bits, codes, bits):
    """X of one-bit rows given as 0 / 1 arrays [n, dim] against codes [dim]: a set bit adds L - c_i, a clear one c_i (3.2d)."""
    L = (1 << bits) - 1
    c = codes.astype(np.float64)
    return rows_bits.astype(np.float64) @ (L - 2 * c) + c.sum()


def _recall(seed, dim, clustered=False, n=4000, n_queries=100, k=10):
    """recall@10 against the exact dot top-10 on 3.2g's recipe: plain (dim bits), block-rotated (dim bits) and
    padded-rotated (P bits) rows, each as one bit, two bits and one bit against 8-bit queries."""
    rng = np.random.default_rng(seed)
    if clustered:
        centres = rng.normal(size=(32, dim))
        scale = rng.uniform(0.8, 1.2, size=dim)
        data = ((centres[rng.integers(0, 32, size=n)] + 0.7 * rng.normal(size=(n, dim))) * scale).astype(f32)
    else:
        scale = rng.uniform(0.3, 1.5, size=dim)
        data = (rng.normal(size=(n, dim)) * scale).astype(f32)
    picks = rng.integers(0, n, size=n_queries)
    queries = (data[picks] + 0.5 * rng.normal(size=(n_queries, dim))).astype(f32)
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    exact = np.argsort(-(queries.astype(np.float64) @ data.astype(np.float64).T), axis=1, kind="stable")[:, :k]
    out = {}
    for name, rows_f, q_f in (("", data, queries), ("blk ", bm.rotate(data), bm.rotate(queries)),
                              ("rot ", rm.rotate(data), rm.rotate(queries))):
        lo, hi = m.thresholds(*m.stats(rows_f), 0.43)
        one_rows, one_q = rows_f > 0, q_f > 0
        two_rows, two_q = m.encode(rows_f, lo, hi, m.U8), m.encode(q_f, lo, hi, m.U8)
        hits = {"one": 0, "two": 0, "one+8": 0}
        for qi in range(n_queries):
            want = set(exact[qi].tolist())
            x = (one_rows != one_q[qi]).sum(axis=1)
            hits["one"] += len(set(np.argsort(x, kind="stable")[:k].tolist()) & want)
            x = m.xor_count(two_rows, two_q[qi])
            hits["two"] += len(set(np.argsort(x, kind="stable")[:k].tolist()) & want)
            codes, _ = sm.codes_of(q_f[qi], 8)
            x = _scalar_planes_xor(one_rows, codes, 8)
            hits["one+8"] += len(set(np.argsort(x, kind="stable")[:k].tolist()) & want)
        for key, v in hits.items():
            out[name + key] = v / (n_queries * k)
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("dim", [384, 768])
def test_block_rotation_recalls_more_than_plain_rows_of_the_same_bytes(dim, seed):
    r = _recall(seed, dim)
    # the padded rotation ("rot", P bits a row against dim) is printed beside them, not asserted
    print(f"dim {dim} seed {seed}: recall@10 " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert r["blk one"] > r["one"]
    assert r["blk two"] > r["two"]
    assert r["blk one+8"] > r["one+8"]


def test_clustered_mixture_is_printed_not_asserted():
    r = _recall(1, 384, clustered=True)
    print("clustered mixture, mild column scales (either rotation is neutral here): recall@10 " +
          ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


# ---------------------------------------------------------------------------------------------------------- refusals
def _vp(dim, count):
    return _lib.VectorParametersC(dim, count, int(D.Dot), 0)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _entry_points(dim, lo, hi, encoding, count=4):
    """(name, status, out) of the three *_enc calls that make a handle; the row and data pointers are never read."""
    L = _lib.lib()
    vp = _vp(dim, count)
    none_stop = _lib.STOP_FN(0)
    data = np.zeros((count, dim), dtype=f32)
    out = C.c_void_p()
    yield "encode_enc", L.qamd_bin_encode_enc(_ptr(data), _lib.MEM_HOST, C.byref(vp), 0, encoding, _ptr(lo), _ptr(hi), none_stop,
                                              None, None, C.byref(out)), out
    yield "encoder_begin_enc", L.qamd_bin_encoder_begin_enc(C.byref(vp), 0, encoding, _ptr(lo), _ptr(hi), none_stop, None, None,
                                                            C.byref(out)), out
    rows = np.zeros(count * (dim // 4 + 16), dtype=np.uint8)
    yield "from_rows_enc", L.qamd_bin_from_rows_enc(_ptr(rows), _lib.MEM_HOST, C.byref(vp), 0, encoding, _ptr(lo), _ptr(hi), None,
                                                    C.byref(out)), out


@pytest.mark.parametrize("encoding", [16, 17, 18, 19, 22, 23, 24, 28, 36, 37])
def test_blocks_without_rotation_and_unknown_values_are_refused_before_a_device_is_needed(encoding):
    for name, st, out in _entry_points(64, None, None, encoding):
        assert st == _lib.ERR_ARGUMENTS and out.value is None, (name, st)
        assert b"unknown binary encoding" in _lib.lib().qamd_last_error()


@pytest.mark.parametrize("encoding", [20, 21])
def test_dimension_refusals_before_a_device_is_needed(encoding):
    L = _lib.lib()
    for name, st, out in _entry_points(100, None, None, encoding):
        assert st == _lib.ERR_ARGUMENTS and out.value is None, (name, st)
        assert b"multiple of 64" in L.qamd_last_error(), L.qamd_last_error()
    for name, st, out in _entry_points(bm.MAX_DIM + 64, None, None, encoding, count=0):  # 16448 = 257 * 64
        assert st == _lib.ERR_ARGUMENTS and out.value is None, (name, st)
        assert b"rotated rows have at most 16384" in L.qamd_last_error()


def test_threshold_refusals_before_a_device_is_needed():
    L = _lib.lib()
    dim = 192
    lo, hi = np.full(dim, -1, f32), np.full(dim, 1, f32)
    for what, (plo, phi, enc) in {"lo alone": (lo, None, 21), "hi alone": (None, hi, 21),
                                  "thresholds with block-rotated one bit": (lo, hi, 20)}.items():
        for name, st, out in _entry_points(dim, plo, phi, enc):
            assert st == _lib.ERR_ARGUMENTS and out.value is None, (what, name, st)
    above = lo.copy()
    above[dim - 1] = 2.0  # the last of dim entries: thresholds of a block-rotated handle have dim of them, not P = 256
    for name, st, out in _entry_points(dim, above, hi, 21):
        assert st == _lib.ERR_ARGUMENTS and out.value is None, (name, st)
        assert b"threshold 191" in L.qamd_last_error()
    out = C.c_void_p()
    vp = _vp(dim, 4)  # block-rotated two-bit rows from storage cannot do without thresholds
    assert L.qamd_bin_from_rows_enc(_ptr(np.zeros(4 * 48, np.uint8)), _lib.MEM_HOST, C.byref(vp), 0, 21, None, None, None,
                                    C.byref(out)) == _lib.ERR_ARGUMENTS
    assert b"need their thresholds" in L.qamd_last_error() and out.value is None
    # the Python layer sizes the arrays by dim as well
    with pytest.raises(qa.EncodingError):
        E.from_storage(np.zeros((4, 48), np.uint8), qa.VectorParameters(dim, 4, D.Dot, False),
                       encoding=B.TwoBitsRotatedBlocks, thresholds=(np.zeros(256, f32), np.ones(256, f32)))


def test_load_refusals_before_a_device_is_needed(tmp_path):
    dim, count = 192, 2
    vpj = {"dim": dim, "count": count, "distance_type": "Dot", "invert": False}
    data = tmp_path / "rows.bin"
    data.write_bytes(bytes(count * m.row_bytes(2 * dim, 0)))
    bad = {
        "arrays of P entries": {"vector_parameters": vpj, "encoding": "TwoBitsRotatedBlocks",
                                "thresholds": {"lo": [0.0] * 256, "hi": [1.0] * 256}},
        "hi of P entries": {"vector_parameters": vpj, "encoding": "TwoBitsRotatedBlocks",
                            "thresholds": {"lo": [0.0] * dim, "hi": [1.0] * 256}},
        "lo one short": {"vector_parameters": vpj, "encoding": "TwoBitsRotatedBlocks",
                         "thresholds": {"lo": [0.0] * (dim - 1), "hi": [1.0] * dim}},
        "no thresholds": {"vector_parameters": vpj, "encoding": "TwoBitsRotatedBlocks"},
        "lo > hi at the last entry": {"vector_parameters": vpj, "encoding": "TwoBitsRotatedBlocks",
                                      "thresholds": {"lo": [0.0] * (dim - 1) + [2.0], "hi": [1.0] * dim}},
        "unknown": {"vector_parameters": vpj, "encoding": "OneBitBlocks"},
    }
    L = _lib.lib()
    vp = _vp(dim, count)
    meta = tmp_path / "meta.json"
    for what, obj in bad.items():
        meta.write_text(json.dumps(obj))
        out = C.c_void_p()
        st = L.qamd_bin_load(os.fsencode(data), os.fsencode(meta), C.byref(vp), 0, C.byref(out))
        assert st == _lib.ERR_IO and out.value is None, (what, st, L.qamd_last_error())
    for name in ("OneBitRotatedBlocks", "TwoBitsRotatedBlocks"):
        for bad_dim, count_ in ((100, 2), (bm.MAX_DIM + 64, 0)):  # not a multiple of 64; past the rotation's limit
            obj = {"vector_parameters": dict(vpj, dim=bad_dim, count=count_), "encoding": name,
                   "thresholds": {"lo": [0.0] * 100, "hi": [1.0] * 100}}
            meta.write_text(json.dumps(obj))
            out = C.c_void_p()
            vpb = _vp(bad_dim, count_)
            st = L.qamd_bin_load(os.fsencode(data), os.fsencode(meta), C.byref(vpb), 0, C.byref(out))
            assert st == _lib.ERR_IO and out.value is None, (name, bad_dim, st, L.qamd_last_error())
            if bad_dim == 100:
                assert b"multiple of 64" in L.qamd_last_error()


# ----------------------------------------------------------------------------------------------------------- surface
def test_surface():
    assert len(_lib.declared_symbols()) == 192  # the flag rides the *_enc calls' argument: no entry point of its own
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "quantization_amd.h")).read()
    consts = dict(re.findall(r"\b(QAMD_BIN_BLOCKS|QAMD_BIN_ONE_BIT_ROTATED_BLOCKS|QAMD_BIN_TWO_BITS_ROTATED_BLOCKS) = (\d+)", hdr))
    assert consts == {"QAMD_BIN_BLOCKS": "16", "QAMD_BIN_ONE_BIT_ROTATED_BLOCKS": "20", "QAMD_BIN_TWO_BITS_ROTATED_BLOCKS": "21"}
    # declared after the frozen typedef, not inside it
    assert hdr.index("QAMD_BIN_BLOCKS = 16") > hdr.index("} qamd_bin_encoding;")
    assert re.search(r"QAMD_BIN_BLOCKS alone \(16\)[^.]*refused", hdr)
    assert re.search(r"block-diagonal rotations\s+\*?\s*with blocks of unequal size", hdr)
    assert (int(B.OneBitRotatedBlocks), int(B.TwoBitsRotatedBlocks)) == (20, 21)
    assert (bm.BLOCKS, bm.ONE_BIT_ROTATED_BLOCKS, bm.TWO_BITS_ROTATED_BLOCKS) == (16, 20, 21)
    for enc in (B.OneBitRotatedBlocks, B.TwoBitsRotatedBlocks):
        assert enc.blocks and enc.rotated and enc.two_bits == (enc == B.TwoBitsRotatedBlocks)
    for enc in (B.OneBit, B.TwoBits, B.OneBitRotated, B.TwoBitsRotated):
        assert not enc.blocks
    assert "largest power of two" in B.__doc__


@pytest.mark.parametrize("dim", [64, 192, 768, 1536, 2112])
@pytest.mark.parametrize("store", [S.U8, S.U128])
def test_row_sizes_are_the_plain_store_s(dim, store):
    vp = qa.VectorParameters(dim, 0, D.Dot, False)
    one = E.get_quantized_vector_size_from_params(vp, store, B.OneBitRotatedBlocks)
    two = E.get_quantized_vector_size_from_params(vp, store, B.TwoBitsRotatedBlocks)
    assert one == E.get_quantized_vector_size_from_params(vp, store) == m.row_bytes(dim, int(store))
    assert two == E.get_quantized_vector_size_from_params(vp, store, B.TwoBits) == m.row_bytes(2 * dim, int(store))
    if dim % 128 == 0:  # (rows are whole 16-byte words: 192 bits take 32 bytes, 384 bits 48)
        assert two == 2 * one == dim // 4  # twice the bits, and at 768 the plain store's 96 bytes a row
    # the padded rotation is as it was
    p = rm.padded_dim(dim)
    assert E.get_quantized_vector_size_from_params(vp, store, B.OneBitRotated) == m.row_bytes(p, int(store))
