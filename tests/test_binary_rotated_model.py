"""Rotated binary rows without a GPU: the numpy model's transform against a float64 Hadamard product on
inputs where f32 is exact, its signs against known answers, IEEE specials, the recall the rotation buys on the
specification's recipe, the refusals that are made before a device is needed, and the public surface."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

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


def _bits(a):
    return np.asarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------- transform
def _hadamard(p):
    h = np.ones((1, 1), dtype=np.float64)
    while h.shape[0] < p:
        h = np.block([[h, h], [h, -h]])
    return h


def test_known_answer_signs():
    # h & 1 of the specification's hash for i = 0 .. 15, worked out by hand-run integer arithmetic (python ints mod 2^32)
    def h(i):
        x = (i * 0x9E3779B1) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        x ^= x >> 16
        return x & 1
    want = [0, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0]
    assert [h(i) for i in range(16)] == want
    assert rm.sign_bits(16).tolist() == want
    assert rm.sign_bits(256)[:16].tolist() == want  # the sign of i does not depend on P


@pytest.mark.parametrize("p", [1, 2, 4, 64, 128, 256])
def test_butterflies_are_the_hadamard_product_where_f32_is_exact(p):
    rng = np.random.default_rng(p)
    for dim in sorted({p, max(1, p - 1), p // 2 + 1}):
        if rm.padded_dim(dim) != p:
            continue
        x = rng.integers(-1000, 1001, size=(5, dim)).astype(f32)  # |sums| <= 256000 < 2^24: every f32 step is exact
        pad = np.zeros((5, p), dtype=np.float64)
        pad[:, :dim] = x
        signs = 1.0 - 2.0 * rm.sign_bits(p).astype(np.float64)
        want = (pad * signs) @ _hadamard(p).T
        got = rm.rotate(x)
        assert got.dtype == f32 and got.shape == (5, p)
        assert np.array_equal(got.astype(np.float64), want), (p, dim)


def test_padded_dim():
    assert [rm.padded_dim(d) for d in (1, 2, 3, 4, 5, 63, 64, 65, 768, 1024, 1025, 16384)] == \
        [1, 2, 4, 4, 8, 64, 64, 128, 1024, 1024, 2048, 16384]
    assert [B.OneBitRotated.encoder_dim(d) for d in (0, 1, 2, 3, 768, 16384)] == [0, 1, 2, 4, 1024, 16384]
    assert B.TwoBits.encoder_dim(768) == 768


def test_specials_follow_ieee():
    sub = f32(1e-45)  # the smallest subnormal: kept, not flushed
    y = rm.rotate(np.array([[sub, sub]], dtype=f32))
    s = 1.0 - 2.0 * rm.sign_bits(2).astype(np.float64)
    want = np.array([s[0] + s[1], s[0] - s[1]]) * float(sub)
    assert np.array_equal(y[0].astype(np.float64), want) and np.any(y != 0)
    x = np.ones((3, 8), dtype=f32)
    x[0, 3] = np.nan
    x[1, 2] = np.inf
    x[2, 2], x[2, 5] = np.inf, np.inf
    y = rm.rotate(x)
    assert np.isnan(y[0]).all()  # every output is a sum over every input
    assert np.isinf(y[1]).all() and not np.isnan(y[1]).any()  # one infinity: +-inf everywhere
    assert np.isnan(y[2]).any()  # two infinities meet as inf - inf somewhere
    zero = rm.rotate(np.zeros((1, 5), dtype=f32))
    assert not (zero > 0).any() and (zero == 0).all()  # an all-zero row has no bit set


# ------------------------------------------------------------------------------------------------------------- recall
def _scalar_planes_xor(rows_bits, codes, bits):
    """X of one-bit rows given as 0 / 1 arrays [n, P] against codes [P]: a set bit adds L - c_i, a clear one c_i (3.2d)."""
    L = (1 << bits) - 1
    c = codes.astype(np.float64)
    return rows_bits.astype(np.float64) @ (L - 2 * c) + c.sum()


def _recall(seed, clustered=False, n=4000, dim=256, n_queries=100, k=10):
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
    for name, rows_f, q_f in (("", data, queries), ("rot ", rm.rotate(data), rm.rotate(queries))):
        p = rows_f.shape[1]
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
        assert p == rm.padded_dim(dim) or name == ""
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rotation_recalls_more_on_columns_of_unequal_scale(seed):
    r = _recall(seed)
    print(f"seed {seed}: recall@10 " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert r["rot one"] > r["one"]
    assert r["rot two"] > r["two"]
    assert r["rot one+8"] > r["one+8"]


def test_clustered_mixture_is_printed_not_asserted():
    r = _recall(1, clustered=True)
    print("clustered mixture, mild column scales (the rotation is neutral to slightly worse here): recall@10 " +
          ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


# ---------------------------------------------------------------------------------------------------------- refusals
def _vp(dim, count):
    return _lib.VectorParametersC(dim, count, int(D.Dot), 0)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _entry_points(dim, data, lo, hi, encoding):
    L = _lib.lib()
    vp = _vp(dim, 4)
    none_stop = _lib.STOP_FN(0)
    out = C.c_void_p()
    yield "encode_enc", L.qamd_bin_encode_enc(_ptr(data), _lib.MEM_HOST, C.byref(vp), 0, encoding, lo, hi, none_stop, None, None,
                                              C.byref(out)), out
    yield "encoder_begin_enc", L.qamd_bin_encoder_begin_enc(C.byref(vp), 0, encoding, lo, hi, none_stop, None, None,
                                                            C.byref(out)), out
    rows = np.zeros(4 * 64, dtype=np.uint8)
    yield "from_rows_enc", L.qamd_bin_from_rows_enc(_ptr(rows), _lib.MEM_HOST, C.byref(vp), 0, encoding, lo, hi, None,
                                                    C.byref(out)), out


@pytest.mark.parametrize("encoding", [2, 3, 6, 7, 8, -1, 12])
def test_unknown_encodings_are_refused_before_a_device_is_needed(encoding):
    data = np.zeros((4, 8), dtype=f32)
    for name, st, out in _entry_points(8, data, None, None, encoding):
        assert st == _lib.ERR_ARGUMENTS and out.value is None, (name, st)
        assert b"unknown binary encoding" in _lib.lib().qamd_last_error()


def test_argument_errors_before_a_device_is_needed():
    L = _lib.lib()
    dim = 6  # P = 8
    data = np.zeros((4, dim), dtype=f32)
    lo, hi = np.full(8, -1, f32), np.full(8, 1, f32)
    for what, (plo, phi, enc) in {"lo alone": (_ptr(lo), None, 5), "hi alone": (None, _ptr(hi), 5),
                                  "thresholds with rotated one bit": (_ptr(lo), _ptr(hi), 4)}.items():
        for name, st, out in _entry_points(dim, data, plo, phi, enc):
            assert st == _lib.ERR_ARGUMENTS and out.value is None, (what, name, st)
    above = lo.copy()
    above[7] = 2.0  # entry 7 exists only because thresholds of a rotated handle have P = 8 entries
    for name, st, out in _entry_points(dim, data, _ptr(above), _ptr(hi), 5):
        assert st == _lib.ERR_ARGUMENTS and out.value is None, (name, st)
        assert b"threshold 7" in L.qamd_last_error()
    out = C.c_void_p()
    vp = _vp(dim, 4)  # rotated two-bit rows from storage cannot do without thresholds
    assert L.qamd_bin_from_rows_enc(_ptr(np.zeros(64, np.uint8)), _lib.MEM_HOST, C.byref(vp), 0, 5, None, None, None,
                                    C.byref(out)) == _lib.ERR_ARGUMENTS
    big = _vp(rm.MAX_DIM + 1, 0)
    for enc in (4, 5):
        assert L.qamd_bin_encode_enc(None, _lib.MEM_HOST, C.byref(big), 0, enc, None, None, _lib.STOP_FN(0), None, None,
                                     C.byref(out)) == _lib.ERR_ARGUMENTS
        assert b"rotated rows have at most 16384" in L.qamd_last_error()
        assert L.qamd_bin_encoder_begin_enc(C.byref(big), 0, enc, None, None, _lib.STOP_FN(0), None, None,
                                            C.byref(out)) == _lib.ERR_ARGUMENTS
    assert L.qamd_bin_from_rows_enc(None, _lib.MEM_HOST, C.byref(big), 0, 4, None, None, None, C.byref(out)) == _lib.ERR_ARGUMENTS
    assert out.value is None


def test_load_refusals_before_a_device_is_needed(tmp_path):
    dim, count = 6, 2  # P = 8 != dim
    vpj = {"dim": dim, "count": count, "distance_type": "Dot", "invert": False}
    data = tmp_path / "rows.bin"
    data.write_bytes(bytes(count * m.row_bytes(16, 0)))
    bad = {
        "arrays of dim entries": {"vector_parameters": vpj, "encoding": "TwoBitsRotated",
                                  "thresholds": {"lo": [0.0] * dim, "hi": [1.0] * dim}},
        "lo of dim entries": {"vector_parameters": vpj, "encoding": "TwoBitsRotated",
                              "thresholds": {"lo": [0.0] * dim, "hi": [1.0] * 8}},
        "no thresholds": {"vector_parameters": vpj, "encoding": "TwoBitsRotated"},
        "lo > hi past dim": {"vector_parameters": vpj, "encoding": "TwoBitsRotated",
                             "thresholds": {"lo": [0.0] * 7 + [2.0], "hi": [1.0] * 8}},
        "unknown": {"vector_parameters": vpj, "encoding": "OneBitRotatedTwice"},
    }
    L = _lib.lib()
    vp = _vp(dim, count)
    for what, obj in bad.items():
        meta = tmp_path / "meta.json"
        meta.write_text(json.dumps(obj))
        out = C.c_void_p()
        st = L.qamd_bin_load(os.fsencode(data), os.fsencode(meta), C.byref(vp), 0, C.byref(out))
        assert st == _lib.ERR_IO and out.value is None, (what, st, L.qamd_last_error())
    big = _vp(rm.MAX_DIM + 1, 0)
    meta = tmp_path / "meta.json"
    meta.write_text(json.dumps({"vector_parameters": dict(vpj, dim=rm.MAX_DIM + 1, count=0), "encoding": "OneBitRotated"}))
    out = C.c_void_p()
    assert L.qamd_bin_load(os.fsencode(data), os.fsencode(meta), C.byref(big), 0, C.byref(out)) == _lib.ERR_IO


# ----------------------------------------------------------------------------------------------------------- surface
def test_surface():
    assert len(_lib.declared_symbols()) == 192  # the flag rides the *_enc calls' argument: no entry point of its own
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "quantization_amd.h")).read()
    assert re.search(r"typedef enum \{ QAMD_BIN_ONE_BIT = 0, QAMD_BIN_TWO_BITS = 1,\s*QAMD_BIN_ROTATED = 4,\s*/\*[^*]*\*/\s*"
                     r"QAMD_BIN_ONE_BIT_ROTATED = 4, QAMD_BIN_TWO_BITS_ROTATED = 5 \} qamd_bin_encoding;", hdr)
    for out_of_scope in ("sharded binary handles", "seeds other than the fixed one", "more than one round",
                         "block-diagonal rotations", "bench.py"):
        assert out_of_scope in hdr
    assert (int(B.OneBit), int(B.TwoBits), int(B.OneBitRotated), int(B.TwoBitsRotated)) == (0, 1, 4, 5)
    assert B.OneBitRotated.rotated and not B.OneBitRotated.two_bits and B.TwoBitsRotated.rotated and B.TwoBitsRotated.two_bits
    assert hasattr(E, "code_bits")


@pytest.mark.parametrize("dim", [1, 100, 128, 129, 768])
@pytest.mark.parametrize("store", [S.U8, S.U128])
def test_row_sizes(dim, store):
    vp = qa.VectorParameters(dim, 0, D.Dot, False)
    p = rm.padded_dim(dim)
    one = E.get_quantized_vector_size_from_params(vp, store, B.OneBitRotated)
    two = E.get_quantized_vector_size_from_params(vp, store, B.TwoBitsRotated)
    assert one == m.row_bytes(p, int(store)) == E.get_quantized_vector_size_from_params(qa.VectorParameters(p, 0, D.Dot, False), store)
    assert two == m.row_bytes(2 * p, int(store))
    # the plain encodings are as they were
    assert E.get_quantized_vector_size_from_params(vp, store) == m.row_bytes(dim, int(store))
    assert E.get_quantized_vector_size_from_params(vp, store, B.TwoBits) == m.row_bytes(2 * dim, int(store))
