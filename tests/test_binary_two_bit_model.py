"""Two-bit binary rows without a GPU: the host-only threshold arithmetic against the numpy model bit for
bit, row sizes, the argument errors and load refusals that are made before a device is needed, and the model's own
properties (Hamming distance = level difference; better recall than one bit on the specification's recipe)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import two_bit_model as m

import quantization_amd as qa
from quantization_amd import _lib

E = qa.EncodedVectorsBin
D = qa.DistanceType
S = qa.BitsStoreType
ONE, TWO = 0, 1


def _bits(a):
    a = np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_header_declares_and_library_exports_the_entry_points():
    new = ["qamd_bin_quantized_vector_size_enc", "qamd_bin_find_stats", "qamd_bin_thresholds_from_stats",
           "qamd_bin_encode_enc", "qamd_bin_encoder_begin_enc", "qamd_bin_encoder_observe", "qamd_bin_from_rows_enc",
           "qamd_bin_get_encoding", "qamd_bin_get_thresholds"]
    declared = set(_lib.declared_symbols())
    L = _lib.lib()
    assert not [s for s in new if s not in declared or not hasattr(L, s)]


def _stat_cases():
    f = np.float32
    big = np.array([3e38, -3e38, 3e38, 3e38], dtype=f).astype(np.float64)
    const = np.full(1000, f(0.1)).astype(np.float64)
    den = np.array([1e-45, 3e-45, -1e-45], dtype=f).astype(np.float64)
    cases = {
        "n0": (0, 0.0, 0.0),
        "n1": (1, 2.5, 6.25),
        "const_0.1f": (1000, np.cumsum(const)[-1], np.cumsum(const * const)[-1]),
        "pm3e38": (4, np.cumsum(big)[-1], np.cumsum(big * big)[-1]),
        "plus3e38": (3, 9e38, 3 * 9e76),
        "denormal": (3, np.cumsum(den)[-1], np.cumsum(den * den)[-1]),
        "f64_denormal_sums": (7, 5e-324, 1e-323),
        "ordinary": (4097, 123.456, 9876.5),
        "negative_var": (3, 3.0000000000000004, 3.0),
    }
    n = np.array([c[0] for c in cases.values()], dtype=np.uint64)
    s = np.array([c[1] for c in cases.values()], dtype=np.float64)
    q = np.array([c[2] for c in cases.values()], dtype=np.float64)
    return list(cases), n, s, q


@pytest.mark.parametrize("t", [0.0, 0.43, 2.0])
def test_thresholds_from_stats_is_the_model_bit_for_bit(t):
    names, n, s, q = _stat_cases()
    lo, hi = E.thresholds_from_stats(n, s, q, t)
    wlo, whi = m.thresholds(n, s, q, t)
    for i, name in enumerate(names):
        assert _bits(lo)[i] == _bits(wlo)[i] and _bits(hi)[i] == _bits(whi)[i], (name, t, lo[i], wlo[i], hi[i], whi[i])
    k = names.index("const_0.1f")
    assert lo[k] <= hi[k]
    k = names.index("negative_var")  # the rounded variance is below zero: clamped, lo == hi == mean
    assert _bits(lo)[k] == _bits(hi)[k]
    k = names.index("n0")
    assert _bits(lo)[k] == 0 and _bits(hi)[k] == 0
    if t == 0.0:
        assert np.array_equal(_bits(lo), _bits(hi))


def test_constant_column_of_point_one_clamps():
    x = np.full((1000, 1), np.float32(0.1))
    n, s, q = m.stats(x)
    for t in (0.43, 2.0):
        lo, hi = E.thresholds_from_stats(n, s, q, t)
        wlo, whi = m.thresholds(n, s, q, t)
        assert _bits(lo)[0] == _bits(wlo)[0] and _bits(hi)[0] == _bits(whi)[0]
        assert lo[0] <= np.float32(0.1) <= hi[0] or lo[0] == hi[0]


@pytest.mark.parametrize("dim", [0, 1, 16, 17, 32, 33, 64, 65, 100, 387, 768, 1024])
@pytest.mark.parametrize("store", [S.U8, S.U128])
def test_row_sizes(dim, store):
    vp = qa.VectorParameters(dim, 0, D.Dot, False)
    two = E.get_quantized_vector_size_from_params(vp, store, qa.BinaryEncoding.TwoBits)
    assert two == m.row_bytes(2 * dim, int(store))
    # = the existing one-bit size of a vector of 2 dim dimensions; the one-bit size itself is unchanged
    assert two == E.get_quantized_vector_size_from_params(qa.VectorParameters(2 * dim, 0, D.Dot, False), store)
    assert E.get_quantized_vector_size_from_params(vp, store) == m.row_bytes(dim, int(store))
    assert E.get_quantized_vector_size_from_params(vp, store, qa.BinaryEncoding.OneBit) == m.row_bytes(dim, int(store))


def _vp(dim, count):
    return _lib.VectorParametersC(dim, count, int(D.Dot), 0)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _entry_points(dim, data, lo, hi, encoding):
    """The three calls that take thresholds, each with the same arguments; they must refuse before touching a device."""
    L = _lib.lib()
    vp = _vp(dim, 4)
    none_stop = _lib.STOP_FN(0)
    out = C.c_void_p()
    yield "encode_enc", L.qamd_bin_encode_enc(_ptr(data), _lib.MEM_HOST, C.byref(vp), 0, encoding, lo, hi, none_stop, None, None,
                                              C.byref(out))
    yield "encoder_begin_enc", L.qamd_bin_encoder_begin_enc(C.byref(vp), 0, encoding, lo, hi, none_stop, None, None, C.byref(out))
    rows = np.zeros(4 * 64, dtype=np.uint8)
    yield "from_rows_enc", L.qamd_bin_from_rows_enc(_ptr(rows), _lib.MEM_HOST, C.byref(vp), 0, encoding, lo, hi, None, C.byref(out))


def test_argument_errors_before_a_device_is_needed():
    dim = 8
    data = np.zeros((4, dim), dtype=np.float32)
    lo, hi = np.full(dim, -1, np.float32), np.full(dim, 1, np.float32)
    nan = lo.copy()
    nan[3] = np.nan
    above = lo.copy()
    above[5] = 2.0
    cases = {
        "lo alone": (_ptr(lo), None, TWO),
        "hi alone": (None, _ptr(hi), TWO),
        "NaN lo": (_ptr(nan), _ptr(hi), TWO),
        "NaN hi": (_ptr(lo), _ptr(nan), TWO),
        "lo > hi": (_ptr(above), _ptr(hi), TWO),
        "thresholds with one bit": (_ptr(lo), _ptr(hi), ONE),
        "unknown encoding": (None, None, 2),
    }
    for what, (plo, phi, enc) in cases.items():
        for name, st in _entry_points(dim, data, plo, phi, enc):
            assert st == _lib.ERR_ARGUMENTS, (what, name, st)
    L = _lib.lib()
    out = C.c_void_p()
    vp = _vp(dim, 4)  # two-bit rows from storage cannot do without thresholds
    assert L.qamd_bin_from_rows_enc(_ptr(np.zeros(64, np.uint8)), _lib.MEM_HOST, C.byref(vp), 0, TWO, None, None, None,
                                    C.byref(out)) == _lib.ERR_ARGUMENTS
    big = _vp((1 << 23) + 1, 0)  # past 2^23 dimensions a score is no exact f32 integer any more
    assert L.qamd_bin_encode_enc(None, _lib.MEM_HOST, C.byref(big), 0, TWO, None, None, _lib.STOP_FN(0), None, None,
                                 C.byref(out)) == _lib.ERR_ARGUMENTS
    assert L.qamd_bin_encoder_begin_enc(C.byref(big), 0, TWO, None, None, _lib.STOP_FN(0), None, None,
                                        C.byref(out)) == _lib.ERR_ARGUMENTS
    assert out.value is None


def _meta(tmp_path, name, obj):
    p = tmp_path / name
    p.write_text(obj if isinstance(obj, str) else json.dumps(obj))
    return p


def test_load_refusals_before_a_device_is_needed(tmp_path):
    dim, count = 4, 2
    vpj = {"dim": dim, "count": count, "distance_type": "Dot", "invert": False}
    data = tmp_path / "rows.bin"
    data.write_bytes(bytes(count * m.row_bytes(2 * dim, 0)))
    ok = {"lo": [0.0] * dim, "hi": [1.0] * dim}
    bad = {
        "unknown encoding": {"vector_parameters": vpj, "encoding": "ThreeBits", "thresholds": ok},
        "encoding of another type": {"vector_parameters": vpj, "encoding": 2, "thresholds": ok},
        "no thresholds": {"vector_parameters": vpj, "encoding": "TwoBits"},
        "no hi": {"vector_parameters": vpj, "encoding": "TwoBits", "thresholds": {"lo": ok["lo"]}},
        "short lo": {"vector_parameters": vpj, "encoding": "TwoBits", "thresholds": {"lo": [0.0] * (dim - 1), "hi": ok["hi"]}},
        "long hi": {"vector_parameters": vpj, "encoding": "TwoBits", "thresholds": {"lo": ok["lo"], "hi": [1.0] * (dim + 1)}},
        "lo > hi": {"vector_parameters": vpj, "encoding": "TwoBits", "thresholds": {"lo": [0.0, 0.0, 2.0, 0.0], "hi": ok["hi"]}},
        "not numbers": {"vector_parameters": vpj, "encoding": "TwoBits", "thresholds": {"lo": [None] * dim, "hi": ok["hi"]}},
    }
    L = _lib.lib()
    vp = _vp(dim, count)
    for what, obj in bad.items():
        out = C.c_void_p()
        st = L.qamd_bin_load(os.fsencode(data), os.fsencode(_meta(tmp_path, "meta.json", obj)), C.byref(vp), 0, C.byref(out))
        assert st == _lib.ERR_IO, (what, st, L.qamd_last_error())
        assert out.value is None


def test_hamming_distance_is_the_level_difference():
    lo, hi = np.float32([0.0]), np.float32([1.0])
    xs = np.float32([-1.0, 0.5, 2.0])  # levels 0, 1, 2
    assert list(m.levels(xs, lo, hi)) == [0, 1, 2]
    for store in (m.U8, m.U128):
        codes = [m.encode([[x]], lo, hi, store) for x in xs]
        for a in range(3):
            for b in range(3):
                assert m.xor_count(codes[a], codes[b])[0] == abs(a - b), (a, b)
    # and over a whole row the counts add up per dimension
    rng = np.random.default_rng(5)
    lo, hi = np.float32(rng.normal(size=37) - 0.5), None
    hi = lo + np.float32(rng.random(37))
    a, b = np.float32(rng.normal(size=37)), np.float32(rng.normal(size=37))
    want = np.abs(m.levels(a, lo, hi) - m.levels(b, lo, hi)).sum()
    assert m.xor_count(m.encode(a, lo, hi, m.U8), m.encode(b, lo, hi, m.U8))[0] == want


def _recall(seed, n=4000, dim=256, n_queries=100, k=10):
    """The specification's recipe: columns of unequal scale, queries = a stored row plus noise, all normalised; the
    top-10 by xor count against the exact dot-product top-10, stable sorts on both sides."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.3, 1.5, size=dim)
    data = (rng.normal(size=(n, dim)) * scale).astype(np.float32)
    picks = rng.integers(0, n, size=n_queries)
    queries = (data[picks] + 0.5 * rng.normal(size=(n_queries, dim))).astype(np.float32)
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    exact = np.argsort(-(queries.astype(np.float64) @ data.astype(np.float64).T), axis=1, kind="stable")[:, :k]
    lo, hi = m.thresholds(*m.stats(data), 0.43)
    zero = np.zeros(dim, dtype=np.float32)
    two_rows, two_q = m.encode(data, lo, hi, m.U8), m.encode(queries, lo, hi, m.U8)
    one_rows = np.packbits(data > zero, axis=1, bitorder="little")
    one_q = np.packbits(queries > zero, axis=1, bitorder="little")
    hits = {"one": 0, "two": 0}
    for qi in range(n_queries):
        for name, rows, q in (("one", one_rows, one_q[qi]), ("two", two_rows, two_q[qi])):
            got = np.argsort(m.xor_count(rows, q), kind="stable")[:k]
            hits[name] += len(set(got.tolist()) & set(exact[qi].tolist()))
    return hits["one"] / (n_queries * k), hits["two"] / (n_queries * k)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_bits_recall_more_than_one_bit(seed):
    one, two = _recall(seed)
    print(f"seed {seed}: recall@10 one-bit {one:.3f}, two-bit (t = 0.43) {two:.3f}")
    assert two > one
