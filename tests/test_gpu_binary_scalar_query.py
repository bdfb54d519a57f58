"""Scalar (4- and 8-bit) queries against binary rows, bit for bit against a numpy restatement.

The reference has no such query, so the definition is restated here (np_encode, np_planes, np_scores) and every
comparison is exact: the codes are single f32 operations in a fixed order, the scores integers below 2^24.  Rows come from
the store's own encoder (Gaussian f32 data with a few +0.0 and -0.0) and are read back with storage_bytes(), so numpy
works on the very bits the kernels scan.

Kernel routes (csrc/bin.hip): dims up to 64 have 4- and 8-byte rows (bin_words_kernel for the scan, the dword form of
bin_pairs_kernel), 8192 + 130 has more than 64 16-byte pieces (bin_words_kernel again), 1024 is the exact-fit
bin_scan_kernel, 387 and 2065 its masked tail, 3000 / 5000 / 8000 its two, three and four pieces per lane.
"""
import numpy as np
import pytest

from util import assert_bits_equal, topk_want

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
D = qa.DistanceType
U8, U128 = qa.BitsStoreType.U8, qa.BitsStoreType.U128

DIMS = (1, 8, 32, 33, 64, 65, 128, 129, 387, 1024, 2065)
ROUTE_DIMS = (3000, 5000, 8000, 8192 + 130)
METRICS = [(dist, inv) for dist in (D.Dot, D.L1, D.L2) for inv in (False, True)]
POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)


# ------------------------------------------------------------------ the definition, in numpy
def np_encode(q, bits):
    """Codes c_i and a = max |q_i| over the finite entries; every operation a single f32 one."""
    q = np.asarray(q, dtype=np.float32)
    L = (1 << bits) - 1
    fin = np.isfinite(q)
    a = np.float32(np.abs(q[fin]).max()) if fin.any() else np.float32(0.0)
    if a == 0:
        c = np.full(q.shape, (L + 1) // 2, dtype=np.uint32)
    else:
        scale = np.float32(L) / np.float32(a + a)
        v = np.where(fin, q, np.float32(0.0)).astype(np.float32)  # NaN counts as 0; the infinities are set below
        t = ((v + a).astype(np.float32) * scale).astype(np.float32)
        c = np.minimum(L, (t + np.float32(0.5)).astype(np.float32).astype(np.uint32)).astype(np.uint32)
    c[q == np.inf] = L
    c[q == -np.inf] = 0
    return c, a


def np_planes(c, nb, bits):
    """Plane b = bit b of every code, bit i in byte i / 8 at position i % 8, zero pad bits; plane 0 first."""
    out = np.zeros((bits, nb), dtype=np.uint8)
    for b in range(bits):
        packed = np.packbits(((c >> b) & 1).astype(np.uint8), bitorder="little")
        out[b, :packed.size] = packed
    return out


def np_metric(x, dim_l, dist, invert):
    """calculate_metric (encoded_vectors_binary.rs:237-252) on X with dim * L in place of dim, in f32."""
    xor = x.astype(np.float32)
    zeros = (np.float32(dim_l) - xor).astype(np.float32)
    zx = (dist == D.Dot) != bool(invert)
    return (zeros - xor if zx else xor - zeros).astype(np.float32)


def np_scores(rows, planes, dim, dist, invert):
    bits = planes.shape[0]
    x = np.zeros(rows.shape[0], dtype=np.uint32)
    for b in range(bits):
        x += POP[rows ^ planes[b][None, :]].sum(axis=1, dtype=np.uint32) << np.uint32(b)
    return np_metric(x, dim * ((1 << bits) - 1), dist, invert)


# ------------------------------------------------------------------ data
def gaussian(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size >= 8:
        at = rng.choice(flat.size, size=max(2, flat.size // 50), replace=False)
        flat[at[::2]] = 0.0
        flat[at[1::2]] = -0.0
    return x


_stores = {}


def store(dim, n=128, kind=U8):
    """(handle for Dot / not inverted, rows as stored, the f32 data), encoded once per shape."""
    key = (dim, n, int(kind))
    if key not in _stores:
        data = gaussian(np.random.default_rng(dim * 7 + n), (n, dim))
        enc = qa.EncodedVectorsBin.encode(data, qa.VectorParameters(dim, n, D.Dot, False), store=kind)
        _stores[key] = (enc, enc.storage_bytes(), data)
    return _stores[key]


def with_metric(rows, dim, dist, invert, kind=U8):
    return qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(dim, rows.shape[0], dist, invert), store=kind)


def query_of(dim, seed=0):
    return gaussian(np.random.default_rng(1000 + dim + seed), (dim,))


def check_encoding(enc, nb, query, bits, what):
    q = enc.encode_query(query, query_bits=bits)
    c, a = np_encode(query, bits)
    assert q.bits == bits, what
    assert_bits_equal(q.max_abs, a, f"{what}: max_abs")
    got = q.encoded_vector
    assert got.shape == (bits, nb), what
    assert np.array_equal(got, np_planes(c, nb, bits)), f"{what}: planes differ"
    return q


# ------------------------------------------------------------------ encoding
@pytest.mark.parametrize("dim,kind", [(d, U8) for d in DIMS] + [(d, U128) for d in (1, 387, 1024)])
def test_encoding_equals_numpy(dim, kind):
    enc, rows, _ = store(dim, kind=kind)
    query = query_of(dim)
    for bits in (4, 8):
        check_encoding(enc, rows.shape[1], query, bits, f"dim {dim} {kind.name} bits {bits}")
    one = enc.encode_query(query, query_bits=1)
    plain = enc.encode_query(query)
    assert one.bits == 1 and plain.bits == 1 and one.max_abs == 0 and plain.max_abs == 0
    assert one.encoded_vector.shape == (rows.shape[1],)
    assert np.array_equal(one.encoded_vector, plain.encoded_vector)


@pytest.mark.parametrize("bits", [4, 8])
def test_encoding_edge_cases(bits):
    torch = pytest.importorskip("torch")
    dim = 387
    enc, rows, _ = store(dim)
    nb = rows.shape[1]
    L = (1 << bits) - 1
    # all zero (both signs): every code (L + 1) / 2
    zero = np.zeros(dim, dtype=np.float32)
    zero[1::2] = -0.0
    q = check_encoding(enc, nb, zero, bits, "all-zero query")
    assert np.array_equal(q.encoded_vector, np_planes(np.full(dim, (L + 1) // 2, dtype=np.uint32), nb, bits))
    # nothing finite: a = 0, NaN takes the middle code, the infinities the ends
    odd = np.full(dim, np.nan, dtype=np.float32)
    odd[3], odd[4] = np.inf, -np.inf
    check_encoding(enc, nb, odd, bits, "no finite entry")
    # NaN, +inf, -inf and -0.0 among finite values
    mixed = query_of(dim, 1)
    mixed[[0, 64, 65, 200, 386]] = [np.nan, np.inf, -np.inf, -0.0, np.nan]
    c, _ = np_encode(mixed, bits)
    assert c[64] == L and c[65] == 0 and c[0] == c[200]
    check_encoding(enc, nb, mixed, bits, "NaN / inf / -0.0")
    # t + 0.5 exactly on an integer, and one f32 to either side of such a value
    for a in (np.float32(1.0), np.float32(3.0), np.float32(0.7)):
        scale = np.float32(L) / np.float32(a + a)
        ks = np.arange(1, L + 1, max(1, L // 40), dtype=np.float32)
        mid = ((ks - np.float32(0.5)) / scale - a).astype(np.float32)
        vals = np.concatenate([mid, np.nextafter(mid, np.float32(-4)), np.nextafter(mid, np.float32(4)),
                               np.float32([a, -a, 0.0])]).astype(np.float32)[:dim]
        ties = np.zeros(dim, dtype=np.float32)
        ties[:vals.size] = np.clip(vals, -a, a)
        ties[dim - 1] = a
        t = (ties + a) * scale + np.float32(0.5)
        if a == 1.0:
            assert np.count_nonzero(t == np.floor(t)) > 10  # the exact ties are really there
        check_encoding(enc, nb, ties, bits, f"ties at a = {a}")
    # a device-resident query gives the same planes as the host one
    host = enc.encode_query(mixed, query_bits=bits)
    dev = enc.encode_query(torch.from_numpy(mixed).cuda(), query_bits=bits)
    assert np.array_equal(host.encoded_vector, dev.encoded_vector)
    assert_bits_equal(host.max_abs, dev.max_abs, "max_abs, device query")


def test_one_handle_across_8_1_4_bits():
    dim = 129
    enc, rows, _ = store(dim)
    nb = rows.shape[1]
    q8, q1, q4 = query_of(dim, 8), query_of(dim, 1), query_of(dim, 4)
    h = enc.encode_query(q8, query_bits=8)
    assert np.array_equal(h.encoded_vector, np_planes(np_encode(q8, 8)[0], nb, 8))
    s8 = enc.score_all(h)
    assert enc.encode_query(q1, reuse=h, query_bits=1) is h
    assert h.bits == 1 and h.max_abs == 0
    plain = enc.encode_query(q1)
    assert np.array_equal(h.encoded_vector, plain.encoded_vector)
    assert_bits_equal(enc.score_all(h), enc.score_all(plain), "binary scores through a handle that held 8 planes")
    enc.encode_query(q4, reuse=h, query_bits=4)
    assert h.bits == 4
    p4 = np_planes(np_encode(q4, 4)[0], nb, 4)
    assert np.array_equal(h.encoded_vector, p4)
    assert_bits_equal(enc.score_all(h), np_scores(rows, p4, dim, D.Dot, False), "4-bit scores after 8 and 1")
    enc.encode_query(q8, reuse=h, query_bits=8)
    assert_bits_equal(enc.score_all(h), s8, "8-bit scores again")


# ------------------------------------------------------------------ scores
@pytest.mark.parametrize("dim", DIMS + ROUTE_DIMS)
def test_scores_equal_numpy(dim):
    base, rows, _ = store(dim)
    n, nb = rows.shape
    query = query_of(dim)
    internal = [base.score_internal(3, 77), base.score_internal(127, 0)]
    planes = {bits: np_planes(np_encode(query, bits)[0], nb, bits) for bits in (4, 8)}
    for dist, inv in METRICS:
        enc = base if (dist, inv) == (D.Dot, False) else with_metric(rows, dim, dist, inv)
        for bits in (4, 8):
            what = f"dim {dim} {dist.name} invert={inv} bits {bits}"
            q = enc.encode_query(query, query_bits=bits)
            want = np_scores(rows, planes[bits], dim, dist, inv)
            got = enc.score_all(q)
            assert_bits_equal(got, want, f"{what}: score_all")
            for i in (0, 77, 127):
                assert_bits_equal(enc.score_point(q, i), got[i], f"{what}: score_point({i})")
            ids = np.array([5, 5, 127, 0], dtype=np.uint32)
            assert_bits_equal(enc.score_ids(q, ids), got[ids], f"{what}: score_ids")
    assert_bits_equal([base.score_internal(3, 77), base.score_internal(127, 0)], internal,
                      "score_internal after scalar queries")
    assert_bits_equal(internal[0], np_scores(rows[77:78], rows[3:4], dim, D.Dot, False), "score_internal is one plane")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_row_count_tails(n):
    dim = 1024
    enc, rows, _ = store(dim, n=n)
    query = query_of(dim, n)
    for bits in (4, 8):
        q = enc.encode_query(query, query_bits=bits)
        want = np_scores(rows, np_planes(np_encode(query, bits)[0], rows.shape[1], bits), dim, D.Dot, False)
        assert_bits_equal(enc.score_all(q), want, f"{n} rows, bits {bits}")
        assert_bits_equal(enc.score_point(q, n - 1), want[n - 1], f"{n} rows, bits {bits}: last row")


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dim", [33, 387, 1024])
def test_known_answers(dim, bits):
    L = (1 << bits) - 1
    n = 128
    rng = np.random.default_rng(dim + bits)
    # every row all-positive: score = sum(2 c_i - L)
    ones = qa.EncodedVectorsBin.encode(np.abs(rng.standard_normal((n, dim))).astype(np.float32) + 1.0,
                                       qa.VectorParameters(dim, n, D.Dot, False))
    query = query_of(dim, bits)
    c, _ = np_encode(query, bits)
    total = int((2 * c.astype(np.int64) - L).sum())
    assert_bits_equal(ones.score_all(ones.encode_query(query, query_bits=bits)), np.full(n, total, dtype=np.float32),
                      "all-positive rows")
    # a query of +-a only: codes 0 or L, score = L x the binary score
    enc, rows, _ = store(dim)
    a = np.float32(0.37)
    pm = np.where(rng.random(dim) < 0.5, -a, a).astype(np.float32)
    c, _ = np_encode(pm, bits)
    assert set(np.unique(c)) <= {0, L}
    binary = enc.score_all(enc.encode_query(pm))
    assert_bits_equal(enc.score_all(enc.encode_query(pm, query_bits=bits)), (np.float32(L) * binary).astype(np.float32),
                      "+-a query against the binary score")


def test_largest_values():
    """dim 65 792 at 8 bits: X reaches dim * L = 16 776 960, still an exact f32."""
    dim, n, L = 65_792, 128, 255
    rows = np.full((n, dim // 8), 0xFF, dtype=np.uint8)
    rows[1::2, 5] = 0xFE  # every other row has one zero bit
    enc = qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(dim, n, D.Dot, False))
    all_l = np.full(dim, np.inf, dtype=np.float32)    # every code L: X = 0 on the all-ones rows
    all_0 = np.full(dim, -np.inf, dtype=np.float32)   # every code 0: X = dim * L
    for query, sign in ((all_l, 1), (all_0, -1)):
        q = enc.encode_query(query, query_bits=8)
        planes = q.encoded_vector
        assert np.all(planes == (0xFF if sign > 0 else 0))
        got = enc.score_all(q)
        want = np.where(np.arange(n) % 2 == 0, dim * L, dim * L - 2 * L).astype(np.float64) * sign
        assert want.max() <= 16_776_960 and abs(want[0]) == 16_776_960
        assert_bits_equal(got, want.astype(np.float32), f"all-ones rows, sign {sign}")
        assert_bits_equal(got, np_scores(rows, planes, dim, D.Dot, False), "against the restatement")
        assert_bits_equal(enc.score_point(q, 1), got[1], "score_point")
        ids, sc = enc.topk(q, 3, largest=sign > 0)
        assert list(ids) == [0, 2, 4] and np.all(np.abs(sc) == 16_776_960)
    vp = qa.VectorParameters(65_793, 2, D.Dot, False)
    nb = qa.EncodedVectorsBin.get_quantized_vector_size_from_params(vp)
    wide = qa.EncodedVectorsBin.from_storage(np.zeros((2, nb), dtype=np.uint8), vp)
    with pytest.raises(qa.EncodingError) as e:
        wide.encode_query(np.ones(65_793, dtype=np.float32), query_bits=8)
    assert e.value.kind == "ArgumentsError"
    assert wide.encode_query(np.ones(65_793, dtype=np.float32), query_bits=4).bits == 4  # 4 bits reach 1 118 481


# ------------------------------------------------------------------ top-k
def _topk_same(enc, q, want_scores, k, what):
    for largest in (True, False):
        ids, sc = enc.topk(q, k, largest=largest)
        wi, ws = topk_want(want_scores, k, largest)
        assert np.array_equal(ids, wi), f"{what} k={k} largest={largest}: ids differ"
        assert_bits_equal(sc, ws, f"{what} k={k} largest={largest}")


def _random_rows_store(n, dim, seed, dist=D.Dot):
    """Random bits in the store's own row size (640 bytes at dim 5000, not 625), pad bits zero as the encoder leaves them."""
    vp = qa.VectorParameters(dim, n, dist, False)
    nb = qa.EncodedVectorsBin.get_quantized_vector_size_from_params(vp)
    bits = np.random.default_rng(seed).integers(0, 2, size=(n, dim), dtype=np.uint8)
    rows = np.zeros((n, nb), dtype=np.uint8)
    packed = np.packbits(bits, axis=1, bitorder="little")
    rows[:, :packed.shape[1]] = packed
    return qa.EncodedVectorsBin.from_storage(rows, vp), rows


@pytest.mark.parametrize("n,dim,ks,route", [
    (3_000, 256, (10, 64), "one launch"),       # bin_topk_small_kernel: n <= 2M, k <= 64, 16-byte pieces
    (3_000, 5000, (10,), "long rows: classic"),  # planes on rows of more than 16 pieces skip the one-launch kernel
    (32_768, 1024, (100,), "fused filter"),     # fused_policy (topk.hip): n >= 32768 and r = ceil(2048 * 512 / n) = 32 <= 64
    (98_304, 256, (1024,), "fused filter"),     # k = 1024: r = ceil(2048 * 3072 / n) <= 64 from 98 304 rows on
])
def test_topk_routes(n, dim, ks, route):
    enc, rows = _random_rows_store(n, dim, n + dim)
    query = query_of(dim, n)
    for bits in (4, 8):
        q = enc.encode_query(query, query_bits=bits)
        want = np_scores(rows, np_planes(np_encode(query, bits)[0], rows.shape[1], bits), dim, D.Dot, False)
        for k in ks:
            _topk_same(enc, q, want, k, f"{route} {n}x{dim} bits {bits}")


def test_topk_classic_route_dim_33():
    """8-byte rows have no 16-byte pieces: the score array (bin_words_kernel) and the exact radix select."""
    n, dim = 3_000, 33
    data = gaussian(np.random.default_rng(33), (n, dim))
    enc = qa.EncodedVectorsBin.encode(data, qa.VectorParameters(dim, n, D.L2, False))
    rows = enc.storage_bytes()
    query = query_of(dim)
    for bits in (4, 8):
        q = enc.encode_query(query, query_bits=bits)
        want = np_scores(rows, np_planes(np_encode(query, bits)[0], rows.shape[1], bits), dim, D.L2, False)
        for k in (10, 100):
            _topk_same(enc, q, want, k, f"classic dim 33 bits {bits}")


def test_topk_heavy_ties():
    """4 096 rows drawn from 8 bit patterns: 8 distinct scores, ties go to the lower id (k <= 64 the one-launch kernel,
    k = 100 the classic path at this count)."""
    n, dim = 4_096, 128
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 256, size=(8, dim // 8), dtype=np.uint8)[rng.integers(0, 8, size=n)]
    enc = qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(dim, n, D.Dot, False))
    query = query_of(dim, 8)
    for bits in (4, 8):
        q = enc.encode_query(query, query_bits=bits)
        want = np_scores(rows, np_planes(np_encode(query, bits)[0], rows.shape[1], bits), dim, D.Dot, False)
        assert np.unique(want).size <= 8
        for k in (10, 64, 100):
            _topk_same(enc, q, want, k, f"heavy ties bits {bits}")


@pytest.mark.parametrize("bits", [4, 8])
def test_topk_rescored_equals_rerank_of_the_candidates(bits):
    n, dim, k, cand = 2_000, 128, 10, 100
    data = gaussian(np.random.default_rng(2000), (n, dim))
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    enc = qa.EncodedVectorsBin.encode(data, vp)
    orig = qa.OriginalVectors.from_data(data, vp)
    query = query_of(dim, bits)
    q = enc.encode_query(query, query_bits=bits)
    for largest in (True, False):
        ids, _ = enc.topk(q, cand, largest=largest)
        wi, ws = orig.rerank(query, ids, k, largest=largest)
        gi, gs = enc.topk_rescored(q, orig, query, k, cand, largest=largest)
        assert np.array_equal(gi, wi), f"bits {bits} largest={largest}"
        assert_bits_equal(gs, ws, f"bits {bits} largest={largest}: rescored scores")


# ------------------------------------------------------------------ errors
def test_errors():
    enc, rows, _ = store(387)
    query = query_of(387)
    for bits in (0, 2, 16):
        with pytest.raises(qa.EncodingError) as e:
            enc.encode_query(query, query_bits=bits)
        assert e.value.kind == "ArgumentsError", bits
    other, _, _ = store(1024)
    q = other.encode_query(query_of(1024), query_bits=8)
    for call in (lambda: enc.score_all(q), lambda: enc.score_point(q, 0), lambda: enc.topk(q, 5),
                 lambda: enc.score_ids(q, np.array([1], dtype=np.uint32))):
        with pytest.raises(qa.EncodingError) as e:
            call()
        assert e.value.kind == "ArgumentsError"
