"""Small helpers shared by the parity tests."""
import numpy as np


def bits(a) -> np.ndarray:
    """f32 array -> its bit patterns (bit-exact comparisons; NaN-safe)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits_equal(got, want, what=""):
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        i = int(bad[0])
        raise AssertionError(
            f"{what}: {bad.size}/{g.size} values differ; first at {i}: "
            f"got {np.asarray(got, dtype=np.float32).ravel()[i]!r} want {np.asarray(want, dtype=np.float32).ravel()[i]!r}")


def topk_want(scores, k: int, largest: bool = True):
    """The top-k contract of include/quantization_amd.h restated on a whole-store score array: the stable best k (ties to
    the lower row id), best first, padded to k as every entry point pads when the store has fewer rows: ids 0xFFFFFFFF,
    scores -inf for `largest`, +inf otherwise.  Returns (ids u32[k], scores f32[k])."""
    scores = np.asarray(scores, dtype=np.float32)
    n = scores.size
    key = -scores if largest else scores
    cand = np.arange(n)
    if 0 < k < n:  # only the rows at least as good as the k-th best (ties included) need the stable sort
        cand = np.flatnonzero(key <= np.partition(key, k - 1)[k - 1])
    order = cand[np.lexsort((cand, key[cand]))][: min(k, n)]
    ids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    sc = np.full(k, -np.inf if largest else np.inf, dtype=np.float32)
    ids[: order.size] = order
    sc[: order.size] = scores[order]
    return ids, sc


def topk_order_keys(scores, largest: bool = True) -> np.ndarray:
    """uint32 sort keys of f32 scores in the total order every top-k route uses on the bit pattern: ascending
    -NaN < -inf < negative finite < -0 < +0 < positive finite < +inf < +NaN, inverted for `largest`; the smallest key is
    the best row.  Among NaNs of one sign the payload counts like a magnitude."""
    u = bits(scores).ravel().copy()
    u ^= np.where(u >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)
    return ~u if largest else u


def topk_total_order(scores, k: int, largest: bool = True):
    """topk_want on the bit patterns instead of the float values: a stable sort on (topk_order_keys, row id), best first,
    padded to k exactly as topk_want pads.  It states what topk_want cannot: where NaNs of either sign and payload rank,
    and that -0 is below +0.  Returned scores are the rows' own bits.  Returns (ids u32[k], scores f32[k])."""
    scores = np.ascontiguousarray(scores, dtype=np.float32).ravel()
    n = scores.size
    key = topk_order_keys(scores, largest)
    cand = np.arange(n)
    if 0 < k < n:  # only the rows whose key is at most the k-th smallest (ties included) need the stable sort
        cand = np.flatnonzero(key <= np.partition(key, k - 1)[k - 1])
    order = cand[np.argsort(key[cand], kind="stable")][: min(k, n)]
    ids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    sc = np.full(k, -np.inf if largest else np.inf, dtype=np.float32)
    ids[: order.size] = order
    sc[: order.size] = scores[order]
    return ids, sc


# The u8 batch shapes of tests/test_gpu_topk_special_scores.py: (kernel family of the filter pass on 256 CUs, rows, dim,
# queries), the smallest store that reaches each family.  Stores below 131072 rows of up to 896 code bytes take rs at every
# batch size; from 131072 rows on: 16 .. 208 bytes qs16 from 385 queries; 256 bytes rq16 from 129; 768 bytes rk16 at
# 129 .. 192 and qr16 at 193 .. 256; 1024-byte rows of a small store pp from 65 queries.  SPECIAL_U8_GEMM_SHAPE at
# multiplier 0 or inf takes u8_gemm_kernel.  tests/test_topk_order_model.py checks all of this against u8_gemm_route().
SPECIAL_U8_FAMILIES = [
    ("rs", 33_000, 64, 5),
    ("pp", 33_000, 1024, 70),
    ("qs16", 131_079, 16, 385),
    ("rq16", 131_079, 256, 129),
    ("rk16", 131_079, 768, 129),
    ("qr16", 131_079, 768, 193),
]
SPECIAL_U8_GEMM_SHAPE = (33_000, 64, 5)
SPECIAL_U8_SHORT_ROW_BATCHES = [(2 ** 20 + 7, 32, 2), (2 ** 20 + 7, 32, 4)]  # rs: rows too short for the vector-ALU pass


# ------------------------------------------------------------------ u8 stores adopted from reference-format rows
# Shared by tests/test_gpu_u8_blocked.py and tests/test_gpu_u8_byte_kernels.py: the test owns every byte of the store.
U8_ALPHA = np.float32(1.0 / 127.0)


def u8_actual_dim(dim):
    return -(-dim // 16) * 16


def u8_multiplier(dist):
    return np.float32(U8_ALPHA * U8_ALPHA) if int(dist) == 0 else np.float32(np.float32(-2.0) * U8_ALPHA * U8_ALPHA)


def store_rows(dim, n, seed=0, codes=None):
    """Reference-format rows [vector_offset f32][codes] with uniform random codes 0..127 (or the given ones) and the
    query that goes with them."""
    ad = u8_actual_dim(dim)
    rng = np.random.default_rng(dim * 131 + n * 7 + seed)
    rows = np.zeros((n, ad + 4), dtype=np.uint8)
    rows[:, :4] = rng.standard_normal(n).astype(np.float32).view(np.uint8).reshape(n, 4)
    rows[:, 4:] = rng.integers(0, 128, size=(n, ad), dtype=np.uint8) if codes is None else codes
    query = rng.random(dim, dtype=np.float32)
    return rows, query


def qa_meta(dim, n, dist):
    """from_storage metadata of a Dot or L2 store (not inverted) at alpha 1 / 127, offset 0."""
    import quantization_amd as qa

    return {"actual_dim": u8_actual_dim(dim), "alpha": U8_ALPHA, "offset": np.float32(0.0), "multiplier": u8_multiplier(dist),
            "vector_parameters": qa.VectorParameters(dim, n, dist, False)}


def oracle_meta(qo, dim, n, dist):
    return qo.Meta(u8_actual_dim(dim), float(U8_ALPHA), 0.0, float(u8_multiplier(dist)), dim, n, int(dist), 0)


def oracle_metas(qo, dim, n, dist, invert):
    """(from_storage metadata, oracle Meta) of a store of any metric and `invert` at alpha 1 / 127, offset 0, as the
    reference's encoder writes them: taken from the oracle's encoder run on one zero vector, so that no formula is
    restated here."""
    import quantization_amd as qa

    _, meta = qo.u8_encode_with(np.zeros((1, dim), dtype=np.float32), int(dist), bool(invert), float(U8_ALPHA), 0.0)
    meta.count = n
    md = {"actual_dim": int(meta.actual_dim), "alpha": np.float32(meta.alpha), "offset": np.float32(meta.offset),
          "multiplier": np.float32(meta.multiplier),
          "vector_parameters": qa.VectorParameters(dim, n, qa.DistanceType(int(dist)), bool(invert))}
    return md, meta


def have_gpu() -> bool:
    try:
        from quantization_amd import _lib
        return _lib.lib().qamd_device_count() > 0
    except Exception:
        return False


def ref_differential_cases():
    """The seeded (dim, q, v) byte-row pairs test_oracle_golden fuzzes the oracle's pair kernels with; the reference's
    outputs for them are stored in tests/golden/ref_differential.npz (tests/golden/make_golden.py)."""
    rng = np.random.default_rng(7)
    cases = []
    for dim in (16, 48, 80, 768, 1536, 3072):
        for hi in (128, 256):
            for _ in range(25):
                q = rng.integers(0, hi, size=dim, dtype=np.uint8)
                v = rng.integers(0, hi, size=dim, dtype=np.uint8)
                cases.append((dim, q, v))
    return cases


def cases_digest(cases) -> str:
    """sha256 of every input byte of ref_differential_cases() (or wide_sum_cases()), in order: proves the stored
    outputs belong to them."""
    import hashlib

    h = hashlib.sha256()
    for *_tag_dim, q, v in cases:
        h.update(q.tobytes())
        h.update(v.tobytes())
    return h.hexdigest()


# Dims and code ranges of the random wide-sum pairs: from 2304 on the AVX2 order's two f32 half sums can pass 2^24
# (for codes <= 127 it is the exact sum rounded once up to actual_dim 2080).
WIDE_DOT_DIMS = (2304, 3072, 4096, 8192, 32768)
WIDE_DOT_LOWS = (64, 110)


def wide_dot_pair_2096():
    """A (q, v) pair at actual_dim 2096 -- the first actual_dim where the AVX2 order can differ from the exact sum
    rounded once -- on which it does.  q is 127 on the bytes of the even i32 lanes (b % 4 < 2: lanes 0, 2, 4, 6 of
    every 16-byte piece) and 0 elsewhere, v the same but for v[0] = 126: the even-lane half sum is 16903065, odd and
    above 2^24, and rounds (ties to even) to 16903064.  Byte 2 (an odd lane) is 1 in both, so the odd half is 1, and
    the AVX2 result rounds 16903064 + 1 down again; the exact sum 16903066 is an f32."""
    d = 2096
    even = (np.arange(d) % 4) < 2
    q = np.where(even, 127, 0).astype(np.uint8)
    v = q.copy()
    v[0] = 126
    q[2] = v[2] = 1
    return q, v


def wide_sum_cases():
    """Seeded (tag, dim, q, v) byte-row pairs whose sums reach past 2^24 (dot) or past a u16 lane (L1, from
    actual_dim 8272 on): the regime where impl_score_dot_avx / impl_score_l1_avx differ from the exact sum.  The
    reference's outputs for them are stored in tests/golden/ref_wide_sums.npz (tests/golden/make_golden.py).
    Tags: dot_* cases are scored with the dot kernels' eyes (codes up to 127), l1_* cases are built for L1."""
    rng = np.random.default_rng(2096)
    cases = []
    for lo in WIDE_DOT_LOWS:
        for dim in WIDE_DOT_DIMS:
            for _ in range(8 if dim < 4096 else 24):
                q = rng.integers(lo, 128, size=dim, dtype=np.uint8)
                v = rng.integers(lo, 128, size=dim, dtype=np.uint8)
                cases.append((f"dot_rand{lo}", dim, q, v))
    q, v = wide_dot_pair_2096()
    cases.append(("dot_edge2096", 2096, q, v))
    even = np.where((np.arange(2096) % 4) < 2, 127, 0).astype(np.uint8)
    cases.append(("dot_even127", 2096, even, even.copy()))
    for dim in (2080, 2096, 4096):
        full = np.full(dim, 127, dtype=np.uint8)
        cases.append(("dot_all127", dim, full, full.copy()))
    # L1: each u16 lane gets actual_dim / 16 differences; all-0 against all-127 is exact at 8256 (516 * 127 = 65532),
    # wraps first at 8272 (517 * 127 = 65659) and is 8064 instead of 1056640 at 8320
    for dim in (8256, 8272, 8320):
        cases.append(("l1_zero127", dim, np.zeros(dim, dtype=np.uint8), np.full(dim, 127, dtype=np.uint8)))
    for dim in (8320, 16384):
        for _ in range(6):
            q = rng.integers(110, 128, size=dim, dtype=np.uint8)
            v = rng.integers(0, 18, size=dim, dtype=np.uint8)
            cases.append(("l1_sat", dim, q, v))
    return cases


# ------------------------------------------------------------------ scalar queries against binary rows, per dimension
# DESIGN.md 3.2d read dimension by dimension: no bit planes, no popcounts.  Integers are int64; the only f32 steps are
# the ones the text names.  tests/test_binary_scalar_query_model.py checks this oracle without a GPU.
def scalar_codes(query, bits: int):
    """(codes uint32[dim], a float32) of a `bits`-bit scalar query: a = max |q_i| over the finite entries (0 when there
    is none); a == 0 -> every code (L + 1) / 2; else scale = (float)L / (a + a), NaN counts as 0.0f,
    t_i = (q_i + a) * scale, c_i = min(L, (uint32)(t_i + 0.5f)); last +inf -> L and -inf -> 0.  Single f32 operations."""
    f32 = np.float32
    q = np.asarray(query, dtype=f32).ravel()
    L = (1 << bits) - 1
    finite = np.isfinite(q)
    a = f32(np.abs(q[finite]).max()) if finite.any() else f32(0.0)
    codes = np.full(q.size, (L + 1) // 2, dtype=np.uint32)
    if a != 0:
        scale = f32(f32(L) / f32(a + a))
        v = np.where(finite, q, f32(0.0))  # NaN counts as 0.0f; the infinite entries are set below
        t = (v + a).astype(f32) * scale    # float32 arrays: numpy rounds each step to f32, element by element
        half = (t.astype(f32) + f32(0.5)).astype(f32)
        codes[:] = np.minimum(L, np.trunc(half).astype(np.int64))  # truncation; t + 0.5 >= 0.5
    codes[np.isposinf(q)] = L
    codes[np.isneginf(q)] = 0
    return codes, a


def scalar_codes_f64(query, bits: int):
    """The same codes in float64, floor((q + a) * L / (2a) + 0.5), over the finite entries; needs a > 0.
    Returns (codes int64[finite entries], t + 0.5 float64[finite entries], finite mask)."""
    q = np.asarray(query, dtype=np.float32).ravel()
    L = (1 << bits) - 1
    finite = np.isfinite(q)
    v = q[finite].astype(np.float64)
    a = np.abs(v).max()
    assert a > 0
    half = (v + a) * L / (2.0 * a) + 0.5
    return np.minimum(L, np.floor(half)).astype(np.int64), half, finite


def scalar_planes(codes, bits: int, nb: int) -> np.ndarray:
    """uint8[bits, nb]: the stored form of a scalar query - bit b of code i at bit i % 8 of byte i / 8 of plane b, zero
    pad bits - set one bit at a time."""
    out = np.zeros((bits, nb), dtype=np.uint8)
    for i, c in enumerate(np.asarray(codes).tolist()):
        for b in range(bits):
            if (c >> b) & 1:
                out[b, i // 8] |= 1 << (i % 8)
    return out


def scalar_xor(rows_u8, codes, dim: int, bits: int) -> np.ndarray:
    """int64[n]: X of every stored bit row.  Bit i of a row is byte i / 8, bit i % 8 (s_i in {0, 1});
    S = sum_i (2 s_i - 1)(2 c_i - L) and X = (dim * L - S) / 2, exact.  Only the first `dim` bits of a row are read.
    `codes` of shape [queries, dim] give int64[queries, n]: the same sum per query, the rows' bits taken apart once."""
    rows_u8 = np.asarray(rows_u8, dtype=np.uint8)
    n = rows_u8.shape[0]
    L = (1 << bits) - 1
    codes = np.asarray(codes, dtype=np.int64)
    centred = 2 * codes[..., :dim] - L
    assert centred.shape[-1] == dim
    at = np.arange(dim)
    x = np.empty(codes.shape[:-1] + (n,), dtype=np.int64)
    for r0 in range(0, n, 2048):
        block = rows_u8[r0:r0 + 2048]
        s = ((block[:, at // 8] >> (at % 8).astype(np.uint8)) & 1).astype(np.int64)
        if centred.ndim == 1:
            dot = (2 * s - 1) @ centred
        else:  # a block of queries: the f64 product (BLAS) of integers whose sums stay far below 2^53 is exact
            assert dim * L < 1 << 50
            dot = ((2 * s - 1).astype(np.float64) @ centred.T.astype(np.float64)).T.astype(np.int64)
        twice = dim * L - dot
        assert not np.any(twice & 1) and np.all(twice >= 0) and np.all(twice <= 2 * dim * L)
        x[..., r0:r0 + 2048] = twice // 2
    return x


def scalar_metric(x, dim: int, bits: int, dist, invert) -> np.ndarray:
    """calculate_metric (encoded_vectors_binary.rs:237-252) on X with dim * L as its `dim`, in f32.
    `dist`: a DistanceType (or its name)."""
    dim_l = dim * ((1 << bits) - 1)
    assert dim_l < 1 << 24, "past this the f32 steps below would round"
    xor_product = np.asarray(x).astype(np.float32)
    zeros_count = (np.float32(dim_l) - xor_product).astype(np.float32)
    is_dot = getattr(dist, "name", str(dist)) == "Dot"
    if is_dot and invert:
        out = xor_product - zeros_count
    elif is_dot:
        out = zeros_count - xor_product
    elif invert:  # L1 | L2, true
        out = zeros_count - xor_product
    else:         # L1 | L2, false
        out = xor_product - zeros_count
    return out.astype(np.float32)


def scalar_scores(rows_u8, codes, dim: int, bits: int, dist, invert) -> np.ndarray:
    """float32[n]: the score of every stored bit row against the codes of a scalar query (scalar_xor, then
    scalar_metric).  bits = 1 with codes (q_i > 0) is the binary score."""
    return scalar_metric(scalar_xor(rows_u8, codes, dim, bits), dim, bits, dist, invert)


# ------------------------------------------------------------------ binary stores the test owns every bit of
# Shared by tests/test_gpu_binary_scalar_query_matrix.py and tests/test_gpu_binary_row_shapes.py.
def gaussian(rng, shape):
    """Standard normal f32 values with a few +0.0 and -0.0 among them (neither is > 0: both encode as a zero bit)."""
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size >= 8:
        at = rng.choice(flat.size, size=max(2, flat.size // 50), replace=False)
        flat[at[::2]] = 0.0
        flat[at[1::2]] = -0.0
    return x


def bin_query_of(dim, seed=0):
    return gaussian(np.random.default_rng(77_000 + 13 * dim + seed), (dim,))


def bin_row_bytes(dim, kind=0):
    """Bytes of a stored bit row; `kind`: a BitsStoreType (0: U8)."""
    import quantization_amd as qa

    return qa.EncodedVectorsBin.get_quantized_vector_size_from_params(
        qa.VectorParameters(dim, 1, qa.DistanceType.Dot, False), qa.BitsStoreType(int(kind)))


def bin_random_rows(n, dim, seed, kind=0):
    """Uniform random bits in the store's own row size, pad bits zero as the encoder leaves them."""
    rows = np.random.default_rng(seed).integers(0, 256, size=(n, bin_row_bytes(dim, kind)), dtype=np.uint8)
    whole, rest = divmod(dim, 8)
    if rest:
        rows[:, whole] &= (1 << rest) - 1
    rows[:, whole + (rest != 0):] = 0
    return rows


def bin_open_rows(rows, dim, dist=None, invert=False, kind=0):
    import quantization_amd as qa

    dist = qa.DistanceType.Dot if dist is None else dist
    return qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(dim, rows.shape[0], dist, invert),
                                             store=qa.BitsStoreType(int(kind)))


def bin_query_codes(query, bits: int) -> np.ndarray:
    """The per-dimension codes of a query: (q_i > 0) for a binary query, scalar_codes for 4 and 8 bits."""
    return (np.asarray(query) > 0).astype(np.uint32) if bits == 1 else scalar_codes(query, bits)[0]


class BinOracle:
    """X of every row for one (rows, query), computed once per bit width; the six metrics are taken from it."""

    def __init__(self, rows, query, dim):
        self.rows, self.query, self.dim, self._x = rows, query, dim, {}

    def scores(self, bits, dist="Dot", invert=False):
        if bits not in self._x:
            self._x[bits] = scalar_xor(self.rows, bin_query_codes(self.query, bits), self.dim, bits)
        return scalar_metric(self._x[bits], self.dim, bits, dist, invert)


# ------------------------------------------------------------------ product quantizer: inputs at the encoder's edges
# tests/test_pq_encode_model.py checks these generators against the oracle without a GPU; the GPU files rely on them.
def assert_bits_equal_nan(got, want, what=""):
    """assert_bits_equal, except that where `want` is a NaN any NaN is accepted (an x86 NaN and a GPU default NaN
    differ in the sign bit).  Everywhere else the bits must match, the sign of zero included."""
    g = np.ascontiguousarray(got, dtype=np.float32).ravel()
    w = np.ascontiguousarray(want, dtype=np.float32).ravel()
    assert g.shape == w.shape, f"{what}: {g.shape} values, want {w.shape}"
    bad = np.flatnonzero(np.where(np.isnan(w), ~np.isnan(g), bits(g) != bits(w)))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size}/{g.size} values differ; first at {i}: got {g[i]!r} "
                             f"({bits(g)[i]:#010x}) want {w[i]!r} ({bits(w)[i]:#010x})")


def pq_sq_dist(a, k, mode: str = "plain") -> np.ndarray:
    """Squared distance over the last axis of f32 arrays, one f32 rounding per operation.
    "plain": t = a - k, d += t * t in index order (encode_vector, encoded_vectors_pq.rs:237-265);
    "rev":   the same with the sum taken from the last index down;
    "fma":   the contracted chain d = f32(f64(t) * f64(t) + f64(d)) (the f64 product of two f32 is exact)."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        t = (np.asarray(a, dtype=f32) - np.asarray(k, dtype=f32)).astype(f32)
        d = np.zeros(t.shape[:-1], dtype=f32)
        js = range(t.shape[-1])
        for j in (reversed(js) if mode == "rev" else js):
            tj = t[..., j]
            if mode == "fma":
                d = (tj.astype(np.float64) * tj.astype(np.float64) + d.astype(np.float64)).astype(f32)
            else:
                d = (d + (tj * tj).astype(f32)).astype(f32)
    return d


PQ_TIE_SLOTS = 128


def pq_tie_slot_indices(chunk: int, slot: int) -> tuple[int, int]:
    """The two centroid indices (low, high) of near-tie slot `slot` of chunk `chunk` of a pq_near_tie_case.  Even
    chunks: both halves of pair `slot`, (2s, 2s + 1) - with (0, 1) and (254, 255).  Odd chunks: across two pairs,
    (2s + 1, 2s + 2) - every boundary between two pipeline steps of pq_encode_cs_kernel is among them, whatever its
    pairs per step (31 | 32, 63 | 64, ...) - and slot 127 takes what is left, (0, 255)."""
    if chunk % 2 == 0:
        return 2 * slot, 2 * slot + 1
    return (2 * slot + 1, 2 * slot + 2) if slot < PQ_TIE_SLOTS - 1 else (0, 255)


class PqTieCase:
    """data [n, m * length], cen [256, m * length]; per cell (chunk, slot): lo / hi centroid indices, the two plain
    f32 distances d_lo / d_hi of the cell's row vector, and what marks it: `contract` (the contracted chain picks the
    other centroid), `order` (the reversed sum does), `tie` (d_lo == d_hi exactly).  slot[r, c]: the cell of row r."""


def pq_near_tie_case(length: int, n: int, seed: int, m: int = 8, first: int = 0) -> PqTieCase:
    """Rows that sit between two centroids at (nearly) the same f32 distance, for chunks of `length` values.

    Candidate: a row vector a near its slot's centre, centroid k1 = fl(a + o) with a small offset o, t = fl(a - k1) and
    k2 = fl(a + rot1(t)): the mirrored centroid with its differences rotated by one place, so that the two distances
    are the same squares summed in a different order, up to the roundings.  The rotation is fixed (a random permutation
    gave 0.7 % contraction-sensitive candidates at length 4 against 7 - 10 %).  The slot's centre is up to 64 in
    coordinate 0, where an f32 has a 2^-17 grid: the row and k1 are drawn on that grid in coordinate 0 and in the last
    coordinate (whose difference the rotation moves to coordinate 0), so that no rounding there pulls the two distances
    apart by more than the few ulps the test is about (13-bit differences: their squares still round); the
    coordinates between are full-precision values around zero.  Every fourth candidate is an exact
    mirror on a 2^-12 grid instead (k1 = a - t, k2 = a + t, nothing rounds): a tie under every evaluation order.  Odd
    candidates put k1 at the higher index of their slot, even ones at the lower.  Slot s lives around (s - 64, 0, 0,
    ...) and nothing of it strays more than 3/16 from there in any coordinate, so every other slot's centroids are far.
    Per slot the candidates on which the contracted chain, the reversed sum, or an exact tie decide the code come first,
    in turn, starting with kind `first` (0, 1, 2 in that order), and chunk c takes the slot's c-th: nearly every cell of
    the case is one of them, and a case of one chunk holds 128 cells of kind `first`."""
    f32 = np.float32
    S = PQ_TIE_SLOTS
    per = max(160, m + 32)
    rng = np.random.default_rng([seed, length])
    centre = np.zeros((S, 1, length), dtype=f32)
    centre[:, 0, 0] = np.arange(S, dtype=f32) - 64
    u = (rng.random((S, per, length), dtype=f32) * 2 - 1) * f32(2.0 ** -4)
    o = (rng.random((S, per, length), dtype=f32) * 2 - 1) * f32(2.0 ** -4)
    for j in {0, length - 1}:  # (see the docstring: these two coordinates stay on a 2^-17 grid)
        u[..., j] = np.round(u[..., j] * f32(2.0 ** 17)) * f32(2.0 ** -17)
        o[..., j] = np.round(o[..., j] * f32(2.0 ** 17)) * f32(2.0 ** -17)
    a = (centre + u).astype(f32)
    k1 = (a + o).astype(f32)
    t = (a - k1).astype(f32)
    k2 = (a + np.roll(t, 1, axis=-1)).astype(f32)
    mirror = np.arange(per) % 4 == 3
    ug = np.round(u[:, mirror] * 4096) / 4096
    tg = np.round(o[:, mirror] * 4096) / 4096
    tg[..., 0] = np.where(np.all(tg == 0, axis=-1), f32(2.0 ** -12), tg[..., 0])
    a[:, mirror] = centre + ug
    k1[:, mirror] = a[:, mirror] - tg
    k2[:, mirror] = a[:, mirror] + tg
    swap = (np.arange(per) % 2 == 1)[None, :, None]
    lo, hi = np.where(swap, k2, k1), np.where(swap, k1, k2)
    pick = {mode: pq_sq_dist(a, hi, mode) < pq_sq_dist(a, lo, mode) for mode in ("plain", "fma", "rev")}
    d_lo, d_hi = pq_sq_dist(a, lo), pq_sq_dist(a, hi)
    contract, order, tie = pick["fma"] != pick["plain"], pick["rev"] != pick["plain"], d_lo == d_hi
    # rank the slot's candidates: the three kinds in turn (starting with kind `first`), then the rest
    cat = np.where(contract, 0, np.where(order, 1, np.where(tie, 2, 3)))
    prio = np.arange(per)[None, :] + per * (mirror[None, :] & (cat == 2))  # drawn ties before the mirrored ones
    by_cat = np.argsort(cat * (4 * per) + prio, axis=1, kind="stable")
    rank = np.empty_like(by_cat)
    np.put_along_axis(rank, by_cat, np.broadcast_to(np.arange(per)[None, :], by_cat.shape), axis=1)
    starts = np.cumsum(np.stack([(cat == k).sum(axis=1) for k in range(4)], axis=1), axis=1) - \
        np.stack([(cat == k).sum(axis=1) for k in range(4)], axis=1)
    pos = rank - np.take_along_axis(starts, cat, axis=1)
    key = np.where(cat < 3, pos * 3 + (cat - first) % 3, 3 * per + prio)
    pick_i = np.argsort(key, axis=1, kind="stable")[:, :m]  # [S, m]: chunk c takes the slot's c-th
    case = PqTieCase()
    case.length, case.m, case.n = length, m, n
    case.cen = np.zeros((256, m * length), dtype=f32)
    ss = np.arange(S)
    idx = np.array([[pq_tie_slot_indices(c, sl) for sl in range(S)] for c in range(2)])  # [layout, S, (lo, hi)]
    case.lo = idx[np.arange(m) % 2, :, 0]
    case.hi = idx[np.arange(m) % 2, :, 1]
    for c in range(m):
        cols = slice(c * length, (c + 1) * length)
        case.cen[case.lo[c], cols] = lo[ss, pick_i[:, c]]
        case.cen[case.hi[c], cols] = hi[ss, pick_i[:, c]]
    gather = lambda x: np.ascontiguousarray(np.swapaxes(x[ss[:, None], pick_i], 0, 1))  # [S, per, ...] -> [m, S, ...]
    cell_a = gather(a)
    case.d_lo, case.d_hi = gather(d_lo), gather(d_hi)
    case.contract, case.order, case.tie = gather(contract), gather(order), gather(tie)
    case.slot = (np.arange(n)[:, None] + 37 * np.arange(m)[None, :]) % S
    case.data = np.ascontiguousarray(cell_a[np.arange(m)[None, :], case.slot].reshape(n, m * length))
    # the code of the plain chain with the strict '<' walk: the lower index unless the higher one is strictly nearer
    case.want = np.where(case.d_hi < case.d_lo, case.hi, case.lo)[np.arange(m)[None, :], case.slot].astype(np.uint8)
    return case


def pq_near_tie_table(dim: int, chunk: int, n: int, seed: int, first: int = 0):
    """(data [n, dim], cen [256, dim], cases) for any (dim, chunk): one pq_near_tie_case per distinct chunk length
    (the ragged last chunk has its own), pasted side by side.  cases: [(first chunk, PqTieCase)]."""
    m = (dim + chunk - 1) // chunk
    last = dim - (m - 1) * chunk
    groups = [(0, m, chunk)] if last == chunk else ([(0, m - 1, chunk)] if m > 1 else []) + [(m - 1, 1, last)]
    data = np.zeros((n, dim), dtype=np.float32)
    cen = np.zeros((256, dim), dtype=np.float32)
    cases = []
    for c0, mg, length in groups:
        case = pq_near_tie_case(length, n, seed, m=mg, first=first)
        data[:, c0 * chunk:c0 * chunk + mg * length] = case.data
        cen[:, c0 * chunk:c0 * chunk + mg * length] = case.cen
        cases.append((c0, case))
    return data, cen, cases


# What tests/test_gpu_pq_encode_edges.py encodes: (chunk, dim) of every pq_encode_cs_kernel<chunk> instantiation, the
# shapes of pq_encode_kernel ((40, 33): the chunk is larger than the dim), and row counts that are no multiple of the
# 256-row workgroup.  Table v of a shape has PQ_EDGE_ROW_COUNTS[v] rows and starts its slots with kind v, so that a
# shape of ONE chunk still sees 128 cells of each kind; tests/test_pq_encode_model.py asserts the counts on these tables.
PQ_EDGE_CS_SHAPES = [(1, 8), (2, 16), (4, 32), (8, 64), (16, 128), (32, 256)]
PQ_EDGE_GENERIC_SHAPES = [(3, 10), (7, 100), (20, 50), (24, 24), (40, 33)]
PQ_EDGE_ROW_COUNTS = (257, 1000, 2051)
_edge_tables = {}


def pq_edge_tie_tables(chunk: int, dim: int):
    """[(data [n, dim], cen [256, dim], cases)] for n in PQ_EDGE_ROW_COUNTS; built once per shape."""
    if (chunk, dim) not in _edge_tables:
        _edge_tables[chunk, dim] = [pq_near_tie_table(dim, chunk, n, seed=chunk * 1000 + dim, first=v)
                                    for v, n in enumerate(PQ_EDGE_ROW_COUNTS)]
    return _edge_tables[chunk, dim]


def describe_code_mismatches(got, want, data, cen, chunk: int, limit: int = 5) -> str:
    """(row, chunk, got, want, the two plain f32 distances) of the first few differing codes."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    out = [f"{len(bad)} of {np.asarray(want).size} codes differ"]
    for r, c in bad[:limit]:
        cols = slice(c * chunk, min((c + 1) * chunk, data.shape[1]))
        g, w = int(got[r, c]), int(want[r, c])
        out.append(f"row {r} chunk {c}: got {g} (d = {pq_sq_dist(data[r, cols], cen[g, cols])!r}) "
                   f"want {w} (d = {pq_sq_dist(data[r, cols], cen[w, cols])!r})")
    return "; ".join(out)


# Scalar values of the special centroids: centroid k holds PQ_SPECIAL_CENTROIDS[k] in every coordinate (but see k = 2);
# 12 .. 254 are 2.0, 2.5, ... and 255 is 1000.25.
PQ_SPECIAL_CENTROIDS = {0: 0.0, 1: 1.0, 2: np.nan, 3: np.inf, 4: -np.inf, 5: 3e38, 6: -3e38, 7: 1e-40, 8: 2e-40,
                        9: -0.0, 10: -1e-40, 11: 3e-20, 255: 1000.25}
# (name, the row's value in every coordinate, its code in every chunk by the reference's walk: d starts at f32::MAX,
# index order, strict '<')
PQ_SPECIAL_ROWS = [
    ("one", 1.0, 1),            # d = 0 at centroid 1; centroid 2 (a NaN in its first coordinate) is skipped: NaN < x is false
    ("plus_inf", np.inf, 0),    # every distance is +inf or NaN (inf - inf): nothing is < f32::MAX, the code stays 0
    ("minus_inf", -np.inf, 0),
    ("big", 3e38, 5),           # 0 at centroid 5; against -3e38 the difference itself overflows
    ("minus_big", -3e38, 6),
    ("overflow", -2.5e38, 0),   # the nearest centroid, -3e38, is 5e37 away: its square overflows like all others
    ("subnormal", 1e-40, 0),    # differences to 0.0, +-1e-40, 2e-40 are subnormal, their squares 0: a tie at 0, index order
    ("minus_subnormal", -1e-40, 0),
    ("minus_zero", -0.0, 0),    # distance +0.0 to centroid 0; centroid 9 (-0.0) ties and comes later
    ("tiny", 2e-20, 11),        # squares 4e-40 (centroids 0, 7 .. 10) against 1e-40 (centroid 11): subnormal, not flushed
    ("last", 1000.25, 255),     # equal to centroid 255: distance 0 at the last index
    ("midway", 0.5, 0),         # 0.25 per coordinate to both 0.0 and 1.0: the exact tie goes to the lower index
    ("nearer_one", 0.625, 1),
]


def pq_special_case(dim: int, chunk: int):
    """(data [14, dim], cen [256, dim], want u8 [14, m]): rows and centroids with NaN, infinities, values whose
    differences overflow, subnormals and negative zero, and the codes the reference's walk gives them (stated in
    PQ_SPECIAL_ROWS, not computed).  Row 0 is all 1.0 with a NaN in its first coordinate: chunk 0 has only NaN
    distances and keeps code 0, the other chunks are 1.  Centroid 2 is 1.0 with a NaN in the first coordinate of every
    chunk (a NaN that enters the sum first and stays)."""
    f32 = np.float32
    m = (dim + chunk - 1) // chunk
    vals = np.array([PQ_SPECIAL_CENTROIDS.get(k, 2.0 + 0.5 * (k - 12)) for k in range(256)], dtype=f32)
    cen = np.repeat(vals[:, None], dim, axis=1)
    cen[2, :] = 1.0
    cen[2, ::chunk] = np.nan
    data = np.zeros((1 + len(PQ_SPECIAL_ROWS), dim), dtype=f32)
    want = np.zeros((data.shape[0], m), dtype=np.uint8)
    data[0, :] = 1.0
    data[0, 0] = np.nan
    want[0, 1:] = 1
    for i, (_name, value, code) in enumerate(PQ_SPECIAL_ROWS, start=1):
        data[i, :] = f32(value)
        want[i, :] = code
    return data, np.ascontiguousarray(cen), want


# ------------------------------------------------------------------ product quantizer: stores the row-shape tests own
# Shared by tests/test_pq_row_shapes_model.py (which proves on the oracle alone that a chunk read too many or too few
# changes the bits of these stores) and tests/test_gpu_pq_row_shapes.py.
PQ_ZERO_CODES = (77, 200)  # all-zero centroids: +0.0 and -0.0 (invert) entries in every chunk table.  Never code 0: the
                           # zero padding of a device row reads table entry 0, which has to count when it is added.
DIST_IDS = {"Dot": 0, "L1": 1, "L2": 2}


def pq_shape_store(m, n, chunk=4, seed=0):
    """(rows u8 [n, m], centroids f32 [256, dim], dim, chunk size): random codes, centroids in (-0.5, 0.5) with the
    PQ_ZERO_CODES centroids zero, a last chunk one dimension short (chunk > 1).  Row 0 is all code 0, row 1 all 255 and
    row 2 all PQ_ZERO_CODES[0], so every chunk table is read at its first, last and a zero entry.  In every other row
    the last chunk walks a random order of the other 252 codes: leaving the last chunk out then changes the score of
    every such row under Dot too (no zero centroid), and against a stored row (whose table is zero at its own code
    under L1 and L2) of all but one row in 252.  A store of fewer rows is a prefix."""
    dim = m * chunk - 1 if chunk > 1 else m
    rng = np.random.default_rng(100_003 * m + 17 * chunk + seed)
    cen = (rng.random((256, dim), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    cen[list(PQ_ZERO_CODES)] = 0.0
    others = rng.permutation([c for c in range(256) if c not in (0, 255) + PQ_ZERO_CODES]).astype(np.uint8)
    rows = rng.integers(0, 256, size=(n, m), dtype=np.uint8)
    rows[0], rows[1], rows[2] = 0, 255, PQ_ZERO_CODES[0]
    rows[3:, m - 1] = others[np.arange(n - 3) % others.size]
    return rows, cen, dim, chunk


def pq_shape_queries(dim, count, seed=0):
    """f32 [count, dim] in (-0.5, 0.5) with a last dimension of at least 0.25: the short last chunk is never a zero."""
    q = (np.random.default_rng(7_000_003 + 31 * dim + seed).random((count, dim), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    q[:, dim - 1] = np.abs(q[:, dim - 1]) + np.float32(0.25)
    return q


def pq_row_table(rows, cen, dim, chunk, dist, i):
    """f32 [m, 256]: entry (c, code) = the metric of centroid rows[i][c] and centroid `code` over chunk c, summed in
    dimension order in f32 from 0.0 (score_internal's inner loop, encoded_vectors_pq.rs:566-593); not inverted."""
    m = rows.shape[1]
    cen = np.ascontiguousarray(cen, dtype=np.float32)
    table = np.zeros((m, 256), dtype=np.float32)
    name = getattr(dist, "name", str(dist))
    for c in range(m):
        lo, hi = c * chunk, min(c * chunk + chunk, dim)
        a, b = cen[int(rows[i, c]), lo:hi], cen[:, lo:hi]
        s = np.zeros(256, dtype=np.float32)
        for t in range(hi - lo):
            if name == "Dot":
                s = s + a[t] * b[:, t]
            elif name == "L1":
                s = s + np.abs(a[t] - b[:, t])
            else:
                d = a[t] - b[:, t]
                s = s + d * d
        table[c] = s
    return table


def pq_seq_scores(rows, table, invert, chunks=None):
    """f32 [n]: score_internal of every row given row i's table - one running f32 sum in chunk order, negated once."""
    total = np.zeros(rows.shape[0], dtype=np.float32)
    for c in range(rows.shape[1] if chunks is None else chunks):
        total = total + table[c][rows[:, c]]
    return -total if invert else total
