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
    S = sum_i (2 s_i - 1)(2 c_i - L) and X = (dim * L - S) / 2, exact.  Only the first `dim` bits of a row are read."""
    rows_u8 = np.asarray(rows_u8, dtype=np.uint8)
    n = rows_u8.shape[0]
    L = (1 << bits) - 1
    centred = 2 * np.asarray(codes, dtype=np.int64)[:dim] - L
    assert centred.size == dim
    at = np.arange(dim)
    x = np.empty(n, dtype=np.int64)
    for r0 in range(0, n, 2048):
        block = rows_u8[r0:r0 + 2048]
        s = ((block[:, at // 8] >> (at % 8).astype(np.uint8)) & 1).astype(np.int64)
        twice = dim * L - (2 * s - 1) @ centred
        assert not np.any(twice & 1) and np.all(twice >= 0) and np.all(twice <= 2 * dim * L)
        x[r0:r0 + 2048] = twice // 2
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
