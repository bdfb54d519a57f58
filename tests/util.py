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
