"""The per-dimension oracle of scalar queries (util.scalar_codes / scalar_scores) checked without a GPU.

The oracle reads a row bit by bit and a query code by code; the restatement in test_gpu_binary_scalar_query works on bit
planes, as the kernels do.  Here the two are compared bit for bit, the f32 codes are compared with a float64
evaluation of the same formula, and the score is tied to what it means - L / a times the dot product of the stored
signs with the query - by a bound that depends on neither.
"""
import numpy as np
import pytest

import test_gpu_binary_scalar_query as R  # the restatement: np_encode, np_planes, np_scores (helpers only)
from util import assert_bits_equal, scalar_codes, scalar_codes_f64, scalar_scores

DIMS = (1, 7, 8, 33, 64, 65, 387, 1024, 2065)
N_ROWS = 41


def random_rows(rng, n, dim, nb):
    """n random bit rows of nb bytes with zero pad bits."""
    bits = rng.integers(0, 2, size=(n, dim), dtype=np.uint8)
    rows = np.zeros((n, nb), dtype=np.uint8)
    packed = np.packbits(bits, axis=1, bitorder="little")
    rows[:, :packed.shape[1]] = packed
    return rows, bits


def tie_vectors(bits, dim=387):
    """The exact-tie queries of test_encoding_edge_cases: t + 0.5 on an integer and one f32 to either side."""
    L = (1 << bits) - 1
    out = []
    for a in (np.float32(1.0), np.float32(3.0), np.float32(0.7)):
        scale = np.float32(L) / np.float32(a + a)
        ks = np.arange(1, L + 1, max(1, L // 40), dtype=np.float32)
        mid = ((ks - np.float32(0.5)) / scale - a).astype(np.float32)
        vals = np.concatenate([mid, np.nextafter(mid, np.float32(-4)), np.nextafter(mid, np.float32(4)),
                               np.float32([a, -a, 0.0])]).astype(np.float32)[:dim]
        ties = np.zeros(dim, dtype=np.float32)
        ties[:vals.size] = np.clip(vals, -a, a)
        ties[dim - 1] = a
        out.append(ties)
    return out


@pytest.mark.parametrize("dim", DIMS)
def test_oracle_equals_the_restatement(dim):
    rng = np.random.default_rng(dim)
    query = R.gaussian(rng, (dim,))
    for nb in sorted({-(-dim // 8), -(-dim // 128) * 16}):  # the U8 and the U128 row sizes
        rows, _ = random_rows(rng, N_ROWS, dim, nb)
        dirty = rows.copy()
        if dim % 8:
            dirty[:, dim // 8] |= np.uint8((0xFF << (dim % 8)) & 0xFF)
        dirty[:, -(-dim // 8):] = 0xFF
        for bits in (4, 8):
            codes, _ = scalar_codes(query, bits)
            planes = R.np_planes(R.np_encode(query, bits)[0], nb, bits)
            for dist, inv in R.METRICS:
                what = f"dim {dim} nb {nb} bits {bits} {dist.name} invert={inv}"
                got = scalar_scores(rows, codes, dim, bits, dist, inv)
                assert_bits_equal(got, R.np_scores(rows, planes, dim, dist, inv), what)
                assert_bits_equal(scalar_scores(dirty, codes, dim, bits, dist, inv), got, what + ": pad bits were read")


@pytest.mark.parametrize("bits", [4, 8])
def test_codes_equal_the_restatement(bits):
    rng = np.random.default_rng(bits)
    L = (1 << bits) - 1
    queries = [R.gaussian(rng, (dim,)) for dim in DIMS for _ in range(3)]
    zero = np.zeros(387, dtype=np.float32)
    zero[1::2] = -0.0
    odd = np.full(387, np.nan, dtype=np.float32)
    odd[3], odd[4] = np.inf, -np.inf
    mixed = R.query_of(387, 1)
    mixed[[0, 64, 65, 200, 386]] = [np.nan, np.inf, -np.inf, -0.0, np.nan]
    queries += [zero, odd, mixed] + tie_vectors(bits)
    for i, q in enumerate(queries):
        got, a = scalar_codes(q, bits)
        want, wa = R.np_encode(q, bits)
        assert_bits_equal(a, wa, f"query {i}: a")
        assert got.dtype == np.uint32 and np.array_equal(got, want), f"query {i} bits {bits}: codes differ"
    assert np.all(scalar_codes(zero, bits)[0] == (L + 1) // 2)
    c, a = scalar_codes(odd, bits)
    assert a == 0 and c[3] == L and c[4] == 0 and np.all(np.delete(c, [3, 4]) == (L + 1) // 2)
    c, _ = scalar_codes(mixed, bits)
    assert c[64] == L and c[65] == 0 and c[0] == c[200]  # NaN counts as 0.0f, and -0.0f + a is a
    ties = tie_vectors(bits)[0]  # a = 1: (q + 1) * L / 2 + 0.5 is exact in f32, so the ties are real
    t = (ties + np.float32(1.0)) * (np.float32(L) / np.float32(2.0)) + np.float32(0.5)
    assert np.count_nonzero(t == np.floor(t)) > 10
    assert np.array_equal(scalar_codes(ties, bits)[0], np.minimum(L, np.floor(t.astype(np.float64))).astype(np.uint32))


@pytest.mark.parametrize("bits", [4, 8])
def test_f32_codes_against_f64(bits):
    """Three f32 roundings (q + a, * scale, + 0.5) of values below L + 1, each at most 2^-24 relative, and the rounding
    of scale itself: the f32 t + 0.5 is within L * 2^-21 of the float64 one, so the codes agree except where the float64
    value lies that close to an integer, and there they differ by 1."""
    rng = np.random.default_rng(100 + bits)
    L = (1 << bits) - 1
    near = L * 2.0 ** -21
    for _ in range(200):
        q = rng.standard_normal(387).astype(np.float32)
        got, _ = scalar_codes(q, bits)
        want, half, finite = scalar_codes_f64(q, bits)
        assert finite.all()
        diff = got.astype(np.int64) - want
        assert np.abs(diff).max() <= 1
        close = np.abs(half - np.rint(half)) <= near
        assert np.all(close[diff != 0]), "codes differ away from a rounding boundary"


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dim", [7, 33, 387, 2065])
def test_score_means_the_dot_product_with_the_stored_signs(dim, bits):
    """Dot / not inverted: |score - (L / a) sum_i q_i (2 s_i - 1)| <= 1.001 dim.  Each centred code 2 c_i - L is
    within 1 of L q_i / a (c_i rounds (q_i + a) L / (2a) to the nearest integer), the f32 roundings add under 1e-4 per
    term.  Plane order, centring or dim instead of dim * L misread move the score by far more."""
    rng = np.random.default_rng(dim * 10 + bits)
    L = (1 << bits) - 1
    rows, s = random_rows(rng, N_ROWS, dim, -(-dim // 8))
    for _ in range(5):
        q = rng.standard_normal(dim).astype(np.float32)
        codes, a = scalar_codes(q, bits)
        assert a > 0
        centred = 2.0 * codes.astype(np.float64) - L
        ideal = L * q.astype(np.float64) / float(a)
        assert np.abs(centred - ideal).max() <= 1.0001
        score = scalar_scores(rows, codes, dim, bits, "Dot", False).astype(np.float64)
        meant = (L / float(a)) * ((2.0 * s.astype(np.float64) - 1.0) @ q.astype(np.float64))
        assert np.abs(score - meant).max() <= 1.001 * dim
        # the other three sign cases of calculate_metric are this score or its negation
        for dist, inv, sign in (("Dot", True, -1), ("L1", False, -1), ("L2", False, -1), ("L1", True, 1), ("L2", True, 1)):
            assert_bits_equal(scalar_scores(rows, codes, dim, bits, dist, inv), (sign * score).astype(np.float32),
                              f"{dist} invert={inv}")
