"""Pin the oracle's pair kernels to the reference's own C kernels.

pair_kernels.npz holds outputs of quantization/cpp/avx2.c + cpp/sse.c compiled with
build.rs's flags (tests/golden/make_golden.py).  Bit-exact comparisons.
"""
import ctypes as C
import os

import numpy as np

from util import cases_digest, ref_differential_cases, wide_dot_pair_2096, wide_sum_cases


def _each(golden):
    for name in golden["case_names"]:
        name = str(name)
        yield name, golden[f"{name}__q"], golden[f"{name}__v"]


def test_dot_avx2_order_matches_reference_bits(qo, golden):
    L = qo.lib()
    for name, q, v in _each(golden):
        want = golden[f"{name}__dot_avx"]
        for i in range(q.shape[0]):
            got = np.float32(L.qo_dot_avx2_order(q[i].ctypes.data, v[i].ctypes.data, q.shape[1]))
            assert got.view(np.uint32) == want[i].view(np.uint32), (name, i, got, want[i])


def test_dot_sse_order_matches_reference_bits(qo, golden):
    L = qo.lib()
    for name, q, v in _each(golden):
        want = golden[f"{name}__dot_sse"]
        for i in range(q.shape[0]):
            got = np.float32(L.qo_dot_sse_order(q[i].ctypes.data, v[i].ctypes.data, q.shape[1]))
            assert got.view(np.uint32) == want[i].view(np.uint32), (name, i)


def test_l1_avx2_order_matches_reference_bits(qo, golden):
    L = qo.lib()
    for name, q, v in _each(golden):
        want = golden[f"{name}__l1_avx"]
        for i in range(q.shape[0]):
            got = np.float32(L.qo_l1_avx2_order(q[i].ctypes.data, v[i].ctypes.data, q.shape[1]))
            assert got.view(np.uint32) == want[i].view(np.uint32), (name, i)


def test_xor_popcnt_matches_reference(qo, golden):
    L = qo.lib()
    for name, q, v in _each(golden):
        want = golden[f"{name}__popcnt128"]
        for i in range(q.shape[0]):
            assert L.qo_xor_popcnt(q[i].ctypes.data, v[i].ctypes.data, q.shape[1]) == want[i]
    q, v = golden["small__q"], golden["small__v"]
    for i in range(q.shape[0]):
        assert L.qo_xor_popcnt(q[i].ctypes.data, v[i].ctypes.data, 16) == golden["small__popcnt64x2"][i]
        assert L.qo_xor_popcnt(q[i].ctypes.data, v[i].ctypes.data, 8) == golden["small__popcnt32x2"][i]


def test_exact_integer_for_encoder_codes_up_to_dim_1040(qo, golden):
    """codes <= 127 and actual_dim <= 1040 => every kernel returns the exact
    integer, so summation order is irrelevant there (simple == AVX2 == SSE)."""
    L = qo.lib()
    for name, q, v in _each(golden):
        if not (name.startswith("codes127") or name.startswith("all127") or name.startswith("sparse")):
            continue
        dim = q.shape[1]
        if dim > 1040:
            continue
        for i in range(q.shape[0]):
            exact = int(np.dot(q[i].astype(np.int64), v[i].astype(np.int64)))
            assert exact < 2 ** 24
            assert golden[f"{name}__dot_avx"][i] == np.float32(exact)
            assert golden[f"{name}__dot_sse"][i] == np.float32(exact)
            assert L.qo_dot_i32(q[i].ctypes.data, v[i].ctypes.data, dim) == exact


def test_live_reference_differential(qo):
    """Fuzz the restatement on seeded inputs against the outputs the compiled reference returned for them
    (tests/golden/ref_differential.npz), and against oracle/_ref itself when it is present (built here, shipped
    prebuilt to the GPU box)."""
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_differential.npz"))
    cases = ref_differential_cases()
    assert cases_digest(cases) == str(want["inputs_sha256"]), "seeded inputs changed: re-run tests/golden/make_golden.py"
    R = qo.ref()
    L = qo.lib()
    for i, (dim, q, v) in enumerate(cases):
        qp, vp = q.ctypes.data, v.ctypes.data
        for key, mine, ref in (("dot_avx", L.qo_dot_avx2_order, R and R.impl_score_dot_avx),
                               ("dot_sse", L.qo_dot_sse_order, R and R.impl_score_dot_sse),
                               ("l1_avx", L.qo_l1_avx2_order, R and R.impl_score_l1_avx)):
            b = np.float32(mine(qp, vp, dim))
            assert b.view(np.uint32) == want[key][i].view(np.uint32), (key, i, dim)
            if R is not None:
                assert np.float32(ref(qp, vp, dim)).view(np.uint32) == b.view(np.uint32), (key, i, dim)
        assert L.qo_xor_popcnt(qp, vp, dim) == want["popcnt128"][i], ("popcnt128", i, dim)
        if R is not None:
            assert R.impl_xor_popcnt_sse_uint128(qp, vp, dim // 16) == want["popcnt128"][i], ("popcnt128", i, dim)


def _wide_sums():
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_wide_sums.npz"))
    cases = wide_sum_cases()
    assert cases_digest(cases) == str(want["inputs_sha256"]), "seeded inputs changed: re-run tests/golden/make_golden.py"
    assert want["dot_avx"].shape == want["l1_avx"].shape == (len(cases),)
    return cases, want


def _exact(q, v):
    q, v = q.astype(np.int64), v.astype(np.int64)
    return int(np.dot(q, v)), int(np.abs(q - v).sum())


def test_wide_sums_digest():
    _wide_sums()


def test_wide_sum_avx2_orders_match_reference_bits(qo):
    """Sums past 2^24 (dot) and u16 lanes past 2^16 (L1): the restated AVX2 orders equal the bits the compiled
    reference returned (tests/golden/ref_wide_sums.npz), and oracle/_ref itself when it is present."""
    cases, want = _wide_sums()
    L, R = qo.lib(), qo.ref()
    for i, (tag, dim, q, v) in enumerate(cases):
        qp, vp = q.ctypes.data, v.ctypes.data
        for key, mine, ref in (("dot_avx", L.qo_dot_avx2_order, R and R.impl_score_dot_avx),
                               ("l1_avx", L.qo_l1_avx2_order, R and R.impl_score_l1_avx)):
            b = np.float32(mine(qp, vp, dim))
            assert b.view(np.uint32) == want[key][i].view(np.uint32), (key, tag, i, dim)
            if R is not None:
                assert np.float32(ref(qp, vp, dim)).view(np.uint32) == b.view(np.uint32), (key, tag, i, dim)


def test_wide_sum_fixture_discriminates():
    """The fixture pins the orders where they differ from the exact sum: at least 15 % of the dot cases (and the
    constructed pair at 2096) have AVX2 != the exact sum rounded once, and L1 cases wrap a u16 lane (all-0 against
    all-127: exact at 8256, wrapped from 8272, 8064 at 8320)."""
    cases, want = _wide_sums()
    dot_diff, n_dot, l1_wraps = 0, 0, []
    for i, (tag, dim, q, v) in enumerate(cases):
        dot, l1 = _exact(q, v)
        if tag.startswith("dot_"):
            assert q.max() <= 127 and v.max() <= 127, (tag, i)
            n_dot += 1
            differs = want["dot_avx"][i] != np.float32(dot)
            dot_diff += differs
            if tag == "dot_edge2096":
                assert dim == 2096 and differs, "the constructed 2096 pair no longer tells the orders apart"
            if dim <= 2080:
                assert not differs, (tag, i, dim)
        elif want["l1_avx"][i] != np.float32(l1):
            l1_wraps.append((tag, dim))
    assert n_dot and dot_diff >= 0.15 * n_dot, f"only {dot_diff}/{n_dot} dot cases differ from the exact sum"
    assert ("l1_zero127", 8320) in l1_wraps and ("l1_zero127", 8272) in l1_wraps, l1_wraps
    assert ("l1_zero127", 8256) not in l1_wraps, l1_wraps
    assert any(t == ("l1_sat", 16384) for t in l1_wraps), l1_wraps
    i8320 = next(i for i, c in enumerate(cases) if c[0] == "l1_zero127" and c[1] == 8320)
    assert want["l1_avx"][i8320] == np.float32(8064)


def test_wide_dot_pair_2096_half_sum():
    """The constructed 2096 pair is what it claims: the even-lane half sum passes 2^24 and is odd."""
    q, v = wide_dot_pair_2096()
    p = q.astype(np.int64) * v.astype(np.int64)
    even_half = int(p[(np.arange(q.size) % 4) < 2].sum())
    assert even_half > 2 ** 24 and even_half % 2 == 1
    assert int(np.float32(even_half)) != even_half  # the half sum rounds


def test_avx2_order_is_exact_sum_up_to_actual_dim_2080(qo):
    """For codes <= 127 and actual_dim <= 2080 every value impl_score_dot_avx forms is an exact f32 integer up to the
    two half sums (each covers actual_dim / 2 bytes: at most 16129 * 1040 < 2^24), so only the last add rounds: the
    AVX2 order IS the exact sum rounded once (ORDER_AVX2 == ORDER_SIMPLE) -- random and adversarial pairs, whole
    32-byte blocks and 16-byte tails.  The library may serve lane mode 1 as mode 0 there."""
    L = qo.lib()
    rng = np.random.default_rng(2080)
    dims = list(range(16, 2081, 16))
    top = (2048, 2064, 2080)

    def check(q, v):
        d = q.size
        a = np.float32(L.qo_dot_avx2_order(q.ctypes.data, v.ctypes.data, d))
        s = np.float32(L.qo_dot_simple(q.ctypes.data, v.ctypes.data, d))
        assert a.view(np.uint32) == s.view(np.uint32), (d, a, s)

    n = 0
    for d in dims + list(top) * 40:
        full = np.full(d, 127, dtype=np.uint8)
        even = np.where((np.arange(d) % 4) < 2, 127, 0).astype(np.uint8)
        odd = np.where((np.arange(d) % 4) >= 2, 127, 0).astype(np.uint8)
        for q, v in ((full, full), (even, even), (odd, odd), (even, full)):
            check(q, v)
            n += 1
        for lo in (0, 64, 110, 120):
            q = rng.integers(lo, 128, size=d, dtype=np.uint8)
            v = rng.integers(lo, 128, size=d, dtype=np.uint8)
            check(q, v)
            # near-saturated even lanes, one byte nudged: odd half sums as large as they get
            e = even.copy()
            e[rng.integers(0, d)] = rng.integers(0, 128)
            check(e, np.maximum(even, v) if lo >= 110 else even)
            n += 2
    assert n >= 3000
