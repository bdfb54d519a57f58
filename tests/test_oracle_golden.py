"""Pin the oracle's pair kernels to the reference's own C kernels.

pair_kernels.npz holds outputs of quantization/cpp/avx2.c + cpp/sse.c compiled with
build.rs's flags (tests/golden/make_golden.py).  Bit-exact comparisons.
"""
import ctypes as C
import os

import numpy as np

from util import cases_digest, ref_differential_cases


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
