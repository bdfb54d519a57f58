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
    """sha256 of every input byte of ref_differential_cases(), in order: proves the stored outputs belong to them."""
    import hashlib

    h = hashlib.sha256()
    for _dim, q, v in cases:
        h.update(q.tobytes())
        h.update(v.tobytes())
    return h.hexdigest()
