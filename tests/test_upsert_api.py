"""CPU-side checks of upsert / reserve / capacity: the header declares the twelve entry points and states
the contract, the library exports them, the ctypes mirror binds them, null handles are refused before any device call,
and the Python surface exists.  No GPU is needed.  (A handle cannot exist without a GPU, so the refusals that need one -
a hole, null data, a borrowed store - are in tests/test_gpu_upsert.py.)"""
import inspect
import os
import re

import numpy as np
import pytest

import quantization_amd as qa
from quantization_amd import _lib

KINDS = ("u8", "pq", "bin", "f32")
NEW = [f"qamd_{k}_{f}" for k in KINDS for f in ("upsert", "reserve", "capacity")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "quantization_amd.h")).read()


def test_header_declares_the_entry_points_and_the_contract():
    hdr = header()
    declared = set(_lib.declared_symbols())
    assert not [s for s in NEW if s not in declared]
    at = hdr.index(" qamd_u8_upsert(")
    comment = hdr[hdr.rindex("/* ===", 0, at):at]
    # the reference has no counterpart; the semantics a caller relies on
    assert re.search(r"NO counterpart", comment) and "upsert_vector" in comment
    assert re.search(r"first_row <= count is required \(a hole is QAMD_ERR_ARGUMENTS\)", comment)
    assert re.search(r"n_rows == 0 is QAMD_OK", comment) and "0xFFFFFFFF" in comment
    assert re.search(r"alpha is 0", comment) and re.search(r"without centroids", comment) and re.search(r"borrowed\s+\*?\s*qamd_f32", comment)
    assert re.search(r"[Ss]harded handles and their shards cannot be upserted", comment) and "`const`" in comment
    assert re.search(r"max\(needed, capacity \+ capacity / 2\)", comment) and re.search(r"round_up\(c, 1024\) \+ 1024", comment)
    assert re.search(r"WRITERS", comment) and re.search(r"`stream` is synchronised", comment)
    # signatures: the three quantizers take f32 rows, the originals a typed buffer
    for k in ("u8", "pq", "bin"):
        assert re.search(rf"qamd_{k}_upsert\(qamd_{k} \*h, uint64_t first_row, const float \*data, qamd_mem data_mem,\s*"
                         rf"uint64_t n_rows, void \*stream\);", hdr), k
    assert re.search(r"qamd_f32_upsert\(qamd_f32 \*h, uint64_t first_row, const void \*data, qamd_dtype data_dtype,\s*"
                     r"qamd_mem data_mem, uint64_t n_rows, void \*stream\);", hdr)
    for k in KINDS:
        assert re.search(rf"qamd_status qamd_{k}_reserve\(qamd_{k} \*h, uint64_t capacity_rows, void \*stream\);", hdr), k
        assert re.search(rf"uint64_t qamd_{k}_capacity\(const qamd_{k} \*h\);", hdr), k


def test_library_exports_and_the_mirror_binds_them():
    L = _lib.lib()
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name
    assert not [s for s in _lib.declared_symbols() if not hasattr(L, s)]
    assert [len(getattr(L, f"qamd_{k}_upsert").argtypes) for k in KINDS] == [6, 6, 6, 7]
    assert all(len(getattr(L, f"qamd_{k}_reserve").argtypes) == 3 for k in KINDS)
    assert all(len(getattr(L, f"qamd_{k}_capacity").argtypes) == 1 for k in KINDS)


def test_null_handles_are_refused_before_any_device_call():
    L = _lib.lib()
    data = np.zeros((2, 4), dtype=np.float32)
    for k in ("u8", "pq", "bin"):
        assert getattr(L, f"qamd_{k}_upsert")(None, 0, data.ctypes.data, _lib.MEM_HOST, 2, None) == _lib.ERR_ARGUMENTS, k
        assert b"null handle" in L.qamd_last_error()
    assert L.qamd_f32_upsert(None, 0, data.ctypes.data, _lib.DTYPE_F32, _lib.MEM_HOST, 2, None) == _lib.ERR_ARGUMENTS
    for k in KINDS:
        assert getattr(L, f"qamd_{k}_reserve")(None, 10, None) == _lib.ERR_ARGUMENTS, k
        assert getattr(L, f"qamd_{k}_capacity")(None) == 0, k


def test_python_surface():
    for cls in (qa.EncodedVectorsU8, qa.EncodedVectorsPQ, qa.EncodedVectorsBin, qa.OriginalVectors):
        assert list(inspect.signature(cls.upsert).parameters) == ["self", "first_row", "data", "stream"], cls
        assert list(inspect.signature(cls.append).parameters) == ["self", "data", "stream"], cls
        assert list(inspect.signature(cls.reserve).parameters) == ["self", "n", "stream"], cls
        assert isinstance(cls.capacity, property), cls


def test_a_borrowed_shard_raises_before_the_library_is_called():
    """owned=False is how a sharded handle hands out its shards: every writer raises on it, whatever the handle."""
    view = qa.EncodedVectorsU8(None, None, owned=False)
    rows = np.zeros((1, 4), dtype=np.float32)
    for call in (lambda: view.upsert(0, rows), lambda: view.append(rows), lambda: view.reserve(10)):
        with pytest.raises(ValueError, match="shard"):
            call()
