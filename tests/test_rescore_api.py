"""CPU-side checks of the rescoring feature: every new entry point is declared in the header, exported by the
library, bound by the ctypes mirror and wrapped in Python.  No GPU is needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import quantization_amd as qa
from quantization_amd import _base, _lib

F32 = ["qamd_f32_from_data", "qamd_f32_get_parameters", "qamd_f32_free", "qamd_f32_score_ids", "qamd_f32_score_ids_batch",
       "qamd_f32_rerank", "qamd_f32_rerank_batch"]
FUSED = [f"qamd_{p}_topk{b}_rescored" for p in ("u8", "pq", "bin") for b in ("", "_batch")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_new_symbol_is_declared():
    declared = set(_lib.declared_symbols())
    missing = [s for s in F32 + FUSED if s not in declared]
    assert not missing, f"not declared in include/quantization_amd.h: {missing}"


def test_every_new_symbol_is_bound_with_a_signature():
    L = _lib.lib()
    for name in F32 + FUSED:
        fn = getattr(L, name)
        assert fn.argtypes is not None, f"{name} has no ctypes signature"
    assert L.qamd_f32_free.restype is None
    assert len(L.qamd_f32_score_ids.argtypes) == 10
    assert len(L.qamd_f32_score_ids_batch.argtypes) == 13
    assert len(L.qamd_f32_rerank.argtypes) == 13
    assert len(L.qamd_f32_rerank_batch.argtypes) == 14
    for p in ("u8", "pq", "bin"):
        assert len(getattr(L, f"qamd_{p}_topk_rescored").argtypes) == 13
        assert len(getattr(L, f"qamd_{p}_topk_batch_rescored").argtypes) == 14


def test_python_wrappers_exist():
    assert qa.OriginalVectors is not None and "OriginalVectors" in qa.__all__
    for m in ("from_data", "score_ids", "score_ids_batch", "rerank", "rerank_batch"):
        assert callable(getattr(qa.OriginalVectors, m)), m
    assert "borrow" in inspect.signature(qa.OriginalVectors.from_data).parameters
    for cls in (qa.EncodedVectorsU8, qa.EncodedVectorsPQ, qa.EncodedVectorsBin):
        assert issubclass(cls, _base.EncodedVectorsBase)
        for m in ("topk_rescored", "topk_batch_rescored"):
            assert callable(getattr(cls, m)), (cls, m)


def test_header_cites_the_reference_for_every_new_entry_point():
    hdr = open(os.path.join(ROOT, "include", "quantization_amd.h")).read()
    for name in F32 + FUSED:
        if name in ("qamd_f32_get_parameters", "qamd_f32_free"):
            continue
        at = hdr.index(f" {name}(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "encoded_vectors.rs:37-45" in comment, name
        if name in FUSED:
            assert "ann_benchmark_data.rs:151-185" in comment, name
    assert re.search(r"Out of scope:.*[Ss]harded.*f16.*host memory.*bench\.py", hdr, re.S)


def test_argument_errors_before_any_gpu_work():
    """Null handles and bad parameters are refused with QAMD_ERR_ARGUMENTS and a message; no GPU is touched."""
    L = _lib.lib()
    out = C.c_void_p()
    vp = _lib.VectorParametersC(4, 2, 7, 0)  # unknown distance type
    data = np.zeros((2, 4), dtype=np.float32)
    assert L.qamd_f32_from_data(data.ctypes.data, _lib.MEM_HOST, C.byref(vp), 0, None, C.byref(out)) == _lib.ERR_ARGUMENTS
    vp = _lib.VectorParametersC(4, 2, 0, 0)
    # host memory cannot be borrowed
    assert L.qamd_f32_from_data(data.ctypes.data, _lib.MEM_HOST, C.byref(vp), 1, None, C.byref(out)) == _lib.ERR_ARGUMENTS
    assert b"borrow" in L.qamd_last_error()
    q = np.zeros(4, dtype=np.float32)
    ids = np.zeros(4, dtype=np.uint32)
    sc = np.zeros(4, dtype=np.float32)
    assert L.qamd_f32_score_ids(None, q.ctypes.data, 4, 0, ids.ctypes.data, 4, 0, sc.ctypes.data, 0, None) == _lib.ERR_ARGUMENTS
    assert L.qamd_f32_rerank(None, q.ctypes.data, 4, 0, ids.ctypes.data, 4, 0, 2, 1, ids.ctypes.data, sc.ctypes.data, 0,
                             None) == _lib.ERR_ARGUMENTS
    for p in ("u8", "pq", "bin"):
        assert getattr(L, f"qamd_{p}_topk_rescored")(None, None, None, q.ctypes.data, 4, 0, 1, 1, 1, ids.ctypes.data,
                                                     sc.ctypes.data, 0, None) == _lib.ERR_ARGUMENTS
    with pytest.raises(qa.EncodingError):
        qa.OriginalVectors.from_data(data, qa.VectorParameters(5, 2, qa.DistanceType.Dot, False))
