"""CPU-side checks of f16 / bf16 originals: the header declares qamd_dtype and the two new entry points, the library
exports them, the ctypes mirror binds them, and OriginalVectors.from_data refuses bad `dtype` arguments before any
device is touched.  No GPU is needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import quantization_amd as qa
from quantization_amd import _lib

NEW = ["qamd_f32_from_data_typed", "qamd_f32_get_dtype"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = qa.VectorParameters(4, 2, qa.DistanceType.Dot, False)


def header():
    return open(os.path.join(ROOT, "include", "quantization_amd.h")).read()


def test_header_declares_the_enum_and_the_entry_points():
    hdr = header()
    assert re.search(r"typedef enum \{ QAMD_DTYPE_F32 = 0, QAMD_DTYPE_F16 = 1, QAMD_DTYPE_BF16 = 2 \} qamd_dtype;", hdr)
    declared = set(_lib.declared_symbols())
    assert not [s for s in NEW if s not in declared]
    assert "qamd_f32_from_data" in declared  # the f32 call stays
    at = hdr.index(" qamd_f32_from_data_typed(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    assert "encoded_vectors.rs:37-45" in comment and "nearest even" in comment
    # the definition of a score on half rows, and what is still out of scope
    assert re.search(r"WIDENED EXACTLY to f32", hdr) and re.search(r"f16 subnormals.*not flushed", hdr, re.S)
    assert re.search(r"Out of scope:.*[Ss]harded.*encoders that\s+\*?\s*read f16 / bf16.*host memory.*bench\.py", hdr, re.S)


def test_library_exports_and_the_mirror_binds_them():
    L = _lib.lib()
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name
    assert len(L.qamd_f32_from_data_typed.argtypes) == 8
    assert len(L.qamd_f32_get_dtype.argtypes) == 2
    assert (_lib.DTYPE_F32, _lib.DTYPE_F16, _lib.DTYPE_BF16) == (0, 1, 2)


def test_python_surface():
    assert "dtype" in inspect.signature(qa.OriginalVectors.from_data).parameters
    assert inspect.signature(qa.OriginalVectors.from_data).parameters["dtype"].default is None
    assert isinstance(qa.OriginalVectors.dtype, property)


def test_bad_dtype_arguments_raise_before_any_gpu_work():
    f32 = np.zeros((2, 4), dtype=np.float32)
    for bad in ("f64", "float16", "", 16):
        with pytest.raises(ValueError):
            qa.OriginalVectors.from_data(f32, VP, dtype=bad)
    bits = np.zeros((2, 4), dtype=np.uint16)
    for dtype in (None, "f32", "f16"):
        with pytest.raises(ValueError):
            qa.OriginalVectors.from_data(bits, VP, dtype=dtype)
    # a half input is never converted to the other half type or to f32
    with pytest.raises(ValueError):
        qa.OriginalVectors.from_data(f32.astype(np.float16), VP, dtype="bf16")
    with pytest.raises(ValueError):
        qa.OriginalVectors.from_data(f32.astype(np.float16), VP, dtype="f32")
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        qa.OriginalVectors.from_data(torch.zeros((2, 4), dtype=torch.bfloat16), VP, dtype="f16")


def test_c_argument_errors_before_any_gpu_work():
    """Unknown element types, pairs that are not allowed and unborrowable buffers return QAMD_ERR_ARGUMENTS."""
    L = _lib.lib()
    out = C.c_void_p()
    vp = _lib.VectorParametersC(4, 2, 0, 0)
    data = np.zeros((2, 4), dtype=np.float32)
    F32, F16, BF16 = _lib.DTYPE_F32, _lib.DTYPE_F16, _lib.DTYPE_BF16

    def make(data_dtype, store_dtype, borrow=0, ptr=data.ctypes.data):
        return L.qamd_f32_from_data_typed(ptr, data_dtype, _lib.MEM_HOST, C.byref(vp), store_dtype, borrow, None, C.byref(out))

    for pair in ((F16, F32), (BF16, F32), (F16, BF16), (BF16, F16), (7, F32), (F32, 3)):
        assert make(*pair) == _lib.ERR_ARGUMENTS, pair
        assert out.value is None
    assert make(F16, F16, borrow=1) == _lib.ERR_ARGUMENTS  # host memory cannot be borrowed
    assert b"borrow" in L.qamd_last_error()
    d = C.c_int()
    assert L.qamd_f32_get_dtype(None, C.byref(d)) == _lib.ERR_ARGUMENTS
