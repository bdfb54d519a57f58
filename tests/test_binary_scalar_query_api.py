"""CPU-side checks of scalar (4- and 8-bit) queries against binary rows: the header declares the new entry points and
says what has no counterpart in the reference and what is left out, the library exports them, the ctypes mirror binds
them, and encode_query has the `query_bits` keyword.  No GPU is needed."""
import ctypes as C
import inspect
import os

import quantization_amd as qa
from quantization_amd import _lib

NEW = ["qamd_bin_encode_query_scalar", "qamd_bin_query_info"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "quantization_amd.h")).read()


def test_header_declares_the_entry_points():
    hdr = header()
    declared = set(_lib.declared_symbols())
    assert not [s for s in NEW if s not in declared]
    assert "qamd_bin_encode_query" in declared and "qamd_bin_query_read" in declared  # the binary calls stay
    for name in NEW:  # each says that the reference has no counterpart and where the definition is
        at = hdr.index(f" {name}(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "counterpart" in comment and "DESIGN.md 3.2d" in comment, name
    at = hdr.index(" qamd_bin_encode_query_scalar(")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    # what is deliberately left out
    assert "qamd_bin_query_batch" in comment and "qamd_bin_sharded_" in comment and "binary-only" in comment


def test_design_holds_the_definition():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.2d" in design and "popcount(plane_b" in design and "2^24" in design


def test_library_exports_and_the_mirror_binds_them():
    L = _lib.lib()
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name
    assert len(L.qamd_bin_encode_query_scalar.argtypes) == 7
    assert len(L.qamd_bin_query_info.argtypes) == 3


def test_python_surface():
    sig = inspect.signature(qa.EncodedVectorsBin.encode_query)
    assert list(sig.parameters)[:4] == ["self", "query", "reuse", "stream"]
    p = sig.parameters["query_bits"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1
    from quantization_amd.encoded_vectors_binary import EncodedBinVector
    assert isinstance(EncodedBinVector.bits, property) and isinstance(EncodedBinVector.max_abs, property)


def test_c_argument_errors_before_any_gpu_work():
    """Plane counts other than 1, 4 and 8, null handles and a null query return QAMD_ERR_ARGUMENTS."""
    L = _lib.lib()
    out = C.c_void_p()
    for bits in (0, 2, 16):
        assert L.qamd_bin_encode_query_scalar(None, None, 0, _lib.MEM_HOST, bits, None, C.byref(out)) == _lib.ERR_ARGUMENTS
        assert str(bits).encode() in L.qamd_last_error()
        assert out.value is None
    for bits in (1, 4, 8):
        assert L.qamd_bin_encode_query_scalar(None, None, 0, _lib.MEM_HOST, bits, None, C.byref(out)) == _lib.ERR_ARGUMENTS
    n = C.c_uint32()
    assert L.qamd_bin_query_info(None, C.byref(n), None) == _lib.ERR_ARGUMENTS
