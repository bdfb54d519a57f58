"""CPU-side checks of batches of scalar (4- and 8-bit) queries against binary rows: the header declares the new entry
points and says what has no counterpart in the reference and what is out of scope, the library exports them, the ctypes
mirror binds them, encode_query_batch has the `query_bits` keyword, and bad bit counts are refused before any device is
touched.  No GPU is needed."""
import ctypes as C
import inspect
import os

import quantization_amd as qa
from quantization_amd import _lib

NEW = ["qamd_bin_encode_query_batch_scalar", "qamd_bin_query_batch_info", "qamd_bin_batch_kernel"]
READ_BACK = "qamd_bin_query_batch_read"  # the planes of one query of a batch, for tests and bindings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "quantization_amd.h")).read()


def comment_before(hdr, name):
    at = hdr.index(f"{name}(")
    return hdr[hdr.rindex("/*", 0, at):at]


def test_header_declares_the_entry_points():
    hdr = header()
    declared = set(_lib.declared_symbols())
    assert not [s for s in NEW + [READ_BACK] if s not in declared]
    for old in ("qamd_bin_encode_query_batch", "qamd_bin_query_batch_free", "qamd_bin_score_batch", "qamd_bin_topk_batch",
                "qamd_bin_score_ids_batch", "qamd_bin_topk_batch_rescored", "qamd_bin_encode_query_scalar"):
        assert old in declared, old  # the existing calls stay
    for name in NEW[:2]:  # each says that the reference has no counterpart and where the definition is
        comment = comment_before(hdr, name)
        assert "counterpart" in comment and "DESIGN.md 3.2d" in comment, name
    comment = comment_before(hdr, "qamd_bin_encode_query_batch_scalar")
    # what is out of scope, and where the measurement behind the thresholds is
    assert "qamd_bin_sharded_" in comment and "binary-only" in comment and "bench.py" in comment
    assert "tuning" in comment and "profiles/bin_scalar_batch.txt" in comment
    assert os.path.exists(os.path.join(ROOT, "profiles", "bin_scalar_batch.txt"))
    comment = comment_before(hdr, "qamd_bin_batch_kernel")
    for kernel in ("bin_gemm_rs_kernel", "bin_gemm_rs4_kernel", "bin_gemm_qs4_kernel", "bin_scan_multi_kernel",
                   "bin_scan_kernel"):
        assert f'"{kernel}"' in comment, kernel
    # the single-query paragraph no longer calls the batch binary-only
    comment = comment_before(hdr, " qamd_bin_encode_query_scalar")
    assert "qamd_bin_encode_query_batch_scalar" in comment


def test_design_states_the_matrix_form():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "= C - P - 2A" in design and "d_i = c_i - H" in design
    assert "qamd_bin_encode_query_batch_scalar" in design and "bin_scalar_batch.txt" in design


def test_library_exports_and_the_mirror_binds_them():
    L = _lib.lib()
    for name in NEW + [READ_BACK]:
        assert getattr(L, name).argtypes is not None, name
    assert len(L.qamd_bin_encode_query_batch_scalar.argtypes) == 8
    assert len(L.qamd_bin_query_batch_info.argtypes) == 3
    assert len(L.qamd_bin_batch_kernel.argtypes) == 3 and L.qamd_bin_batch_kernel.restype is C.c_char_p
    assert len(L.qamd_bin_query_batch_read.argtypes) == 5
    assert not [s for s in _lib.declared_symbols() if not hasattr(L, s)]  # (test_library_exports_every_declared_symbol)


def test_python_surface():
    sig = inspect.signature(qa.EncodedVectorsBin.encode_query_batch)
    assert list(sig.parameters)[:4] == ["self", "queries", "reuse", "stream"]
    p = sig.parameters["query_bits"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1
    from quantization_amd.encoded_vectors_binary import EncodedBinQueryBatch
    assert qa.EncodedVectorsBin._batch_cls is EncodedBinQueryBatch
    assert isinstance(EncodedBinQueryBatch.bits, property) and callable(EncodedBinQueryBatch.encoded_vector)
    assert callable(qa.EncodedVectorsBin.batch_kernel)
    # the other quantizers' batches are what they were
    from quantization_amd._base import EncodedVectorsBase
    assert list(inspect.signature(EncodedVectorsBase.encode_query_batch).parameters) == ["self", "queries", "reuse", "stream"]
    assert qa.EncodedVectorsPQ.encode_query_batch is EncodedVectorsBase.encode_query_batch


def test_c_argument_errors_before_any_gpu_work():
    """Bit counts other than 1, 4 and 8, null handles and a null batch return QAMD_ERR_ARGUMENTS."""
    L = _lib.lib()
    out = C.c_void_p()
    for bits in (0, 2, 16):
        assert L.qamd_bin_encode_query_batch_scalar(None, None, 0, 0, _lib.MEM_HOST, bits, None,
                                                    C.byref(out)) == _lib.ERR_ARGUMENTS
        assert str(bits).encode() in L.qamd_last_error()
        assert out.value is None
    for bits in (1, 4, 8):
        assert L.qamd_bin_encode_query_batch_scalar(None, None, 0, 0, _lib.MEM_HOST, bits, None,
                                                    C.byref(out)) == _lib.ERR_ARGUMENTS
        assert out.value is None
    bits, n = C.c_uint32(), C.c_uint64()
    assert L.qamd_bin_query_batch_info(None, C.byref(bits), C.byref(n)) == _lib.ERR_ARGUMENTS
    assert L.qamd_bin_query_batch_read(None, 0, None, 0, C.byref(n)) == _lib.ERR_ARGUMENTS
    assert L.qamd_bin_batch_kernel(None, None, 0) is None
