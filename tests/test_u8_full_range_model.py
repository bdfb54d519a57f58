"""Full-range scalar-u8 stores without a GPU: the ABI's constant and its five legal values, the Python
surface, and every refusal that comes before a device call (the metadata key: tests/test_gpu_u8_full_range.py)."""
import ctypes as C
import inspect
import os
import re

import pytest

import u8_compact_model as cm
import u8_four_bit_model as fm
import u8_full_range_model as wm
import u8_rotated_model as um

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

D = qa.DistanceType
ROOT = os.path.dirname(_lib.HERE)


def test_header_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "quantization_amd.h")).read()
    assert re.search(r"enum \{ QAMD_FULL = 64,\s*/\*[^*]*\*/\s*QAMD_DOT_FULL = 64, QAMD_L1_FULL = 65, QAMD_L2_FULL = 66, "
                     r"QAMD_DOT_ROTATED_FULL = 72, QAMD_L2_ROTATED_FULL = 74 \};", hdr)
    assert wm.LEGAL == (64, 65, 66, 72, 74) and wm.FULL == qa.encoded_vectors.FULL == 64
    assert len(_lib.declared_symbols()) == 192 and "DESIGN.md 3.1w" in hdr
    assert "### 3.1w" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "full_range=True" in open(os.path.join(ROOT, "README.md")).read()


def test_python_surface():
    E = qa.EncodedVectorsU8
    for fn in (E.encode, E.encode_stream):
        p = inspect.signature(fn).parameters["full_range"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(qa.VectorParameters.to_c).parameters)[1:] == ["rotated", "bits", "compact", "full_range"]
    vp = qa.VectorParameters(128, 7, D.L2, True)
    assert [qa.VectorParameters(128, 7, d, False).to_c(r, full_range=True).distance_type
            for d, r in ((D.Dot, False), (D.L1, False), (D.L2, False), (D.Dot, True), (D.L2, True))] == list(wm.LEGAL)
    assert vp.to_c(bits=8).distance_type == 2  # bits=8 alone stays the reference's 7 bits in a byte
    assert qa.VectorParameters.from_c(vp.to_c(True, full_range=True)) == vp
    with pytest.raises(qa.EncodingError, match="bits"):
        vp.to_c(bits=4, full_range=True)
    c = vp.to_c(full_range=True)
    assert _lib.lib().qamd_u8_quantized_vector_size(C.byref(c)) == 132


def test_legal_values_pass_the_flag_check():
    """A legal value and shape get as far as the null data pointer: the flag itself is accepted (fails without the feature)."""
    L, out = _lib.lib(), C.c_void_p()
    for dt, dim in ((64, 128), (65, 100), (66, 16384), (72, 128), (74, 16384)):
        v = _lib.VectorParametersC(dim, 3, dt, 0)
        st = L.qamd_u8_encode(None, 0, C.byref(v), None, None, _lib.STOP_FN(), None, None, C.byref(out))
        assert st == _lib.ERR_ARGUMENTS and L.qamd_last_error() == b"data is null" and out.value is None, (dt, L.qamd_last_error())


def test_refusals_need_no_device(tmp_path):
    got = wm.refusals(_lib, tmp_path)
    assert len(got) == 12 * 3 + 5 * 11 + 8
    for what, st, want, out in got:
        assert st == want and out is None, (what, st, want)
    for other in (cm, fm, um):  # the three older flags' lists hold as before
        for what, st, want, out in other.refusals(_lib, tmp_path):
            assert st == want and out is None, (what, st, want)
