"""Compact 4-bit scalar-u8 stores without a GPU: the ABI's constant and its four legal values, the
Python surface, every refusal that comes before a device call, the key order of the metadata file, and the numpy
restatement of the nibble gather address and expansion against u8_four_bit_model's pack and blocked image."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import u8_compact_model as cm
import u8_four_bit_model as fm
import u8_rotated_model as um
from oracle import qoracle as qo

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

f32 = np.float32
D = qa.DistanceType
ROOT = os.path.dirname(_lib.HERE)


def test_header_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "quantization_amd.h")).read()
    assert re.search(r"QAMD_L2_ROTATED_BITS4 = 42 \};\nenum \{ QAMD_COMPACT = 128,\s*/\*[^*]*\*/\s*QAMD_DOT_BITS4_COMPACT = 160, "
                     r"QAMD_L2_BITS4_COMPACT = 162, QAMD_DOT_ROTATED_BITS4_COMPACT = 168,\s*QAMD_L2_ROTATED_BITS4_COMPACT = 170 \};",
                     hdr)
    assert len(_lib.declared_symbols()) == 192  # the flag rides qamd_vector_parameters: no entry point of its own
    assert "192 entry points" in hdr and "DESIGN.md 3.1z" in hdr and "2^24" in hdr
    assert cm.LEGAL == tuple(cm.COMPACT | fm.BITS4 | base | rot for rot in (0, um.ROTATED) for base in (0, 2)) == (160, 162, 168, 170)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.1z" in design and "192 entry points" in design
    assert "compact=True" in open(os.path.join(ROOT, "README.md")).read()
    # the product library has no symbol of the feature; the developer library's accessor is not in the header
    assert not [s for s in _lib.declared_symbols() if "compact" in s or "store_bytes" in s]


def test_python_surface():
    E = qa.EncodedVectorsU8
    for fn in (E.encode, E.encode_stream):
        p = inspect.signature(fn).parameters["compact"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(E.from_storage).parameters["compact"].default is False
    assert isinstance(E.compact, property)
    vp = qa.VectorParameters(128, 7, D.L2, True)
    assert vp.to_c(bits=4, compact=True).distance_type == 162 and vp.to_c(True, 4, True).distance_type == 170
    assert qa.VectorParameters(128, 7, D.Dot, False).to_c(bits=4, compact=True).distance_type == 160
    assert qa.VectorParameters(128, 7, D.Dot, False).to_c(rotated=True, bits=4, compact=True).distance_type == 168
    assert vp.to_c(bits=4, compact=False).distance_type == 34
    for c in (vp.to_c(bits=4, compact=True), vp.to_c(True, 4, True)):  # every flag is taken off on the way back
        back = qa.VectorParameters.from_c(c)
        assert back == vp and isinstance(back.distance_type, D)
    for bits in (8, 7):
        with pytest.raises(qa.EncodingError, match="bits"):
            vp.to_c(bits=bits, compact=True)
    with pytest.raises(qa.EncodingError, match="bits"):
        E.encode(np.zeros((7, 128), f32), vp, compact=True)
    with pytest.raises(qa.EncodingError, match="bits"):
        E.encode_stream(lambda: iter([np.zeros((7, 128), f32)]), vp, compact=True)
    with pytest.raises(qa.EncodingError, match="bits"):
        E.from_storage(np.zeros((0, 132), np.uint8), {"actual_dim": 128, "alpha": 1.0, "offset": 0.0, "multiplier": 1.0,
                                                      "vector_parameters": qa.VectorParameters(128, 0, D.Dot, False),
                                                      "compact": True})
    with pytest.raises(qa.EncodingError, match="compact"):
        qa.ShardedVectorsU8.encode(np.zeros((4, 128), f32), qa.VectorParameters(128, 4, D.Dot, False), [0], bits=4, compact=True)
    # dim alone decides the sizes of the reference's rows, which is what a compact store exports and saves
    c = vp.to_c(bits=4, compact=True)
    assert _lib.lib().qamd_u8_quantized_vector_size(C.byref(c)) == 132 and _lib.lib().qamd_u8_actual_dim(C.byref(c)) == 128


def test_refusals_need_no_device(tmp_path):
    """Every refusal of the flag is an argument (load: an IO) error raised before the library touches a device, and the
    refusals the two older flags pin hold as before."""
    got = cm.refusals(_lib, tmp_path)
    assert len(got) == cm.N_REFUSALS
    for what, st, want, out in got:
        assert st == want and out is None, (what, st, want)
    for other in (fm, um):
        for what, st, want, out in other.refusals(_lib, tmp_path):
            assert st == want and out is None, (what, st, want)


def test_metadata_key_order():
    """save writes the base metric, then "rotation", then "bits":4, then the last key "compact":true - stated here from the
    writer's source, which a test without a device cannot run."""
    src = open(os.path.join(ROOT, "quantization_amd", "csrc", "u8.hip")).read()
    body = src[src.index("qamd_status qamd_u8_save("):]
    body = body[:body.index("save_file(meta_path")]
    keys = re.findall(r'\\"([a-z_]+)\\":', body)
    assert keys == ["actual_dim", "alpha", "offset", "multiplier", "vector_parameters", "rotation", "bits", "compact"]
    assert re.search(r'h->compact \? ",\\"compact\\":true" : ""\) \+ "\}"', body)


@pytest.mark.parametrize("rc", [2, 3, 16, 17, 48, 96, 127, 128])
def test_gather_address_and_expansion(rc):
    """unpack_row and pair_sum, written from the image format, against u8_four_bit_model's pack_rows / block_image and
    the oracle's integer pair sums: rows at both ends of a block and in the last, partly filled one; odd rc."""
    rng = np.random.default_rng(rc)
    n, ad = 131, 16 * rc
    codes = rng.integers(0, 16, size=(n, ad), dtype=np.uint8)
    codes[64] = 15
    blocked = fm.block_image(fm.pack_rows(codes), 192)
    p = cm.chunks_of(ad)
    assert p == (rc + 1) // 2 and blocked.size == 192 * p * 16
    assert cm.gather_index(0, 0, p) == 0 and cm.gather_index(63, p - 1, p) == (p - 1) * 64 + 63
    assert cm.gather_index(64, 0, p) == p * 64 and cm.gather_index(130, 1 % p, p) == (2 * p + 1 % p) * 64 + 2
    q = rng.integers(0, 16, size=ad, dtype=np.uint8)
    for r in (0, 1, 63, 64, 65, 127, 128, 130):
        assert np.array_equal(cm.unpack_row(blocked, r, rc), codes[r]), r
        for query in (q, np.full(ad, 15, np.uint8)):
            want = int(qo.lib().qo_dot_i32(qo._p(query), qo._p(np.ascontiguousarray(codes[r])), ad))
            assert cm.pair_sum(blocked, r, rc, qcodes=query) == want == fm.lane_sum(fm.pack_rows(codes[r:r + 1])[0], query, rc)
        for other in (64, 130, r):
            want = int(qo.lib().qo_dot_i32(qo._p(np.ascontiguousarray(codes[other])), qo._p(np.ascontiguousarray(codes[r])), ad))
            assert cm.pair_sum(blocked, r, rc, qrow=other) == want
    assert cm.pair_sum(blocked, 64, rc, qrow=64) == 225 * ad < 1 << 24  # the largest sum: exact in f32 in either lane mode
    assert not cm.unpack_row(blocked, 131, rc).any()  # a padding row
    assert cm.store_bytes(2048, 768) == 2048 * 388
