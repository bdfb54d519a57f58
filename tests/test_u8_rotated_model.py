"""Rotated scalar-u8 stores without a GPU: the ABI's constants, the Python surface, the refusals that
come before any device call, the scale c, and what the rotation is for - on the ORACLE's encoder, rows whose columns
differ widely in scale are ranked better after the rotation than before it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import rotated_blocks_model as bm
import u8_rotated_model as um
from oracle import qoracle as qo

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

f32 = np.float32
D = qa.DistanceType


def test_header_and_symbols():
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "quantization_amd.h")).read()
    assert "typedef enum { QAMD_DOT = 0, QAMD_L1 = 1, QAMD_L2 = 2 } qamd_distance;\n" in hdr
    assert re.search(r"\} qamd_distance;\nenum \{ QAMD_ROTATED = 8,\s*/\*[^*]*\*/\s*QAMD_DOT_ROTATED = 8, QAMD_L2_ROTATED = 10 \};", hdr)
    assert len(_lib.declared_symbols()) == 192  # the flag rides qamd_vector_parameters: no entry point of its own
    assert "192 entry points" in hdr
    assert (um.ROTATED, um.DOT_ROTATED, um.L2_ROTATED) == (8, 0 | 8, 2 | 8)


def test_python_surface():
    E = qa.EncodedVectorsU8
    for fn in (E.encode, E.encode_stream):
        p = inspect.signature(fn).parameters["rotated"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert isinstance(E.rotated, property)
    vp = qa.VectorParameters(128, 7, D.L2, True)
    assert vp.to_c().distance_type == 2 and vp.to_c(True).distance_type == 10
    assert qa.VectorParameters(128, 7, D.Dot, False).to_c(rotated=True).distance_type == 8
    back = qa.VectorParameters.from_c(vp.to_c(True))  # the flag is taken off on the way back: distance_type is a DistanceType
    assert back == vp and isinstance(back.distance_type, D)
    # the base metric decides the sizes
    assert E.get_quantized_vector_size(vp) == 128 + 4 and E.get_actual_dim(vp) == 128
    c = vp.to_c(True)
    assert _lib.lib().qamd_u8_quantized_vector_size(C.byref(c)) == 132 and _lib.lib().qamd_u8_actual_dim(C.byref(c)) == 128
    with pytest.raises(qa.EncodingError, match="rotated"):
        qa.ShardedVectorsU8.encode(np.zeros((4, 128), f32), qa.VectorParameters(128, 4, D.Dot, False), [0], rotated=True)
    with pytest.raises(qa.EncodingError, match="rotation"):
        E.from_storage(np.zeros((0, 132), np.uint8), {"actual_dim": 128, "alpha": 1.0, "offset": 0.0, "multiplier": 1.0,
                                                      "vector_parameters": qa.VectorParameters(128, 0, D.Dot, False),
                                                      "rotation": "Givens"})


def test_refusals_need_no_device(tmp_path):
    """Every refusal of the flag is an argument (load: an IO) error raised before the library touches a device; null
    handles are refused as before."""
    got = um.refusals(_lib, tmp_path)
    assert len(got) == 7 * 3 + 2 * 14 + 5
    for what, st, want, out in got:
        assert st == want and out is None, (what, st, want)
    L = _lib.lib()
    md = _lib.U8MetadataC()
    assert L.qamd_u8_get_metadata(None, C.byref(md)) == _lib.ERR_ARGUMENTS
    q = C.c_void_p()
    assert L.qamd_u8_encode_query(None, None, 0, 0, None, C.byref(q)) == _lib.ERR_ARGUMENTS
    assert L.qamd_u8_upsert(None, 0, None, 0, 0, None) == _lib.ERR_ARGUMENTS
    assert L.qamd_u8_save(None, b"a", b"b") == _lib.ERR_ARGUMENTS


@pytest.mark.parametrize("b,bits", [(64, 0x3E000000), (128, 0x3DB504F3), (256, 0x3D800000), (512, 0x3D3504F3)])
def test_scale(b, bits):
    """c = 2^(-log2(B) / 2): 1/8 and 1/16 exactly; for B = 128 and 512 the f32 nearest to 2^-3.5 and 2^-4.5, the
    significand of sqrt(2) / 2 = 0x3F3504F3."""
    c = um.scale(b)
    assert c.dtype == f32 and int(c.view(np.uint32)) == bits
    assert abs(float(c) ** 2 * b - 1.0) < 2.0 ** -23  # c^2 B = 1 to f32 rounding: the scaled rotation is orthonormal


@pytest.mark.parametrize("dim", [64, 128, 192, 768, 1536])
def test_rotation_keeps_dot_products(dim):
    """y^ = c H_B (signs * x) is orthonormal up to rounding: dot products and squared distances survive to a few ulp of
    the norms' product.  Each value of y^ is a sum of B terms of f32 rounding 2^-24 each, log2(B) levels deep."""
    rng = np.random.default_rng(dim)
    x = rng.normal(size=(40, dim)).astype(f32)
    y = um.rotate(x)
    assert y.shape == x.shape and y.dtype == f32
    exact, rot = x.astype(np.float64) @ x.astype(np.float64).T, y.astype(np.float64) @ y.astype(np.float64).T
    norms = np.sqrt(np.diag(exact))
    depth = bm.block(dim).bit_length()  # butterfly levels + the multiply
    assert np.abs(rot - exact).max() <= 2.0 ** -23 * depth * np.outer(norms, norms).max()
    assert np.abs(rot - exact).max() > 0.0  # (a rotation, not a copy)


def _recall(seed, rotated):
    """recall@10 of the oracle's u8 Dot scores against the exact f32 ranking: 20000 x 128 rows with column scales
    exp(N(0, 1)), normalised; 100 queries = rows plus noise."""
    rng = np.random.default_rng(seed)
    n, dim, nq, k = 20000, 128, 100, 10
    x = rng.normal(size=(n, dim)) * np.exp(rng.normal(size=dim))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(f32)
    q = x[rng.choice(n, nq, replace=False)] + (0.3 / np.sqrt(dim)) * rng.normal(size=(nq, dim))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    exact = q.astype(np.float64) @ x.astype(np.float64).T
    rows, meta = um.encode(x, qo.DOT, False) if rotated else qo.u8_encode(x, qo.DOT, False)
    hits = 0
    for i in range(nq):
        codes, qoff = um.encode_query(meta, q[i]) if rotated else qo.u8_encode_query(meta, q[i])
        got = qo.u8_score_all(meta, rows, codes, qoff)
        hits += len(set(np.argsort(-got, kind="stable")[:k]) & set(np.argsort(-exact[i], kind="stable")[:k]))
    return hits / (nq * k)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rotation_improves_recall_on_unequal_columns(seed):
    plain, rot = _recall(seed, False), _recall(seed, True)
    print(f"seed {seed}: recall@10 plain {plain:.3f}, rotated {rot:.3f}")
    assert rot > plain
