"""4-bit scalar-u8 stores without a GPU: the ABI's constants, the Python surface, the refusals that come
before any device call, the numpy model of the nibble image and of one lane's sums against the oracle's integer pair
sums, and what the model says about recall: 4-bit rows need the rotation, and the code must round to nearest."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import u8_four_bit_model as fm
import u8_rotated_model as um
from oracle import qoracle as qo

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

f32 = np.float32
D = qa.DistanceType


def test_header_and_symbols():
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "quantization_amd.h")).read()
    assert re.search(r"QAMD_DOT_ROTATED = 8, QAMD_L2_ROTATED = 10 \};\nenum \{ QAMD_BITS4 = 32,\s*/\*[^*]*\*/\s*QAMD_DOT_BITS4 = 32, "
                     r"QAMD_L2_BITS4 = 34, QAMD_DOT_ROTATED_BITS4 = 40, QAMD_L2_ROTATED_BITS4 = 42 \};", hdr)
    assert len(_lib.declared_symbols()) == 192  # the flag rides qamd_vector_parameters: no entry point of its own
    assert "192 entry points" in hdr and "DESIGN.md 3.1y" in hdr and "1156" in hdr
    assert (fm.BITS4, fm.DOT_BITS4, fm.L2_BITS4, fm.DOT_ROTATED_BITS4, fm.L2_ROTATED_BITS4) == (32, 0 | 32, 2 | 32, 0 | 8 | 32,
                                                                                                 2 | 8 | 32)
    root = os.path.dirname(_lib.HERE)
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "### 3.1y" in design and "192 entry points" in design
    assert "QAMD_BITS4" in open(os.path.join(root, "INTEGRATION.md")).read()
    assert "bits=4" in open(os.path.join(root, "README.md")).read()


def test_python_surface():
    E = qa.EncodedVectorsU8
    for fn in (E.encode, E.encode_stream):
        p = inspect.signature(fn).parameters["bits"]
        assert p.default == 8 and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert isinstance(E.bits, property)
    vp = qa.VectorParameters(128, 7, D.L2, True)
    assert vp.to_c().distance_type == 2 and vp.to_c(bits=8).distance_type == 2
    assert vp.to_c(bits=4).distance_type == 34 and vp.to_c(True, 4).distance_type == 42
    assert qa.VectorParameters(128, 7, D.Dot, False).to_c(rotated=True, bits=4).distance_type == 40
    assert qa.VectorParameters(128, 7, D.Dot, False).to_c(False, 4).distance_type == 32
    for c in (vp.to_c(bits=4), vp.to_c(True, 4)):  # both flags are taken off on the way back
        back = qa.VectorParameters.from_c(c)
        assert back == vp and isinstance(back.distance_type, D)
    with pytest.raises(qa.EncodingError, match="bits"):
        vp.to_c(bits=7)
    # dim alone decides the sizes
    assert E.get_quantized_vector_size(vp) == 128 + 4 and E.get_actual_dim(vp) == 128
    for c in (vp.to_c(bits=4), vp.to_c(True, 4), qa.VectorParameters(20, 7, D.Dot, False).to_c(bits=4)):
        ad = (int(c.dim) + 15) // 16 * 16
        assert _lib.lib().qamd_u8_quantized_vector_size(C.byref(c)) == ad + 4 and _lib.lib().qamd_u8_actual_dim(C.byref(c)) == ad
    with pytest.raises(qa.EncodingError, match="4-bit"):
        qa.ShardedVectorsU8.encode(np.zeros((4, 128), f32), qa.VectorParameters(128, 4, D.Dot, False), [0], bits=4)
    with pytest.raises(qa.EncodingError, match="bits"):
        E.from_storage(np.zeros((0, 132), np.uint8), {"actual_dim": 128, "alpha": 1.0, "offset": 0.0, "multiplier": 1.0,
                                                      "vector_parameters": qa.VectorParameters(128, 0, D.Dot, False),
                                                      "bits": 2})


def test_refusals_need_no_device(tmp_path):
    """Every refusal of the flag is an argument (load: an IO) error raised before the library touches a device, and the
    rotated flag's own refusals - bit 16 among them - hold as before."""
    got = fm.refusals(_lib, tmp_path)
    assert len(got) == 11 * 3 + 4 * 14 + 9
    for what, st, want, out in got:
        assert st == want and out is None, (what, st, want)
    for what, st, want, out in um.refusals(_lib, tmp_path):
        assert st == want and out is None, (what, st, want)


def test_code_is_rounded_three_f32_operations():
    """code() on hand-worked values: alpha = 0.1f, offset = -0.75f."""
    a, o = f32(0.1), f32(-0.75)
    v = np.array([-0.75, -0.70, -0.7000001, 0.75, 0.70, 0.6999, 1e30, -1e30, np.inf, -np.inf, np.nan, -0.0], f32)
    want = []
    for x in v:
        t = f32(f32(f32(x - o) / a) + f32(0.5))
        want.append(0 if np.isnan(t) else int(min(max(t, f32(0)), f32(15))))
    with np.errstate(all="ignore"):
        assert fm.code(v, a, o).tolist() == want
    assert want[0] == 0 and want[3] == 15 and want[6] == 15 and want[7] == 0 and want[8] == 15 and want[9] == 0 and want[10] == 0
    assert fm.code(v, a, o, rounded=False).tolist()[1] == 0 and want[1] == 1  # 0.5 steps up: rounds to 1, truncates to 0
    # the pad codes: 0.0 for Dot, offset for L2, through code()
    rows, meta = fm.encode_values(np.full((1, 20), 0.3, f32), qo.DOT, False, a, o)
    assert rows.shape == (1, 36) and set(rows[0, 4 + 20:]) == {int(fm.code(f32(0.0), a, o))} == {8}
    rows, meta = fm.encode_values(np.full((1, 20), 0.3, f32), qo.L2, False, a, o)
    assert set(rows[0, 4 + 20:]) == {0}
    assert meta.actual_dim == 32 and f32(meta.multiplier) == f32(-2.0) * a * a


@pytest.mark.parametrize("distance", [qo.DOT, qo.L2])
@pytest.mark.parametrize("invert", [False, True])
def test_row_and_query_offsets_are_the_references(distance, invert):
    """The model's row and query offsets against the oracle's own encoder run with the model's alpha and offset on values
    that lie ON the 4-bit levels shifted by half a step - where truncation and rounding give the same code."""
    rng = np.random.default_rng(5 + distance)
    a, o = f32(0.125), f32(-1.0)
    lv = rng.integers(0, 16, size=(9, 40))
    y = (o + a * lv.astype(f32)).astype(f32)  # exact in f32: powers of two
    rows, meta = fm.encode_values(y, distance, invert, a, o)
    assert np.array_equal(rows[:, 4:44], lv)
    ref_rows, ref_meta = qo.u8_encode_with(y, distance, invert, a, o)  # truncating code on exact levels: the same codes
    assert np.array_equal(ref_rows, rows)
    for f in ("actual_dim", "alpha", "offset", "multiplier", "dim", "count", "distance_type", "invert"):
        assert getattr(meta, f) == getattr(ref_meta, f), f
    qc, qoff = fm.encode_query(meta, y[3], rotated=False)
    rc, roff = qo.u8_encode_query(ref_meta, y[3])
    assert np.array_equal(qc, rc) and qoff.view(np.uint32) == roff.view(np.uint32)


@pytest.mark.parametrize("rc", [1, 2, 3, 16, 17, 18, 32, 48, 96, 127, 128])
def test_nibble_pack_and_lane_sums(rc):
    """The pack keeps every code, and a lane's sums over it are the oracle's integer pair sums: odd rc (the last chunk
    has no high half), rc = 2 (one chunk), and every code 15 against a query of 15s (the largest sums)."""
    rng = np.random.default_rng(rc)
    n, ad = 5, 16 * rc
    codes = rng.integers(0, 16, size=(n, ad), dtype=np.uint8)
    codes[0] = 15
    q = rng.integers(0, 16, size=ad, dtype=np.uint8)
    img = fm.pack_rows(codes)
    assert img.shape == (n, (rc + 1) // 2, 16)
    lo, hi = (img & 0x0F).reshape(n, -1), (img >> 4).reshape(n, -1)
    back = np.stack([lo.reshape(n, -1, 16), hi.reshape(n, -1, 16)], axis=2).reshape(n, -1)[:, :ad]
    assert np.array_equal(back, codes)
    if rc % 2:
        assert not (img[:, -1] >> 4).any()
    for query in (q, np.full(ad, 15, np.uint8)):
        for r in range(n):
            want = int(qo.lib().qo_dot_i32(qo._p(query), qo._p(np.ascontiguousarray(codes[r])), ad))
            assert fm.lane_sum(img[r], query, rc) == want
    assert fm.lane_sum(img[0], np.full(ad, 15, np.uint8), rc) == 225 * ad
    # the blocked image: chunk j of row r at 16-byte index ((r / 64) * P4 + j) * 64 + r % 64
    many = rng.integers(0, 16, size=(70, ad), dtype=np.uint8)
    blocked = fm.block_image(fm.pack_rows(many), 128).reshape(-1, 16)
    p4 = (rc + 1) // 2
    for r, j in ((0, 0), (63, p4 - 1), (64, 0), (69, p4 - 1)):
        assert np.array_equal(blocked[((r // 64) * p4 + j) * 64 + r % 64], fm.pack_rows(many[r:r + 1])[0, j])
    assert not blocked[(p4 + 0) * 64 + 6:(p4 + 1) * 64].any()  # rows 70 .. 127 of block 1, chunk 0


def _recall(seed, rotated, quantile=None, rounded=True):
    """recall@10 of the model's 4-bit Dot scores against the exact f32 ranking, by the recipe of
    test_u8_rotated_model._recall: 20000 x 128 rows with column scales exp(N(0, 1)), normalised; 100 queries = rows plus
    noise."""
    rng = np.random.default_rng(seed)
    n, dim, nq, k = 20000, 128, 100, 10
    x = rng.normal(size=(n, dim)) * np.exp(rng.normal(size=dim))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(f32)
    q = x[rng.choice(n, nq, replace=False)] + (0.3 / np.sqrt(dim)) * rng.normal(size=(nq, dim))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    exact = q.astype(np.float64) @ x.astype(np.float64).T
    rows, meta = fm.encode(x, qo.DOT, False, rotated, quantile=quantile, rounded=rounded)
    hits = 0
    for i in range(nq):
        codes, qoff = fm.encode_query(meta, q[i], rotated, rounded=rounded)
        got = qo.u8_score_all(meta, rows, codes, qoff)
        hits += len(set(np.argsort(-got, kind="stable")[:k]) & set(np.argsort(-exact[i], kind="stable")[:k]))
    return hits / (nq * k)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_four_bit_needs_the_rotation_and_the_rounding(seed):
    """Four comparisons per seed, for the model alone: rotated > plain (min/max and quantile 0.99 intervals alike) and,
    on the rotated store, rounded > truncated with min/max and with quantile 0.99."""
    plain, rot = _recall(seed, False), _recall(seed, True)
    rot_q, rot_trunc, rot_q_trunc = _recall(seed, True, 0.99), _recall(seed, True, rounded=False), _recall(seed, True, 0.99, False)
    print(f"seed {seed}: recall@10 4-bit plain {plain:.3f}, rotated {rot:.3f}, rotated quantile 0.99 {rot_q:.3f}, "
          f"rotated truncating {rot_trunc:.3f}, rotated quantile 0.99 truncating {rot_q_trunc:.3f}")
    assert rot > plain
    assert rot_q > plain
    assert rot > rot_trunc
    assert rot_q > rot_q_trunc
