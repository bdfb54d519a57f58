"""Rotated scalar-u8 stores on the GPU, every comparison on raw bits.

1. Encode parity with the model (u8_rotated_model.py: the numpy block rotation, one f32 multiply, the oracle's encoder).
2. Same bytes, same answers: a PLAIN handle adopted from the rotated store's bytes answers every scoring call with the
   same bits when it is asked with the already-rotated query - no scan route knows about the rotation.
3. The other write paths (streaming encoder, upsert / append, save / load, metadata / from_storage) and rescoring.
4. The refusals, each before any launch.

The dims are the smallest at which each path of the two kernel forms can go wrong: a single block with even and with odd
log2(B) (the inexact c), idle lanes in the only chunk, the workload's dim, a chunk stage, and the workgroup-per-row form
with many small blocks and with one large one; 1, 65 and 1025 rows are one wave, one pass of several workgroups, and
more rows than one pass of the wave-per-row grid's workgroup holds, with a last tile that is not full."""
import functools

import numpy as np
import pytest

import u8_rotated_model as um
from oracle import qoracle as qo
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

E = qa.EncodedVectorsU8
D = qa.DistanceType
f32 = np.float32

# dim: (B, metric, invert)
SHAPES = {
    64: (64, D.Dot, False),      # single block, even log2 B
    128: (128, D.L2, True),      # odd log2 B, inexact c
    192: (64, D.Dot, False),     # 3 blocks, idle lanes in the only chunk
    768: (256, D.L2, False),     # the workload's dim
    1536: (512, D.Dot, True),    # odd log2 B, one chunk stage
    2112: (64, D.L2, True),      # 33 blocks, LDS form
    4096: (4096, D.L2, False),   # one block, LDS form; L2 code sums past 2^24
}
ROWS = (1, 65, 1025)
CASES = [(dim, n) for dim in SHAPES for n in ROWS]
# Every K = ceil(dim / 256) of the wave-per-row frame, its chunk stages taken and not taken, and the ends of the
# workgroup-per-row frame: encode parity and same bytes at 65 rows (one pass of several workgroups).
MORE_SHAPES = {
    256: (256, D.Dot, False),      # K = 1, all six lane stages
    320: (64, D.L2, False),        # K = 2, half-empty last chunk
    512: (512, D.Dot, True),       # K = 2, the chunk stage
    832: (64, D.L2, True),         # K = 4 with B = 64: the chunk stages 1 and 2 present but not taken
    1024: (1024, D.L2, False),     # K = 4, chunk stages 1 and 2
    1280: (256, D.Dot, False),     # K = 5
    1792: (256, D.L2, True),       # K = 7
    1984: (64, D.Dot, True),       # K = 8, idle lanes, B = 64
    2048: (2048, D.L2, False),     # K = 8, chunk stages 1, 2, 4
    12288: (4096, D.Dot, False),   # LDS form, B = 4096, three blocks
    16384: (16384, D.L2, False),   # the largest row
}
SHAPES.update(MORE_SHAPES)
MORE_CASES = CASES + [(dim, 65) for dim in MORE_SHAPES]


def _data(n, dim, seed):
    """Gaussian rows with one column 100 x the rest, and -0.0 entries."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, dim)).astype(f32)
    x[:, (7 * dim) // 13] *= f32(100.0)
    x[n // 2, ::5] = f32(-0.0)
    return x


def _specials(x, nan_only):
    """x with a NaN planted and (unless nan_only) +inf and -inf, in different rows where there are three."""
    n, dim = x.shape
    x = x.copy()
    x[0, dim // 3] = np.nan
    if not nan_only:
        x[(n // 3) % n, dim // 2] = np.inf
        x[(2 * n // 3) % n, dim - 1] = -np.inf
    return x


@functools.lru_cache(maxsize=None)
def _case(dim, n):
    """The data and the model's stores of a shape, computed once and shared (nothing here is written to)."""
    _, dist, invert = SHAPES[dim]
    x = _data(n, dim, dim * 10 + n)
    rows, meta = um.encode(x, int(dist), invert)
    rng = np.random.default_rng(dim + n)
    q = rng.normal(size=dim).astype(f32)
    qs = rng.normal(size=(5, dim)).astype(f32)
    for a in (x, rows, q, qs):
        a.setflags(write=False)
    return {"x": x, "dist": dist, "invert": invert, "vp": qa.VectorParameters(dim, n, dist, invert), "rows": rows,
            "meta": meta, "q": q, "qs": qs}


def _check_store(h, rows, meta, what, nan_offsets=False):
    """nan_offsets: the interval is infinite and every row offset a NaN, whose sign and payload are the machine's: the
    offsets are then compared as numbers, NaN equal to NaN; the codes and the interval stay bits."""
    md = h.metadata
    assert h.rotated and md["rotation"] == um.ROTATION_NAME, what
    assert_bits_equal(np.array([md["alpha"], md["offset"], md["multiplier"]], f32),
                      np.array([meta.alpha, meta.offset, meta.multiplier], f32), f"{what}: alpha, offset, multiplier")
    got = h.storage_bytes()
    if nan_offsets:
        assert np.array_equal(got[:, 4:], rows[:, 4:]), f"{what}: codes differ from the model"
        g, w = np.ascontiguousarray(got[:, :4]).view(f32), np.ascontiguousarray(rows[:, :4]).view(f32)
        assert np.array_equal(g, w, equal_nan=True), f"{what}: row offsets"
    else:
        assert np.array_equal(got, rows), f"{what}: rows differ from the model"


def _check_query(h, meta, q, what):
    eq = h.encode_query(q)
    codes, off = um.encode_query(meta, q)
    assert np.array_equal(eq.encoded_query, codes), f"{what}: query codes"
    assert_bits_equal(np.array([eq.offset], f32), np.array([off], f32), f"{what}: query offset")
    return eq


# ------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("dim,n", MORE_CASES)
def test_encode_parity(dim, n):
    import torch

    c = _case(dim, n)
    x, vp, dist, invert = c["x"], c["vp"], int(c["dist"]), c["invert"]
    # min/max, from a device tensor (encoded in place), from host rows (staged) and from a device tensor that is not
    # 16-byte aligned (dword loads)
    off1 = torch.zeros(n * dim + 1, dtype=torch.float32, device="cuda")
    off1[1:] = torch.from_numpy(x.copy()).cuda().reshape(-1)
    for src in (torch.from_numpy(x.copy()).cuda(), x, off1[1:].view(n, dim)):
        h = E.encode(src, vp, rotated=True)
        _check_store(h, c["rows"], c["meta"], "min/max")
        assert h.vector_parameters == vp  # the base metric: distance_type stays a DistanceType
    _check_query(h, c["meta"], c["q"], "min/max")
    # many queries at once: their scores are the oracle's on the model's query codes (the batch keeps its codes on the device)
    got = h.score_batch(h.encode_query_batch(c["qs"]))
    for i in (0, len(c["qs"]) - 1):
        codes, off = um.encode_query(c["meta"], c["qs"][i])
        assert_bits_equal(got[i], qo.u8_score_all(c["meta"], c["rows"], codes, off, order=qo.ORDER_SIMPLE), f"batch query {i}")
    # quantile (a no-op below 127 rows, as in the reference)
    rows, meta = um.encode(x, dist, invert, quantile=0.99)
    h = E.encode(x, vp, 0.99, rotated=True)
    _check_store(h, rows, meta, "quantile")
    _check_query(h, meta, c["q"], "quantile")
    # a given interval, from a source that is not 16-byte aligned (dword loads), rows holding NaN and +-inf
    xs = _specials(x, nan_only=False)
    ao = (float(c["meta"].alpha), float(c["meta"].offset))
    rows, meta = um.encode(xs, dist, invert, alpha_offset=ao)
    flat = torch.zeros(n * dim + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(xs).cuda().reshape(-1)
    h = E.encode(flat[1:].view(n, dim), vp, alpha_offset=ao, rotated=True)
    _check_store(h, rows, meta, "alpha_offset, unaligned, specials")
    # min/max skips NaN as the reference's `value < min` does
    xn = _specials(x, nan_only=True)
    rows, meta = um.encode(xn, dist, invert)
    _check_store(E.encode(xn, vp, rotated=True), rows, meta, "min/max with NaN")
    # ... and takes infinities for what they are
    rows, meta = um.encode(xs, dist, invert)
    _check_store(E.encode(xs, vp, rotated=True), rows, meta, "min/max with +-inf", nan_offsets=True)


@pytest.mark.parametrize("dim", [64, 1024, 1536, 2048, 2112])
def test_zero_extreme_keeps_the_first_zeros_sign(dim):
    """Rows of zeros: every rotated value is a zero, and min == max == 0 carry the sign of the first one in row order."""
    for first in (0.0, -0.0):
        x = np.zeros((3, dim), f32)
        x[0, :4] = f32(first)
        x[1, 5::2] = f32(-0.0)
        rows, meta = um.encode(x, qo.DOT, False)
        h = E.encode(x, qa.VectorParameters(dim, 3, D.Dot, False), rotated=True)
        _check_store(h, rows, meta, f"zeros, first {first!r}")


@pytest.mark.parametrize("dim", [1536, 2048, 2112])
def test_l2_offsets_past_2_24(dim):
    """An L2 row whose sum of squared codes reaches 2^24 takes the reference's sequential f32 sum: an interval that puts
    every code at 110 or above (110^2 * 1536 > 2^24), in the wave form and in the workgroup form."""
    x = _data(65, dim, 5)
    y = um.rotate(x)
    alpha = float(f32((y.max() - y.min()) / 17.0))
    ao = (alpha, float(f32(y.min() - 110.0 * alpha)))
    rows, meta = um.encode(x, qo.L2, False, alpha_offset=ao)
    assert rows[:, 4:].min() >= 100 and (rows[:, 4:].astype(np.int64) ** 2).sum(axis=1).min() >= 1 << 24
    h = E.encode(x, qa.VectorParameters(dim, 65, D.L2, False), alpha_offset=ao, rotated=True)
    _check_store(h, rows, meta, "L2 past 2^24")


# ------------------------------------------------------------------------------- 2. same bytes, same answers
@pytest.mark.parametrize("dim,n", MORE_CASES)
def test_same_bytes_same_answers(dim, n):
    c = _case(dim, n)
    rot = E.encode(c["x"], c["vp"], rotated=True)
    md = dict(rot.metadata)
    del md["rotation"]
    plain = E.from_storage(rot.storage_bytes(), md)
    assert not plain.rotated and plain.vector_parameters == rot.vector_parameters
    q_r, q_p = rot.encode_query(c["q"]), plain.encode_query(um.rotate(c["q"])[0])
    b_r, b_p = rot.encode_query_batch(c["qs"]), plain.encode_query_batch(um.rotate(c["qs"]))
    assert np.array_equal(q_r.encoded_query, q_p.encoded_query)
    rng = np.random.default_rng(n)
    ids = rng.integers(0, n, size=min(n, 40)).astype(np.uint32)
    k = min(n, 10)
    srows = rng.integers(0, n, size=3).astype(np.uint32)
    offs = np.array([0, min(2, len(ids)), min(2, len(ids)), len(ids)], np.uint32)  # ragged, one empty list
    lists_q = np.array([0, 1, 1, len(ids)], np.uint32)
    i, j = int(srows[0]), int(ids[0])

    def both(call):
        return call(rot, q_r, b_r), call(plain, q_p, b_p)

    def same(call, what):
        g, w = both(call)
        for a, b in zip(g if isinstance(g, tuple) else (g,), w if isinstance(w, tuple) else (w,)):
            a, b = np.asarray(a), np.asarray(b)
            if a.dtype == np.float32:
                assert_bits_equal(a, b, what)
            else:
                assert np.array_equal(a, b), what

    same(lambda h, q, b: h.score_all(q), "score_all")
    same(lambda h, q, b: h.score_ids(q, ids), "score_ids")
    same(lambda h, q, b: np.array([h.score_point(q, j)], f32), "score_point")
    same(lambda h, q, b: h.topk(q, k), "topk")
    same(lambda h, q, b: h.topk(q, k, largest=False), "topk smallest")
    same(lambda h, q, b: h.score_batch(b), "score_batch")
    same(lambda h, q, b: h.topk_batch(b, k), "topk_batch")
    same(lambda h, q, b: h.score_ids_batch(h.encode_query_batch(c["qs"][:3] if h is rot else um.rotate(c["qs"][:3])),
                                           lists_q, ids), "score_ids_batch")
    same(lambda h, q, b: np.array([h.score_internal(i, j)], f32), "score_internal")
    same(lambda h, q, b: h.score_internal_ids(i, ids), "score_internal_ids")
    same(lambda h, q, b: h.score_internal_all(i), "score_internal_all")
    same(lambda h, q, b: h.topk_internal(i, k), "topk_internal")
    same(lambda h, q, b: h.score_internal_ids_batch(srows, offs, ids), "score_internal_ids_batch")
    same(lambda h, q, b: h.score_internal_all_batch(srows), "score_internal_all_batch")
    same(lambda h, q, b: h.topk_internal_batch(srows, k), "topk_internal_batch")
    # and the scores are the oracle's on the model's bytes
    codes, off = um.encode_query(c["meta"], c["q"])
    assert_bits_equal(rot.score_all(q_r), qo.u8_score_all(c["meta"], c["rows"], codes, off, order=qo.ORDER_SIMPLE), "oracle")


# -------------------------------------------------------------------------------------- 3. other write paths
@pytest.mark.parametrize("dim,n", CASES)
def test_write_paths(dim, n, tmp_path):
    c = _case(dim, n)
    x, vp, dist, invert = c["x"], c["vp"], int(c["dist"]), c["invert"]
    cuts = sorted({0, min(n, 1), min(n, 38), min(n, 39), min(n, 700), n})  # uneven batches, an empty one included

    def batches():
        yield x[:0]
        for a, b in zip(cuts[:-1], cuts[1:]):
            yield x[a:b]

    st = E.encode_stream(batches, vp, rotated=True)
    _check_store(st, c["rows"], c["meta"], "streaming, min/max")
    rows_q, meta_q = um.encode(x, dist, invert, quantile=0.98)
    _check_store(E.encode_stream(batches, vp, 0.98, rotated=True), rows_q, meta_q, "streaming, quantile")
    # upsert and append: the final data under the store's own interval
    rng = np.random.default_rng(n + dim)
    extra = rng.normal(size=(n + 3, dim)).astype(f32)
    final = np.concatenate([x, extra[n:]])
    final[n // 2:n // 2 + 1] = extra[:1]
    st.upsert(n // 2, extra[:1])
    st.append(extra[n:])
    ao = (float(c["meta"].alpha), float(c["meta"].offset))
    rows_f, meta_f = um.encode(final, dist, invert, alpha_offset=ao)
    assert st.count == n + 3 and st.rotated
    assert np.array_equal(st.storage_bytes(), rows_f), "upsert / append"
    q_enc = _check_query(st, c["meta"], c["q"], "after upsert")
    # the scans of the written store (its 7-bit image follows the rows): the oracle's scores on the model's bytes
    codes, off = um.encode_query(c["meta"], c["q"])
    assert_bits_equal(st.score_all(q_enc), qo.u8_score_all(meta_f, rows_f, codes, off, order=qo.ORDER_SIMPLE), "scores after upsert")
    # save -> load and metadata -> from_storage
    st.save(tmp_path / "rows.bin", tmp_path / "meta.json")
    text = (tmp_path / "meta.json").read_text()
    assert text.endswith(',"rotation":"HadamardBlocks"}') and f'"distance_type":"{c["dist"].name}"' in text
    ld = E.load(tmp_path / "rows.bin", tmp_path / "meta.json", qa.VectorParameters(dim, n + 3, c["dist"], invert))
    fs = E.from_storage(st.storage_bytes(), st.metadata)
    for h in (ld, fs):
        assert h.rotated and h.metadata == st.metadata
        assert np.array_equal(h.storage_bytes(), rows_f)
        _check_query(h, c["meta"], c["q"], "reloaded")
        assert_bits_equal(h.score_all(h.encode_query(c["q"])), st.score_all(q_enc), "reloaded scores")
    # a plain file stays plain
    plain = E.encode(x, vp)
    plain.save(tmp_path / "p.bin", tmp_path / "p.json")
    assert "rotation" not in (tmp_path / "p.json").read_text() and "rotation" not in plain.metadata and not plain.rotated
    assert not E.load(tmp_path / "p.bin", tmp_path / "p.json", vp).rotated
    # rescoring against PLAIN originals: the base metric matches, the candidates come from the rotated scan
    orig = qa.OriginalVectors.from_data(final, qa.VectorParameters(dim, n + 3, c["dist"], invert))
    k, cand = min(n + 3, 5), min(n + 3, 50)
    cids, _ = st.topk(q_enc, cand)
    ids_r, sc_r = st.topk_rescored(q_enc, orig, c["q"], k, cand)
    ids_w, sc_w = orig.rerank(c["q"], cids, k)
    assert np.array_equal(ids_r, ids_w)
    assert_bits_equal(sc_r, sc_w, "rescored")
    ids_b, sc_b = st.topk_batch_rescored(st.encode_query_batch(c["qs"]), orig, c["qs"], k, cand)
    ids_1, sc_1 = st.topk_rescored(st.encode_query(c["qs"][1]), orig, c["qs"][1], k, cand)
    assert np.array_equal(ids_b[1], ids_1)
    assert_bits_equal(sc_b[1], sc_1, "batch rescored")


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals(tmp_path):
    got = um.refusals(_lib, tmp_path)
    assert len(got) == 7 * 3 + 2 * 14 + 5
    for what, st, want, out in got:
        assert st == want and out is None, (what, st, want)
    x = np.ones((4, 128), f32)
    with pytest.raises(qa.EncodingError, match="L1"):
        E.encode(x, qa.VectorParameters(128, 4, D.L1, False), rotated=True)
    with pytest.raises(qa.EncodingError, match="multiple of 64"):
        E.encode(x[:, :100], qa.VectorParameters(100, 4, D.Dot, False), rotated=True)
    with pytest.raises(qa.EncodingError, match="multiple of 64"):
        E.encode_stream(lambda: iter([x[:, :96]]), qa.VectorParameters(96, 4, D.L2, False), rotated=True)
    with pytest.raises(qa.EncodingError, match="rotated"):
        qa.ShardedVectorsU8.encode(x, qa.VectorParameters(128, 4, D.Dot, False), [0, 0], rotated=True)
    h = E.encode(x, qa.VectorParameters(128, 4, D.Dot, False), rotated=True)
    with pytest.raises(qa.EncodingError, match="128"):  # a rotated store takes queries of its own dim only
        h.encode_query(np.ones(64, f32))
    with pytest.raises(qa.EncodingError, match="128"):
        h.encode_query_batch(np.ones((3, 192), f32))
    # rescoring compares the base metric: originals of another metric are still refused
    other = qa.OriginalVectors.from_data(x, qa.VectorParameters(128, 4, D.L2, False))
    with pytest.raises(qa.EncodingError):
        h.topk_rescored(h.encode_query(x[0]), other, x[0], 1, 1)
